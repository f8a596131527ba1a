#!/usr/bin/env python3
"""Compare the device code of two builds of the libraries, kernel by kernel.

    compare_kernels.py OLD/libtvae_hip.so NEW/libtvae_hip.so [OLD/libtvae_cluster.so NEW/libtvae_cluster.so]
    compare_kernels.py --units build/           # which object file emits which kernel (one line per kernel)

For every gfx code object embedded in a library it reads the kernels' names and resource metadata (VGPRs, AGPRs, SGPRs,
LDS, private segment, wavefront size: the notes) and hashes the bytes of each kernel's code (symbol offset and size in
.text).  It reports: the number of code objects and the copies of each name in either build, whether the copies of a
name WITHIN a build are identical, and every name whose bytes or metadata differ BETWEEN the builds (a name whose old copies
differ from one another, the new build holding one of them, is listed apart: `--units` tells which old object held which).
Exit status 1 if the sets of names differ or any kernel differs.  It hashes bytes and reads metadata; it inspects no instruction."""
import collections
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

READELF = os.environ.get('LLVM_READELF', '/opt/rocm/lib/llvm/bin/llvm-readelf')
MAGIC = b'\x7fELF\x02\x01\x01\x40'                       # ELF64, little endian, OS ABI 64 = AMDGPU HSA
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'wavefront_size',
        'max_flat_workgroup_size', 'kernarg_segment_size')


def code_objects(path):
    """The embedded code objects of a library or object file, one bytes object each (cut at the next one's start)."""
    data = open(path, 'rb').read()
    offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    return [data[o:e] for o, e in zip(offs, offs[1:] + [len(data)])]


def kernels_of(co):
    """{name: (sha1 of the code bytes, size, metadata tuple)} of one code object."""
    with tempfile.NamedTemporaryFile(suffix='.co') as f:
        f.write(co)
        f.flush()
        run = lambda *a: subprocess.run([READELF, *a, f.name], capture_output=True, text=True).stdout
        notes, secs, syms = run('--notes'), run('-S', '-W'), run('-s', '-W')
    m = re.search(r'\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', secs)
    if not m:
        return {}
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    meta = {}
    for blk in re.split(r'\n  - ', notes):                # one entry of amdhsa.kernels each; its own keys are indented by four
        blk = '    ' + blk
        n = re.search(r'^    \.name:\s+(\S+)', blk, re.M)
        if n and re.search(r'^    \.vgpr_count:', blk, re.M):
            meta[n.group(1)] = tuple(int(re.search(r'^    \.%s:\s+(\d+)' % k, blk, re.M).group(1)) for k in META)
    out = {}
    for ln in syms.splitlines():
        p = ln.split()
        if len(p) == 8 and p[3] == 'FUNC' and p[7] in meta:
            a, size = int(p[1], 16), int(p[2])
            out[p[7]] = (hashlib.sha1(co[off + a - addr: off + a - addr + size]).hexdigest(), size, meta[p[7]])
    assert set(out) == set(meta), sorted(set(out) ^ set(meta))
    return out


def library(path):
    """(number of code objects, {name: [record of every copy]})"""
    cos = code_objects(path)
    copies = collections.defaultdict(list)
    for co in cos:
        for n, r in kernels_of(co).items():
            copies[n].append(r)
    return len(cos), copies


def compare(old, new):
    (no, ko), (nn, kn) = library(old), library(new)
    bad = 0
    for tag, n, k in (('old', no, ko), ('new', nn, kn)):
        tot = sum(len(v) for v in k.values())
        print('%s %s: %d code objects, %d distinct kernels, %d copies, %d bytes of kernel code, %d names in more than one object'
              % (tag, path_tail(old if tag == 'old' else new), n, len(k), tot, sum(r[1] for v in k.values() for r in v),
                 sum(len(v) > 1 for v in k.values())))
        for name, v in sorted(k.items()):
            if len(set(v)) > 1:
                print('  %s: copies of %s differ from one another: %s' % (tag, name, sorted(set(v))))
    for name in sorted(set(ko) ^ set(kn)):
        print('  only in %s: %s' % ('old' if name in ko else 'new', name))
        bad += 1
    same = 0
    for name in sorted(set(ko) & set(kn)):
        a, b = set(ko[name]), set(kn[name])
        if a == b:
            same += 1
            continue
        if b < a:            # the old build's copies differ from one another and the new build has one of them
            print('  one of the old copies: %s\n    old %s\n    new %s' % (name, sorted(a), sorted(b)))
            continue
        bad += 1
        ra, rb = sorted(a)[0], sorted(b)[0]
        what = ('code bytes ' if ra[:2] != rb[:2] else '') + ('metadata' if ra[2] != rb[2] else '')
        print('  DIFFERS (%s): %s\n    old %s\n    new %s' % (what.strip(), name, ra, rb))
    print('identical code bytes and metadata: %d of %d common names' % (same, len(set(ko) & set(kn))))
    return bad


def path_tail(p):
    return os.sep.join(p.split(os.sep)[-2:])


def units(build_dir):
    for o in sorted(glob.glob(os.path.join(build_dir, '*.o'))):
        for co in code_objects(o):
            for n, r in sorted(kernels_of(co).items()):
                print('%s %s %6d %s %s' % (os.path.basename(o)[:-2], r[0][:12], r[1], r[2], n))


if __name__ == '__main__':
    a = sys.argv[1:]
    if len(a) == 2 and a[0] == '--units':
        units(a[1])
        sys.exit(0)
    if len(a) not in (2, 4):
        sys.exit(__doc__)
    sys.exit(1 if sum(compare(a[i], a[i + 1]) for i in range(0, len(a), 2)) else 0)
