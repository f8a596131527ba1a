"""Guard bands around every tensor of a C-ABI call: an out-of-bounds WRITE detector (and, with replay, an out-of-bounds
READ and determinism check) for libtvae_hip.so.  A plain helper module, used by the GPU test files.

Every launch goes through tvae._lib.call, which consults tvae._lib.CALL_HOOK.  `GuardedCalls` installs itself there and
runs each call like this:

  1. the tensor arguments are collected; arguments whose byte ranges overlap (in-place calls, two views of one buffer)
     form one group;
  2. every group gets a fresh allocation  band | interior | band  (BAND_WORDS four-byte words per side) and the current
     contents of its tensors are copied into the interior.  The interior keeps the original address modulo ALIGN bytes:
     launchers pick a vector or a scalar instance from the alignment of a pointer, and the guarded run has to take the
     instance production takes.  The bands hold a known word (a NaN or 1e4, as int32 so that NaN compares);
  3. the entry point runs on the relocated tensors (same scalars, same stream);
  4. every band is compared word for word, every interior is copied back over the original tensor;
  5. replay=True: the call runs a second time from the same PRE-CALL contents under the other band word, and every
     interior must be bit-for-bit the same after both runs (what a kernel reads beyond its tensors, or a result that
     depends on the order of atomics, differs between the two).

An error code of the entry point is raised exactly as without the guard, after the bands have been looked at; a rejected
call must also have left every interior as it was.  Comparisons stay on the device and are read back once, in check()
(GuardedCalls.__exit__), so a test synchronises once; the report still names the call: entry point, argument positions,
side, byte offsets of the first and last changed word counted from the tensor (0 = the word that touches it) and the
scalar arguments.

The core (group_ranges, Relocation) only uses torch tensor operations and data_ptr(): it runs on CPU tensors too, with a
Python function standing in for the entry point (tests/test_host_cpu.py).
"""
import struct

import torch

BAND_WORDS = 8192          # per side; the read test of tests/test_hip_modules.py uses the same
ALIGN = 256
FILL_NAN = struct.unpack('<i', struct.pack('<I', 0x7FC00000))[0]
FILL_1E4 = struct.unpack('<i', struct.pack('<f', 1e4))[0]
FILLS = (FILL_NAN, FILL_1E4)

# entry points that have run under a guard in this process (tests/test_hip_primitives.py compares it with SIGNATURES)
GUARDED_NAMES = set()

# entry points exempt from the BITWISE part of replay (they keep the band check): name -> reason.  None so far.
REPLAY_EXEMPT = {}


class GuardViolation(AssertionError):
    def __init__(self, violations):
        self.violations = violations
        super().__init__('\n'.join(v['text'] for v in violations))


def group_ranges(ranges):
    """ranges: list of (start, end) byte addresses (end exclusive).  Returns [(start, end, [indices])]: ranges that overlap
    (share at least one byte), directly or through a chain, form one group; ranges that merely touch stay apart."""
    order = sorted(range(len(ranges)), key=lambda i: ranges[i])
    groups = []
    for i in order:
        s, e = ranges[i]
        if groups and s < groups[-1][1]:
            groups[-1][1] = max(groups[-1][1], e)
            groups[-1][2].append(i)
        else:
            groups.append([s, e, [i]])
    return [(s, e, idx) for s, e, idx in groups]


def _words(t):
    """A contiguous tensor as a flat int32 view (bit patterns: NaN compares)."""
    return t.reshape(-1).view(torch.int32)


def _diff_stats(a, b):
    """a: (rows, W) int32, b: broadcastable.  (rows, 3) int64: number of differing words, index of the first, of the last."""
    bad = a != b
    W = a.shape[1]
    idx = torch.arange(W, device=a.device)
    return torch.stack([bad.sum(1), torch.where(bad, idx, W).amin(1), torch.where(bad, idx, -1).amax(1)], 1)


class Relocation:
    """Guard-banded copies of the tensors `tensors` (contiguous, non-empty, same device; any mix of 4- and 8-byte dtypes).
    .tensors: the relocated views, in the same order, same shapes and dtypes."""

    def __init__(self, tensors, fill, band_words=BAND_WORDS):
        self.orig, self.fill, self.band = list(tensors), fill, band_words * 4
        rng = []
        for t in self.orig:
            nb = t.numel() * t.element_size()
            assert t.is_contiguous() and nb > 0 and nb % 4 == 0 and t.data_ptr() % 4 == 0, (t.shape, t.dtype)
            rng.append((t.data_ptr(), t.data_ptr() + nb))
        self.ranges, self.groups = rng, group_ranges(rng)
        self.tensors = [None] * len(self.orig)
        self.bufs, self.offs = [], []
        for s, e, idx in self.groups:
            dev = self.orig[idx[0]].device
            assert all(self.orig[i].device == dev for i in idx)
            buf = torch.empty(2 * self.band + (e - s) + ALIGN, dtype=torch.uint8, device=dev)
            base = buf.data_ptr()
            assert base % 8 == 0
            off = self.band + (s - (base + self.band)) % ALIGN          # (base + off) = s  (mod ALIGN)
            w = buf[:buf.numel() // 4 * 4].view(torch.int32)
            w[:off // 4].fill_(fill)
            w[(off + e - s) // 4:].fill_(fill)
            for i in idx:
                t = self.orig[i]
                o = off + rng[i][0] - s
                v = buf[o:o + rng[i][1] - rng[i][0]].view(t.dtype).view(t.shape)
                v.copy_(t.detach())
                self.tensors[i] = v
            self.bufs.append(buf)
            self.offs.append(off)

    def interior(self, g):
        s, e, _ = self.groups[g]
        return self.bufs[g][self.offs[g]:self.offs[g] + e - s].view(torch.int32)

    def band_stats(self):
        """(2 * groups, 3) int64 on the device: rows 2g (in front of group g; word index counted BACKWARDS from the tensor) and
        2g + 1 (behind it; counted forwards) hold [changed words, first index, last index]."""
        rows = []
        for g, (s, e, _) in enumerate(self.groups):
            off, buf = self.offs[g], self.bufs[g]
            rows.append(buf[off - self.band:off].view(torch.int32).flip(0))
            rows.append(buf[off + e - s:off + e - s + self.band].view(torch.int32))
        return _diff_stats(torch.stack(rows), self.fill)

    def untouched_stats(self):
        """(tensors, 3): every relocated tensor against its original (a rejected call has to leave them alone)."""
        return torch.cat([_diff_stats(_words(v)[None], _words(t.detach())[None]) for v, t in zip(self.tensors, self.orig)])

    def copy_back(self):
        with torch.no_grad():
            for v, t in zip(self.tensors, self.orig):
                t.data.copy_(v)                # .data: saved-for-backward tensors keep their version


class GuardedCalls:
    """Context manager: every tvae._lib.call inside runs under guard bands (see the module docstring).  check() -- called on
    exit -- raises GuardViolation listing every finding; .violations keeps them as dicts
    {entry, kind ('band' | 'replay' | 'rejected'), args (positions), side, count, first, last, scalars, text}."""

    def __init__(self, replay=False, band_words=BAND_WORDS, install=True):
        self.replay, self.band_words, self.install = replay, band_words, install
        self._pending, self.violations, self.calls = [], [], 0

    def __enter__(self):
        if self.install:
            from tvae import _lib
            self._old = _lib.set_call_hook(self.run)
        return self

    def __exit__(self, et, ev, tb):
        if self.install:
            from tvae import _lib
            _lib.set_call_hook(self._old)
        self.check()
        return False

    # -- one call -------------------------------------------------------------------------------------------------------
    def run(self, name, sig, args, do_call):
        GUARDED_NAMES.add(name)
        self.calls += 1
        pos = [p for p, (c, a) in enumerate(zip(sig, args))
               if c == 'p' and torch.is_tensor(a) and a.numel() > 0 and a.is_contiguous()]
        scalars = {p: a for p, (c, a) in enumerate(zip(sig, args)) if c != 'p'}
        tens = [args[p] for p in pos]

        def attempt(fill):
            rel = Relocation(tens, fill, self.band_words)
            new = list(args)
            for p, v in zip(pos, rel.tensors):
                new[p] = v
            err = None
            try:
                do_call(tuple(new))
            except Exception as e:                       # the entry point's error code: raised after the bookkeeping
                err = e
            # per group: (bytes, positions of the arguments that start at its first byte, ... that end at its last)
            edges = [(e - s, tuple(pos[i] for i in idx if rel.ranges[i][0] == s),
                      tuple(pos[i] for i in idx if rel.ranges[i][1] == e)) for s, e, idx in rel.groups]
            self._pending.append(('band', name, scalars, pos, edges, rel.band_stats()))
            if err is not None:
                self._pending.append(('rejected', name, scalars, pos, None, rel.untouched_stats()))
            return rel, err

        first, err = attempt(FILLS[0])
        if err is None and self.replay:
            second, err2 = attempt(FILLS[1])             # the originals still hold the pre-call contents
            if err2 is not None:
                self._pending.append(('replay-error', name, scalars, pos, None, repr(err2)))
            elif name not in REPLAY_EXEMPT:
                st = torch.cat([_diff_stats(first.interior(g)[None], second.interior(g)[None])
                                for g in range(len(first.groups))])
                self._pending.append(('replay', name, scalars, pos, first.groups, st))
        first.copy_back()
        if err is not None:
            raise err

    # -- deferred verdict -----------------------------------------------------------------------------------------------
    def check(self):
        pend, self._pending = self._pending, []
        found = []
        stats = [r[5] for r in pend if torch.is_tensor(r[5])]
        flat = torch.cat([s.reshape(-1, 3).to('cpu', torch.int64) for s in stats]).tolist() if stats else []
        at = 0
        for kind, name, scalars, pos, groups, st in pend:
            if not torch.is_tensor(st):
                found.append(dict(entry=name, kind=kind, args=tuple(pos), side=None, count=None, first=None, last=None,
                                  scalars=scalars, text=f'{name}: the replayed call failed where the first run passed: {st}; '
                                                        f'scalars {scalars}'))
                continue
            rows = flat[at:at + st.shape[0]]
            at += st.shape[0]
            for r, (n, lo, hi) in enumerate(rows):
                if n == 0:
                    continue
                if kind == 'band':
                    nbytes, front, back = groups[r // 2]
                    side, who = ('behind', back) if r % 2 else ('in front of', front)
                    text = (f'{name}: {n} word(s) written {side} argument(s) {who}: first at byte offset {4 * lo}, last at '
                            f'{4 * hi} from the tensor ({nbytes} bytes); scalars {scalars}')
                elif kind == 'replay':
                    s, e, idx = groups[r]
                    side, who = 'interior', tuple(pos[i] for i in idx)
                    text = (f'{name}: two runs from the same inputs differ in {n} word(s) of argument(s) {who} (first at byte '
                            f'{4 * lo}, last at {4 * hi} of {e - s}) under different guard-band contents; scalars {scalars}')
                else:
                    side, who = 'interior', (pos[r],)
                    text = (f'{name}: the call was rejected but changed {n} word(s) of argument {pos[r]} (first at byte '
                            f'{4 * lo}, last at {4 * hi}); scalars {scalars}')
                found.append(dict(entry=name, kind=kind, args=who, side=side, count=n, first=4 * lo, last=4 * hi,
                                  scalars=scalars, text=text))
        self.violations += found
        if found:
            raise GuardViolation(found)
