#!/usr/bin/env python3
"""Time the reassignment against the class averages on one GPU, two routes over the same stack, poses, candidate lists and
references:

  fused   tvae.classify.classify_poses (tvae_pose_classify in slices of the stack that bound its workspace)
  mcall   what the repository offered before: M calls of tvae.refine.refine_poses with cls = cand[:, m], then torch.stack /
          max / gather for the winner and its pose

The mcall route runs on the library named by --parent-lib (the parent commit's libtvae_cluster.so), so that the refactored
refine_corr_kernel of this tree cannot flatter the comparison.  The binding checks every symbol of its tables when it loads a
library, and the parent's library lacks the new entry point, so TVAE_CLUSTER_LIB alone cannot name it for this package: the
tool loads it beside the current one with the tables minus the new names.  Without --parent-lib both routes use the current
library and the JSON says so.

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route, their ratio and the peak of the extra device memory each route allocates (its
workspace and intermediates: torch.cuda.max_memory_allocated over the route minus what was allocated before it) are
reported, and whether the two routes agree on every label.  One JSON line per (shape, M) on stdout, all of them in --out:

  python profiles/tools/classify_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--candidates 10,4]
                                          [--angle-steps 8] [--shift 2] [--reps 10] [--warmup 2] [--parent-lib PATH]
                                          [--tag NAME] [--out profiles/classify_bench_NAME.json]
"""
import argparse
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch

NEW_NAMES = ('tvae_pose_classify', 'tvae_pose_classify_ws_floats')


def parse_shape(s):
    N, n = s.split('x')
    return int(N), int(n)


def build_parser():
    ap = argparse.ArgumentParser('Reassignment: tvae_pose_classify against M calls of tvae_pose_refine')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '20000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--candidates', type=lambda s: [int(v) for v in s.split(',')], default=[10, 4], help='M, comma separated')
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shift', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libtvae_cluster.so for the mcall route")
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/classify_bench_<tag>.json')
    return ap


def load_parent(path):
    """The parent's library under the binding's tables minus the names it cannot have."""
    from tvae import _cluster_lib as CL, _lib
    sigs = {k: v for k, v in CL.SIGNATURES.items() if k not in NEW_NAMES}
    queries = {k: v for k, v in CL.QUERIES.items() if k not in NEW_NAMES}
    return _lib.load_library(path, sigs, queries, 'tvae_cluster_abi_version', CL.ABI_VERSION, 'pass the path of a built library')


class using_lib:
    """Route every call of tvae._cluster_lib through `L` inside the block (None: the current library)."""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        from tvae import _cluster_lib as CL
        self.saved = CL.lib
        if self.L is not None:
            CL.lib = lambda: self.L

    def __exit__(self, *exc):
        from tvae import _cluster_lib as CL
        CL.lib = self.saved


def mcall_route(refine, images, theta, dx, cand, refs, t, A, step, S):
    """-> (labels, theta', dx', best scores [N][M]) the way it had to be done before: ties go wherever torch.max puts them."""
    M = cand.shape[1]
    res = [refine.refine_poses(images, theta, dx, cand[:, m].contiguous(), refs, t, A, step, S) for m in range(M)]
    sb = torch.stack([r[2][:, 1] for r in res], 1)
    win = sb.max(1).indices
    th = torch.stack([r[0] for r in res], 1).gather(1, win[:, None])[:, 0]
    d = torch.stack([r[1] for r in res], 1).gather(1, win[:, None, None].expand(-1, 1, 2))[:, 0]
    return cand.gather(1, win[:, None])[:, 0], th, d, sb


def main(args):
    from tvae import classify, refine
    if not torch.cuda.is_available():
        raise SystemExit('classify_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    parent = load_parent(args.parent_lib) if args.parent_lib else None
    A, S, K, t = args.angle_steps, args.shift, args.clusters, 1.0
    step = math.pi / 8 / max(A, 1)
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, K=K, A=A, S=S,
                angle_step=step, mcall_library='parent' if parent is not None else 'current',
                timing='HIP events per route, routes alternated inside a repetition')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        N, n = parse_shape(shp)
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.rand(N, 1, n, n, device=dev, generator=g)
        refs = torch.rand(K, 1, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        labels = torch.randint(0, K, (N,), device=dev, generator=g)
        latents = torch.rand(N, 2, device=dev, generator=g)
        for M in args.candidates:
            cand = classify.candidate_lists(labels, K, latents, min(M, K))
            out = {}

            def fused():
                out['fused'] = classify.classify_poses(images, theta, dx, cand, refs, t, A, step, S)

            def mcall():
                with using_lib(parent):
                    out['mcall'] = mcall_route(refine, images, theta, dx, cand, refs, t, A, step, S)

            routes = [('fused', fused), ('mcall', mcall)]
            times = {nm: [] for nm, _ in routes}
            peak = {nm: 0 for nm, _ in routes}
            for rep in range(args.warmup + args.reps):
                for nm, fn in routes:
                    out.pop(nm, None)
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    peak[nm] = max(peak[nm], torch.cuda.max_memory_allocated() - base)
                    if rep >= args.warmup:
                        times[nm].append(e0.elapsed_time(e1))
            row = dict(N=N, n=n, C=1, K=K, M=cand.shape[1], A=A, S=S)
            for nm, _ in routes:
                row[nm + '_ms'] = round(float(np.median(times[nm])), 3)
                row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
                row[nm + '_peak_extra_bytes'] = int(peak[nm])
            row['mcall_over_fused'] = round(row['mcall_ms'] / row['fused_ms'], 3)
            row['labels_differ'] = int((out['fused'][0] != out['mcall'][0]).sum())
            row['best_scores_bitwise_equal'] = bool(torch.equal(out['fused'][3][:, :, 1], out['mcall'][3]))
            print(json.dumps(row), flush=True)
            rows.append(row)
            out.clear()
            torch.cuda.empty_cache()
        del images
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'classify_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
