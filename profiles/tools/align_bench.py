#!/usr/bin/env python3
"""Time the aligned class averages on one GPU, three routes over the same stack, poses and labels:

  fused   tvae_class_average (tvae.align.class_averages without its allocations): the stack is read once, the aligned
          images are never written
  plain   tvae_align_stack, then a segmented mean of its output in torch (index_select by class order + segment_reduce)
  aten    affine_grid + grid_sample(align_corners=True, padding_mode='zeros', bilinear) with y_grid = -x1, then index_add_
          and a division by the counts

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route are reported with the effective bandwidth stack bytes / median time, and the
largest difference of the plain and the ATen averages from the fused ones.  One JSON line per (shape, K) on stdout, all of
them in --out:

  python profiles/tools/align_bench.py [--shapes 20000x64,100000x128] [--clusters 10,100] [--channels 1] [--reps 10]
                                       [--warmup 2] [--skip-aten] [--tag NAME] [--out profiles/align_bench_NAME.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch


def parse_shape(s):
    N, n = s.split('x')
    return int(N), int(n)


def build_parser():
    ap = argparse.ArgumentParser('Aligned class averages: fused kernel against align + mean and against ATen')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['20000x64', '100000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=lambda s: [int(v) for v in s.split(',')], default=[10, 100])
    ap.add_argument('--channels', type=int, default=1)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-aten', action='store_true')
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/align_bench_<tag>.json')
    return ap


def aten_matrices(theta, dx, t):
    """[N][2][3] for affine_grid: the grid's x is u0 and its y is -u1, so the sampling point (x0, -x1) is
    (gx c - gy s + t dx0,  gx s + gy c - t dx1)."""
    c, s = torch.cos(theta), torch.sin(theta)
    return torch.stack([torch.stack([c, -s, t * dx[:, 0]], 1), torch.stack([s, c, -t * dx[:, 1]], 1)], 1)


def aten_align(images, theta, dx, t):
    grid = torch.nn.functional.affine_grid(aten_matrices(theta, dx, t), list(images.shape), align_corners=True)
    return torch.nn.functional.grid_sample(images, grid, mode='bilinear', padding_mode='zeros', align_corners=True)


def main(args):
    from tvae import _cluster_lib as CL
    from tvae import align
    if not torch.cuda.is_available():
        raise SystemExit('align_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup,
                channels=args.channels, timing='HIP events per route, routes alternated inside a repetition')
    print(json.dumps(head), flush=True)
    rows = []
    C, t = args.channels, 1.0
    for shp in args.shapes:
        N, n = parse_shape(shp)
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.rand(N, C, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        for K in args.clusters:
            labels = torch.randint(0, K, (N,), device=dev, generator=g)
            order, seg, counts = align.segments(labels, K)
            wsf = CL.query('tvae_class_average_ws_floats', N, K, C, n)
            ws = torch.empty(wsf, device=dev)
            avg = torch.empty(K, C, n, n, device=dev)
            aligned = torch.empty_like(images)
            lengths = counts.to(torch.int64)
            order64, denom = order.to(torch.int64), counts.clamp(min=1).float().view(K, 1, 1, 1)
            out = {}

            def fused():
                CL.call('tvae_class_average', images, theta, dx, order, seg, avg, ws, wsf, N, C, n, K, t)
                out['fused'] = avg

            def plain():
                CL.call('tvae_align_stack', images, theta, dx, aligned, N, C, n, t)
                out['plain'] = torch.segment_reduce(aligned.index_select(0, order64), 'mean', lengths=lengths, axis=0,
                                                    initial=0.0)

            def aten():
                a = aten_align(images, theta, dx, t)
                acc = torch.zeros(K, C, n, n, device=dev)
                acc.index_add_(0, labels, a)
                out['aten'] = acc / denom

            routes = [('fused', fused), ('plain', plain)] + ([] if args.skip_aten else [('aten', aten)])
            times = {nm: [] for nm, _ in routes}
            errors = {}
            for rep in range(args.warmup + args.reps):
                for nm, fn in routes:
                    if nm in errors:
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    try:
                        e0.record()
                        fn()
                        e1.record()
                        torch.cuda.synchronize()
                    except (RuntimeError, NotImplementedError) as e:            # a route this torch build lacks
                        errors[nm] = repr(e)[:300]
                        continue
                    if rep >= args.warmup:
                        times[nm].append(e0.elapsed_time(e1))
                    if rep == 0 and nm != 'fused' and 'fused' in out:
                        out[nm + '_diff'] = float((out[nm] - out['fused']).abs().max())
                    if nm != 'fused':
                        out.pop(nm, None)                                       # let go of the route's result
            stack_bytes = 4.0 * N * C * n * n
            row = dict(N=N, n=n, C=C, K=K, stack_gb=round(stack_bytes / 1e9, 3), ws_mb=round(4.0 * wsf / 1e6, 1),
                       chunk=align.chunk_members(N, K, C, n))
            for nm, _ in routes:
                if nm in errors:
                    row[nm + '_error'] = errors[nm]
                    continue
                ms = float(np.median(times[nm]))
                row[nm + '_ms'] = round(ms, 3)
                row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
                row[nm + '_gbs'] = round(stack_bytes / ms / 1e6, 1)
                if nm + '_diff' in out:
                    row[nm + '_max_abs_diff_from_fused'] = out[nm + '_diff']
            if 'aten_ms' in row:
                row['fused_speedup_over_aten'] = round(row['aten_ms'] / row['fused_ms'], 2)
            if 'plain_ms' in row:
                row['fused_speedup_over_plain'] = round(row['plain_ms'] / row['fused_ms'], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del ws, avg, aligned, out
            torch.cuda.empty_cache()
        del images
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'align_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
