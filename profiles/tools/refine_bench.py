#!/usr/bin/env python3
"""Time the pose refinement against the class averages on one GPU, two routes over the same stack, poses, labels and
references:

  hip     tvae.refine.refine_poses (tvae_pose_refine in slices of the stack that bound its workspace)
  aten    for every angle affine_grid + grid_sample(align_corners=True, padding_mode='zeros', bilinear) of the images' references
          on the extended grid, then unfold / einsum over the shifts for num, avg_pool2d of the squares for pp, the scores and
          an argmax; in chunks of images that bound the unfolded operand to 1 GB

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route are reported, the multiply-adds per second of the hip route (NA NS^2 n^2 C per image:
the correlations alone) and their share of the fp32 vector peak (157.3 TFLOPS = 78.65e12 multiply-adds per second), and the
largest difference between the best scores of the two routes.  One JSON line per (shape, S) on stdout, all of them in --out:

  python profiles/tools/refine_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--angle-steps 8] [--shifts 2,3]
                                        [--reps 10] [--warmup 2] [--skip-route aten] [--tag NAME]
                                        [--out profiles/refine_bench_NAME.json]
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

PEAK_FMA_PER_S = 157.3e12 / 2


def parse_shape(s):
    N, n = s.split('x')
    return int(N), int(n)


def multiply_adds(n, C, A, S):
    """The correlations of one image: NA NS^2 n^2 C."""
    return (2 * A + 1) * (2 * S + 1) ** 2 * n * n * C


def build_parser():
    ap = argparse.ArgumentParser('Pose refinement: tvae_pose_refine against the ATen route')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '20000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shifts', type=lambda s: [int(v) for v in s.split(',')], default=[2, 3])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-route', default=None, choices=['hip', 'aten'])
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/refine_bench_<tag>.json')
    return ap


def aten_refine(images, theta, dx, labels, refs, t, A, step, S):
    """-> the best score of every image [N].  The grid of affine_grid spans the EXTENDED frame: x = e g with
    e = (n + 2S - 1) / (n - 1); the sampling point of the reference is (u0, -u1) with u = (x - t dx) R(theta)."""
    N, C, n, _ = images.shape
    ne, NS = n + 2 * S, 2 * S + 1
    e = (ne - 1) / (n - 1)
    chunk = max(1, (1 << 28) // (NS * NS * n * n * C))
    best = torch.empty(N, device=images.device)
    for i0 in range(0, N, chunk):
        y = images[i0:i0 + chunk]
        r = refs[labels[i0:i0 + chunk]]
        d = dx[i0:i0 + chunk]
        yy = (y * y).sum(dim=(1, 2, 3))
        top = torch.full((y.shape[0],), -math.inf, device=images.device)
        for a in range(-A, A + 1):
            th = theta[i0:i0 + chunk] + a * step
            c, s = torch.cos(th), torch.sin(th)
            m = torch.stack([torch.stack([e * c, e * s, -t * (d[:, 0] * c - d[:, 1] * s)], 1),
                             torch.stack([-e * s, e * c, t * (d[:, 0] * s + d[:, 1] * c)], 1)], 1)
            grid = torch.nn.functional.affine_grid(m, [y.shape[0], C, ne, ne], align_corners=True)
            T = torch.nn.functional.grid_sample(r, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
            win = T.unfold(2, n, 1).unfold(3, n, 1)                              # [M][C][NS][NS][n][n]
            num = torch.einsum('mcijrq,mcrq->mij', win, y)
            pp = torch.nn.functional.avg_pool2d(T * T, n, stride=1).sum(1) * float(n * n)
            score = num / torch.sqrt(pp * yy.view(-1, 1, 1)).clamp(min=1e-30)
            top = torch.maximum(top, score.flatten(1).max(1).values)
        best[i0:i0 + chunk] = top
    return best


def main(args):
    from tvae import refine
    if not torch.cuda.is_available():
        raise SystemExit('refine_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    A, K, t = args.angle_steps, args.clusters, 1.0
    step = math.pi / 8 / max(A, 1)
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, K=K, A=A,
                angle_step=step, timing='HIP events per route, routes alternated inside a repetition')
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
        for S in args.shifts:
            out = {}

            def hip():
                out['hip'] = refine.refine_poses(images, theta, dx, labels, refs, t, A, step, S)[2][:, 1]

            def aten():
                out['aten'] = aten_refine(images, theta, dx, labels, refs, t, A, step, S)

            routes = [(nm, fn) for nm, fn in (('hip', hip), ('aten', aten)) if nm != args.skip_route]
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
            macs = float(N) * multiply_adds(n, 1, A, S)
            row = dict(N=N, n=n, C=1, K=K, A=A, S=S, multiply_adds=macs)
            for nm, _ in routes:
                if nm in errors:
                    row[nm + '_error'] = errors[nm]
                    continue
                ms = float(np.median(times[nm]))
                row[nm + '_ms'] = round(ms, 3)
                row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
            if 'hip_ms' in row:
                rate = macs / (row['hip_ms'] * 1e-3)
                row['hip_multiply_adds_per_s'] = rate
                row['hip_share_of_fp32_vector_peak'] = round(rate / PEAK_FMA_PER_S, 4)
            if 'hip_ms' in row and 'aten_ms' in row:
                row['hip_speedup_over_aten'] = round(row['aten_ms'] / row['hip_ms'], 2)
                row['best_score_max_abs_diff'] = float((out['hip'] - out['aten']).abs().max())
            print(json.dumps(row), flush=True)
            rows.append(row)
            out.clear()
            torch.cuda.empty_cache()
        del images
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'refine_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
