#!/usr/bin/env python3
"""Measure the sub-pixel pose polish on one GPU: what an evaluation and a whole polish cost beside the grid search, and what
the polish buys on a planted stack with noise.

Time, per shape N x n (C = 1, K classes), the four routes alternated inside every repetition, HIP events around each:
  moments   one tvae_pose_moments launch (one template per image with its derivatives, 15 sums)
  refine00  one tvae_pose_refine call at A = 0, S = 0: the existing launch that builds the same single template per image
  polish    tvae.polish.polish_poses, `--iterations` trial poses (1 + iterations evaluations and as many step launches)
  grid      one tvae.refine.refine_poses round at A = --angle-steps, S = --shift
With --gather-lib PATH (a libtvae_cluster.so whose abi_polish was compiled with -DTVAE_POLISH_STAGED=0) the moments launch of
that build, which gathers the reference from L2 instead of staging its plane in LDS, is timed beside the others.

Quality, on a planted stack N x n with K smooth references, Gaussian noise of standard deviation --sigma on blobs of amplitude
about 1, starts off by up to 10 degrees and 2 pixels: refine_rounds alone against refine_rounds + polish_rounds (cross_halves
both).  Recorded: the half-set FRC resolution of every class (tvae.resolution, pixels at 0.143 and 0.5; mean over the classes),
and the median and largest shift error in pixels against the planted translations, raw and after the median offset of the
image's class is taken out (a class average may sit anywhere; only the spread around it blurs the average).

One JSON line per measurement on stdout, all of them in --out:
  python profiles/tools/polish_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--iterations 8] [--reps 10]
                                        [--warmup 2] [--quality 20000x64] [--sigma 0.3,1.0] [--gather-lib PATH] [--tag NAME]
"""
import argparse
import ctypes
import json
import math
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
    ap = argparse.ArgumentParser('Pose polish: tvae_pose_moments and the whole polish beside the grid search')
    ap.add_argument('--shapes', type=lambda s: [v for v in s.split(',') if v], default=['100000x64', '20000x128'],
                    help='N x n, comma separated; empty: no timing')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--iterations', type=int, default=8)
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shift', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--quality', default='20000x64', help='N x n of the planted stack; empty: no quality run')
    ap.add_argument('--sigma', type=lambda s: [float(v) for v in s.split(',')], default=[0.3, 1.0])
    ap.add_argument('--gather-lib', default=None, help='a build of libtvae_cluster.so whose moments kernel gathers from L2')
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/polish_bench_<tag>.json')
    return ap


def foreign_moments(path):
    """tvae_pose_moments of another build of the library, called through ctypes on the current stream."""
    L = ctypes.CDLL(path)
    f = L.tvae_pose_moments
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_float] * 3 + [ctypes.c_void_p]

    def call(Y, th, dx, cls, refs, mom, N, C, n, K, t):
        rc = f(Y.data_ptr(), th.data_ptr(), dx.data_ptr(), cls.data_ptr(), refs.data_ptr(), mom.data_ptr(), N, C, n, K, t, 0.0, 0.0,
               torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('tvae_pose_moments of {} returned {}'.format(path, rc))
    return call


def time_routes(routes, reps, warmup):
    times = {nm: [] for nm, _ in routes}
    for rep in range(warmup + reps):
        for nm, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[nm].append(e0.elapsed_time(e1))
    return times


def timing(args, dev, rows):
    from tvae import _cluster_lib as CL
    from tvae import polish, refine
    K, A, S, t = args.clusters, args.angle_steps, args.shift, 1.0
    gather = foreign_moments(args.gather_lib) if args.gather_lib else None
    for shp in args.shapes:
        N, n = parse_shape(shp)
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.rand(N, 1, n, n, device=dev, generator=g)
        refs = torch.rand(K, 1, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        labels = torch.randint(0, K, (N,), device=dev, generator=g)
        cls = labels.to(torch.int32)
        mom, mom2 = torch.empty(N, 15, device=dev), torch.empty(N, 15, device=dev)
        routes = [('moments', lambda: CL.call('tvae_pose_moments', images, theta, dx, cls, refs, mom, N, 1, n, K, t, 0.0, 0.0)),
                  ('refine00', lambda: refine.refine_poses(images, theta, dx, labels, refs, t, 0, 0.0, 0)),
                  ('polish', lambda: polish.polish_poses(images, theta, dx, labels, refs, t, args.iterations)),
                  ('grid', lambda: refine.refine_poses(images, theta, dx, labels, refs, t, A, None, S))]
        if gather:
            routes.insert(1, ('moments_gather', lambda: gather(images, theta, dx, cls, refs, mom2, N, 1, n, K, t)))
        times = time_routes(routes, args.reps, args.warmup)
        row = dict(kind='time', N=N, n=n, C=1, K=K, iterations=args.iterations, grid_A=A, grid_S=S)
        for nm, _ in routes:
            row[nm + '_ms'] = round(float(np.median(times[nm])), 3)
            row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
        row['moments_over_refine00'] = round(row['moments_ms'] / row['refine00_ms'], 3)
        row['polish_over_grid'] = round(row['polish_ms'] / row['grid_ms'], 3)
        # what an evaluation has to move at the least: the image once, 15 sums out (the references stay in cache)
        row['moments_image_bytes_per_s'] = float(N) * n * n * 4 / (row['moments_ms'] * 1e-3)
        if gather:
            row['gather_build_same_bits'] = bool(torch.equal(mom.view(torch.int32), mom2.view(torch.int32)))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del images, mom, mom2
        torch.cuda.empty_cache()


def smooth_refs(n, K, dev, g):
    """[K][1][n][n]: sums of four Gaussians, off-centre, small at the border of the frame."""
    ax = torch.arange(n, device=dev) - (n - 1) / 2
    ii, jj = torch.meshgrid(ax, ax, indexing='ij')
    refs = torch.zeros(K, 1, n, n, device=dev)
    u = lambda lo, hi: float(torch.rand((), device=dev, generator=g)) * (hi - lo) + lo
    for k in range(K):
        for _ in range(4):
            ci, cj, sig = u(-0.22, 0.22) * n, u(-0.22, 0.22) * n, u(0.05, 0.09) * n
            refs[k, 0] += u(0.5, 1.5) * torch.exp(-((ii - ci) ** 2 + (jj - cj) ** 2) / (2 * sig * sig))
    return refs


def render(refs, labels, theta, dx, t):
    """The images that show refs[labels] at the poses: the reference sampled at (u0, -u1), u = (x - t dx) R(theta)."""
    n = refs.shape[-1]
    out = torch.empty(labels.numel(), 1, n, n, device=refs.device)
    for i0 in range(0, labels.numel(), 4096):
        sl = slice(i0, i0 + 4096)
        c, s, d = torch.cos(theta[sl]), torch.sin(theta[sl]), dx[sl]
        m = torch.stack([torch.stack([c, s, -t * (d[:, 0] * c - d[:, 1] * s)], 1),
                         torch.stack([-s, c, t * (d[:, 0] * s + d[:, 1] * c)], 1)], 1)
        grid = torch.nn.functional.affine_grid(m, [c.numel(), 1, n, n], align_corners=True)
        out[sl] = torch.nn.functional.grid_sample(refs[labels[sl]], grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return out


def shift_errors(dx, dx_true, labels, K, n, t):
    """-> (median, largest) raw and (median, largest) after the median offset of the image's class is taken out, in pixels."""
    e = (dx - dx_true).double() * t * (n - 1) / 2
    raw = e.abs().amax(1)
    rel = e.clone()
    for k in range(K):
        m = labels == k
        if m.any():
            rel[m] -= e[m].median(0).values
    rel = rel.abs().amax(1)
    return [float(raw.median()), float(raw.max())], [float(rel.median()), float(rel.max())]


def quality(args, dev, rows):
    from tvae import polish, refine
    N, n = parse_shape(args.quality)
    K, t = args.clusters, 1.0
    for sigma in args.sigma:
        g = torch.Generator(device=dev).manual_seed(7 + N + n)
        refs = smooth_refs(n, K, dev, g)
        labels = torch.randint(0, K, (N,), device=dev, generator=g)
        th_true = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx_true = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.12
        images = render(refs, labels, th_true, dx_true, t) + sigma * torch.randn(N, 1, n, n, device=dev, generator=g)
        th0 = th_true + (torch.rand(N, device=dev, generator=g) * 2 - 1) * math.radians(10)
        dx0 = dx_true + (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 2 * 2 / (n - 1)
        lab = labels.cpu().numpy()
        res = lambda th, d: refine._resolutions(images, th, d, lab, K, t).mean(0).tolist()
        row = dict(kind='quality', N=N, n=n, K=K, sigma=sigma, iterations=args.iterations)
        row['start'] = dict(resolution_px=res(th0, dx0), shift_error_px=shift_errors(dx0, dx_true, labels, K, n, t))
        th1, d1, _ = refine.refine_rounds(images, th0, dx0, lab, K, t, cross_halves=True)
        row['refined'] = dict(resolution_px=res(th1, d1), shift_error_px=shift_errors(d1, dx_true, labels, K, n, t))
        th2, d2, hist = polish.polish_rounds(images, th1, d1, lab, K, t, rounds=2, iterations=args.iterations, cross_halves=True)
        row['polished'] = dict(resolution_px=res(th2, d2), shift_error_px=shift_errors(d2, dx_true, labels, K, n, t),
                               mean_scores=hist['scores'].tolist(), mean_accepted_steps=hist['steps'].tolist())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del images
        torch.cuda.empty_cache()


def main(args):
    if not torch.cuda.is_available():
        raise SystemExit('polish_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup,
                timing='HIP events per route, routes alternated inside a repetition, medians',
                resolution_px='[at FRC 0.143, at FRC 0.5], mean over the classes', shift_error_px='[[median, largest] raw, '
                '[median, largest] after the class median offset]')
    print(json.dumps(head), flush=True)
    rows = []
    if args.shapes:
        timing(args, dev, rows)
    if args.quality:
        quality(args, dev, rows)
    path = args.out or os.path.join(HERE, '..', 'polish_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
