#!/usr/bin/env python3
"""Time the class statistics on one GPU.

Half sets and variance, three routes over the same stack, poses and labels:

  halves   tvae_class_halves (tvae.align.class_halves without its allocations): one pass, three accumulators per pixel
  average  tvae_class_average of the same build: the pass that tvae_class_halves extends (one accumulator)
  route    the only way to the same outputs without it: tvae_class_average on the 2 K labels 2 k + parity, then
           tvae_align_stack, then a segmented mean of the squared aligned images in ATen and the variance from it

Ring correlation of --frc-planes pairs of planes at every side of --frc-sides:

  frc      tvae_class_frc (direct two-stage DFT and ring sums)
  fft      torch.fft.fft2 of both stacks, the three products and index_add_ ring sums in fp64

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route are reported.  One JSON line per measurement on stdout, all of them in --out:

  python profiles/tools/class_stats_bench.py [--shapes 20000x64,100000x128] [--clusters 10] [--channels 1]
        [--frc-planes 100] [--frc-sides 128,256] [--reps 10] [--warmup 2] [--skip-route] [--tag NAME] [--out FILE]
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
    ap = argparse.ArgumentParser('Class statistics: the fused half-set pass and the ring correlation against their baselines')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['20000x64', '100000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=lambda s: [int(v) for v in s.split(',')], default=[10])
    ap.add_argument('--channels', type=int, default=1)
    ap.add_argument('--frc-planes', type=int, default=100)
    ap.add_argument('--frc-sides', type=lambda s: [int(v) for v in s.split(',')], default=[128, 256])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--skip-route', action='store_true', help='leave out the align_stack + ATen route (it needs a second stack)')
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/class_stats_bench_<tag>.json')
    return ap


def timed(routes, reps, warmup):
    """routes: [(name, fn)] -> {name: [ms]}; alternated inside every repetition."""
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


def summary(row, times):
    for nm, ts in times.items():
        row[nm + '_ms'] = round(float(np.median(ts)), 3)
        row[nm + '_ms_min_max'] = [round(min(ts), 3), round(max(ts), 3)]


def ring_table(n, dev):
    k = torch.fft.fftfreq(n, device=dev).mul(n).round().to(torch.int64)
    s4 = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    r = torch.zeros_like(s4)
    for q in range(1, n + 1):                                             # the integer rule, no float comparison
        r += (s4 >= (2 * q - 1) ** 2).to(torch.int64)
    return r.reshape(-1)


def main(args):
    from tvae import _cluster_lib as CL
    from tvae import align
    if not torch.cuda.is_available():
        raise SystemExit('class_stats_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup,
                channels=args.channels, timing='HIP events per route, routes alternated inside a repetition, medians')
    print(json.dumps(head), flush=True)
    rows = []
    C, t = args.channels, 1.0
    for shp in args.shapes:
        N, n = parse_shape(shp)
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.randn(N, C, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        for K in args.clusters:
            labels = torch.randint(0, K, (N,), device=dev, generator=g)
            order, seg, counts = align.segments(labels, K)
            # the labels 2 k + parity of the position within the class: what tvae_class_halves deals out itself
            pos = torch.arange(N, device=dev) - seg[:-1].to(torch.int64).repeat_interleave(counts.to(torch.int64))
            split = torch.empty(N, dtype=torch.int64, device=dev)
            split[order.to(torch.int64)] = 2 * labels[order.to(torch.int64)] + pos % 2
            order2, seg2, _ = align.segments(split, 2 * K)
            wsh = CL.query('tvae_class_halves_ws_floats', N, K, C, n)
            wsa = CL.query('tvae_class_average_ws_floats', N, 2 * K, C, n)
            ws = torch.empty(max(wsh, wsa), device=dev)
            avg = torch.empty(K, C, n, n, device=dev)
            half = torch.empty(2, K, C, n, n, device=dev)
            var = torch.empty(K, C, n, n, device=dev)
            cnt = torch.empty(K, 2, dtype=torch.int32, device=dev)
            avg2 = torch.empty(2 * K, C, n, n, device=dev)
            out = {}

            def halves():
                CL.call('tvae_class_halves', images, theta, dx, order, seg, avg, half, var, cnt, ws, wsh, N, C, n, K, t)

            def average():
                CL.call('tvae_class_average', images, theta, dx, order, seg, avg2[:K], ws, wsa, N, C, n, K, t)

            routes = [('halves', halves), ('average', average)]
            if not args.skip_route:
                aligned = torch.empty_like(images)
                lengths = counts.to(torch.int64)
                order64 = order.to(torch.int64)
                m = counts.to(torch.float64).view(K, 1, 1, 1)

                def route():
                    CL.call('tvae_class_average', images, theta, dx, order2, seg2, avg2, ws, wsa, N, C, n, 2 * K, t)
                    CL.call('tvae_align_stack', images, theta, dx, aligned, N, C, n, t)
                    sq = torch.segment_reduce(aligned.index_select(0, order64).square_(), 'sum', lengths=lengths, axis=0,
                                              initial=0.0).double()
                    mean = torch.segment_reduce(aligned.index_select(0, order64), 'sum', lengths=lengths, axis=0,
                                                initial=0.0).double() / m
                    out['var'] = ((sq - m * mean * mean) / (m - 1).clamp(min=1)).clamp(min=0).float()

                routes.append(('route', route))
            times = timed(routes, args.reps, args.warmup)
            stack_bytes = 4.0 * N * C * n * n
            row = dict(what='halves', N=N, n=n, C=C, K=K, stack_gb=round(stack_bytes / 1e9, 3), ws_mb=round(4.0 * wsh / 1e6, 1))
            summary(row, times)
            row['halves_gbs'] = round(stack_bytes / row['halves_ms'] / 1e6, 1)
            row['halves_over_average'] = round(row['halves_ms'] / row['average_ms'], 3)
            if 'route_ms' in row:
                row['route_over_halves'] = round(row['route_ms'] / row['halves_ms'], 2)
                row['var_max_abs_diff_from_route'] = float((out['var'] - var).abs().max())
                row['halves_max_abs_diff_from_route'] = float((avg2.view(K, 2, C, n, n).transpose(0, 1) - half).abs().max())
                del aligned
            print(json.dumps(row), flush=True)
            rows.append(row)
            del ws, out
            torch.cuda.empty_cache()
        del images
        torch.cuda.empty_cache()
    P = args.frc_planes
    for n in args.frc_sides:
        g = torch.Generator(device=dev).manual_seed(n)
        base = torch.randn(P, n, n, device=dev, generator=g)
        a = base + torch.randn(P, n, n, device=dev, generator=g)
        b = base + torch.randn(P, n, n, device=dev, generator=g)
        R = CL.query('tvae_frc_rings', n)
        wsf = CL.query('tvae_class_frc_ws_floats', P, n)
        ws = torch.empty(wsf, device=dev)
        curve = torch.empty(P, R, device=dev)
        sums = torch.empty(P, R, 3, dtype=torch.float64, device=dev)
        ring = ring_table(n, dev)
        keep = ring < R
        ring_kept = ring[keep]
        out = {}

        def frc():
            CL.call('tvae_class_frc', a, b, curve, sums, ws, wsf, P, n, 0.0, 0.0)

        def fft():
            fa, fb = torch.fft.fft2(a).reshape(P, -1)[:, keep], torch.fft.fft2(b).reshape(P, -1)[:, keep]
            terms = torch.stack([(fa * fb.conj()).real, fa.abs() ** 2, fb.abs() ** 2], -1).double()
            s = torch.zeros(P, R, 3, dtype=torch.float64, device=dev)
            s.index_add_(1, ring_kept, terms)
            out['frc'] = (s[..., 0] / (s[..., 1] * s[..., 2]).sqrt()).float()

        times = timed([('frc', frc), ('fft', fft)], args.reps, args.warmup)
        row = dict(what='frc', P=P, n=n, ws_mb=round(4.0 * wsf / 1e6, 1))
        summary(row, times)
        row['fft_over_frc'] = round(row['fft_ms'] / row['frc_ms'], 2)
        row['frc_max_abs_diff_from_fft'] = float((out['frc'] - curve).abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del ws, a, b, base, out
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'class_stats_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
