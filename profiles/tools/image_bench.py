#!/usr/bin/env python3
"""Time the Fourier downsample of a particle stack on one GPU, three routes over the same stack:

  resample   tvae_image_resample (tvae.image.resample_window without its allocation): one launch, the batched sandwich
             product with the shape's four tables, nothing intermediate in HBM
  fft        torch.fft.rfft2 -> the reference's slice / concatenate -> torch.fft.irfft2 on the same GPU (it materialises the
             B x M x (N / 2 + 1) complex spectrum)
  numpy      the same three steps with numpy on the host for --host-images images, EXTRAPOLATED linearly to the stack and
             labelled as such

and tvae_image_normalize on the downsampled stack.  HIP events around each GPU route, every shape warmed up first, the
routes alternated inside every repetition; medians, least and largest times.  A stack larger than --chunk images goes
through both GPU routes in chunks of that size (the intermediate spectrum of the fft route bounds it).  GB/s is the stack
read once over the resample time; TFLOP/s counts the matrix products the kernel ISSUES (whole 32 x 32 x 2 blocks, padding
included), not the useful ones.  One JSON line per measurement on stdout, all of them in --out:

  python profiles/tools/image_bench.py [--shapes 256-64,256-128,128-64] [--images 20000,100000] [--chunk 20000]
        [--host-images 200] [--reps 10] [--warmup 2] [--tag NAME] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch


def parse_shape(s):
    M, m = s.split('-')
    return int(M), int(m)


def build_parser():
    ap = argparse.ArgumentParser('Fourier downsample of a stack: the fused kernel against torch.fft and numpy')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['256-64', '256-128', '128-64'], help='M-m, comma separated')
    ap.add_argument('--images', type=lambda s: [int(v) for v in s.split(',')], default=[20000, 100000])
    ap.add_argument('--chunk', type=int, default=20000)
    ap.add_argument('--host-images', type=int, default=200)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/image_bench_<tag>.json')
    return ap


def issued_flop(B, M, N, m, n, imag):
    """Floating-point operations of the 32 x 32 x 2 blocks image_resample_kernel issues (csrc/image_kernels.hpp)."""
    nj = 2 if n > 64 else 1
    tiles = -(-m // 64) * -(-n // (64 * nj))
    block = 2 * 32 * 32 * 2
    per_tile = 0
    for cc in range(0, N, 64):
        ck = min(64, N - cc)
        per_tile += -(-M // 16) * 8 * (2 if imag else 1) * 4                    # stage 1: four 32 x 32 tiles of U (and V)
        per_tile += -(-ck // 16) * 8 * nj * (2 if imag else 1) * 4              # stage 2
    return float(B) * tiles * per_tile * block


def timed(routes, reps, warmup):
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


def fft_route(x, m, n):
    M, N = x.shape[-2:]
    F = torch.fft.rfft2(x)
    F = torch.cat([F[..., 0:m // 2, 0:n // 2 + 1], F[..., M - (m - m // 2):, 0:n // 2 + 1]], dim=-2)
    F *= (m * n) / (M * N)
    return torch.fft.irfft2(F, s=(m, n))


def numpy_route(x, m, n):
    M, N = x.shape[-2:]
    F = np.fft.rfft2(x)
    F = np.concatenate([F[..., 0:m // 2, 0:n // 2 + 1], F[..., M - (m - m // 2):, 0:n // 2 + 1]], axis=-2)
    F *= (m * n) / (M * N)
    return np.fft.irfft2(F, s=(m, n)).astype(x.dtype)


def main(args):
    from tvae import _cluster_lib as CL
    from tvae import image
    if not torch.cuda.is_available():
        raise SystemExit('image_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, chunk=args.chunk,
                timing='HIP events per route, routes alternated inside a repetition, medians; numpy: wall clock of '
                       '--host-images images on the host, extrapolated linearly')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        M, m = parse_shape(shp)
        N, n = M, m
        Ar, Ai, Br, Bi = image.device_tables(M, N, m, n, dev)
        scale = 1.0 / (M * N)
        host = np.random.default_rng(M + m).standard_normal((args.host_images, M, N)).astype(np.float32)
        numpy_route(host[:8], m, n)
        t0 = time.perf_counter()
        host_out = numpy_route(host, m, n)
        host_ms_per_image = (time.perf_counter() - t0) * 1e3 / args.host_images
        for B in args.images:
            need = 4.0 * B * M * N + 4.0 * B * m * n + 12.0 * min(B, args.chunk) * M * (N // 2 + 1) + (1 << 30)
            if need > torch.cuda.mem_get_info(0)[0]:
                print(json.dumps(dict(what='downsample', B=B, M=M, m=m, skipped='not enough free memory')), flush=True)
                continue
            g = torch.Generator(device=dev).manual_seed(B + M)
            x = torch.randn(B, M, N, device=dev, generator=g)
            x[:args.host_images] = torch.from_numpy(host).to(dev)
            out = torch.empty(B, m, n, device=dev)
            keep = {}
            spans = [(b0, min(b0 + args.chunk, B)) for b0 in range(0, B, args.chunk)]

            def resample():
                for b0, b1 in spans:
                    CL.call('tvae_image_resample', x[b0:b1], Ar, Ai, Br, Bi, out[b0:b1], b1 - b0, M, N, 0, 0, M, N, m, n, scale)

            def fft():
                for b0, b1 in spans:
                    keep['fft'] = fft_route(x[b0:b1], m, n)

            wsf = CL.query('tvae_image_normalize_ws_floats', B, m, n)
            ws = torch.empty(wsf // 2, dtype=torch.float64, device=dev).view(torch.float32)
            normed, stats = torch.empty_like(out), torch.empty(B, 2, dtype=torch.float64, device=dev)

            def normalize():
                CL.call('tvae_image_normalize', out, normed, stats, ws, wsf, B, m, n, 0.0)

            times = timed([('resample', resample), ('fft', fft), ('normalize', normalize)], args.reps, args.warmup)
            row = dict(what='downsample', B=B, M=M, N=N, m=m, n=n, stack_gb=round(4.0 * B * M * N / 1e9, 3),
                       second_term=Ai is not None)
            summary(row, times)
            flop = issued_flop(B, M, N, m, n, Ai is not None)
            row['resample_gbs'] = round(4.0 * B * M * N / row['resample_ms'] / 1e6, 1)
            row['resample_issued_tflops'] = round(flop / row['resample_ms'] / 1e9, 2)
            row['issued_mflop_per_image'] = round(flop / B / 1e6, 2)
            row['fft_over_resample'] = round(row['fft_ms'] / row['resample_ms'], 3)
            row['numpy_ms_extrapolated'] = round(host_ms_per_image * B, 1)
            row['numpy_images_measured'] = args.host_images
            row['numpy_extrapolated_over_resample'] = round(host_ms_per_image * B / row['resample_ms'], 1)
            last = spans[-1]
            row['max_abs_diff_from_fft'] = float((keep['fft'] - out[last[0]:last[1]]).abs().max())
            row['max_abs_diff_from_numpy'] = float(np.abs(out[:args.host_images].cpu().numpy() - host_out).max())
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x, out, normed, ws, keep
            torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'image_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
