#!/usr/bin/env python3
"""Time the per-image CTF filter of a particle stack on one GPU:

  filter     tvae.ctf.filter_stack in coefficient mode (tvae_fourier_filter: one workgroup per plane, H formed in registers,
             n <= 128 without the spectrum or H in HBM) against
  fft        torch.fft.rfft2 * H -> torch.fft.irfft2 on the same GPU, H from tvae_ctf_eval (built once, outside the timing;
             the route materialises the B x n x (n / 2 + 1) complex spectrum, in chunks of --chunk planes)
  wiener     tvae.ctf.class_averages_ctf (filter, aligned class means, power sums, Wiener weights, filter) against
             tvae_class_average alone (tvae.align.class_averages) on the same stack
  bank       tvae.ctf.filter_bank against src.ctf.ctf_filter on the host for --host-rows rows, EXTRAPOLATED linearly to the
             table and labelled as such

HIP events around each GPU route, every shape warmed up first, the routes alternated inside every repetition; medians, least
and largest times.  TFLOP/s counts the matrix products the kernel ISSUES (whole 32 x 32 x 2 blocks, padding included).  One
JSON line per measurement on stdout, all of them in --out:

  python profiles/tools/ctf_bench.py [--shapes 100000x128,20000x64,20000x256] [--bank-shapes 100000x127,100000x63]
        [--wiener-shape 100000x128] [--clusters 10] [--host-rows 200] [--reps 10] [--warmup 2] [--tag NAME] [--out FILE]
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

FFT_CHUNK = 20000


def parse_shape(s):
    B, n = s.split('x')
    return int(B), int(n)


def build_parser():
    ap = argparse.ArgumentParser('Per-image CTF filter of a stack: the direct-DFT kernel against torch.fft')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x128', '20000x64', '20000x256'],
                    help='BxN, comma separated')
    ap.add_argument('--bank-shapes', type=lambda s: s.split(','), default=['100000x127', '100000x63'])
    ap.add_argument('--wiener-shape', default='100000x128')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--host-rows', type=int, default=200)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/ctf_bench_<tag>.json')
    return ap


def issued_flop(B, n):
    """Floating-point operations of the 32 x 32 x 2 blocks ctf_filter_kernel issues (csrc/ctf_kernels.hpp)."""
    R = n // 2 + 1
    T, TK = -(-n // 32), -(-R // 32)
    steps, steps4 = -(-n // 2), -(-R // 2)
    return float(B) * 2 * 32 * 32 * 2 * (T * TK * steps * 2 + T * TK * steps * 4 * 2 + T * T * steps4 * 2)


def table(rng, N):
    t = np.zeros((N, 8))
    t[:, 0] = rng.uniform(1.0, 3.0, N)
    t[:, 1], t[:, 2], t[:, 3], t[:, 5] = 2.7, 300.0, 1.2, 7.0
    t[:, 4] = rng.uniform(50.0, 150.0, N)
    return t


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


def main(args):
    from tvae import align, ctf
    if not torch.cuda.is_available():
        raise SystemExit('ctf_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup,
                timing='HIP events per route, routes alternated inside a repetition, medians; host: wall clock of '
                       '--host-rows rows of src.ctf.ctf_filter, extrapolated linearly')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        B, n = parse_shape(shp)
        need = 2 * 4.0 * B * n * n + 4.0 * B * n * (n // 2 + 1) + 20.0 * min(B, FFT_CHUNK) * n * n + (1 << 30)
        if need > torch.cuda.mem_get_info(0)[0]:
            print(json.dumps(dict(what='filter', B=B, n=n, skipped='not enough free memory')), flush=True)
            continue
        rng = np.random.default_rng(B + n)
        coef = torch.from_numpy(ctf.coefficients(table(rng, B))).to(dev)
        x = torch.randn(B, n, n, device=dev, generator=torch.Generator(device=dev).manual_seed(B + n))
        H = ctf.transfer(coef, n)
        keep = {}

        def filt():
            keep['filter'] = ctf.filter_stack(x, coef=coef)

        def fft():
            out = torch.empty_like(x)
            for b0 in range(0, B, FFT_CHUNK):
                out[b0:b0 + FFT_CHUNK] = torch.fft.irfft2(torch.fft.rfft2(x[b0:b0 + FFT_CHUNK]) * H[b0:b0 + FFT_CHUNK], s=(n, n))
            keep['fft'] = out

        times = timed([('filter', filt), ('fft', fft)], args.reps, args.warmup)
        row = dict(what='filter', B=B, n=n, stack_gb=round(4.0 * B * n * n / 1e9, 3), route='lds' if n <= 128 else 'workspace')
        summary(row, times)
        row['filter_issued_tflops'] = round(issued_flop(B, n) / row['filter_ms'] / 1e9, 2)
        row['issued_mflop_per_plane'] = round(issued_flop(1, n) / 1e6, 2)
        row['fft_over_filter'] = round(row['fft_ms'] / row['filter_ms'], 3)
        row['max_abs_diff_from_fft'] = float((keep['fft'] - keep['filter']).abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        if shp == args.wiener_shape:
            K = args.clusters
            g = torch.Generator(device=dev).manual_seed(K)
            theta = (torch.rand(B, device=dev, generator=g) * 2 - 1) * np.pi
            dx = (torch.rand(B, 2, device=dev, generator=g) - 0.5) * 0.2
            lab = torch.randint(0, K, (B,), device=dev, generator=g)
            x4 = x[:, None]
            times = timed([('wiener', lambda: ctf.class_averages_ctf(x4, theta, dx, lab, coef, K)),
                           ('flip', lambda: ctf.class_averages_ctf(x4, theta, dx, lab, coef, K, correct='flip')),
                           ('plain', lambda: align.class_averages(x4, theta, dx, lab, K))], args.reps, args.warmup)
            row = dict(what='class_averages_ctf', B=B, n=n, K=K)
            summary(row, times)
            row['wiener_over_plain'] = round(row['wiener_ms'] / row['plain_ms'], 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del x, H, keep, coef
        torch.cuda.empty_cache()
    import pandas as pd
    from src import ctf as C
    for shp in args.bank_shapes:
        B, n = parse_shape(shp)
        tab = table(np.random.default_rng(B + n), B)
        frame = pd.DataFrame({c: tab[:args.host_rows, k] for k, c in enumerate(ctf.COLUMNS)})
        C.ctf_filter(frame.iloc[:8], n, n)
        t0 = time.perf_counter()
        host = C.ctf_filter(frame, n, n)
        host_ms_per_row = (time.perf_counter() - t0) * 1e3 / args.host_rows
        keep = {}

        def bank():
            keep['bank'] = ctf.filter_bank(tab, n)

        times = timed([('bank', bank)], args.reps, args.warmup)
        row = dict(what='filter_bank', B=B, n=n)
        summary(row, times)
        row['host_ms_extrapolated'] = round(host_ms_per_row * B, 1)
        row['host_rows_measured'] = args.host_rows
        row['host_extrapolated_over_bank'] = round(host_ms_per_row * B / row['bank_ms'], 1)
        row['max_abs_diff_from_host'] = float(np.abs(keep['bank'][:args.host_rows].cpu().numpy() - host).max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del keep
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'ctf_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
