#!/usr/bin/env python3
"""Time the ring power of a particle stack and the per-group radial filter on one GPU:

  power      tvae.spectrum.raw_ring_power (tvae_ring_power: one workgroup per plane, window and mean on the fly, n <= 128
             without the spectrum in HBM) against
    fft        (x - mu) w -> torch.fft.rfft2 -> |.|^2 with the Hermitian weights -> index_add_ over the ring index (fp64), in
               chunks of --chunk planes; the window and the ring index are built once, outside the timing
    frc        tvae.align.frc(a, a): tvae_class_frc in slices of at most 65 535 planes (rings 0 .. n / 2 only, inside mask
               only); its workspace is reported beside it
  filter     tvae.spectrum.radial_filter with --groups groups (tvae_radial_filter: H looked up per coefficient in registers)
             against
    planes     tvae.ctf.filter_stack with the B planes Hp expanded from the same profiles (built outside the timing; the
               extra HBM is reported)
    fft        torch.fft.rfft2 * H[g] -> torch.fft.irfft2 from the G expanded planes, in chunks of --chunk planes

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; medians, least and
largest times.  One JSON line per measurement on stdout, all of them in --out:

  python profiles/tools/spectrum_bench.py [--shapes 100000x64,100000x128,20000x256] [--groups 50] [--reps 10] [--warmup 2]
        [--chunk 20000] [--tag NAME] [--out FILE]
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
    B, n = s.split('x')
    return int(B), int(n)


def build_parser():
    ap = argparse.ArgumentParser('Ring power and radial filter of a stack: the direct-DFT kernels against torch.fft and the FRC')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '100000x128', '20000x256'],
                    help='BxN, comma separated')
    ap.add_argument('--groups', type=int, default=50)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=20000, help='planes per trip of the torch.fft routes')
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/spectrum_bench_<tag>.json')
    return ap


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


def half_planes(prof, n):
    """prof [G][Rr] fp32 -> [G][n][R] fp32: the linear interpolation of tvae_radial_filter, on the host in fp64."""
    R = n // 2 + 1
    k = np.rint(np.fft.fftfreq(n) * n)
    s = np.sqrt(k[:, None] ** 2 + np.arange(R)[None, :] ** 2)
    r0 = np.minimum(np.floor(s).astype(np.int64), prof.shape[1] - 2)
    p = prof.astype(np.float64)
    return (p[:, r0] + (p[:, r0 + 1] - p[:, r0]) * (s - r0)).astype(np.float32)


def main(args):
    from tvae import _cluster_lib as CL, align, ctf, spectrum
    if not torch.cuda.is_available():
        raise SystemExit('spectrum_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, groups=args.groups,
                fft_chunk=args.chunk, timing='HIP events per route, routes alternated inside a repetition, medians')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        B, n = parse_shape(shp)
        R, Rr = n // 2 + 1, spectrum.radial_rings(n)
        need = 3 * 4.0 * B * n * n + 4.0 * B * n * R + 28.0 * min(B, args.chunk) * n * n + (2 << 30)
        if need > torch.cuda.mem_get_info(0)[0]:
            print(json.dumps(dict(what='spectrum', B=B, n=n, skipped='not enough free memory')), flush=True)
            continue
        x = torch.randn(B, n, n, device=dev, generator=torch.Generator(device=dev).manual_seed(B + n)) + 0.5
        radius, edge = spectrum.default_background(n)
        w = torch.from_numpy(spectrum.window(n, radius, edge, True)).to(dev, torch.float32)
        wsum = w.sum(dtype=torch.float64)
        ring = torch.from_numpy(spectrum.ring_table(n)[:, :R].reshape(-1)).to(dev)
        herm = torch.full((R,), 2.0, dtype=torch.float64, device=dev)
        herm[0] = 1.0
        if n % 2 == 0:
            herm[-1] = 1.0
        keep = {}

        def power():
            keep['power'] = spectrum.raw_ring_power(x, radius, edge, True, True)

        def fft_power():
            out = torch.zeros(B, Rr, dtype=torch.float64, device=dev)
            for b0 in range(0, B, args.chunk):
                xs = x[b0:b0 + args.chunk]
                mu = ((xs * w).sum((1, 2), dtype=torch.float64) / wsum).to(torch.float32)
                F = torch.fft.rfft2((xs - mu[:, None, None]) * w)
                p = (F.real.double() ** 2 + F.imag.double() ** 2) * herm
                out[b0:b0 + args.chunk].index_add_(1, ring, p.reshape(p.shape[0], -1))
            keep['fft'] = out

        def frc_power():
            keep['frc'] = align.frc(x, x, radius, edge)[1]

        times = timed([('power', power), ('fft', fft_power), ('frc', frc_power)], args.reps, args.warmup)
        row = dict(what='ring_power', B=B, n=n, rings=Rr, stack_gb=round(4.0 * B * n * n / 1e9, 3),
                   route='lds' if n <= 128 else 'workspace')
        summary(row, times)
        row['fft_over_power'] = round(row['fft_ms'] / row['power_ms'], 3)
        row['frc_over_power'] = round(row['frc_ms'] / row['power_ms'], 3)
        row['power_ws_bytes'] = 4 * CL.query('tvae_ring_power_ws_floats', CL.slice_step(B, CL.MAX_PLANES, spectrum.WS_FLOATS // max(
            CL.query('tvae_ring_power_ws_floats', 1, n), 1)), n)
        per = CL.query('tvae_class_frc_ws_floats', 1, n)
        row['frc_ws_bytes_as_run'] = 4 * per * CL.slice_step(B, 65535, align.FRC_WS_FLOATS // per)
        row['frc_ws_bytes_one_slice_of_65535'] = 4 * per * min(B, 65535)
        row['frc_note'] = 'the background window is not available to tvae_class_frc: it ran with the inside mask of the same disc'
        scale = keep['power'].abs().max()
        row['max_rel_diff_from_fft'] = float((keep['power'] - keep['fft']).abs().max() / scale)
        print(json.dumps(row), flush=True)
        rows.append(row)
        keep.clear()
        torch.cuda.empty_cache()

        G = args.groups
        rng = np.random.default_rng(B + n)
        prof = (0.25 + rng.random((G, Rr))).astype(np.float32)
        groups = torch.from_numpy(rng.integers(0, G, B)).to(dev)
        Hg = torch.from_numpy(half_planes(prof, n)).to(dev)
        Hp = Hg[groups].contiguous()

        def radial():
            keep['radial'] = spectrum.radial_filter(x, prof, groups)

        def planes():
            keep['planes'] = ctf.filter_stack(x, planes=Hp)

        def fft_filter():
            out = torch.empty_like(x)
            for b0 in range(0, B, args.chunk):
                out[b0:b0 + args.chunk] = torch.fft.irfft2(torch.fft.rfft2(x[b0:b0 + args.chunk]) * Hg[groups[b0:b0 + args.chunk]],
                                                           s=(n, n))
            keep['fft'] = out

        times = timed([('radial', radial), ('planes', planes), ('fft', fft_filter)], args.reps, args.warmup)
        row = dict(what='radial_filter', B=B, n=n, G=G, stack_gb=round(4.0 * B * n * n / 1e9, 3),
                   route='lds' if n <= 128 else 'workspace')
        summary(row, times)
        row['planes_over_radial'] = round(row['planes_ms'] / row['radial_ms'], 3)
        row['fft_over_radial'] = round(row['fft_ms'] / row['radial_ms'], 3)
        row['planes_extra_hbm_bytes'] = 4 * B * n * R
        row['max_abs_diff_from_planes'] = float((keep['radial'] - keep['planes']).abs().max())
        row['max_abs_diff_from_fft'] = float((keep['radial'] - keep['fft']).abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, Hp, Hg, keep
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'spectrum_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
