#!/usr/bin/env python3
"""Time the CTF-aware hard search on one GPU at the project's standard stacks:

  select0   tvae_pose_select with the template power per angle (pp_per_shift = 0) on whole-stack tables, against the torch
            route that stands for what a user would write without it: expand ppc over the NS^2 shifts, score in fp64, argmax
            over (slot, angle, shift), gather the label and the pose.  (The torch route has no centre priority: the number of
            images on which its choice differs is reported, not asserted.)  select0 and select1 call the entry point directly
            into preallocated outputs; select0_wrapper is tvae.ctf.select_poses, with its checks, conversions and allocations.
  select1   tvae_pose_select with the power per candidate (pp_per_shift = 1) on whole-stack tables.  What it stands beside is
            classify_select_kernel's share of a tvae_pose_classify call, which no event pair can isolate: --trace runs
            classify_poses(tables=True) on 16 384 images and tvae_pose_select on those same tables, three times per shape; run
            that under a kernel-stats profile of its own (no counter collection in the same run) and give the CSV to
            --kernel-stats: the averages of both kernels go into the JSON.
  rounds    one round of classify_rounds and of refine_rounds with ctf=coef beside the plain round of the same call, and inside
            the CTF round of classify_poses the shares of its three parts (tables, template_power, select).

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; medians of --reps
with the least and the largest time.  One JSON line per measurement on stdout, all of them in --out:

  python profiles/tools/ctf_search_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--candidates 4] [--angle-steps 8]
                                            [--shift 2] [--reps 10] [--warmup 2] [--kernel-stats CSV] [--trace]
                                            [--tag NAME] [--out profiles/ctf_search_bench_NAME.json]
"""
import argparse
import csv
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch

TRACE_IMAGES = 16384              # images of a --trace call: one slice of the E-step's size


def build_parser():
    ap = argparse.ArgumentParser('CTF-aware hard search: tvae_pose_select alone, against torch ops, and in a round')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '20000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--candidates', type=int, default=4)
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shift', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-rounds', action='store_true', help='leave the rounds away')
    ap.add_argument('--trace', action='store_true', help='only run classify_poses(tables) and both selections three times per '
                                                         'shape: the workload of a kernel-stats profile')
    ap.add_argument('--kernel-stats', default=None, help='kernel_stats.csv of such a profile: its averages go into the JSON')
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/ctf_search_bench_<tag>.json')
    return ap


def timed(routes, reps, warmup):
    """routes: [(name, fn)] -> {name: [ms]}, the routes alternated inside every repetition."""
    times = {nm: [] for nm, _ in routes}
    for rep in range(warmup + reps):
        for nm, fn in routes:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                times[nm].append(e0.elapsed_time(e1))
    return times


def summary(row, times):
    for nm, v in times.items():
        row[nm + '_ms'] = round(float(np.median(v)), 3)
        row[nm + '_ms_min_max'] = [round(min(v), 3), round(max(v), 3)]
    return row


def torch_select(num, ppc, yy, cand, theta, dx, n, K, A, S, t, step):
    """The selection in torch ops: -> (labels, theta', dx', flat index of the winner)."""
    N, M, NA, NS, _ = num.shape
    pp = ppc[:, :, :, None, None].expand(-1, -1, -1, NS, NS).double()
    y = yy.double()[:, None, None, None, None]
    zero = (pp == 0) | (y == 0)
    s = torch.where(zero, torch.zeros_like(pp), num.double() / torch.sqrt(torch.where(zero, torch.ones_like(pp), pp * y))).float()
    live = ((cand >= 0) & (cand < K))[:, :, None, None, None] & torch.isfinite(s)
    win = torch.where(live, s, torch.full_like(s, -math.inf)).reshape(N, -1).argmax(1)
    cnd = NA * NS * NS
    m, e = win // cnd, win % cnd
    a, sy, sx = e // (NS * NS) - A, (e // NS) % NS - S, e % NS - S
    th = theta + a.float() * step
    d = dx + torch.stack([2 * sx, -2 * sy], 1).float() / (n - 1) / t
    return cand.gather(1, m[:, None])[:, 0], th, d, win


def read_stats(path):
    """kernel name -> (calls, average ns) for the two selection kernels of a kernel-stats CSV."""
    out = {}
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            name = r.get('Name') or r.get('KernelName') or ''
            for key in ('classify_select_kernel', 'pose_select_kernel', 'classify_corr_kernel'):
                if key in name:
                    calls = int(float(r.get('Calls') or 0))
                    total = float(r.get('TotalDurationNs') or 0)
                    had = out.get(key, dict(calls=0, total_ns=0.0))
                    out[key] = dict(calls=had['calls'] + calls, total_ns=had['total_ns'] + total)
    for v in out.values():
        v['average_us'] = round(v['total_ns'] / max(v['calls'], 1) / 1e3, 2)
    return out


def main(args):
    from tvae import _cluster_lib as CL
    from tvae import classify, ctf, ml2d, refine
    if not torch.cuda.is_available():
        raise SystemExit('ctf_search_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    A, S, K, M, t = args.angle_steps, args.shift, args.clusters, args.candidates, 1.0
    NA, NS = 2 * A + 1, 2 * S + 1
    step = math.pi / 8 / max(A, 1)
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, K=K, M=M, A=A, S=S,
                angle_step=step, timing='HIP events per route, routes alternated inside a repetition, medians; select0 and select1 are the entry point '
                       'called directly into preallocated outputs, select0_wrapper is tvae.ctf.select_poses with its checks, the '
                       'int64 -> int32 conversion of the candidates and its allocations')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        N, n = (int(v) for v in shp.split('x'))
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.rand(N, 1, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        labels = torch.randint(0, K, (N,), device=dev, generator=g)
        latents = torch.rand(N, 2, device=dev, generator=g)
        defocus = 1.0 + 1.5 * torch.rand(N, generator=torch.Generator().manual_seed(N)).numpy().astype(np.float64)
        table = np.stack([defocus, np.full(N, 2.7), np.full(N, 300.0), np.full(N, 2.0), np.full(N, 100.0), np.full(N, 7.0), np.zeros(N),
                          np.zeros(N)], 1)
        coef = torch.from_numpy(ctf.coefficients(table)).to(dev)
        cand = classify.candidate_lists(labels, K, latents, min(M, K))
        refs = ctf.class_averages_ctf(images, theta, dx, labels, coef, K, t)[0]
        if args.trace:                                        # both kernels select from the same tables of TRACE_IMAGES images
            Nt = min(N, TRACE_IMAGES)
            for _ in range(3):
                r = classify.classify_poses(images[:Nt], theta[:Nt], dx[:Nt], cand[:Nt], refs, t, A, step, S, tables=True)
                k = ctf.select_poses(r[5], r[6], r[7], cand[:Nt], theta[:Nt], dx[:Nt], n, K, t, A, step, S)
                assert all(torch.equal(x, y) for x, y in zip(r[:5], k))
            torch.cuda.synchronize()
            print(json.dumps(dict(traced=shp, images=Nt)), flush=True)
            continue
        # ---- whole-stack tables: random words with the statistics of real ones are enough for a kernel that only reads them
        num = torch.randn(N, M, NA, NS, NS, device=dev, generator=g)
        ppc = torch.rand(N, M, NA, device=dev, generator=g) + 0.5
        pp = torch.rand(N, M, NA, NS, NS, device=dev, generator=g) + 0.5
        yy = torch.rand(N, device=dev, generator=g) + 0.5
        cand32 = cand.to(torch.int32).contiguous()
        outs = (torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, 4, dtype=torch.int32, device=dev),
                torch.empty(N, device=dev), torch.empty(N, 2, device=dev), torch.empty(N, cand.shape[1], 2, device=dev))

        def kernel(power):                                    # the entry point itself: no checks, no conversions, outputs in place
            CL.call('tvae_pose_select', theta, dx, cand32, num, power, yy, *outs, N, n, K, cand.shape[1], A, S, int(power.dim() == 5),
                    t, step)

        out = {}
        routes = [('select0', lambda: kernel(ppc)), ('select1', lambda: kernel(pp)),
                  ('select0_wrapper', lambda: out.__setitem__('k0', ctf.select_poses(num, ppc, yy, cand, theta, dx, n, K, t, A, step, S))),
                  ('torch', lambda: out.__setitem__('t', torch_select(num, ppc, yy, cand, theta, dx, n, K, A, S, t, step)))]
        row = summary(dict(what='select', N=N, n=n, M=M, A=A, S=S, table_bytes=num.numel() * 4), timed(routes, args.reps, args.warmup))
        row['torch_over_select0'] = round(row['torch_ms'] / row['select0_ms'], 2)
        row['select0_GBps'] = round((num.numel() + ppc.numel()) * 4 / row['select0_ms'] / 1e6, 1)
        row['select1_GBps'] = round(2 * num.numel() * 4 / row['select1_ms'] / 1e6, 1)
        row['torch_labels_differ'] = int((out['k0'][0] != out['t'][0]).sum())
        best = out['k0'][4].to(torch.int64)
        flat = (best[:, 0] * NA + best[:, 1] + A) * NS * NS + (best[:, 2] + S) * NS + best[:, 3] + S
        row['torch_winners_differ'] = int((flat != out['t'][3]).sum())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del num, pp, ppc
        out.clear()
        torch.cuda.empty_cache()
        if args.no_rounds:
            continue
        # ---- the parts of classify_poses(ctf=...) over the whole stack, slice by slice as it runs them
        scored = ctf.filter_stack(images, coef=coef, mode='multiply')
        yy_raw = ml2d.raw_sum_squares(images)
        stepN = ml2d._slices(N, cand.shape[1], A, S)
        slices = [slice(i0, min(i0 + stepN, N)) for i0 in range(0, N, stepN)]
        keep = {}

        def tables():
            keep['num'] = [classify.classify_poses(scored[sl], theta[sl], dx[sl], cand[sl], refs, t, A, step, S, tables=True)[5] for sl in slices]

        def power():
            keep['ppc'] = [ctf.template_power(theta[sl], dx[sl], cand[sl], refs, coef[sl], t, A, step) for sl in slices]

        def select():
            for sl, a, b in zip(slices, keep['num'], keep['ppc']):
                ctf.select_poses(a, b, yy_raw[sl], cand[sl], theta[sl], dx[sl], n, K, t, A, step, S)

        row = summary(dict(what='parts of classify_poses(ctf)', N=N, n=n, M=cand.shape[1], slices=len(slices)),
                      timed([('tables', tables), ('template_power', power), ('select', select)], max(args.reps // 2, 3), 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        keep.clear()
        del scored
        torch.cuda.empty_cache()
        # ---- one round of each tool, with and without the CTF
        routes = [('classify_plain', lambda: classify.classify_rounds(images, theta, dx, labels, K, t, 1, math.pi / 8, A, S, latents=latents,
                                                                      candidates=M)),
                  ('classify_ctf', lambda: classify.classify_rounds(images, theta, dx, labels, K, t, 1, math.pi / 8, A, S, latents=latents,
                                                                    candidates=M, ctf=coef)),
                  ('refine_plain', lambda: refine.refine_rounds(images, theta, dx, labels, K, t, 1, math.pi / 8, A, S)),
                  ('refine_ctf', lambda: refine.refine_rounds(images, theta, dx, labels, K, t, 1, math.pi / 8, A, S, ctf=coef))]
        row = summary(dict(what='one round', N=N, n=n, M=M), timed(routes, max(args.reps // 2, 3), 1))
        row['classify_ctf_over_plain'] = round(row['classify_ctf_ms'] / row['classify_plain_ms'], 2)
        row['refine_ctf_over_plain'] = round(row['refine_ctf_ms'] / row['refine_plain_ms'], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del images
        torch.cuda.empty_cache()
    if args.trace:
        return
    doc = dict(head, results=rows)
    if args.kernel_stats:
        doc['kernel_stats'] = dict(source='kernel-stats profile of `ctf_search_bench.py --trace`, a run of its own',
                                   note=f'every kernel on the same tables of {TRACE_IMAGES} images per call (pp per candidate), '
                                        'three calls per shape', kernels=read_stats(args.kernel_stats))
    path = args.out or os.path.join(HERE, '..', 'ctf_search_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
