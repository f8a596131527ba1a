#!/usr/bin/env python3
"""Time the two kernels of the maximum-likelihood class averages on one GPU, each against the same computation in torch ops
on the same GPU, and one full round beside its tvae_pose_classify share:

  posterior   tvae.ml2d.pose_posteriors (tvae_pose_posterior) on the tables of the whole stack against torch: the residuals
              and log weights in fp64, logsumexp, softmax, topk (keep) and gathers for the classes and poses
  average     tvae.ml2d.weighted_class_averages (tvae_class_average_weighted) on the entries of that posterior against
              affine_grid + grid_sample + a weighted index_add_ per class, in slices of the entries that bound its memory
  round       classify_poses(tables=True) -> pose_posteriors -> entries_by_class -> weighted_class_averages, slice by slice
              as tvae.ml2d.ml_rounds runs it, and the classify_poses part of it alone

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route and how far the two routes are apart are reported.  One JSON line per shape on
stdout, all of them in --out:

  python profiles/tools/ml_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--candidates 4] [--angle-steps 8]
                                    [--shift 2] [--keep 8] [--reps 10] [--warmup 2] [--tag NAME]
                                    [--out profiles/ml_bench_NAME.json]
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

ATEN_SLICE = 1 << 16              # entries per grid_sample call of the ATen route


def parse_shape(s):
    N, n = s.split('x')
    return int(N), int(n)


def build_parser():
    ap = argparse.ArgumentParser('Maximum-likelihood class averages: the two kernels against torch ops, and one round')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '20000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--candidates', type=int, default=4)
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shift', type=int, default=2)
    ap.add_argument('--keep', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/ml_bench_<tag>.json')
    return ap


def torch_posterior(num, pp, yy, cand, theta, dx, n, K, sigma2, P, t, A, step, S):
    """The posterior of tvae_pose_posterior in torch ops (no ties rule, no dead candidates: the bench's tables have none)."""
    N, M = cand.shape
    NS = 2 * S + 1
    cnd = (2 * A + 1) * NS * NS
    r = ((yy.double()[:, None] - 2 * num.reshape(N, -1).double()) + pp.reshape(N, -1).double())
    l = -r * (0.5 / float(np.float32(sigma2)))
    lse = torch.logsumexp(l, 1)
    w = torch.exp(l - lse[:, None])
    r2 = (w * r).sum(1)
    resp = w.reshape(N, M, cnd).sum(2).float()
    top, idx = torch.topk(w, P, dim=1)
    W = top.sum(1)
    m, c = idx // cnd, idx % cnd
    a, sy, sx = c // (NS * NS) - A, (c // NS) % NS - S, c % NS - S
    ent_theta = theta[:, None] + a.float() * step
    shift = torch.stack([2 * sx, -2 * sy], 2).float() / (n - 1) / t
    return dict(idx=idx, cls=cand.gather(1, m), theta=ent_theta, dx=dx[:, None, :] + shift, w=(top / W[:, None]).float(), resp=resp,
                lse=lse, r2=r2, kept=W.float())


def aten_average(images, ent, K, t):
    """sum w A / sum w per class by affine_grid + grid_sample + index_add_, in slices of the entries."""
    N, C, n, _ = images.shape
    acc = torch.zeros(K, C, n, n, device=images.device)
    E = ent['img'].numel()
    cls = torch.bucketize(torch.arange(E, device=images.device), ent['seg'][1:].to(torch.int64), right=True)
    for e0 in range(0, E, ATEN_SLICE):
        sl = slice(e0, min(e0 + ATEN_SLICE, E))
        th, d = ent['theta'][sl], ent['dx'][sl]
        c, s = torch.cos(th), torch.sin(th)
        mat = torch.stack([torch.stack([c, -s, t * d[:, 0]], 1), torch.stack([s, c, -t * d[:, 1]], 1)], 1)
        src = images[ent['img'][sl].to(torch.int64)]
        grid = torch.nn.functional.affine_grid(mat, list(src.shape), align_corners=True)
        a = torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        acc.index_add_(0, cls[sl], a * ent['w'][sl][:, None, None, None])
    wsum = torch.zeros(K, dtype=torch.float64, device=images.device).index_add_(0, cls, ent['w'].double())
    return acc / wsum.clamp(min=1e-300)[:, None, None, None].float(), wsum


def main(args):
    from tvae import classify, ml2d
    if not torch.cuda.is_available():
        raise SystemExit('ml_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    A, S, K, M, P, t = args.angle_steps, args.shift, args.clusters, args.candidates, args.keep, 1.0
    step = math.pi / 8 / max(A, 1)
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, K=K, M=M, A=A, S=S,
                P=P, angle_step=step, timing='HIP events per route, routes alternated inside a repetition')
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
        cand = classify.candidate_lists(labels, K, latents, min(M, K))
        num, pp, yy = classify.classify_poses(images, theta, dx, cand, refs, t, A, step, S, tables=True)[5:]
        s2 = float(ml2d.min_residuals(num, pp, yy, cand, K).mean() / (n * n))
        out = {}

        def k_posterior():
            out['post'] = ml2d.pose_posteriors(num, pp, yy, cand, theta, dx, n, K, s2, None, P, t, A, step, S)

        def t_posterior():
            out['tpost'] = torch_posterior(num, pp, yy, cand, theta, dx, n, K, s2, P, t, A, step, S)

        k_posterior()
        ent = ml2d.entries_by_class(out['post']['cls'], out['post']['w'], out['post']['theta'], out['post']['dx'], K)

        def k_average():
            out['avg'] = ml2d.weighted_class_averages(images, ent, K, t)

        def t_average():
            out['tavg'] = aten_average(images, ent, K, t)

        def share():
            out['share'] = classify.classify_poses(images, theta, dx, cand, refs, t, A, step, S, tables=True)[0]

        def full_round():
            post = ml2d.e_step(images, theta, dx, cand, refs, s2, None, P, t, A, step, S, None, 0.0)
            e = ml2d.entries_by_class(post['cls'], post['w'], post['theta'], post['dx'], K)
            out['round'] = ml2d.weighted_class_averages(images, e, K, t)

        routes = [('posterior_kernel', k_posterior), ('posterior_torch', t_posterior), ('average_kernel', k_average),
                  ('average_aten', t_average), ('classify_tables', share), ('round', full_round)]
        times = {nm: [] for nm, _ in routes}
        for rep in range(args.warmup + args.reps):
            for nm, fn in routes:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[nm].append(e0.elapsed_time(e1))
        row = dict(N=N, n=n, C=1, K=K, M=cand.shape[1], A=A, S=S, P=P, E=int(ent['img'].numel()), sigma2=s2)
        for nm, _ in routes:
            row[nm + '_ms'] = round(float(np.median(times[nm])), 3)
            row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
        row['posterior_torch_over_kernel'] = round(row['posterior_torch_ms'] / row['posterior_kernel_ms'], 3)
        row['average_aten_over_kernel'] = round(row['average_aten_ms'] / row['average_kernel_ms'], 3)
        row['classify_share_of_round'] = round(row['classify_tables_ms'] / row['round_ms'], 3)
        row['lse_max_rel_diff'] = float(((out['post']['lse'] - out['tpost']['lse']).abs() / out['tpost']['lse'].abs()).max())
        row['top1_differ'] = int((out['post']['idx'][:, 0].to(torch.int64) != out['tpost']['idx'][:, 0]).sum())
        row['avg_max_abs_diff'] = float((out['avg'][0] - out['tavg'][0]).abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        out.clear()
        del images, num, pp, yy, ent
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'ml_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
