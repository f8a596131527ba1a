#!/usr/bin/env python3
"""Time the CTF in the template of the maximum-likelihood class averages on one GPU:

  template_power   tvae.ctf.template_power (tvae_template_ctf_power) on the whole stack: N M NA templates, each built, transformed
                   and summed by one workgroup
  classify_tables  the tvae_pose_classify pass of the same stack (classify_poses(tables=True)), what a plain E-step costs
  round_ctf        one whole round of ml_rounds(ctf=coef) as it runs it: e_step on the filtered stack with the three substituted
                   tables, entries_by_class, weighted_class_averages, power_weighted and the Wiener filter of the means
  round_plain      one whole plain round of the same stack on the same commit
  torch route      template_power against torch on the same GPU: affine_grid + grid_sample templates -> rfft2 -> the H^2-weighted
                   sum, in slices that bound its memory.  Both are timed on the first --torch-images images of the stack (the
                   torch route holds every template and its spectrum in memory and would take minutes on the whole stack).

HIP events around each route, every shape warmed up first, the routes alternated inside every repetition; the median, the
least and the largest time of each route are reported.  One JSON line per shape on stdout, all of them in --out:

  python profiles/tools/ctf_pose_bench.py [--shapes 100000x64,20000x128] [--clusters 10] [--candidates 4] [--angle-steps 8]
                                          [--shift 2] [--keep 8] [--reps 10] [--warmup 2] [--torch-images 2000] [--tag NAME]
                                          [--out profiles/ctf_pose_bench_NAME.json]
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

TORCH_SLICE = 1 << 13             # templates per grid_sample / rfft2 call of the torch route


def parse_shape(s):
    N, n = s.split('x')
    return int(N), int(n)


def build_parser():
    ap = argparse.ArgumentParser('CTF in the template: tvae_template_ctf_power alone, in a round, and against torch ops')
    ap.add_argument('--shapes', type=lambda s: s.split(','), default=['100000x64', '20000x128'], help='N x n, comma separated')
    ap.add_argument('--clusters', type=int, default=10)
    ap.add_argument('--candidates', type=int, default=4)
    ap.add_argument('--angle-steps', type=int, default=8)
    ap.add_argument('--shift', type=int, default=2)
    ap.add_argument('--keep', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--torch-images', type=int, default=2000)
    ap.add_argument('--tag', default='mi355x')
    ap.add_argument('--out', default=None, help='default: profiles/ctf_pose_bench_<tag>.json')
    return ap


def defocus_rows(N, n):
    """[N][5] fp64: a weak-phase CTF whose first zero runs from a quarter to half of the Nyquist radius over eight defoci."""
    w = 0.07
    q0 = np.linspace(0.25, 0.5, 8) ** 2 / 4.0
    out = np.zeros((N, 5))
    out[:, 0], out[:, 1], out[:, 4] = -math.sqrt(1 - w * w), -w, 2.0
    out[:, 2] = (-0.5 / q0)[np.arange(N) % 8]
    return out


def torch_template_power(theta, dx, cand, refs, H2w, t, A, step):
    """sum_k w_kx H^2 |rfft2(T)|^2 / n^2 with T by affine_grid + grid_sample (no mask), in slices of the templates."""
    N, M = cand.shape
    K, C, n, _ = refs.shape
    NA = 2 * A + 1
    a = torch.arange(-A, A + 1, device=refs.device, dtype=torch.float32) * step
    th = (theta[:, None, None] + a[None, None, :]).expand(N, M, NA).reshape(-1)
    d = dx[:, None, None, :].expand(N, M, NA, 2).reshape(-1, 2)
    k = cand[:, :, None].expand(N, M, NA).reshape(-1).to(torch.int64)
    img = torch.arange(N, device=refs.device)[:, None, None].expand(N, M, NA).reshape(-1)
    out = torch.empty(N * M * NA, device=refs.device)
    for e0 in range(0, th.numel(), TORCH_SLICE):
        sl = slice(e0, min(e0 + TORCH_SLICE, th.numel()))
        c, s = torch.cos(th[sl]), torch.sin(th[sl])
        # the template reads the reference at u = R(theta) (x - t dx), x1 pointing up; affine_grid's y points down
        tx, ty = t * d[sl, 0], t * d[sl, 1]
        mat = torch.stack([torch.stack([c, s, s * ty - c * tx], 1), torch.stack([-s, c, s * tx + c * ty], 1)], 1)
        src = refs[k[sl]]
        grid = torch.nn.functional.affine_grid(mat, list(src.shape), align_corners=True)
        T = torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        F = torch.fft.rfft2(T)
        out[sl] = ((F.real ** 2 + F.imag ** 2) * H2w[img[sl]][:, None]).sum((1, 2, 3)) / (n * n)
    return out.reshape(N, M, NA)


def main(args):
    from tvae import classify, ctf, ml2d
    if not torch.cuda.is_available():
        raise SystemExit('ctf_pose_bench.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    A, S, K, M, P, t, tau = args.angle_steps, args.shift, args.clusters, args.candidates, args.keep, 1.0, 0.1
    step = math.pi / 8 / max(A, 1)
    head = dict(gpu=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, warmup=args.warmup, K=K, M=M, A=A, S=S,
                P=P, angle_step=step, timing='HIP events per route, routes alternated inside a repetition')
    print(json.dumps(head), flush=True)
    rows = []
    for shp in args.shapes:
        N, n = parse_shape(shp)
        Nt = min(N, args.torch_images)
        g = torch.Generator(device=dev).manual_seed(N + n)
        images = torch.rand(N, 1, n, n, device=dev, generator=g)
        refs = torch.rand(K, 1, n, n, device=dev, generator=g)
        theta = (torch.rand(N, device=dev, generator=g) * 2 - 1) * np.pi
        dx = (torch.rand(N, 2, device=dev, generator=g) * 2 - 1) * 0.25
        labels = torch.randint(0, K, (N,), device=dev, generator=g)
        latents = torch.rand(N, 2, device=dev, generator=g)
        cand = classify.candidate_lists(labels, K, latents, min(M, K))
        coef = torch.from_numpy(defocus_rows(N, n)).to(dev)
        filtered = ctf.filter_stack(images, coef=coef, mode='multiply')
        yy_raw = ml2d.raw_sum_squares(images)
        H = ctf.transfer(coef[:8], n)
        wk = torch.full((n // 2 + 1,), 2.0, device=dev)
        wk[0] = 1.0
        if n % 2 == 0:
            wk[-1] = 1.0
        H2w = (H * H * wk)[torch.arange(Nt, device=dev) % 8]
        num, pp, yy = classify.classify_poses(images, theta, dx, cand, refs, t, A, step, S, tables=True)[5:]
        s2 = float(ml2d.min_residuals(num, pp, yy, cand, K).mean() / (n * n))
        del num, pp, yy
        out = {}

        def k_power():
            out['ppc'] = ctf.template_power(theta, dx, cand, refs, coef, t, A, step)

        def k_power_subset():
            out['ppc_sub'] = ctf.template_power(theta[:Nt], dx[:Nt], cand[:Nt], refs, coef[:Nt], t, A, step)

        def t_power_subset():
            out['tppc_sub'] = torch_template_power(theta[:Nt], dx[:Nt], cand[:Nt], refs, H2w, t, A, step)

        def share():
            out['share'] = classify.classify_poses(images, theta, dx, cand, refs, t, A, step, S, tables=True)[0]

        def round_plain():
            post = ml2d.e_step(images, theta, dx, cand, refs, s2, None, P, t, A, step, S, None, 0.0)
            e = ml2d.entries_by_class(post['cls'], post['w'], post['theta'], post['dx'], K)
            out['round'] = ml2d.weighted_class_averages(images, e, K, t)

        def round_ctf():
            post = ml2d.e_step(filtered, theta, dx, cand, refs, s2, None, P, t, A, step, S, None, 0.0, (coef, yy_raw))
            e = ml2d.entries_by_class(post['cls'], post['w'], post['theta'], post['dx'], K)
            mean, _, _ = ml2d.weighted_class_averages(filtered, e, K, t)
            D, W, _ = ctf.power_weighted(coef, e, n, K)
            G = (1.0 / (D / W.clamp(min=1e-300)[:, None, None] + tau)).to(torch.float32).contiguous()
            out['round_ctf'] = ctf.filter_stack(mean, planes=G)

        routes = [('template_power', k_power), ('classify_tables', share), ('round_ctf', round_ctf), ('round_plain', round_plain),
                  ('template_power_subset', k_power_subset), ('torch_subset', t_power_subset)]
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
        row = dict(N=N, n=n, C=1, K=K, M=cand.shape[1], A=A, S=S, P=P, templates=N * cand.shape[1] * (2 * A + 1), torch_images=Nt,
                   sigma2=s2)
        for nm, _ in routes:
            row[nm + '_ms'] = round(float(np.median(times[nm])), 3)
            row[nm + '_ms_min_max'] = [round(min(times[nm]), 3), round(max(times[nm]), 3)]
        row['template_power_over_classify'] = round(row['template_power_ms'] / row['classify_tables_ms'], 3)
        row['round_ctf_over_plain'] = round(row['round_ctf_ms'] / row['round_plain_ms'], 3)
        row['template_power_share_of_round_ctf'] = round(row['template_power_ms'] / row['round_ctf_ms'], 3)
        row['torch_over_kernel_subset'] = round(row['torch_subset_ms'] / row['template_power_subset_ms'], 3)
        row['torch_max_rel_diff'] = float(((out['ppc_sub'] - out['tppc_sub']).abs() / out['ppc_sub'].abs().clamp(min=1e-30)).max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        out.clear()
        del images, filtered
        torch.cuda.empty_cache()
    path = args.out or os.path.join(HERE, '..', 'ctf_pose_bench_{}.json'.format(args.tag))
    with open(path, 'w') as f:
        json.dump(dict(head, results=rows), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main(build_parser().parse_args())
