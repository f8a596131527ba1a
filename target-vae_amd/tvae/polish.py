"""Sub-pixel pose polish against the class averages on the GPU: the continuous step after tvae.refine.  The grid searches
(refine_poses, classify, ml2d) find shifts on a whole-pixel grid, so every image keeps a translation error of up to half a
pixel per axis; the polish removes it by a few Levenberg-Marquardt steps on the cosine score between the image and the
average of its class rendered at the image's pose, inside a trust region around the pose it starts from.
include/tvae_cluster.h states the definition in full.

The kernels are tvae_pose_moments (one template per image with its derivatives, reduced to 15 sums) and
tvae_pose_polish_step (a thread per image, fp64) of libtvae_cluster.so: no CPU fallback, no float atomics, bitwise
reproducible, and the result of an image depends on that image, its pose and its class's reference alone.  The loop is
launches only -- nothing is read back between the iterations.  n > 128 is out of scope, as in tvae.refine: Fourier-downsample
the stack with tvae.image first -- poses are in coordinate units and carry over unchanged.

`polish_rounds` alternates averaging and polishing.  With cross_halves=True every image is scored against the half-set
average it is NOT a member of (tvae.refine.cross_half_labels).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import align, refine
from ._lib import TvaeHipError

MOMENTS = 15
SLICE = 1 << 20                   # images per call: bounds nothing but the launch grid


def polish_poses(images, theta, dx, labels, refs, t_scale=1.0, iterations=8, max_shift=1.0, max_angle=0.05, mask_radius=None,
                 mask_edge=0.0):
    """images [N][C][n][n], theta [N] or [N][1], dx [N][2], refs [K][C][n][n] (CUDA fp32), labels [N] integers (any device or
    numpy; a label outside [0, K) leaves its image alone) -> (theta' [N], dx' [N][2], scores [N][2] = (start, final),
    steps int32 [N], the accepted steps).  `iterations` trial poses are evaluated after the start pose; no pose leaves the
    trust region of max_shift pixels per axis and max_angle radians around its start."""
    what = 'polish_poses'
    N, C, n, _, lab = align._check_labels(images, theta, dx, labels, 1, what)
    K = refine._check_refs(images, refs, what)
    if n > refine.MAX_SIDE:
        raise TvaeHipError(f'{what}: n = {n} is above {refine.MAX_SIDE}: '
                           'Fourier-downsample the stack with tvae.image first; poses are in coordinate units and carry '
                           'over unchanged')
    if not C <= refine.MAX_CHANNELS:
        raise TvaeHipError(f'{what}: C={C} outside the supported range (C <= {refine.MAX_CHANNELS})')
    t, its = float(t_scale), int(iterations)
    shift, angle = float(max_shift), float(max_angle)
    radius = 0.0 if mask_radius is None else float(mask_radius)
    edge = float(mask_edge)
    if not (np.isfinite(t) and t > 0):
        raise TvaeHipError(f'{what}: t_scale = {t_scale} must be finite and positive')
    if not (its >= 0 and np.isfinite(shift) and shift >= 0 and np.isfinite(angle) and angle >= 0):
        raise TvaeHipError(f'{what}: iterations = {iterations}, max_shift = {max_shift} and max_angle = {max_angle} must be '
                           'finite and not negative')
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'{what}: mask_radius = {mask_radius} and mask_edge = {mask_edge} must be finite, the edge not negative')
    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise TvaeHipError(f'{what}: labels must be a one-dimensional integer array')
    lim = torch.iinfo(torch.int32)
    cls = lab.to(torch.int64).clamp(-1, lim.max).to(torch.int32).contiguous()      # (anything negative is outside [0, K) as -1 is)
    dev = images.device
    f32 = dict(dtype=torch.float32, device=dev)
    th_in = theta.reshape(N)
    th_out, dx_out, score = torch.empty(N, **f32), torch.empty(N, 2, **f32), torch.empty(N, 2, **f32)
    steps = torch.empty(N, dtype=torch.int32, device=dev)
    # Images are independent and an image's addition order depends on (n, C) alone, so a call on a slice of the stack cannot
    # change a bit of any image's result: the slices only bound the launch grid and the state.
    stepN = CL.slice_step(N, CL.MAX_PLANES, SLICE)
    th_try, dx_try = torch.empty(stepN, **f32), torch.empty(stepN, 2, **f32)
    mom_try, mom_cur = torch.empty(stepN, MOMENTS, **f32), torch.empty(stepN, MOMENTS, **f32)
    lam = torch.empty(stepN, dtype=torch.float64, device=dev)
    ended = torch.empty(stepN, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for i0 in range(0, N, stepN):
            i1 = min(i0 + stepN, N)
            sl, M = slice(i0, i1), i1 - i0
            state = (th_try[:M], dx_try[:M], th_out[sl], dx_out[sl], mom_cur[:M], score[sl], lam[:M], steps[sl], ended[:M])
            CL.call('tvae_pose_moments', images[sl], th_in[sl], dx[sl], cls[sl], refs, mom_try[:M], M, C, n, K, t, radius, edge)
            CL.call('tvae_pose_polish_step', cls[sl], th_in[sl], dx[sl], mom_try[:M], *state, M, n, K, 1, t, shift, angle)
            for _ in range(its):
                CL.call('tvae_pose_moments', images[sl], th_try[:M], dx_try[:M], cls[sl], refs, mom_try[:M], M, C, n, K, t,
                        radius, edge)
                CL.call('tvae_pose_polish_step', cls[sl], th_in[sl], dx[sl], mom_try[:M], *state, M, n, K, 0, t, shift, angle)
    return th_out, dx_out, score, steps


def polish_rounds(images, theta, dx, labels, n_clusters=None, t_scale=1.0, rounds=1, iterations=8, max_shift=1.0,
                  max_angle=0.05, mask_radius=None, mask_edge=0.0, cross_halves=False):
    """`rounds` times: the class averages of the current poses (tvae.align.class_averages; with cross_halves=True the two
    half-set averages of tvae.align.class_halves as 2K references, every image scored against the half it is not in), then
    polish_poses; the trust region of every round is centred on the poses that round starts from.
    -> (theta' [N], dx' [N][2], history): history['scores'] fp64 [rounds][2], the mean start and final score over the images of
    a class in each round, history['steps'] fp64 [rounds], their mean number of accepted steps, and the last round's per-image
    record history['image_scores'] fp32 [N][2] and history['image_steps'] int32 [N]."""
    what = 'polish_rounds'
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, what)
    if int(rounds) < 1:
        raise TvaeHipError(f'{what}: rounds = {rounds} must be positive')
    th, d = theta.reshape(N).contiguous(), dx
    lab64 = lab.to(torch.int64)
    member = (lab64 >= 0) & (lab64 < K)
    cls = refine.cross_half_labels(lab64, K) if cross_halves else lab64
    scores, steps = [], []
    for _ in range(int(rounds)):
        if cross_halves:
            refs = align.class_halves(images, th, d, lab64, K, t_scale)[1].reshape(2 * K, C, n, n)
        else:
            refs = align.class_averages(images, th, d, lab64, K, t_scale)[0]
        th, d, sc, st = polish_poses(images, th, d, cls, refs, t_scale, iterations, max_shift, max_angle, mask_radius, mask_edge)
        m = sc[member].double()
        scores.append(m.mean(0).cpu().numpy() if m.numel() else np.zeros(2))
        steps.append(float(st[member].double().mean()) if m.numel() else 0.0)
    return th, d, dict(scores=np.stack(scores), steps=np.asarray(steps), image_scores=sc.cpu().numpy(), image_steps=st.cpu().numpy())


# ---- polish_poses.py: polished poses and averages from the files a clustering or refinement run wrote -------------------------
def build_parser() -> argparse.ArgumentParser:
    """A parser of its own: the flags of refine_poses.py that still apply, as that script declares them, and the three of the
    polish.  tvae.refine.build_parser() is left as it is."""
    base = refine.build_parser()
    p = argparse.ArgumentParser('Polish the poses of a clustered stack to sub-pixel accuracy against its aligned 2-D class averages')
    keep = {'stack', 'rotations', 'translations', 'clusters', 't_inf', 'crop', 'n_clusters', 'out_dir', 'device', 'mask_radius',
            'mask_edge', 'cross_halves'}
    for a in base._actions:
        if a.dest in keep:
            p._add_action(a)
    p.add_argument('--rounds', default=1, type=int, help='rounds of averaging and polishing')
    p.add_argument('--iterations', default=8, type=int, help='trial poses per image and round')
    p.add_argument('--max-shift', default=1.0, type=float, help='trust region: pixels per axis around the pose a round starts from')
    p.add_argument('--max-angle', default=math.degrees(0.05), type=float, help='trust region: degrees around the starting angle')
    return p


def run(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available() or args.device == -1:
        raise SystemExit('the MI355X build has no CPU compute path')
    torch.cuda.set_device(args.device)
    device = torch.device('cuda', args.device)
    stack = align.load_stack(args.stack, args.crop)
    particles = args.stack.endswith('mrc') or args.stack.endswith('mrcs')
    images = torch.from_numpy(stack).to(device)
    theta = torch.from_numpy(np.asarray(np.load(args.rotations), dtype=np.float32).reshape(-1)).to(device)
    dx = torch.from_numpy(np.ascontiguousarray(np.asarray(np.load(args.translations), dtype=np.float32))).to(device)
    clusters = np.asarray(np.load(args.clusters)).reshape(-1)
    t = align.translation_scale(args.t_inf)
    try:
        K = align._check_labels(images, theta, dx, clusters, args.n_clusters, 'polish_poses')[3]
        before = refine._resolutions(images, theta, dx, clusters, K, t)
        th, d, hist = polish_rounds(images, theta, dx, clusters, K, t, args.rounds, args.iterations, args.max_shift,
                                    math.radians(args.max_angle), args.mask_radius, args.mask_edge, args.cross_halves)
        avg, counts = align.class_averages(images, th, d, clusters, K, t)
        after = refine._resolutions(images, th, d, clusters, K, t)
    except TvaeHipError as e:
        raise SystemExit(str(e)) from e
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(os.path.join(args.out_dir, 'rotations_polished.npy'), th.cpu().numpy().reshape(np.load(args.rotations).shape))
    np.save(os.path.join(args.out_dir, 'translations_polished.npy'), d.cpu().numpy())
    np.save(os.path.join(args.out_dir, 'polish_scores.npy'), hist['image_scores'])      # [N][2] = (start, final) of the last round
    np.save(os.path.join(args.out_dir, 'polish_steps.npy'), hist['image_steps'])        # [N] accepted steps of the last round
    align.save_outputs(args.out_dir, avg.cpu().numpy(), counts.cpu().numpy(), particles, 'class_averages_polished')
    print('# class  members  resolution[px]@0.143 before -> after  resolution[px]@0.5 before -> after')
    cnt = counts.cpu().numpy()
    for k in range(K):
        print('{} {} {:.4f} -> {:.4f} {:.4f} -> {:.4f}'.format(k, int(cnt[k]), before[k, 0], after[k, 0], before[k, 1],
                                                               after[k, 1]))
    print('# polished the poses of {} images in {} classes, {} rounds, mean score {:.6f} -> {:.6f}: {}'.format(
        images.shape[0], K, args.rounds, hist['scores'][0, 0], hist['scores'][-1, 1], args.out_dir), file=sys.stderr)
    return th, d, hist
