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
from . import align, refine, stack_cli
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
    K, _, t, radius, edge = refine.check_search(what, images, refs, t_scale=t_scale, mask_radius=mask_radius, mask_edge=mask_edge,
                                                side_note='')
    its, shift, angle = int(iterations), float(max_shift), float(max_angle)
    if not (its >= 0 and np.isfinite(shift) and shift >= 0 and np.isfinite(angle) and angle >= 0):
        raise TvaeHipError(f'{what}: iterations = {iterations}, max_shift = {max_shift} and max_angle = {max_angle} must be '
                           'finite and not negative')
    cls = refine.class_index(lab, f'{what}: labels must be a one-dimensional integer array')
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
        refs = refine.round_references(images, th, d, lab64, K, t_scale, cross_halves)
        th, d, sc, st = polish_poses(images, th, d, cls, refs, t_scale, iterations, max_shift, max_angle, mask_radius, mask_edge)
        m = sc[member].double()
        scores.append(m.mean(0).cpu().numpy() if m.numel() else np.zeros(2))
        steps.append(float(st[member].double().mean()) if m.numel() else 0.0)
    return th, d, dict(scores=np.stack(scores), steps=np.asarray(steps), image_scores=sc.cpu().numpy(), image_steps=st.cpu().numpy())


# ---- polish_poses.py: polished poses and averages from the files a clustering or refinement run wrote -------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser('Polish the poses of a clustered stack to sub-pixel accuracy against its aligned 2-D class averages')
    stack_cli.add_stack_flags(p)
    stack_cli.add_mask_flags(p, 0.0, 'default: no mask', cross_halves=True)
    p.add_argument('--rounds', default=1, type=int, help='rounds of averaging and polishing')
    p.add_argument('--iterations', default=8, type=int, help='trial poses per image and round')
    p.add_argument('--max-shift', default=1.0, type=float, help='trust region: pixels per axis around the pose a round starts from')
    p.add_argument('--max-angle', default=math.degrees(0.05), type=float, help='trust region: degrees around the starting angle')
    return p


def save_outputs(out_dir, theta, dx, hist, avg, counts, particles, rot_shape):
    """rotations_polished.npy (in `rot_shape`, the shape of the rotations that came in), translations_polished.npy,
    polish_scores.npy ([N][2] = (start, final) of the last round), polish_steps.npy ([N], its accepted steps) and
    class_averages_polished.npy (.mrcs, .jpg): polish_poses.py and TVAE_POLISH_POSES=1 write these."""
    np.save(os.path.join(out_dir, 'polish_scores.npy'), hist['image_scores'])
    np.save(os.path.join(out_dir, 'polish_steps.npy'), hist['image_steps'])
    stack_cli.save_poses(out_dir, 'polished', theta, dx, avg, counts, particles, rot_shape)


def run(argv=None):
    args = build_parser().parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters, t = inp.images, inp.theta, inp.dx, inp.clusters, inp.t_scale
    with stack_cli.hip_errors():
        K = align._check_labels(images, theta, dx, clusters, args.n_clusters, 'polish_poses')[3]
        before = refine._resolutions(images, theta, dx, clusters, K, t)
        th, d, hist = polish_rounds(images, theta, dx, clusters, K, t, args.rounds, args.iterations, args.max_shift,
                                    math.radians(args.max_angle), args.mask_radius, args.mask_edge, args.cross_halves)
        avg, counts = align.class_averages(images, th, d, clusters, K, t)
        after = refine._resolutions(images, th, d, clusters, K, t)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, th, d, hist, avg, counts, inp.particles, inp.rot_shape)
    stack_cli.print_resolution_table(before, after, counts.cpu().numpy())
    print('# polished the poses of {} images in {} classes, {} rounds, mean score {:.6f} -> {:.6f}: {}'.format(
        images.shape[0], K, args.rounds, hist['scores'][0, 0], hist['scores'][-1, 1], args.out_dir), file=sys.stderr)
    return th, d, hist
