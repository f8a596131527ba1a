"""Pose refinement against the class averages on the GPU: the step after class_averages.py.  Every image is scored against
the average of its class over a small neighbourhood of poses -- the average rendered into the image's frame at 2A + 1 angles
around the predicted one and compared at (2S + 1)^2 whole-pixel shifts, the score the cosine between the image and the
prediction -- and keeps the best pose; the averages are then formed again.  include/tvae_cluster.h states the definition
in full (the inverse of the map of tvae.align: the reference is resampled, not the image).

The kernel is tvae_pose_refine of libtvae_cluster.so: no CPU fallback, no float atomics, bitwise reproducible, and the
result of an image depends on that image, its pose and its class's reference alone.  n > 128 is out of scope (one image
plane and one extended template have to fit the LDS): Fourier-downsample the stack with tvae.image first -- poses are in
coordinate units and carry over unchanged.

This module is also the home of the argument rules that every pose search against references shares (tvae.classify,
tvae.polish and, for its part, tvae.ml2d): `check_search`, `class_index` and `round_references`.

`refine_rounds` alternates averaging and refining and halves the angle step after every round.  With cross_halves=True
every image is scored against the half-set average it is NOT a member of, so that no image is aligned to an average that
contains it.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import align, stack_cli
from ._lib import TvaeHipError

MAX_SIDE, MAX_CHANNELS, MAX_ANGLE_STEPS, MAX_SHIFT = 128, 16, 32, 8
WS_FLOATS = 1 << 26               # workspace of one tvae_pose_refine call: 256 MB


def _check_refs(images, refs, what):
    CL.require_f32(refs, what, 'refs')
    N, C, n, _ = images.shape
    if refs.dim() != 4 or tuple(refs.shape[1:]) != (C, n, n) or refs.device != images.device:
        raise TvaeHipError(f'{what}: refs must be [K][C][n][n] = [K][{C}][{n}][{n}] on the device of the images, got '
                           f'{tuple(refs.shape)}')
    K = refs.shape[0]
    if not 1 <= K <= align.MAX_CLUSTERS:
        raise TvaeHipError(f'{what}: {K} references outside [1, {align.MAX_CLUSTERS}]')
    return K


def angle_step_of(angle_steps, angle_step=None):
    """angle_step None: pi / 8 divided by max(A, 1)."""
    return math.pi / 8 / max(int(angle_steps), 1) if angle_step is None else float(angle_step)


LDS_NOTE = ' (one image plane and one extended template must fit the LDS)'


def check_search(what, images, refs, angle_steps=None, shift=None, angle_step=None, t_scale=1.0, mask_radius=None,
                 mask_edge=0.0, side_note=LDS_NOTE):
    """THE statement of the argument rules of a pose search against references (refine_poses, classify_poses, polish_poses),
    after the stack has passed tvae.align's checks: the references, the side, the ranges of C, A and S, t_scale, the angle
    step and the mask.  A search without a grid (the polish) leaves angle_steps, shift and angle_step away, and its messages
    do not speak of them.  -> (K, step, t, radius, edge), normalised."""
    K = _check_refs(images, refs, what)
    C, n = images.shape[1], images.shape[-1]
    grid = angle_steps is not None
    A, S = (int(angle_steps), int(shift)) if grid else (0, 0)
    if n > MAX_SIDE:
        raise TvaeHipError(f'{what}: n = {n} is above {MAX_SIDE}{side_note}: Fourier-downsample the stack with tvae.image first; '
                           'poses are in coordinate units and carry over unchanged')
    if not (C <= MAX_CHANNELS and 0 <= A <= MAX_ANGLE_STEPS and 0 <= S <= MAX_SHIFT):
        if not grid:
            raise TvaeHipError(f'{what}: C={C} outside the supported range (C <= {MAX_CHANNELS})')
        raise TvaeHipError(f'{what}: C={C}, angle_steps={A}, shift={S} outside the supported range (C <= {MAX_CHANNELS}, '
                           f'0 <= angle_steps <= {MAX_ANGLE_STEPS}, 0 <= shift <= {MAX_SHIFT})')
    step, t = angle_step_of(A, angle_step), float(t_scale)
    radius = 0.0 if mask_radius is None else float(mask_radius)
    edge = float(mask_edge)
    if not (np.isfinite(t) and t > 0 and np.isfinite(step)):
        raise TvaeHipError(f'{what}: t_scale = {t_scale} must be finite and positive' +
                           (f' and angle_step = {angle_step} finite' if grid else ''))
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'{what}: mask_radius = {mask_radius} and mask_edge = {mask_edge} must be finite, the edge not negative')
    return K, step, t, radius, edge


def class_index(values, message):
    """Integer labels or candidates -> contiguous int32 for the kernels, clamped into int32 (anything negative is outside
    [0, K) as -1 is, anything above int32 as 2^31 - 1 is); floating and bool tensors raise `message`."""
    if values.dtype.is_floating_point or values.dtype == torch.bool:
        raise TvaeHipError(message)
    return values.to(torch.int64).clamp(-1, torch.iinfo(torch.int32).max).to(torch.int32).contiguous()


def round_references(images, theta, dx, lab64, K, t_scale, cross_halves):
    """The references a round scores against, [K][C][n][n] (tvae.align.class_averages of the current poses) or, with
    cross_halves, [2K][C][n][n] = [half 0 of class 0 .. K - 1, half 1 of class 0 .. K - 1] (tvae.align.class_halves)."""
    if cross_halves:
        return align.class_halves(images, theta, dx, lab64, K, t_scale)[1].reshape(2 * K, *images.shape[1:])
    return align.class_averages(images, theta, dx, lab64, K, t_scale)[0]


def half_set_labels(lab64, K):
    """labels int64 [N] -> int64 [N]: the label h K + k among the 2K half-set classes [half 0 of class 0 .. K - 1, half 1 of
    class 0 .. K - 1] of the half the image is IN (cross_half_labels names the other one); -1 outside [0, K).  A class average
    over these labels with 2K classes has the layout of round_references(cross_halves=True)."""
    own = cross_half_labels(lab64, K)
    return torch.where(own >= 0, (own + K) % (2 * K), own)


def round_references_ctf(images, theta, dx, lab64, K, t_scale, cross_halves, coef, tau):
    """round_references under a CTF: the Wiener averages tvae.ctf.class_averages_ctf of the RAW images, [K][C][n][n] or, with
    cross_halves, those of half_set_labels, [2K][C][n][n]."""
    from . import ctf
    if cross_halves:
        return ctf.class_averages_ctf(images, theta, dx, half_set_labels(lab64, K), coef, 2 * K, t_scale, 'wiener', tau)[0]
    return ctf.class_averages_ctf(images, theta, dx, lab64, coef, K, t_scale, 'wiener', tau)[0]


def refine_poses(images, theta, dx, labels, refs, t_scale=1.0, angle_steps=8, angle_step=None, shift=2, mask_radius=None,
                 mask_edge=0.0, tables=False, ctf=None):
    """images [N][C][n][n], theta [N] or [N][1], dx [N][2], refs [K][C][n][n] (CUDA fp32), labels [N] integers (any device or
    numpy; a label outside [0, K) leaves its image alone) -> (theta' [N], dx' [N][2], scores [N][2] = (centre, best),
    best int32 [N][3] = (a, sy, sx)) and with tables=True also (num, pp [N][NA][NS][NS], yy [N]), the raw sums.
    angle_steps = A steps of angle_step radians to each side (None: pi / 8 divided by max(A, 1)); shift = S pixels.
    ctf = (coef [N][5] on the device, yy fp32 [N] of the RAW images): `images` is the stack filtered with H_i already and the
    score of a candidate is num / sqrt(ppc yy), ppc = tvae.ctf.template_power of the image's class (tvae.ctf.search_poses with
    one slot per image: tvae_pose_refine for num, then tvae_pose_select).  With tables=True pp is ppc [N][NA] and yy the raw
    one."""
    what = 'refine_poses'
    if ctf is not None:
        return _refine_poses_ctf(what, images, theta, dx, labels, refs, t_scale, angle_steps, angle_step, shift, mask_radius,
                                 mask_edge, tables, ctf)
    N, C, n, _, lab = align._check_labels(images, theta, dx, labels, 1, what)
    A, S = int(angle_steps), int(shift)
    K, step, t, radius, edge = check_search(what, images, refs, A, S, angle_step, t_scale, mask_radius, mask_edge)
    cls = class_index(lab, f'{what}: labels must be a one-dimensional integer array')
    dev = images.device
    NA, NS = 2 * A + 1, 2 * S + 1
    th_in = theta.reshape(N)
    th_out = torch.empty(N, dtype=torch.float32, device=dev)
    dx_out = torch.empty(N, 2, dtype=torch.float32, device=dev)
    score = torch.empty(N, 2, dtype=torch.float32, device=dev)
    best = torch.empty(N, 3, dtype=torch.int32, device=dev)
    num = pp = yy = None
    if tables:
        num = torch.empty(N, NA, NS, NS, dtype=torch.float32, device=dev)
        pp = torch.empty(N, NA, NS, NS, dtype=torch.float32, device=dev)
        yy = torch.empty(N, dtype=torch.float32, device=dev)
    # Images are independent and an image's workgroups and addition order depend on (n, C, A, S) alone, so a call on a slice
    # of the stack cannot change a bit of any image's result: the slices only bound the workspace.
    per = CL.query('tvae_pose_refine_ws_floats', 1, C, n, A, S)
    if per <= 0:
        raise TvaeHipError(f'{what}: N={N}, C={C}, n={n}, angle_steps={A}, shift={S} outside the supported range')
    stepN = CL.slice_step(N, CL.MAX_PLANES, WS_FLOATS // per)
    wsf = CL.query('tvae_pose_refine_ws_floats', stepN, C, n, A, S)
    ws = torch.empty(wsf, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for i0 in range(0, N, stepN):
            i1 = min(i0 + stepN, N)
            sl = slice(i0, i1)
            CL.call('tvae_pose_refine', images[sl], th_in[sl], dx[sl], cls[sl], refs, th_out[sl], dx_out[sl], score[sl],
                    best[sl], None if num is None else num[sl], None if pp is None else pp[sl],
                    None if yy is None else yy[sl], ws, wsf, i1 - i0, C, n, K, A, S, t, step, radius, edge)
    if tables:
        return th_out, dx_out, score, best, num, pp, yy
    return th_out, dx_out, score, best


def _refine_poses_ctf(what, images, theta, dx, labels, refs, t_scale, angle_steps, angle_step, shift, mask_radius, mask_edge,
                      tables, ctf):
    from . import ctf as ctf_mod
    N, C, n, _, lab = align._check_labels(images, theta, dx, labels, 1, what)
    A, S = int(angle_steps), int(shift)
    step = check_search(what, images, refs, A, S, angle_step, t_scale, mask_radius, mask_edge)[1]
    cls = class_index(lab, f'{what}: labels must be a one-dimensional integer array')
    th = theta.reshape(N)
    # (the tables of tvae_pose_refine have the layout of one slot)
    num_of = lambda sl: refine_poses(images[sl], th[sl], dx[sl], cls[sl], refs, t_scale, A, step, S, mask_radius, mask_edge,
                                     tables=True)[4].unsqueeze(1)
    out = ctf_mod.search_poses(what, num_of, th, dx, cls[:, None], refs, ctf, n, t_scale, A, step, S, mask_radius, mask_edge, tables)
    th_out, dx_out, score, best = out[1], out[2], out[3].reshape(N, 2), out[4][:, 1:].contiguous()
    if tables:
        return th_out, dx_out, score, best, out[5].squeeze(1), out[6].squeeze(1), out[7]
    return th_out, dx_out, score, best


def cross_half_labels(labels, n_clusters):
    """labels [N] (integers, any device) -> int64 [N] on the same device: the index among the 2K references
    [half 0 of class 0 .. K - 1, half 1 of class 0 .. K - 1] of the half-set average that does NOT contain the image.  Half
    membership is the rule of tvae_class_halves: the position of the image within its class in `segments` order, even =
    half 0, odd = half 1.  So an image of half 0 gets K + k and one of half 1 gets k; a label outside [0, K) gets -1."""
    lab = torch.as_tensor(labels)
    K = int(n_clusters)
    order, seg, _ = align.segments(lab, K)
    order, seg = order.to(torch.int64), seg.to(torch.int64)
    N = order.numel()
    pos = torch.arange(N, device=order.device)
    key = torch.where((lab.to(torch.int64) >= 0) & (lab.to(torch.int64) < K), lab.to(torch.int64),
                      torch.full_like(lab.to(torch.int64), K))[order]      # class of every position (K: none)
    valid = key < K
    first = seg[key.clamp(max=K - 1)]
    odd = ((pos - first) % 2) == 1
    ref = torch.where(odd, key, key + K)
    out = torch.full((N,), -1, dtype=torch.int64, device=order.device)
    out[order] = torch.where(valid, ref, torch.full_like(ref, -1))
    return out


def refine_rounds(images, theta, dx, labels, n_clusters=None, t_scale=1.0, rounds=3, angle_range=math.pi / 8, angle_steps=8,
                  shift=2, mask_radius=None, mask_edge=0.0, cross_halves=False, ctf=None, wiener_tau=0.1):
    """`rounds` times: the class averages of the current poses (tvae.align.class_averages; with cross_halves=True the two
    half-set averages of tvae.align.class_halves as 2K references, every image scored against the half it is not in), then
    refine_poses, then half the angle step: round j searches angle_range / 2^j to each side in angle_steps steps, inside the
    cell that the previous round chose.  -> (theta' [N], dx' [N][2], history): history['steps'] the angle step of every round
    and history['scores'] fp64 [rounds][2], the mean centre and best score over the images of a class in each round.
    ctf: coef rows [N][5] (tvae.ctf.coefficients) or None.  With them the score is that of the model Y_i = H_i (*) P_j + noise
    (refine_poses(ctf=...)): the stack filtered with H_i and the raw sums of squares are formed once, and every round's
    references are round_references_ctf, the Wiener averages (wiener_tau) of the current poses.  The history then also holds
    'averages', 'members' and 'ctf_power' -- the Wiener averages of the returned poses, their members and D [K][n][R] -- and the
    last round's 'references' with 'slots' int64 [N], the reference every image was scored against.  ctf None: every line runs
    as without the argument."""
    what = 'refine_rounds'
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, what)
    A = int(angle_steps)
    if int(rounds) < 1:
        raise TvaeHipError(f'{what}: rounds = {rounds} must be positive')
    th, d = theta.reshape(N).contiguous(), dx
    lab64 = lab.to(torch.int64)
    member = (lab64 >= 0) & (lab64 < K)
    cls = cross_half_labels(lab64, K) if cross_halves else lab64
    steps, scores = [], []
    refs = None
    if ctf is not None:                                       # the stack num is formed from, and the record of refine_poses
        from . import ctf as ctf_mod
        coef, tau, scored, extra = ctf_mod.search_record(what, images, ctf, wiener_tau)
    for j in range(int(rounds)):
        step = float(angle_range) / max(A, 1) / 2 ** j
        if ctf is None:
            refs = round_references(images, th, d, lab64, K, t_scale, cross_halves)
            th, d, sc, _ = refine_poses(images, th, d, cls, refs, t_scale, A, step, shift, mask_radius, mask_edge)
        else:
            refs = round_references_ctf(images, th, d, lab64, K, t_scale, cross_halves, coef, tau)
            th, d, sc, _ = refine_poses(scored, th, d, cls, refs, t_scale, A, step, shift, mask_radius, mask_edge, ctf=extra)
        steps.append(step)
        m = sc[member].double()
        scores.append(m.mean(0).cpu().numpy() if m.numel() else np.zeros(2))
    hist = dict(steps=steps, scores=np.stack(scores))
    if ctf is not None:
        avg, counts, D = ctf_mod.class_averages_ctf(images, th, d, lab64, coef, K, t_scale, 'wiener', tau)
        hist.update(averages=avg, members=counts, ctf_power=D, references=refs, slots=cls)
    return th, d, hist


# ---- refine_poses.py: refined poses and averages from the files a clustering run wrote ---------------------------------------
def build_parser(ctf=False) -> argparse.ArgumentParser:
    """ctf=True adds --ctf, --wiener-tau and --scale (what refine_poses.py parses); the default is the parser without them."""
    p = argparse.ArgumentParser('Refine the poses of a clustered stack against its aligned 2-D class averages')
    stack_cli.add_stack_flags(p)
    stack_cli.add_grid_flags(p)
    if ctf:
        align.add_ctf_flags(p, ())
    return p


def _resolutions(images, theta, dx, clusters, K, t):
    from . import resolution
    res = resolution.class_resolution(images, theta, dx, clusters, K, t)
    curve = resolution.combined(res['sums'].cpu().numpy())
    n = images.shape[-1]
    return np.stack([resolution.resolution(curve, n, thr) for thr in resolution.THRESHOLDS], 1)


def save_outputs(out_dir, theta, dx, hist, avg, counts, particles, rot_shape):
    """rotations_refined.npy (in `rot_shape`, the shape of the rotations that came in), translations_refined.npy,
    refine_scores.npy and class_averages_refined.npy (.mrcs, .jpg): refine_poses.py and TVAE_REFINE_POSES=1 write these; and
    class_ctf_power_refined.npy, the per-class sums of H^2, when the rounds ran with a CTF."""
    np.save(os.path.join(out_dir, 'refine_scores.npy'), hist['scores'])
    if hist.get('ctf_power') is not None:
        np.save(os.path.join(out_dir, 'class_ctf_power_refined.npy'), stack_cli.host(hist['ctf_power']))
    stack_cli.save_poses(out_dir, 'refined', theta, dx, avg, counts, particles, rot_shape)


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters, t = inp.images, inp.theta, inp.dx, inp.clusters, inp.t_scale
    with stack_cli.hip_errors():
        coef = align.load_ctf_coefficients(args.ctf, images.shape[0], args.scale) if args.ctf else None
        K = align._check_labels(images, theta, dx, clusters, args.n_clusters, 'refine_poses')[3]
        before = _resolutions(images, theta, dx, clusters, K, t)
        th, d, hist = refine_rounds(images, theta, dx, clusters, K, t, args.rounds, math.radians(args.angle_range),
                                    args.angle_steps, args.shift, args.mask_radius, args.mask_edge, args.cross_halves, coef,
                                    args.wiener_tau)
        avg, counts = (hist['averages'], hist['members']) if args.ctf else align.class_averages(images, th, d, clusters, K, t)
        after = _resolutions(images, th, d, clusters, K, t)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, th, d, hist, avg, counts, inp.particles, inp.rot_shape)
    stack_cli.print_resolution_table(before, after, counts.cpu().numpy())
    print('# refined the poses of {} images in {} classes, {} rounds, mean score {:.6f} -> {:.6f}: {}'.format(
        images.shape[0], K, args.rounds, hist['scores'][0, 0], hist['scores'][-1, 1], args.out_dir), file=sys.stderr)
    return th, d, hist
