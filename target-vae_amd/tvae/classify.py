"""Reassignment against the class averages on the GPU: the other half of the averaging loop (multi-reference alignment).
tvae.refine scores an image against the average of ITS class and never moves it to another; here every image is scored
against M candidate classes over the same small neighbourhood of poses (2A + 1 angles, (2S + 1)^2 whole-pixel shifts, the
cosine between the image and the prediction) and goes to the class whose best pose scores highest.  All classes share the
decoder's canonical frame, so the predicted pose is close to right for every class and no global angular search is needed.
include/tvae_cluster.h states the definition in full: a slot is tvae_pose_refine bit for bit, the slots are visited in
ascending order and a later one wins only with a strictly greater score, so ties stay with slot 0, the incumbent.

The kernel is tvae_pose_classify of libtvae_cluster.so: no CPU fallback, no float atomics, bitwise reproducible, and the
result of an image depends on that image, its pose, its row of candidates and the references that row names alone.  n > 128
is out of scope as it is for tvae.refine.

`classify_rounds` alternates averaging and reassigning -- averages -> score against every candidate class -> move ->
averages -- a reference-based 2-D classification seeded by the VAE's k-means labels.
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

MAX_CANDIDATES = 64               # TVAE_CLASSIFY_MAX_CANDIDATES


def _as_table(candidates, N, device, what):
    cand = torch.as_tensor(candidates)
    message = f'{what}: candidates must be an [N][M] = [{N}][M] integer array, got {tuple(cand.shape)} of {cand.dtype}'
    if cand.dim() != 2 or cand.shape[0] != N:
        raise TvaeHipError(message)
    idx = refine.class_index(cand.to(device), message)
    M = cand.shape[1]
    if not 1 <= M <= MAX_CANDIDATES:
        raise TvaeHipError(f'{what}: {M} candidates per image outside [1, {MAX_CANDIDATES}]')
    return idx, M


def classify_poses(images, theta, dx, candidates, refs, t_scale=1.0, angle_steps=8, angle_step=None, shift=2, mask_radius=None,
                   mask_edge=0.0, tables=False, ctf=None):
    """images [N][C][n][n], theta [N] or [N][1], dx [N][2], refs [K][C][n][n] (CUDA fp32), candidates [N][M] integers (any
    device or numpy; slot 0 by convention the image's current class, a value outside [0, K) is skipped) -> (labels' int64 [N],
    theta' [N], dx' [N][2], scores [N][M][2] = (centre, best) of every slot, best int32 [N][4] = (m*, a, sy, sx)) and with
    tables=True also (num, pp [N][M][NA][NS][NS], yy [N]), the raw sums.  An image with no valid slot keeps its pose and its
    slot-0 value.  angle_steps, angle_step, shift and the mask as in tvae.refine.refine_poses.
    ctf = (coef [N][5] on the device, yy fp32 [N] of the RAW images), the record of tvae.ml2d.e_step: `images` is the stack
    filtered with H_i already, and the score of a candidate is num / sqrt(ppc yy) with num from these images, ppc =
    tvae.ctf.template_power [N][M][NA] and yy the raw images' (tvae.ctf.search_poses: tvae_pose_classify for the tables, then
    tvae_pose_select).  Labels, poses, scores and best are that kernel's; with tables=True pp is ppc and yy the raw one."""
    what = 'classify_poses'
    if ctf is not None:
        return _classify_poses_ctf(what, images, theta, dx, candidates, refs, t_scale, angle_steps, angle_step, shift, mask_radius,
                                   mask_edge, tables, ctf)
    N, C, n = align._check_stack(images, theta, dx, what)
    A, S = int(angle_steps), int(shift)
    K, step, t, radius, edge = refine.check_search(what, images, refs, A, S, angle_step, t_scale, mask_radius, mask_edge)
    cand, M = _as_table(candidates, N, images.device, what)
    dev = images.device
    NA, NS = 2 * A + 1, 2 * S + 1
    th_in = theta.reshape(N)
    cls_out = torch.empty(N, dtype=torch.int32, device=dev)
    best = torch.empty(N, 4, dtype=torch.int32, device=dev)
    th_out = torch.empty(N, dtype=torch.float32, device=dev)
    dx_out = torch.empty(N, 2, dtype=torch.float32, device=dev)
    score = torch.empty(N, M, 2, dtype=torch.float32, device=dev)
    num = pp = yy = None
    if tables:
        num = torch.empty(N, M, NA, NS, NS, dtype=torch.float32, device=dev)
        pp = torch.empty(N, M, NA, NS, NS, dtype=torch.float32, device=dev)
        yy = torch.empty(N, dtype=torch.float32, device=dev)
    # Images are independent and an image's workgroups and addition order depend on (n, C, A, S) and its own row of
    # candidates alone, so a call on a slice of the stack cannot change a bit of any image's result: the slices only bound
    # the workspace (to the bound of tvae.refine, read when the call is made).
    per = CL.query('tvae_pose_classify_ws_floats', 1, M, C, n, A, S)
    if per <= 0:
        raise TvaeHipError(f'{what}: N={N}, M={M}, C={C}, n={n}, angle_steps={A}, shift={S} outside the supported range')
    stepN = CL.slice_step(N, CL.MAX_PLANES, refine.WS_FLOATS // per)
    wsf = CL.query('tvae_pose_classify_ws_floats', stepN, M, C, n, A, S)
    ws = torch.empty(wsf, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for i0 in range(0, N, stepN):
            i1 = min(i0 + stepN, N)
            sl = slice(i0, i1)
            CL.call('tvae_pose_classify', images[sl], th_in[sl], dx[sl], cand[sl], refs, cls_out[sl], best[sl], th_out[sl],
                    dx_out[sl], score[sl], None if num is None else num[sl], None if pp is None else pp[sl],
                    None if yy is None else yy[sl], ws, wsf, i1 - i0, C, n, K, M, A, S, t, step, radius, edge)
    out = (cls_out.to(torch.int64), th_out, dx_out, score, best)
    return out + (num, pp, yy) if tables else out


def _classify_poses_ctf(what, images, theta, dx, candidates, refs, t_scale, angle_steps, angle_step, shift, mask_radius, mask_edge,
                        tables, ctf):
    from . import ctf as ctf_mod
    N, C, n = align._check_stack(images, theta, dx, what)
    A, S = int(angle_steps), int(shift)
    step = refine.check_search(what, images, refs, A, S, angle_step, t_scale, mask_radius, mask_edge)[1]
    cand, _ = _as_table(candidates, N, images.device, what)
    th = theta.reshape(N)
    num_of = lambda sl: classify_poses(images[sl], th[sl], dx[sl], cand[sl], refs, t_scale, A, step, S, mask_radius, mask_edge,
                                       tables=True)[5]
    return ctf_mod.search_poses(what, num_of, th, dx, cand, refs, ctf, n, t_scale, A, step, S, mask_radius, mask_edge, tables)


def candidate_lists(labels, n_clusters, latents=None, m=None):
    """labels [N] (integers, any device or numpy) -> int64 [N][M] on the labels' device: the candidate classes of every image.
    Slot 0 is the current label, or -1 where the label is outside [0, K).  Without `latents` the other classes follow in
    ascending order (M = K unless `m` is given; K > 64 without `m` raises).  With `latents` [N][d] the m - 1 other classes
    follow whose centroid -- the mean latent of the class's current members, in fp64 -- is nearest to the image: ascending
    distance, ties to the lower class, empty classes last.  An image outside every class has no class of its own to leave
    out: its slots 1 .. m - 1 are the first m - 1 of all K classes in that order."""
    what = 'candidate_lists'
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise TvaeHipError(f'{what}: labels must be a one-dimensional integer array')
    K = int(n_clusters)
    if K < 1:
        raise TvaeHipError(f'{what}: n_clusters = {K} must be positive')
    if m is None:
        if K > MAX_CANDIDATES:
            raise TvaeHipError(f'{what}: {K} classes are more than the {MAX_CANDIDATES} candidates an image may have: give m '
                               '(and latents, so that the nearest classes are the candidates)')
        m = K
    m = int(m)
    if not 1 <= m <= min(K, MAX_CANDIDATES):
        raise TvaeHipError(f'{what}: m = {m} outside [1, min(n_clusters, {MAX_CANDIDATES})] = [1, {min(K, MAX_CANDIDATES)}]')
    lab = lab.to(torch.int64)
    dev = lab.device
    N = lab.numel()
    member = (lab >= 0) & (lab < K)
    own = torch.where(member, lab, torch.full_like(lab, -1))
    if latents is None:
        d2 = torch.arange(K, dtype=torch.float64, device=dev).expand(N, K).clone()
    else:
        z = torch.as_tensor(latents).to(dev).to(torch.float64)
        if z.dim() != 2 or z.shape[0] != N:
            raise TvaeHipError(f'{what}: latents must be [N][d] = [{N}][d], got {tuple(z.shape)}')
        onehot = torch.zeros(N, K, dtype=torch.float64, device=dev)
        onehot[member, lab[member]] = 1.0
        counts = onehot.sum(0)
        cen = (onehot.t() @ z) / counts.clamp(min=1.0)[:, None]
        d2 = ((z[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
        d2[:, counts == 0] = math.inf
    rows = torch.arange(N, device=dev)
    d2[rows[member], lab[member]] = -1.0                      # the own class sorts first: slot 0
    order = torch.sort(d2, dim=1, stable=True).indices        # (stable: ties to the lower class)
    out = torch.where(member[:, None], order[:, :m], torch.cat([own[:, None], order[:, :m - 1]], 1))
    return out.contiguous()


def cross_half_candidates(labels, candidates, n_clusters):
    """The reference index of every slot when the 2K references are [half 0 of class 0 .. K - 1, half 1 of class 0 .. K - 1]
    (tvae.align.class_halves): the slot for class k, own class or not, is K + k for an image at an even position of its own
    class and k at an odd one.  For the own class that is the half that does not contain the image
    (tvae.refine.cross_half_labels); neither half of another class contains it.  An image outside every class counts as
    even; a slot outside [0, K) stays -1.  Map a result back with % K."""
    K = int(n_clusters)
    cand = torch.as_tensor(candidates).to(torch.int64)
    own = refine.cross_half_labels(torch.as_tensor(labels).to(cand.device), K)
    odd = (own >= 0) & (own < K)
    valid = (cand >= 0) & (cand < K)
    return torch.where(valid, torch.where(odd[:, None], cand, cand + K), torch.full_like(cand, -1))


def classify_rounds(images, theta, dx, labels, n_clusters=None, t_scale=1.0, rounds=3, angle_range=math.pi / 8, angle_steps=8,
                    shift=2, mask_radius=None, mask_edge=0.0, cross_halves=False, latents=None, candidates=None, ctf=None,
                    wiener_tau=0.1):
    """`rounds` times: the class averages of the current labels and poses (tvae.align.class_averages; with cross_halves=True
    the two half-set averages of tvae.align.class_halves as 2K references, see cross_half_candidates), the candidate lists
    of the current labels (candidate_lists with `latents` and m = `candidates`), classify_poses, the labels and poses set to
    its results, then half the angle step.
    An empty class has a zero reference, scores exactly 0 against every image and so stays empty unless 0 is the best
    score an image reaches (every other candidate's cosine negative or undefined): reassignment does not revive a class.
    -> (labels' int64 [N], theta' [N], dx' [N][2], history): history['steps'] the angle step of every round,
    history['scores'] fp64 [rounds][2] the mean incumbent-centre score (slot 0) and the mean winning score over the images
    that were members of a class when the round began, history['moved'] int [rounds] the images whose label changed,
    history['counts'] int [rounds + 1][K] the class sizes before the first round and after each, and the last round's
    history['candidates'] int64 [N][M] (classes) with their history['slot_scores'] fp32 [N][M][2].
    ctf: coef rows [N][5] (tvae.ctf.coefficients) or None.  With them the score is that of the model Y_i = H_i (*) P_j + noise
    (classify_poses(ctf=...)): the stack filtered with H_i and the raw sums of squares are formed once, and every round's
    references are tvae.ctf.class_averages_ctf(..., 'wiener', wiener_tau) of the current labels and poses -- with cross_halves of
    the 2K half-set labels of tvae.refine.half_set_labels.  The history then also holds 'averages', 'members' and 'ctf_power', the
    Wiener averages of the returned labels and poses with their members and D [K][n][R], and the last round's 'references' with
    the reference index of every slot, 'slots' int64 [N][M].  ctf None: every line runs as without the argument."""
    what = 'classify_rounds'
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, what)
    A = int(angle_steps)
    if int(rounds) < 1:
        raise TvaeHipError(f'{what}: rounds = {rounds} must be positive')
    th, d = theta.reshape(N).contiguous(), dx
    lab64 = lab.to(torch.int64)
    if latents is not None:
        latents = torch.as_tensor(latents).to(images.device)
    count = lambda l: torch.bincount(l[(l >= 0) & (l < K)], minlength=K).cpu().numpy()
    steps, scores, moved, counts = [], [], [], [count(lab64)]
    cand = sc = refs = slots = None
    if ctf is not None:                                       # the stack num is formed from, and the record of classify_poses
        from . import ctf as ctf_mod
        coef, tau, scored, extra = ctf_mod.search_record(what, images, ctf, wiener_tau)
    for j in range(int(rounds)):
        step = float(angle_range) / max(A, 1) / 2 ** j
        cand = candidate_lists(lab64, K, latents, candidates)
        if ctf is None:
            refs = refine.round_references(images, th, d, lab64, K, t_scale, cross_halves)
        else:
            refs = refine.round_references_ctf(images, th, d, lab64, K, t_scale, cross_halves, coef, tau)
        slots = cross_half_candidates(lab64, cand, K) if cross_halves else cand
        if ctf is None:
            new, th, d, sc, best = classify_poses(images, th, d, slots, refs, t_scale, A, step, shift, mask_radius, mask_edge)
        else:
            new, th, d, sc, best = classify_poses(scored, th, d, slots, refs, t_scale, A, step, shift, mask_radius, mask_edge,
                                                  ctf=extra)
        if cross_halves:
            new = torch.where(new >= 0, new % K, new)
        member = (lab64 >= 0) & (lab64 < K)
        win = sc[torch.arange(N, device=sc.device), best[:, 0].to(torch.int64), 1]
        pair = torch.stack([sc[:, 0, 0], win], 1)[member].double()
        scores.append(pair.mean(0).cpu().numpy() if pair.numel() else np.zeros(2))
        moved.append(int((new != lab64).sum()))
        lab64 = new
        steps.append(step)
        counts.append(count(lab64))
    hist = dict(steps=steps, scores=np.stack(scores), moved=np.asarray(moved, dtype=np.int64), counts=np.stack(counts),
                candidates=cand, slot_scores=sc)
    if ctf is not None:
        avg, members, D = ctf_mod.class_averages_ctf(images, th, d, lab64, coef, K, t_scale, 'wiener', tau)
        hist.update(averages=avg, members=members, ctf_power=D, references=refs, slots=slots)
    return lab64, th, d, hist


def class_scores(candidates, slot_scores, n_clusters):
    """candidates int64 [N][M] (classes), slot_scores [N][M][2] -> fp32 [N][K] numpy: the best score of every image against
    every class, NaN where a class was not among its candidates."""
    cand = torch.as_tensor(candidates).cpu().to(torch.int64)
    sc = torch.as_tensor(slot_scores).cpu()[:, :, 1]
    K = int(n_clusters)
    out = torch.full((cand.shape[0], K), float('nan'), dtype=torch.float32)
    valid = (cand >= 0) & (cand < K)
    rows = torch.arange(cand.shape[0])[:, None].expand_as(cand)
    out[rows[valid], cand[valid]] = sc[valid]
    return out.numpy()


# ---- reclassify_particles.py: new labels, poses and averages from the files a clustering run wrote ----------------------------
def build_parser(ctf=False) -> argparse.ArgumentParser:
    """ctf=True adds --ctf, --wiener-tau and --scale (what reclassify_particles.py parses); the default is the parser without
    them."""
    p = argparse.ArgumentParser('Reassign the images of a clustered stack to their best-matching aligned 2-D class average')
    stack_cli.add_stack_flags(p)
    stack_cli.add_grid_flags(p)
    stack_cli.add_candidate_flags(p)
    if ctf:
        align.add_ctf_flags(p, ())
    return p


def save_outputs(out_dir, labels, theta, dx, hist, avg, counts, particles, rot_shape):
    """clusters_reclassified.npy, rotations_reclassified.npy (in `rot_shape`, the shape of the rotations that came in),
    translations_reclassified.npy, classify_scores.npy, classify_moved.npy, class_scores.npy ([N][K], class_scores) and
    class_averages_reclassified.npy (.mrcs, .jpg): reclassify_particles.py and TVAE_RECLASSIFY=1 write these; and
    class_ctf_power_reclassified.npy, the per-class sums of H^2, when the rounds ran with a CTF."""
    save = lambda name, a: np.save(os.path.join(out_dir, name), a)
    save('clusters_reclassified.npy', stack_cli.host(labels))
    if hist.get('ctf_power') is not None:
        save('class_ctf_power_reclassified.npy', stack_cli.host(hist['ctf_power']))
    save('classify_scores.npy', hist['scores'])
    save('classify_moved.npy', hist['moved'])
    save('class_scores.npy', class_scores(hist['candidates'], hist['slot_scores'], avg.shape[0]))
    stack_cli.save_poses(out_dir, 'reclassified', theta, dx, avg, counts, particles, rot_shape)


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters, t = inp.images, inp.theta, inp.dx, inp.clusters, inp.t_scale
    with stack_cli.hip_errors():
        coef = align.load_ctf_coefficients(args.ctf, images.shape[0], args.scale) if args.ctf else None
        K = align._check_labels(images, theta, dx, clusters, args.n_clusters, 'classify_rounds')[3]
        before = refine._resolutions(images, theta, dx, clusters, K, t)
        lab, th, d, hist = classify_rounds(images, theta, dx, clusters, K, t, args.rounds, math.radians(args.angle_range),
                                           args.angle_steps, args.shift, args.mask_radius, args.mask_edge, args.cross_halves,
                                           inp.latents, args.candidates, coef, args.wiener_tau)
        new = lab.cpu().numpy()
        avg, counts = (hist['averages'], hist['members']) if args.ctf else align.class_averages(images, th, d, new, K, t)
        after = refine._resolutions(images, th, d, new, K, t)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, new, th, d, hist, avg, counts, inp.particles, inp.rot_shape)
    stack_cli.print_resolution_table(before, after, hist['counts'][0], hist['counts'][-1])
    print('# reassigned {} images among {} classes, {} rounds, moved {}, mean score {:.6f} -> {:.6f}: {}'.format(
        images.shape[0], K, args.rounds, hist['moved'].tolist(), hist['scores'][0, 0], hist['scores'][-1, 1], args.out_dir),
        file=sys.stderr)
    return lab, th, d, hist
