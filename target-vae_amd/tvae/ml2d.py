"""Maximum-likelihood 2-D class averages on the GPU: the soft form of the averaging loop of tvae.classify.  There every image
gets exactly one class and one pose, the arg-max; at the signal-to-noise ratio of real particle stacks the arg-max is often
wrong and a hard average is biased towards its own noise.  Here every image contributes to every (class, angle, shift) it is
compatible with, with its posterior weight under white Gaussian noise; the noise variance and the class priors are
re-estimated, and the loop repeats (expectation-maximisation over a fixed discrete set of poses, as in RELION's 2-D
classification).

E-step: tvae_pose_classify writes the tables num, pp, yy, from which the squared residual of image i against candidate j is
yy - 2 num_j + pp_j exactly; tvae_pose_posterior turns them into the posterior over (slot, angle, shift), keeps the `keep`
heaviest candidates of every image as (class, pose, weight) entries and reports the log-likelihood and the expected residual.
M-step: tvae_class_average_weighted, the weighted aligned average over the entries grouped by class.  include/tvae_cluster.h
states both definitions in full.  No CPU fallback, no atomics, bitwise reproducible.  `entries_by_class` and the update
helpers are torch code that does not care where its tensors live.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import align, classify, refine, stack_cli
from . import ctf as ctf_mod
from ._lib import TvaeHipError

MAX_KEEP = 64                     # TVAE_POSTERIOR_MAX_KEEP


def pose_posteriors(num, pp, yy, candidates, theta, dx, n, n_clusters, sigma2, logprior=None, keep=8, t_scale=1.0,
                    angle_steps=8, angle_step=None, shift=2):
    """The tables of classify_poses(..., tables=True) -- num, pp [N][M][NA][NS][NS], yy [N] (CUDA fp32) -- with the
    candidates [N][M] they were made for, the poses theta [N] and dx [N][2] the grid is centred on and the side n of the
    images -> dict(idx, cls int32 [N][P], theta [N][P], dx [N][P][2], w [N][P], resp [N][M], lse, r2 fp64 [N], kept [N]):
    the P = `keep` heaviest candidates of every image in rank order (idx = -1 behind the last), the posterior of every slot,
    the log of the summed likelihood, the expected squared residual and the posterior mass the kept entries carry.  logprior:
    fp64 [K] or None (0 for every class); angle_steps, angle_step and shift as they were given to classify_poses."""
    what = 'pose_posteriors'
    for nm, t in (('num', num), ('pp', pp), ('yy', yy), ('theta', theta), ('dx', dx)):
        CL.require_f32(t, what, nm)
    N = yy.numel()
    cand, M = classify._as_table(candidates, N, yy.device, what)
    A, S, P, K, n = int(angle_steps), int(shift), int(keep), int(n_clusters), int(n)
    NA, NS = 2 * A + 1, 2 * S + 1
    if tuple(num.shape) != (N, M, NA, NS, NS) or num.shape != pp.shape:
        raise TvaeHipError(f'{what}: num and pp must be [N][M][NA][NS][NS] = {(N, M, NA, NS, NS)}, got {tuple(num.shape)} and '
                           f'{tuple(pp.shape)}')
    if theta.numel() != N or tuple(dx.shape) != (N, 2):
        raise TvaeHipError(f'{what}: theta must hold N = {N} angles and dx must be [N][2]')
    if not (1 <= P <= MAX_KEEP and 1 <= K <= CL.MAX_CLASSES and 2 <= n <= refine.MAX_SIDE and 0 <= A <= refine.MAX_ANGLE_STEPS
            and 0 <= S <= refine.MAX_SHIFT and 1 <= N <= CL.MAX_PLANES):
        raise TvaeHipError(f'{what}: N={N}, n={n}, K={K}, keep={P}, angle_steps={A}, shift={S} outside the supported range '
                           f'(1 <= keep <= {MAX_KEEP})')
    step = refine.angle_step_of(A, angle_step)
    t, s2 = float(t_scale), float(np.float32(sigma2))
    if not (np.isfinite(t) and t > 0 and np.isfinite(step) and np.isfinite(s2) and s2 > 0):
        raise TvaeHipError(f'{what}: t_scale = {t_scale} and sigma2 = {sigma2} must be finite and positive (in fp32) and '
                           f'angle_step = {angle_step} finite')
    dev = yy.device
    lp = None
    if logprior is not None:
        lp = torch.as_tensor(logprior).to(dev, torch.float64).contiguous()
        if tuple(lp.shape) != (K,):
            raise TvaeHipError(f'{what}: logprior must hold K = {K} values, got {tuple(lp.shape)}')
    out = dict(idx=torch.empty(N, P, dtype=torch.int32, device=dev), cls=torch.empty(N, P, dtype=torch.int32, device=dev),
               theta=torch.empty(N, P, dtype=torch.float32, device=dev), dx=torch.empty(N, P, 2, dtype=torch.float32, device=dev),
               w=torch.empty(N, P, dtype=torch.float32, device=dev), resp=torch.empty(N, M, dtype=torch.float32, device=dev),
               lse=torch.empty(N, dtype=torch.float64, device=dev), r2=torch.empty(N, dtype=torch.float64, device=dev),
               kept=torch.empty(N, dtype=torch.float32, device=dev))
    with torch.cuda.device(dev):
        CL.call('tvae_pose_posterior', num, pp, yy.reshape(N), cand, lp, theta.reshape(N), dx, out['idx'], out['cls'],
                out['theta'], out['dx'], out['w'], out['resp'], out['lse'], out['r2'], out['kept'], N, n, K, M, A, S, P, t,
                step, s2)
    return out


def entries_by_class(ent_cls, ent_w, ent_theta, ent_dx, n_clusters):
    """ent_cls [N][P] (integers), ent_w, ent_theta [N][P], ent_dx [N][P][2] -> dict(img int32 [E], theta [E], dx [E][2],
    w [E], seg int32 [K + 1]): the entries flattened, those whose class is outside [0, K) dropped, sorted stably by class so
    that within a class the order is ascending (image, rank); class k is the entries seg[k] .. seg[k + 1].  Pure torch: works
    on CPU tensors as on the GPU."""
    cls = torch.as_tensor(ent_cls)
    if cls.dim() != 2 or cls.dtype.is_floating_point or cls.dtype == torch.bool:
        raise TvaeHipError('entries_by_class: ent_cls must be an [N][P] integer array')
    K = int(n_clusters)
    if K < 1:
        raise TvaeHipError(f'entries_by_class: n_clusters = {K} must be positive')
    N, P = cls.shape
    dev = cls.device
    w, th, d = torch.as_tensor(ent_w).to(dev), torch.as_tensor(ent_theta).to(dev), torch.as_tensor(ent_dx).to(dev)
    if tuple(w.shape) != (N, P) or tuple(th.shape) != (N, P) or tuple(d.shape) != (N, P, 2):
        raise TvaeHipError(f'entries_by_class: ent_w and ent_theta must be [N][P] = {(N, P)} and ent_dx [N][P][2]')
    flat = cls.reshape(-1).to(torch.int64)
    keep = torch.nonzero((flat >= 0) & (flat < K)).reshape(-1)             # ascending (image, rank)
    order = keep[torch.sort(flat[keep], stable=True).indices]
    seg = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(torch.bincount(flat[keep], minlength=K), 0)
    return dict(img=(order // P).to(torch.int32), theta=th.reshape(-1)[order].contiguous(),
                dx=d.reshape(-1, 2)[order].contiguous(), w=w.reshape(-1)[order].contiguous(), seg=seg.to(torch.int32))


def chunk_entries(E, K, C, n) -> int:
    """Entries of a class per partial sum of tvae_class_average_weighted (0 for unsupported arguments)."""
    return CL.query('tvae_class_average_weighted_chunk', E, K, C, n)


def weighted_class_averages(images, entries, n_clusters, t_scale=1.0):
    """images [N][C][n][n] (CUDA fp32), entries as entries_by_class returns them (on the images' device) -> (avg fp32
    [K][C][n][n], wsum fp64 [K], counts int32 [K]): avg[k] = sum w_e A_e / sum w_e over the live entries of class k, A_e image
    img[e] resampled at the entry's pose; zeros for a class without weight."""
    what = 'weighted_class_averages'
    CL.require_f32(images, what, 'images')
    if images.dim() != 4 or images.shape[-1] != images.shape[-2]:
        raise TvaeHipError(f'{what}: images must be [N][C][n][n] (square), got {tuple(images.shape)}')
    N, C, n, _ = images.shape
    K = int(n_clusters)
    dev = images.device
    img, th, d, w, seg = (entries[k] for k in ('img', 'theta', 'dx', 'w', 'seg'))
    E = img.numel()
    for nm, t, dt, shape in (('img', img, torch.int32, (E,)), ('theta', th, torch.float32, (E,)), ('dx', d, torch.float32, (E, 2)),
                             ('w', w, torch.float32, (E,)), ('seg', seg, torch.int32, (K + 1,))):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise TvaeHipError(f'{what}: entries[{nm!r}] must be a contiguous {dt} tensor of shape {shape} on the images\' device')
    avg = torch.zeros(K, C, n, n, dtype=torch.float32, device=dev)
    wsum = torch.zeros(K, dtype=torch.float64, device=dev)
    counts = torch.zeros(K, dtype=torch.int32, device=dev)
    if E == 0:                                                # nothing to add: every class is empty
        if not 1 <= K <= CL.MAX_CLASSES:
            raise TvaeHipError(f'{what}: n_clusters = {K} outside [1, {CL.MAX_CLASSES}]')
        return avg, wsum, counts
    wsf = CL.query('tvae_class_average_weighted_ws_floats', E, K, C, n)
    if wsf <= 0:
        raise TvaeHipError(f'{what}: E={E}, K={K}, C={C}, n={n} outside the supported range or more than one launch covers')
    ws = CL.workspace(wsf, dev)
    with torch.cuda.device(dev):
        CL.call('tvae_class_average_weighted', images, img, th, d, w, seg, avg, wsum, counts, ws, wsf, N, E, C, n, K,
                float(t_scale))
    return avg, wsum, counts


# ---- the updates of a round: fp64 torch, any device ------------------------------------------------------------------------------
def update_sigma2(r2, live, C, n) -> float:
    """sigma^2 <- sum of r2 over the live images / (N_live C n^2), in fp64; NaN when no image is live."""
    r2, live = torch.as_tensor(r2).to(torch.float64), torch.as_tensor(live).to(torch.bool)
    n_live = int(live.sum())
    if n_live == 0:
        return float('nan')
    return float(r2[live].sum() / (n_live * int(C) * int(n) * int(n)))


def update_priors(wsum):
    """wsum fp64 [K] -> (pi fp64 [K], logprior fp64 [K]): pi_k = wsum_k / sum wsum; a class without weight gets log-prior
    -inf and so stays empty.  No weight at all: pi = 0 and logprior = -inf throughout."""
    w = torch.as_tensor(wsum).to(torch.float64)
    total = w.sum()
    pi = w / total if float(total) > 0 else torch.zeros_like(w)
    return pi, torch.where(pi > 0, torch.log(pi.clamp(min=torch.finfo(torch.float64).tiny)), torch.full_like(pi, -math.inf))


def log_likelihood(lse, live, C, n, sigma2, angle_steps, shift) -> float:
    """sum lse - N_live (C n^2 / 2) log(2 pi sigma^2) - N_live log(NA NS^2) over the live images, in fp64."""
    lse, live = torch.as_tensor(lse).to(torch.float64), torch.as_tensor(live).to(torch.bool)
    n_live = int(live.sum())
    poses = (2 * int(angle_steps) + 1) * (2 * int(shift) + 1) ** 2
    return float(lse[live].sum()) - n_live * (int(C) * int(n) * int(n) / 2.0) * math.log(2 * math.pi * float(sigma2)) \
        - n_live * math.log(poses)


def class_entropy(resp):
    """resp [N][M] -> fp64 [N]: -sum_m resp log resp, the entropy of every image's posterior over its slots."""
    r = torch.as_tensor(resp).to(torch.float64)
    return -(torch.where(r > 0, r * torch.log(r.clamp(min=torch.finfo(torch.float64).tiny)), torch.zeros_like(r))).sum(1)


def min_residuals(num, pp, yy, candidates, n_clusters):
    """The smallest live r_j = yy - 2 num_j + pp_j of every image in fp64 (+inf for an image with no live candidate)."""
    cand = torch.as_tensor(candidates).to(num.device)
    r = (yy.double()[:, None, None, None, None] - 2 * num.double()) + pp.double()
    ok = ((cand >= 0) & (cand < int(n_clusters)))[:, :, None, None, None] & torch.isfinite(r)
    return torch.where(ok, r, torch.full_like(r, math.inf)).reshape(r.shape[0], -1).amin(1)


def _slices(N, M, A, S):
    """Images per slice of the E-step: the tables of a slice stay within the workspace bound of tvae.refine."""
    per = 2 * M * (2 * A + 1) * (2 * S + 1) ** 2 + 1
    return CL.slice_step(N, CL.MAX_PLANES, refine.WS_FLOATS // per)


def raw_sum_squares(images, chunk=4096):
    """images [N][C][n][n] -> fp32 [N]: the fp64 sum of squares of every image, rounded to fp32 once (torch, slice by slice)."""
    N = images.shape[0]
    out = torch.empty(N, dtype=torch.float32, device=images.device)
    for i0 in range(0, N, chunk):
        out[i0:i0 + chunk] = images[i0:i0 + chunk].double().pow(2).reshape(min(chunk, N - i0), -1).sum(1).to(torch.float32)
    return out


def e_step(images, theta, dx, slots, refs, sigma2, logprior, keep, t_scale, A, step, S, mask_radius, mask_edge, ctf=None):
    """classify_poses(tables=True) -> pose_posteriors, slice by slice over the stack: the tables never exist for more than a
    slice.  -> the dict of pose_posteriors for the whole stack.  sigma2 None: only dict(rmin) is returned, the smallest live
    residual of every image.
    ctf = (coef [N][5] on the device, yy fp32 [N] of the RAW images): `images` is the stack filtered with H_i already, so num is
    <H_i (*) Y_i, P_j>; pp is tvae.ctf.template_power expanded over the NS^2 shifts and yy the raw images': the three tables of
    the residual |Y_i - H_i (*) P_j|^2."""
    N, n, K = images.shape[0], images.shape[-1], refs.shape[0]
    M = slots.shape[1]
    NS = 2 * S + 1
    stepN = _slices(N, M, A, S)
    parts = []
    for i0 in range(0, N, stepN):
        sl = slice(i0, min(i0 + stepN, N))
        num, pp, yy = classify.classify_poses(images[sl], theta[sl], dx[sl], slots[sl], refs, t_scale, A, step, S, mask_radius,
                                              mask_edge, tables=True)[5:]
        if ctf is not None:
            ppc = ctf_mod.template_power(theta[sl], dx[sl], slots[sl], refs, ctf[0][sl], t_scale, A, step, mask_radius, mask_edge)
            pp = ppc[:, :, :, None, None].expand(-1, -1, -1, NS, NS).contiguous()
            yy = ctf[1][sl].contiguous()
        if sigma2 is None:
            parts.append(dict(rmin=min_residuals(num, pp, yy, slots[sl], K)))
        else:
            parts.append(pose_posteriors(num, pp, yy, slots[sl], theta[sl], dx[sl], n, K, sigma2, logprior, keep, t_scale, A,
                                         step, S))
        del num, pp, yy
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def ml_rounds(images, theta, dx, labels, n_clusters=None, t_scale=1.0, rounds=3, angle_range=math.pi / 8, angle_steps=8,
              shift=2, mask_radius=None, mask_edge=0.0, keep=8, sigma2=None, latents=None, candidates=None,
              cross_halves=False, ctf=None, wiener_tau=0.1):
    """Expectation-maximisation over a fixed discrete set of poses.  The references start as the hard class averages of
    (labels, theta, dx); the pose grid stays centred on the INPUT poses in every round and the angle step angle_range /
    angle_steps is fixed.  Per round: candidate_lists of the current labels -> classify_poses(tables=True) ->
    pose_posteriors -> weighted_class_averages; then sigma^2 <- sum r2 / (N_live C n^2) and pi_k <- wsum_k / sum wsum (an empty
    class gets the log-prior -inf and stays empty).  sigma2 None starts from the mean over the images of the smallest live
    residual divided by C n^2, from the first round's tables: the tables exist slice by slice only, so that first round runs
    the tvae_pose_classify pass twice, once for the estimate and once for the posterior, and costs about two rounds (give
    sigma2 to avoid it).  cross_halves: the images are split by the parity of their
    position in their starting class, the M-step fills the two half-set averages and every image is scored against the half
    it is not in.
    ctf: coef rows [N][5] (tvae.ctf.coefficients) or None.  With them the model is Y_i = H_i (*) P_j + noise: the E-step takes
    num from the stack filtered with H_i (formed once), pp from tvae.ctf.template_power and yy from the raw images; the M-step is
    the Wiener form of tvae.ctf.class_averages_ctf with posterior weights, mean_k = weighted_class_averages of the filtered
    stack, D_k = tvae.ctf.power_weighted, G_k = 1 / (D_k / W_k + wiener_tau) in fp64 rounded once (zeros where W_k = 0) and the
    reference filter_stack(mean, planes=G); the start references are class_averages_ctf(..., 'wiener', wiener_tau).  The shift
    of a candidate enters num by windows of the extended template and pp circularly: the two agree exactly while the masked
    support moved by `shift` stays inside the frame.  history['ctf_power'] is then D [K][n][R] of the returned averages.
    ctf None: every line runs as without the argument.
    -> (avg fp32 [K][C][n][n], wsum fp64 [K], labels' int64 [N] = the arg-max of the slot posterior mapped through the
    candidates (ties to the lowest slot; an image with no live candidate keeps its label), theta' [N], dx' [N][2] the top-1
    poses, history): history['log_likelihood'], ['sigma2'] (the value each round's E-step used), ['kept'] per round,
    ['pi'] [rounds][K] after each round, ['sigma2_next'] and the last round's ['entropy'] fp64 [N], ['resp'],
    ['candidates'], ['posterior'] (the dict of pose_posteriors) and ['entries'] (that of entries_by_class)."""
    what = 'ml_rounds'
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, what)
    A, S, P = int(angle_steps), int(shift), int(keep)
    if int(rounds) < 1:
        raise TvaeHipError(f'{what}: rounds = {rounds} must be positive')
    if not 1 <= P <= MAX_KEEP:
        raise TvaeHipError(f'{what}: keep = {keep} outside [1, {MAX_KEEP}]')
    dev = images.device
    th0, d0 = theta.reshape(N).contiguous(), dx
    lab64 = lab.to(torch.int64)
    if latents is not None:
        latents = torch.as_tensor(latents).to(dev)
    step = float(angle_range) / max(A, 1)
    R = 2 * K if cross_halves else K                         # references: [half 0 | half 1] with cross_halves
    coef = tau = Dk = None
    scored, extra = images, None                              # what num is formed from, and the tables that replace pp and yy
    if ctf is not None:
        coef, tau = ctf_mod._coef_tensor(ctf, dev, what), float(wiener_tau)
        if coef.shape[0] != N:
            raise TvaeHipError(f'{what}: ctf must hold N = {N} rows, got {coef.shape[0]}')
        if not tau > 0:
            raise TvaeHipError(f'{what}: wiener_tau = {wiener_tau} must be positive')
        scored = ctf_mod.filter_stack(images, coef=coef, mode='multiply')
        extra = (coef, raw_sum_squares(images))
    if cross_halves:
        own = refine.cross_half_labels(lab64, K)
        half = ((own >= 0) & (own < K)).to(torch.int64)      # an image at an odd position of its class is in half 1
    if ctf is None:
        refs = refine.round_references(images, th0, d0, lab64, K, t_scale, cross_halves)
    elif cross_halves:                                        # the half-set split of refine.round_references: half h of class k
        inside = torch.where(own >= 0, (own + K) % (2 * K), own)          # is the label h K + k of the half the image is IN
        refs = ctf_mod.class_averages_ctf(images, th0, d0, inside, coef, R, t_scale, 'wiener', tau)[0]
    else:
        refs = ctf_mod.class_averages_ctf(images, th0, d0, lab64, coef, K, t_scale, 'wiener', tau)[0]

    def m_step(entries, classes):
        """-> (references [classes][C][n][n], wsum fp64 [classes], D or None)"""
        if ctf is None:
            avg_, wsum_, _ = weighted_class_averages(images, entries, classes, t_scale)
            return avg_, wsum_, None
        mean, wsum_, _ = weighted_class_averages(scored, entries, classes, t_scale)
        D, W, _ = ctf_mod.power_weighted(coef, entries, n, classes)
        Wc = W[:, None, None]
        G = torch.where(Wc > 0, 1.0 / (D / torch.where(Wc > 0, Wc, torch.ones_like(Wc)) + tau), torch.zeros_like(D))
        return ctf_mod.filter_stack(mean, planes=G.to(torch.float32).contiguous()), wsum_, D
    logprior = None
    s2 = None if sigma2 is None else float(np.float32(sigma2))
    hist = dict(log_likelihood=[], sigma2=[], kept=[], pi=[])
    cur = lab64
    post = cand = ent = None
    for _ in range(int(rounds)):
        cand = classify.candidate_lists(cur, K, latents, candidates)
        slots = classify.cross_half_candidates(lab64, cand, K) if cross_halves else cand
        if s2 is None:
            rmin = e_step(scored, th0, d0, slots, refs, None, None, P, t_scale, A, step, S, mask_radius, mask_edge,
                          extra)['rmin']
            ok = torch.isfinite(rmin)
            if not bool(ok.any()):
                raise TvaeHipError(f'{what}: no image has a live candidate: sigma2 cannot be estimated')
            s2 = float(np.float32(float(rmin[ok].mean() / (C * n * n))))     # the fp32 value the kernel gets
        lp = logprior if (logprior is None or not cross_halves) else torch.cat([logprior, logprior])
        post = e_step(scored, th0, d0, slots, refs, s2, lp, P, t_scale, A, step, S, mask_radius, mask_edge, extra)
        live = post['kept'] > 0
        cls = post['cls'].to(torch.int64)
        if cross_halves:                                      # an entry of class k goes to the half its image is in
            fill = torch.where(cls >= 0, cls % K + K * half[:, None], cls)
            ent = entries_by_class(fill, post['w'], post['theta'], post['dx'], R)
            refs, wsum2, Dk = m_step(ent, R)
            wsum = wsum2[:K] + wsum2[K:]
            cls = torch.where(cls >= 0, cls % K, cls)
        else:
            ent = entries_by_class(cls, post['w'], post['theta'], post['dx'], K)
            refs, wsum, Dk = m_step(ent, K)
        hist['log_likelihood'].append(log_likelihood(post['lse'], live, C, n, s2, A, S))
        hist['sigma2'].append(s2)
        hist['kept'].append(float(post['kept'][live].double().mean()) if bool(live.any()) else 0.0)
        pi, logprior = update_priors(wsum)
        hist['pi'].append(pi.cpu().numpy())
        new_s2 = update_sigma2(post['r2'], live, C, n)
        if np.isfinite(new_s2) and float(np.float32(new_s2)) > 0:
            s2 = float(np.float32(new_s2))
        top = torch.argmax(post['resp'], 1)                  # (the first of equal maxima: ties to the lowest slot)
        won = cand.to(dev)[torch.arange(N, device=dev), top]
        cur = torch.where(live, won, cur)
    if cross_halves:                                          # the averages of the whole classes from the last entries
        ent = entries_by_class(cls, post['w'], post['theta'], post['dx'], K)
        avg, wsum, Dk = m_step(ent, K)
    else:
        avg = refs
    hist = dict(log_likelihood=np.asarray(hist['log_likelihood']), sigma2=np.asarray(hist['sigma2']),
                kept=np.asarray(hist['kept']), pi=np.stack(hist['pi']), sigma2_next=s2, entropy=class_entropy(post['resp']),
                resp=post['resp'], candidates=cand, entries=ent, posterior=post)
    if ctf is not None:
        hist['ctf_power'] = Dk
    return avg, wsum, cur, post['theta'][:, 0].contiguous(), post['dx'][:, 0].contiguous(), hist


# ---- ml_class_averages.py: soft averages, labels and poses from the files a clustering run wrote -----------------------------
def build_parser(ctf=False) -> argparse.ArgumentParser:
    """ctf=True adds --ctf, --wiener-tau and --scale (what ml_class_averages.py parses; no --ctf-correct: the model fixes the
    correction); the default is the parser without them."""
    p = argparse.ArgumentParser('Maximum-likelihood 2-D class averages of a clustered stack: soft assignment over classes and poses')
    stack_cli.add_stack_flags(p)
    stack_cli.add_grid_flags(p)
    stack_cli.add_candidate_flags(p)
    p.add_argument('--keep', default=8, type=int, help='(class, pose) entries an image contributes to the averages (at most 64)')
    p.add_argument('--sigma2', default=None, type=float, help='noise variance per pixel of the first round; default: estimated '
                                                              'from the best residuals')
    if ctf:
        align.add_ctf_flags(p, ())
    return p


def save_outputs(out_dir, avg, wsum, labels, theta, dx, hist, particles, rot_shape):
    """class_weights.npy, clusters_ml.npy, rotations_ml.npy (in `rot_shape`, the shape of the rotations that came in),
    translations_ml.npy, ml_log_likelihood.npy, ml_sigma2.npy, ml_entropy.npy and class_averages_ml.npy (.mrcs, .jpg; the
    montage counts the members by the new labels): ml_class_averages.py and TVAE_ML_AVERAGES=1 write these; and
    class_ctf_power_ml.npy, the weighted per-class sums of H^2, when the rounds ran with a CTF.
    -> those counts, int [K]."""
    save = lambda name, a: np.save(os.path.join(out_dir, name), stack_cli.host(a))
    new, K = stack_cli.host(labels), avg.shape[0]
    save('class_weights.npy', wsum)
    save('clusters_ml.npy', new)
    save('ml_log_likelihood.npy', hist['log_likelihood'])
    save('ml_sigma2.npy', hist['sigma2'])
    save('ml_entropy.npy', hist['entropy'])
    if hist.get('ctf_power') is not None:
        save('class_ctf_power_ml.npy', hist['ctf_power'])
    counts = np.bincount(new[(new >= 0) & (new < K)], minlength=K)
    stack_cli.save_poses(out_dir, 'ml', theta, dx, avg, counts, particles, rot_shape)
    return counts


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters, t = inp.images, inp.theta, inp.dx, inp.clusters, inp.t_scale
    with stack_cli.hip_errors():
        coef = align.load_ctf_coefficients(args.ctf, images.shape[0], args.scale) if args.ctf else None
        K = align._check_labels(images, theta, dx, clusters, args.n_clusters, 'ml_rounds')[3]
        before = refine._resolutions(images, theta, dx, clusters, K, t)
        avg, wsum, lab, th, d, hist = ml_rounds(images, theta, dx, clusters, K, t, args.rounds, math.radians(args.angle_range),
                                                args.angle_steps, args.shift, args.mask_radius, args.mask_edge, args.keep,
                                                args.sigma2, inp.latents, args.candidates, args.cross_halves, coef,
                                                args.wiener_tau)
        after = refine._resolutions(images, th, d, lab.cpu().numpy(), K, t)
    os.makedirs(args.out_dir, exist_ok=True)
    counts = save_outputs(args.out_dir, avg, wsum, lab, th, d, hist, inp.particles, inp.rot_shape)
    was = np.bincount(clusters[(clusters >= 0) & (clusters < K)].astype(np.int64), minlength=K)
    stack_cli.print_resolution_table(before, after, was, counts)
    print('# maximum-likelihood averages of {} images in {} classes, {} rounds, log-likelihood {:.6e} -> {:.6e}, sigma2 {:.6e} '
          '-> {:.6e}: {}'.format(images.shape[0], K, args.rounds, hist['log_likelihood'][0], hist['log_likelihood'][-1],
                                 hist['sigma2'][0], hist['sigma2'][-1], args.out_dir), file=sys.stderr)
    return avg, wsum, lab, th, d, hist
