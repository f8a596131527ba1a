"""Eigenimages of the aligned classes (multivariate statistical analysis): the leading principal components of the aligned,
mean-subtracted members of every class, each particle's coordinates along them and its residual norm -- how the members of
a class differ from their average, where tvae.resolution's variance map only shows where.  The step after
class_averages.py / class_resolution.py: a class that mixes views shows it in its first eigenimage, tvae.cluster.kmeans on
the coordinates splits it, and the residual norm finds the junk.

With d_q = m * (A_q - mean[k]) the masked residual of member q of class k (A_q its aligned image, tvae.align) and R_k the
matrix whose rows are the d_q, the eigenimages are the leading eigenvectors of R_k^T R_k / (m_k - 1).  The aligned stack is
never written: tvae_class_project computes R V and tvae_class_backproject R^T (R V) for a block of vectors per class, each in
one streaming pass over the stack (include/tvae_cluster.h states both), and `class_eigenimages` runs a randomized subspace
iteration around them.  The L x L algebra is fp64; its eigendecompositions run on the host (they are tiny, and no batched
solver of the torch build is relied on).  There is no CPU fallback for the kernels.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import align, resolution, stack_cli
from ._lib import TvaeHipError

MAX_COMPONENTS = 16                # TVAE_EIGEN_MAX_COMPONENTS
RANK_FLOOR = 2.0 ** -40            # a direction whose Gram eigenvalue is below this share of the largest is dropped


def chunk_members(N, K, C, n, J) -> int:
    """Members of a class per partial sum of tvae_class_backproject (0 for unsupported arguments)."""
    return CL.query('tvae_class_eigen_chunk', N, K, C, n, J)


def _mask(radius, edge, what):
    radius = 0.0 if radius is None else float(radius)
    edge = float(edge)
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'{what}: mask_radius = {radius} and mask_edge = {edge} must be finite, the edge not negative')
    return radius, edge


def _check(images, theta, dx, order, seg, mean, block, last, what):
    """Shapes, dtypes and devices of one call; `block` is V [K][J][C][n][n] (last = None) or coef [N][J] (last = 'coef')."""
    N, C, n = align._check_stack(images, theta, dx, what)
    dev = images.device
    for nm, t in (('order', order), ('seg', seg)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1):
            raise TvaeHipError(f'{what}: {nm} must be a one-dimensional contiguous CUDA int32 tensor (no CPU fallback)')
    CL.require_f32(mean, what, 'mean')
    CL.require_f32(block, what, 'coef' if last else 'V')
    K = seg.numel() - 1
    if order.numel() != N or not 1 <= K <= align.MAX_CLUSTERS:
        raise TvaeHipError(f'{what}: order must hold N = {N} entries and seg K + 1 boundaries with 1 <= K <= '
                           f'{align.MAX_CLUSTERS}, got {order.numel()} and {seg.numel()}')
    if tuple(mean.shape) != (K, C, n, n):
        raise TvaeHipError(f'{what}: mean must be [K][C][n][n] = {(K, C, n, n)}, got {tuple(mean.shape)}')
    if last:
        if block.dim() != 2 or block.shape[0] != N:
            raise TvaeHipError(f'{what}: coef must be [N][J] with N = {N}, got {tuple(block.shape)}')
        J = block.shape[1]
    else:
        if block.dim() != 5 or block.shape[0] != K or tuple(block.shape[2:]) != (C, n, n):
            raise TvaeHipError(f'{what}: V must be [K][J][C][n][n] with K, C, n = {(K, C, n)}, got {tuple(block.shape)}')
        J = block.shape[1]
    if not 1 <= J <= MAX_COMPONENTS:
        raise TvaeHipError(f'{what}: J = {J} outside [1, {MAX_COMPONENTS}]')
    for t in (order, seg, mean, block):
        if t.device != dev:
            raise TvaeHipError(f'{what}: every tensor must live on the device of images')
    return N, C, n, K, J


def project(images, theta, dx, order, seg, mean, V, t_scale=1.0, mask_radius=None, mask_edge=0.0):
    """-> (coef fp32 [N][J], norm2 fp32 [N]), rows by POSITION in `order`: the inner products of every member's masked
    residual against mean[k] with the J vectors V[k] of its class, and the residual's squared norm (tvae_class_project).
    order, seg: int32 on the device, as tvae.align.segments returns them.  mask_radius None or <= 0: no mask."""
    N, C, n, K, J = _check(images, theta, dx, order, seg, mean, V, None, 'project')
    radius, edge = _mask(mask_radius, mask_edge, 'project')
    wsf = CL.query('tvae_class_project_ws_floats', N, K, C, n, J)
    if wsf <= 0:
        raise TvaeHipError(f'project: N={N}, K={K}, C={C}, n={n}, J={J} is more than one launch covers')
    coef = torch.empty(N, J, dtype=torch.float32, device=images.device)
    norm2 = torch.empty(N, dtype=torch.float32, device=images.device)
    ws = CL.workspace(wsf, images.device)
    with torch.cuda.device(images.device):
        CL.call('tvae_class_project', images, theta.reshape(N), dx, order, seg, mean, V, coef, norm2, ws, wsf, N, C, n, K, J,
                float(t_scale), radius, edge)
    return coef, norm2


def backproject(images, theta, dx, order, seg, mean, coef, t_scale=1.0, mask_radius=None, mask_edge=0.0):
    """-> (W fp32 [K][J][C][n][n], counts int32 [K]): W[k][j] = the sum over the members q of class k of coef[q][j] times the
    member's masked residual (tvae_class_backproject); coef [N][J] by position in `order`, as `project` returns it."""
    N, C, n, K, J = _check(images, theta, dx, order, seg, mean, coef, 'coef', 'backproject')
    radius, edge = _mask(mask_radius, mask_edge, 'backproject')
    wsf = CL.query('tvae_class_backproject_ws_floats', N, K, C, n, J)
    if wsf <= 0:
        raise TvaeHipError(f'backproject: N={N}, K={K}, C={C}, n={n}, J={J} is more than one launch covers')
    W = torch.empty(K, J, C, n, n, dtype=torch.float32, device=images.device)
    counts = torch.empty(K, dtype=torch.int32, device=images.device)
    ws = CL.workspace(wsf, images.device)
    with torch.cuda.device(images.device):
        CL.call('tvae_class_backproject', images, theta.reshape(N), dx, order, seg, mean, coef, W, counts, ws, wsf, N, C, n,
                K, J, float(t_scale), radius, edge)
    return W, counts


def orthonormalise(W):
    """W [K][L][P] -> (Q fp64 [K][L][P], rank [K] numpy): per class an orthonormal basis of the rows' span, the rows of Q in
    descending order of the Gram eigenvalue they came from and exact zeros behind the rank.  Gram-based in fp64, applied twice
    (the second pass removes what the first one's conditioning left); a direction whose Gram eigenvalue is below 2^-40 of the
    class's largest, and everything of a class whose Gram matrix is zero or not finite, becomes a zero vector."""
    Q = W.to(torch.float64)
    K, L, _ = Q.shape
    rank = np.zeros(K, dtype=np.int64)
    for _ in range(2):
        G = torch.bmm(Q, Q.transpose(1, 2)).cpu().numpy()
        ok = np.isfinite(G).all(axis=(1, 2))
        e, U = np.linalg.eigh(np.where(ok[:, None, None], G, 0.0))
        e, U = e[:, ::-1], U[:, :, ::-1]                               # descending
        keep = (e > e[:, :1] * RANK_FLOOR) & (e > 0) & ok[:, None]
        scale = np.where(keep, 1.0 / np.sqrt(np.where(keep, e, 1.0)), 0.0)
        M = np.ascontiguousarray((U * scale[:, None, :]).transpose(0, 2, 1))      # row i = u_i^T / sqrt(e_i)
        if not ok.all():                                               # (0 * NaN is NaN: such a class becomes zeros here)
            Q = torch.where(torch.from_numpy(ok).to(Q.device)[:, None, None], Q, torch.zeros_like(Q))
        Q = torch.bmm(torch.from_numpy(M).to(Q.device), Q)
        rank = keep.sum(1)
    return Q, rank


def class_eigenimages(images, theta, dx, labels, n_clusters=None, components=4, oversample=4, power_iterations=2,
                      t_scale=1.0, mean=None, mask_radius=None, mask_edge=None, seed=0):
    """-> dict of device tensors:
        eigenimages [K][J][C][n][n] fp32   unit norm, the entry of largest magnitude (lowest index at ties) positive
        eigenvalues [K][J] fp64            descending: the variance of the class along each eigenimage
        total_variance [K] fp64            sum of the members' squared residual norms / (m - 1)
        coordinates [N][J] fp32            of every image along the eigenimages of its class (NaN for an image in no class)
        residual [N] fp32                  squared norm of what the J eigenimages leave, clamped at 0 (NaN likewise)
        counts [K] int32, mean [K][C][n][n], mask_radius, mask_edge
    J = components.  Randomized subspace iteration on L = components + oversample <= 16 vectors per class: a Gaussian start
    from a CPU generator seeded with `seed`, (power_iterations + 1) times project, backproject and `orthonormalise`, then a
    final projection and Rayleigh-Ritz on T = coef^T coef / (m - 1) in fp64.  mean None: tvae.align.class_averages of the
    same poses.  The mask defaults are tvae.resolution.default_mask.  A class of fewer than two members gives zeros; where the
    rank is below J the trailing eigenimages and eigenvalues are exact zeros."""
    what = 'class_eigenimages'
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, what)
    J, L = int(components), int(components) + int(oversample)
    if J < 1 or int(oversample) < 0 or L > MAX_COMPONENTS or int(power_iterations) < 0:
        raise TvaeHipError(f'{what}: components = {components} (>= 1) plus oversample = {oversample} (>= 0) must be at most '
                           f'{MAX_COMPONENTS}, power_iterations = {power_iterations} not negative')
    dev = images.device
    radius, edge = resolution.default_mask(n, mask_radius, mask_edge)
    radius, edge = _mask(radius, edge, what)
    order, seg, counts = align.segments(lab, K)
    if mean is None:
        mean, _ = align.class_averages(images, theta, dx, lab, K, t_scale)
    th = theta.reshape(N)
    gen = torch.Generator().manual_seed(int(seed))
    V = torch.randn(K, L, C, n, n, generator=gen, dtype=torch.float32).to(dev)
    P = C * n * n
    Q = rank = None
    for _ in range(int(power_iterations) + 1):
        coef, _ = project(images, th, dx, order, seg, mean, V, t_scale, radius, edge)
        W, _ = backproject(images, th, dx, order, seg, mean, coef, t_scale, radius, edge)
        Q, rank = orthonormalise(W.reshape(K, L, P))
        V = Q.to(torch.float32).reshape(K, L, C, n, n).contiguous()
    coef, norm2 = project(images, th, dx, order, seg, mean, V, t_scale, radius, edge)

    # Rayleigh-Ritz per class, within the class's own rank: the directions behind it stay exact zeros with eigenvalue 0
    bounds, m = seg.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)
    live = [k for k in range(K) if m[k] >= 2 and rank[k] > 0]
    T = torch.zeros(K, L, L, dtype=torch.float64, device=dev)
    total = torch.zeros(K, dtype=torch.float64, device=dev)
    for k in live:
        c = coef[bounds[k]:bounds[k + 1]].to(torch.float64)
        T[k] = (c.t() @ c) / (m[k] - 1)
        total[k] = norm2[bounds[k]:bounds[k + 1]].to(torch.float64).sum() / (m[k] - 1)
    Th = T.cpu().numpy()
    rot = np.zeros((K, L, L))
    lam = np.zeros((K, L))
    for k in live:
        r = int(rank[k])
        if not np.isfinite(Th[k]).all():
            lam[k] = np.nan
            continue
        e, U = np.linalg.eigh(Th[k, :r, :r])
        rot[k, :r, :r] = U[:, ::-1]
        lam[k, :r] = np.maximum(e[::-1], 0.0)
    rot_d = torch.from_numpy(rot).to(dev)
    E = torch.bmm(rot_d.transpose(1, 2), Q)[:, :J]                     # [K][J][P] fp64, orthonormal rows or zeros
    top = E.abs().amax(-1, keepdim=True)
    at = torch.where(E.abs() == top, torch.arange(P, device=dev), P).amin(-1, keepdim=True).clamp_(max=P - 1)
    sign = torch.where(torch.gather(E, 2, at) < 0, -1.0, 1.0)         # [K][J][1]
    E = E * sign
    coords = torch.full((N, J), float('nan'), dtype=torch.float32, device=dev)
    resid = torch.full((N,), float('nan'), dtype=torch.float32, device=dev)
    who = order.to(torch.int64)
    for k in range(K):
        s, e = int(bounds[k]), int(bounds[k + 1])
        if e <= s:
            continue
        y = (coef[s:e].to(torch.float64) @ rot_d[k])[:, :J] * sign[k, :, 0]
        coords[who[s:e]] = y.to(torch.float32)
        resid[who[s:e]] = (norm2[s:e].to(torch.float64) - (y * y).sum(1)).clamp_(min=0).to(torch.float32)
    return dict(eigenimages=E.to(torch.float32).reshape(K, J, C, n, n), eigenvalues=torch.from_numpy(lam[:, :J].copy()).to(dev),
                total_variance=total, coordinates=coords, residual=resid, counts=counts.to(dev), mean=mean,
                mask_radius=radius, mask_edge=edge)


def save_outputs(out_dir, res, particles=False):
    """class_eigenimages.npy ([K][J][C][n][n]; .mrcs for particles), class_eigenvalues.npy, eigen_coordinates.npy,
    eigen_residual.npy and class_eigen.txt (one line per class: members, total variance and the share of it every component
    explains); class_eigenimages.jpg when matplotlib is present (stderr says so when it is not)."""
    from . import figures
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}
    eig, lam, total, counts = host['eigenimages'], host['eigenvalues'], host['total_variance'], host['counts']
    np.save(os.path.join(out_dir, 'class_eigenimages.npy'), eig)
    np.save(os.path.join(out_dir, 'class_eigenvalues.npy'), lam)
    np.save(os.path.join(out_dir, 'eigen_coordinates.npy'), host['coordinates'])
    np.save(os.path.join(out_dir, 'eigen_residual.npy'), host['residual'])
    if particles:
        from src import mrc
        with open(os.path.join(out_dir, 'class_eigenimages.mrcs'), 'wb') as f:
            mrc.write(f, eig.reshape(-1, eig.shape[-2], eig.shape[-1]))
    with open(os.path.join(out_dir, 'class_eigen.txt'), 'w') as f:
        f.write('# n = {}, mask radius {:g} and edge {:g} pixels\n'.format(eig.shape[-1], host['mask_radius'], host['mask_edge']))
        f.write('# class  members  total_variance  explained share of components 0 .. {}\n'.format(lam.shape[1] - 1))
        for k in range(lam.shape[0]):
            share = lam[k] / total[k] if total[k] > 0 else np.zeros_like(lam[k])
            f.write('{} {} {:.6g} {}\n'.format(k, int(counts[k]), total[k], ' '.join('{:.4f}'.format(s) for s in share)))
    try:
        figures._plt()
    except ImportError as e:
        print('# matplotlib is not available ({}): class_eigenimages.jpg is skipped'.format(e), file=sys.stderr)
        return
    figures.save_class_eigenimages(out_dir, eig, lam, counts)


# ---- class_eigenimages.py: the same from the files a clustering run wrote -------------------------------------------------
def build_parser(ctf=False) -> argparse.ArgumentParser:
    """The flags of class_resolution.py that mean something here (not --apix and --threshold) and those of the iteration;
    ctf=True adds --ctf, --ctf-correct flip and --scale (what class_eigenimages.py parses)."""
    p = argparse.ArgumentParser('Eigenimages of the aligned 2-D classes, particle coordinates and residual norms')

    def own(q):
        stack_cli.add_mask_flags(q, resolution.MASK_EDGE, 'default (n - 1) / 2 - 4')
        q.add_argument('--components', default=4, type=int, help='eigenimages per class')
        q.add_argument('--oversample', default=4, type=int,
                       help='extra vectors of the subspace iteration (components + oversample <= 16)')
        q.add_argument('--power-iterations', default=2, type=int, help='passes of the subspace iteration after the first')
        q.add_argument('--seed', default=0, type=int, help='seed of the Gaussian start')

    stack_cli.add_stack_flags(p, 'where the .npy files, class_eigen.txt and the figure go', own)
    if ctf:
        align.add_ctf_flags(p, ('flip',), wiener=False)
    return p


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters = inp.images, inp.theta, inp.dx, inp.clusters
    with stack_cli.hip_errors():
        if args.ctf:
            # phase-flipped in place, in the chunks of tvae.ctf.filter_stack: the averages and the residuals are those of the
            # corrected stack
            from . import ctf
            coef = align.load_ctf_coefficients(args.ctf, images.shape[0], args.scale)
            ctf.filter_stack(images, coef=coef, mode='flip', inplace=True)
        res = class_eigenimages(images, theta, dx, clusters, args.n_clusters, args.components, args.oversample,
                                args.power_iterations, inp.t_scale, None, args.mask_radius, args.mask_edge, args.seed)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, res, inp.particles)
    print('# class eigenimages of {} images in {} classes, {} components: {}'.format(
        images.shape[0], res['eigenvalues'].shape[0], res['eigenvalues'].shape[1], args.out_dir), file=sys.stderr)
    return res
