"""Aligned images and aligned 2-D class averages of a clustered stack on the GPU: the step after clustering_*.py, the
picture at the top of the reference's README.  Every image is resampled into the canonical frame with the rotation and
translation the encoder predicted for it, and the resampled images are averaged per cluster.

The pose convention is the model's (train_*.py: eval_minibatch; coordinates tvae.tables.image_coords): a pixel at
coordinate x shows canonical content at u = (x - t dx) R(theta), so the aligned image at the grid point u reads its
image at x = u R(theta)^T + t dx, bilinearly, with a zero border.  t is 1 where the translation was inferred by attention
and 0.1 for --t-inf unimodal (the reference's dx_scale, which get_latent does not apply to the dx it returns):
`translation_scale`.  include/tvae_cluster.h states the definition in full.

`class_halves` and `frc` measure the quality of the averages: the two half-set averages and the variance map of every
class in the same single pass, and the Fourier ring correlation of the halves (tvae.resolution turns it into a number).

The kernels are tvae_align_stack, tvae_class_average, tvae_class_halves and tvae_class_frc of libtvae_cluster.so.  The
class averages are fused: the aligned stack is never written, the stack is read once, there are no float atomics and the result is bitwise reproducible;
avg[k] depends on class k's members alone, not on the other classes or on the number of classes.  There is no CPU
fallback for the kernels; `segments` is torch code that does not care where its tensors live.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import stack_cli
from ._lib import TvaeHipError

MAX_IMAGES = CL.MAX_PLANES
MAX_CLUSTERS = CL.MAX_CLASSES


def translation_scale(t_inf: str) -> float:
    """Factor between the dx a clustering run saves and coordinate units."""
    if t_inf == 'attention':
        return 1.0
    if t_inf == 'unimodal':
        return 0.1
    raise ValueError(f"t_inf must be 'attention' or 'unimodal', got {t_inf!r}")


def segments(labels, n_clusters):
    """labels [N] (integers, any device) -> (order int32 [N], seg int32 [K + 1], counts int32 [K]): the image indices
    grouped by class, ascending index within a class (a stable sort on the labels' device); class k is
    order[seg[k]:seg[k + 1]].  Labels outside [0, K) go to no class: their indices sit behind seg[K]."""
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise TvaeHipError('segments: labels must be a one-dimensional integer array')
    K = int(n_clusters)
    if K < 1:
        raise TvaeHipError(f'segments: n_clusters = {K} must be positive')
    lab = lab.to(torch.int64)
    key = torch.where((lab >= 0) & (lab < K), lab, torch.full_like(lab, K))
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=K + 1)[:K]
    seg = torch.zeros(K + 1, dtype=torch.int64, device=lab.device)
    seg[1:] = torch.cumsum(counts, 0)
    return order.to(torch.int32), seg.to(torch.int32), counts.to(torch.int32)


def _check_stack(images, theta, dx, what):
    for nm, t in (('images', images), ('theta', theta), ('dx', dx)):
        CL.require_f32(t, what, nm)
    if images.dim() != 4 or images.shape[-1] != images.shape[-2]:
        raise TvaeHipError(f'{what}: images must be [N][C][n][n] (square), got {tuple(images.shape)}')
    N, C, n, _ = images.shape
    if not (1 <= N <= MAX_IMAGES and 1 <= C <= 1024 and 2 <= n <= CL.MAX_SIDE):
        raise TvaeHipError(f'{what}: N={N}, C={C}, n={n} outside the supported range '
                           '(1 <= N <= 2^24, 1 <= C <= 1024, 2 <= n <= 1024)')
    if theta.numel() != N or theta.dim() > 2 or tuple(dx.shape) != (N, 2):
        raise TvaeHipError(f'{what}: theta must hold N = {N} angles and dx must be [N][2], got {tuple(theta.shape)} '
                           f'and {tuple(dx.shape)}')
    if theta.device != images.device or dx.device != images.device:
        raise TvaeHipError(f'{what}: images, theta and dx must live on one device')
    return N, C, n


def align_stack(images, theta, dx, t_scale=1.0):
    """images [N][C][n][n], theta [N] or [N][1], dx [N][2] (CUDA fp32) -> the aligned images, same shape."""
    N, C, n = _check_stack(images, theta, dx, 'align_stack')
    out = torch.empty_like(images)
    with torch.cuda.device(images.device):
        CL.call('tvae_align_stack', images, theta.reshape(N), dx, out, N, C, n, float(t_scale))
    return out


def chunk_members(N, K, C, n) -> int:
    """Members of a class per partial sum of tvae_class_average (0 for unsupported arguments)."""
    return CL.query('tvae_class_average_chunk', N, K, C, n)


def class_averages(images, theta, dx, labels, n_clusters=None, t_scale=1.0):
    """-> (avg fp32 [K][C][n][n], counts int32 [K]) on the device of `images`: avg[k] is the mean of the aligned images
    with label k (zeros for an empty class).  labels: [N] integers on any device or a numpy array; a label outside
    [0, K) belongs to no class.  n_clusters None: the largest label + 1."""
    N, C, n, K, lab = _check_labels(images, theta, dx, labels, n_clusters, 'class_averages')
    order, seg, counts = segments(lab, K)
    wsf = CL.query('tvae_class_average_ws_floats', N, K, C, n)
    if wsf <= 0:
        raise TvaeHipError(f'class_averages: N={N}, K={K}, C={C}, n={n} is more than one launch covers')
    avg = torch.empty(K, C, n, n, dtype=torch.float32, device=images.device)
    ws = torch.empty(wsf, dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        CL.call('tvae_class_average', images, theta.reshape(N), dx, order, seg, avg, ws, wsf, N, C, n, K, float(t_scale))
    return avg, counts


def _check_labels(images, theta, dx, labels, n_clusters, what):
    N, C, n = _check_stack(images, theta, dx, what)
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.numel() != N:
        raise TvaeHipError(f'{what}: labels must hold N = {N} entries, got {tuple(lab.shape)}')
    lab = lab.to(images.device)
    K = int(n_clusters) if n_clusters is not None else int(lab.max()) + 1
    if not 1 <= K <= MAX_CLUSTERS:
        raise TvaeHipError(f'{what}: n_clusters = {K} outside [1, {MAX_CLUSTERS}]')
    return N, C, n, K, lab


def class_halves(images, theta, dx, labels, n_clusters=None, t_scale=1.0):
    """-> (avg fp32 [K][C][n][n], halves fp32 [2][K][C][n][n], var fp32 [K][C][n][n], counts int32 [K][2]) on the device of
    `images`, in ONE pass over the stack (tvae_class_halves): the members of a class in ascending image index go
    alternately to half 0 and half 1, halves[h][k] is the mean of the aligned images of half h, avg[k] that of the whole
    class and var[k] its per-pixel sample variance (sum-of-squares form, 0 for fewer than two members).  Arguments and
    checks as class_averages.  avg agrees with class_averages to rounding, not bit for bit.  Both halves share one encoder
    and one set of poses: a ring correlation of them is not a gold-standard one and reads optimistic."""
    N, C, n, K, lab = _check_labels(images, theta, dx, labels, n_clusters, 'class_halves')
    order, seg, _ = segments(lab, K)
    wsf = CL.query('tvae_class_halves_ws_floats', N, K, C, n)
    if wsf <= 0:
        raise TvaeHipError(f'class_halves: N={N}, K={K}, C={C}, n={n} is more than one launch covers')
    dev = images.device
    avg = torch.empty(K, C, n, n, dtype=torch.float32, device=dev)
    halves = torch.empty(2, K, C, n, n, dtype=torch.float32, device=dev)
    var = torch.empty(K, C, n, n, dtype=torch.float32, device=dev)
    counts = torch.empty(K, 2, dtype=torch.int32, device=dev)
    ws = torch.empty(wsf, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        CL.call('tvae_class_halves', images, theta.reshape(N), dx, order, seg, avg, halves, var, counts, ws, wsf, N, C, n, K,
                float(t_scale))
    return avg, halves, var, counts


FRC_WS_FLOATS = 1 << 26           # workspace of one tvae_class_frc call: 256 MB


def frc(a, b, mask_radius=None, mask_edge=0.0):
    """a, b [...][n][n] (CUDA fp32, equal shapes) -> (frc fp32 [...][R], sums fp64 [...][R][3]), R = n // 2 + 1: the Fourier
    ring correlation of every pair of planes under the soft circular mask (mask_radius None or <= 0: no mask) and the ring
    sums (Re(Fa conj Fb), |Fa|^2, |Fb|^2) it is the ratio of.  include/tvae_cluster.h states the definition."""
    for nm, t in (('a', a), ('b', b)):
        CL.require_f32(t, 'frc', nm)
    if a.shape != b.shape or a.device != b.device or a.dim() < 2 or a.shape[-1] != a.shape[-2]:
        raise TvaeHipError(f'frc: a and b must be [...][n][n] of one shape on one device, got {tuple(a.shape)} and '
                           f'{tuple(b.shape)}')
    n = a.shape[-1]
    R = CL.query('tvae_frc_rings', n)
    P = a.numel() // (n * n) if n else 0
    if R <= 0 or P < 1:
        raise TvaeHipError(f'frc: n={n} with {P} planes outside the supported range (2 <= n <= 1024, at least one plane)')
    radius = 0.0 if mask_radius is None else float(mask_radius)
    edge = float(mask_edge)
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'frc: mask_radius = {mask_radius} and mask_edge = {mask_edge} must be finite, the edge not negative')
    lead = tuple(a.shape[:-2])
    a2, b2 = a.reshape(P, n, n), b.reshape(P, n, n)
    out = torch.empty(P, R, dtype=torch.float32, device=a.device)
    sums = torch.empty(P, R, 3, dtype=torch.float64, device=a.device)
    # Planes are independent and a plane's workgroups, addition order and twiddles depend on n alone, so a call on a slice
    # of the planes cannot change a bit of any plane's result: the slices only bound the workspace.
    per = CL.query('tvae_class_frc_ws_floats', 1, n)
    step = CL.slice_step(P, 65535, FRC_WS_FLOATS // per)    # (65535: the planes are the y dimension of the launch grids)
    wsf = CL.query('tvae_class_frc_ws_floats', step, n)
    ws = CL.workspace(wsf, a.device)
    with torch.cuda.device(a.device):
        for p0 in range(0, P, step):
            p1 = min(p0 + step, P)
            CL.call('tvae_class_frc', a2[p0:p1], b2[p0:p1], out[p0:p1], sums[p0:p1], ws, wsf, p1 - p0, n, radius, edge)
    return out.reshape(lead + (R,)), sums.reshape(lead + (R, 3))


def save_outputs(out_dir, avg, counts, particles=False, stem='class_averages'):
    """class_averages.npy ([K][C][n][n]) and class_counts.npy; class_averages.mrcs ([K * C][n][n]) for particles; the
    montage class_averages.jpg when matplotlib is present (stderr says so when it is not).  Another `stem` (the
    CTF-corrected averages, class_averages_ctf) names the three files and leaves class_counts.npy alone."""
    from . import figures
    avg, counts = np.asarray(avg, dtype=np.float32), np.asarray(counts)
    np.save(os.path.join(out_dir, stem + '.npy'), avg)
    if stem == 'class_averages':
        np.save(os.path.join(out_dir, 'class_counts.npy'), counts)
    if particles:
        from src import mrc
        with open(os.path.join(out_dir, stem + '.mrcs'), 'wb') as f:
            mrc.write(f, avg.reshape(-1, avg.shape[-2], avg.shape[-1]))
    try:
        figures._plt()
    except ImportError as e:
        print('# matplotlib is not available ({}): {}.jpg is skipped'.format(e, stem), file=sys.stderr)
        return
    figures.save_class_averages(out_dir, avg, counts, stem + '.jpg')


# ---- class_averages.py: the averages from the files a clustering run wrote ------------------------------------------------
def add_ctf_flags(p, corrections, wiener=True):
    """--ctf, --ctf-correct and --scale (and --wiener-tau): the CTF correction of class_averages.py and class_resolution.py.
    Empty `corrections`: no --ctf-correct (ml_class_averages.py, whose model fixes the correction)."""
    p.add_argument('--ctf', default=None, help='CTF parameters, one row per image (the eight-column table of training): '
                                               'also write the CTF-corrected results')
    if corrections:
        p.add_argument('--ctf-correct', default=corrections[0], choices=list(corrections), help='phase flipping or Wiener weights')
    if wiener:
        p.add_argument('--wiener-tau', default=0.1, type=float, help='regularisation of the Wiener weights, 1 / SNR')
    p.add_argument('--scale', default=1, type=float, help='downsampling factor of the stack against the pixel size in --ctf')


def load_ctf_coefficients(path, n_images, scale=1):
    """The rows of --ctf as tvae.ctf.coefficients (fp64 [N][5]); one row per image is required."""
    from src import ctf as C
    from . import ctf
    table = C.parse_ctf(path)
    if len(table) != n_images:
        raise SystemExit(f'--ctf holds {len(table)} rows for {n_images} images: one row per image is required')
    return ctf.coefficients(table, scale=scale)


def build_parser(ctf=False) -> argparse.ArgumentParser:
    """ctf=True adds the CTF flags (what class_averages.py parses); the default is the parser without them."""
    p = argparse.ArgumentParser('Aligned 2-D class averages of a clustered stack')
    stack_cli.add_stack_flags(p, own=lambda q: q.add_argument('--write-aligned', action='store_true',
                                                              help='also write the aligned images, aligned.npy'))
    if ctf:
        add_ctf_flags(p, ('wiener', 'flip'))
    return p


def load_stack(path, crop=0):
    """-> float32 [N][C][n][m] on the host."""
    if path.endswith('mrc') or path.endswith('mrcs'):
        from src import mrc
        a = np.asarray(mrc.open_stack(path)[0], dtype=np.float32)
    else:
        a = np.asarray(np.load(path), dtype=np.float32)
    if a.ndim == 3:
        a = a[:, None]
    if a.ndim != 4:
        raise SystemExit(f'--stack must hold [N][n][n] or [N][C][n][n], got {a.shape}')
    if crop > 0:
        si, sj = (a.shape[-2] - crop) // 2, (a.shape[-1] - crop) // 2
        a = a[..., si:si + crop, sj:sj + crop]
    return np.ascontiguousarray(a)


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters, particles, t = inp.images, inp.theta, inp.dx, inp.clusters, inp.particles, inp.t_scale
    with stack_cli.hip_errors():
        avg, counts = class_averages(images, theta, dx, clusters, args.n_clusters, t)
        aligned = align_stack(images, theta, dx, t) if args.write_aligned else None
        corrected = None
        if args.ctf:
            from . import ctf
            coef = load_ctf_coefficients(args.ctf, images.shape[0], args.scale)
            corrected = ctf.class_averages_ctf(images, theta, dx, clusters, coef, args.n_clusters, t, args.ctf_correct,
                                               args.wiener_tau)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, avg.cpu().numpy(), counts.cpu().numpy(), particles)
    if corrected is not None:
        save_outputs(args.out_dir, corrected[0].cpu().numpy(), corrected[1].cpu().numpy(), particles, 'class_averages_ctf')
        np.save(os.path.join(args.out_dir, 'class_ctf_power.npy'), corrected[2].cpu().numpy())
    if aligned is not None:
        np.save(os.path.join(args.out_dir, 'aligned.npy'), aligned.cpu().numpy())
    print('# class averages of {} images in {} classes: {}'.format(images.shape[0], avg.shape[0], args.out_dir),
          file=sys.stderr)
    return avg, counts
