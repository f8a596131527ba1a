"""Radial spectra on the GPU: the windowed ring power of every image of a stack (a noise model), whitening with the radial
profile of an image's group, and the filtering of class averages to their FRC.

The likelihood of tvae.ml2d and the cosine scores of the pose tools assume white noise; cryo-EM noise has a steep radial
spectrum.  `whiten` estimates the radial noise power from the background of the particles (outside a soft disc), per group
(micrograph, defocus group) where groups are given, and divides every image's spectrum by its square root, so that the
background of the result is white with the variance it had on average.  `filter_averages` turns the FRC curves of
tvae.resolution into the filter a user applies first: the weight sqrt(2 FRC / (1 + FRC)) or a hard low-pass at the crossing.

include/tvae_cluster.h (section "Radial spectra") states the definitions; the kernels are tvae_ring_power,
tvae_ring_power_groups and tvae_radial_filter of libtvae_cluster.so: the direct DFT of tvae.ctf (any n, no spectrum in
memory up to n = 128, no atomics, a plane's result independent of the batch), rings by the exact integer rule of the FRC,
extended over the corners of the plane.  There is no CPU fallback; `ring_counts`, `window`, `whitening_profile` and
`frc_profile` are host arithmetic in fp64.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import stack_cli
from ._lib import TvaeHipError

WS_FLOATS = 1 << 26               # bound of the workspace of one call: 256 MB
INTERP = {'nearest': 0, 'linear': 1, 0: 0, 1: 1}
FLOOR = 1e-3


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------
def radial_rings(n) -> int:
    """Rings of the whole n x n plane, 1 + ring(n // 2, n // 2): 92 for n = 128, 46 for n = 64."""
    Rr = CL.query('tvae_radial_rings', int(n))
    if Rr <= 0:
        raise TvaeHipError(f'radial_rings: n = {n} outside the supported range (2 <= n <= 1024)')
    return Rr


def ring_table(n):
    """int64 [n][n]: the ring of every coefficient of the full plane in numpy's fftfreq order, by the integer rule
    (2r - 1)^2 <= 4 (ky^2 + kx^2) < (2r + 1)^2."""
    k = np.rint(np.fft.fftfreq(int(n)) * int(n)).astype(np.int64)
    s4 = 4 * (k[:, None] ** 2 + k[None, :] ** 2)
    q = np.floor(np.sqrt(s4.astype(np.float64))).astype(np.int64)         # floor(sqrt(s4)), made exact in integers
    q -= q * q > s4
    q += (q + 1) ** 2 <= s4
    return (q + 1) // 2                                                   # 2r - 1 <= q < 2r + 1


def ring_counts(n):
    """fp64 [Rr]: the number of coefficients of the full plane on every ring (they sum to n^2)."""
    return np.bincount(ring_table(n).reshape(-1)).astype(np.float64)


def window(n, mask_radius=None, mask_edge=0.0, background=True):
    """fp64 [n][n]: the window of tvae_ring_power.  m = 1 within mask_radius of ((n - 1) / 2, (n - 1) / 2), a raised cosine
    over mask_edge, 0 beyond; w = 1 - m for the background, m otherwise; no mask (None or <= 0) is 1 everywhere."""
    n = int(n)
    radius = 0.0 if mask_radius is None else float(np.float32(mask_radius))
    edge = float(np.float32(mask_edge))
    if not radius > 0:
        return np.ones((n, n))
    c = 0.5 * (n - 1)
    d = np.sqrt((np.arange(n)[:, None] - c) ** 2 + (np.arange(n)[None, :] - c) ** 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        soft = 0.5 * (1.0 + np.cos(np.pi * (d - radius) / edge)) if edge > 0 else np.zeros_like(d)
    m = np.where(d <= radius, 1.0, np.where(d >= radius + edge, 0.0, soft))
    m = m.astype(np.float32).astype(np.float64)               # the kernel rounds the mask to fp32
    return (1.0 - m.astype(np.float32)).astype(np.float64) if background else m


def default_background(n, mask_radius=None, mask_edge=None):
    """(radius, edge) of the particle disc whose outside is the background: 0.375 n and n / 16 pixels unless given."""
    return (0.375 * n if mask_radius is None else float(mask_radius), n / 16.0 if mask_edge is None else float(mask_edge))


def _even_side(Rr):
    """The even n with radial_rings(n) = Rr (ring(h, h) is strictly increasing in h)."""
    for h in range(1, CL.MAX_SIDE // 2 + 1):
        if 1 + (math.isqrt(8 * h * h) + 1) // 2 == Rr:
            return 2 * h
    raise ValueError(f'{Rr} rings belong to no even n; pass n')


def whitening_profile(spec, floor=FLOOR, n=None):
    """spec [..][Rr] (mean power per coefficient and ring) -> fp64 [..][Rr]: 1 / sqrt(max(spec, floor * median(spec))) per row,
    scaled so that white noise of unit variance keeps unit variance: sum_r counts[r] H[r]^2 = n^2.  n: the side the rings
    belong to (default: the even one)."""
    s = np.asarray(spec, dtype=np.float64)
    if s.ndim < 1 or s.shape[-1] < 2:
        raise ValueError(f'whitening_profile: spec must be [..][Rr], got {s.shape}')
    if not float(floor) > 0:
        raise ValueError(f'whitening_profile: floor = {floor} must be positive')
    n = _even_side(s.shape[-1]) if n is None else int(n)
    cnt = ring_counts(n)
    if cnt.size != s.shape[-1]:
        raise ValueError(f'whitening_profile: {s.shape[-1]} rings do not belong to n = {n}')
    med = np.median(s, axis=-1, keepdims=True)
    H = 1.0 / np.sqrt(np.maximum(s, float(floor) * med))
    return H / np.sqrt((cnt * H * H).sum(-1, keepdims=True) / float(n * n))


def frc_profile(frc, n, kind='cref', threshold=0.143, corners=False):
    """frc [..][R] (R = n // 2 + 1, ring 0 first) -> fp64 [..][Rr], a radial filter of the averages the curve belongs to.
      'cref'  sqrt(2 FRC / (1 + FRC)), 0 where FRC < 0;      'hard'  1.
    Both are 0 from the first ring r >= 1 whose FRC is below `threshold` on (a monotone cut: a curve that rises again stays
    cut).  The corner rings beyond n // 2, which the FRC does not measure, are 0; corners=True gives them the value of the
    last measured ring instead."""
    if kind not in ('cref', 'hard'):
        raise ValueError(f"frc_profile: kind must be 'cref' or 'hard', got {kind!r}")
    f = np.asarray(frc, dtype=np.float64)
    n = int(n)
    R = n // 2 + 1
    if f.ndim < 1 or f.shape[-1] != R or R < 2:
        raise ValueError(f'frc_profile: {f.shape[-1] if f.ndim else 0} rings do not belong to n = {n}')
    Rr = ring_counts(n).size
    if kind == 'cref':
        pos = np.clip(f, 0.0, None)
        val = np.sqrt(2.0 * pos / (1.0 + pos))
    else:
        val = np.ones_like(f)
    below = f < float(threshold)
    below[..., 0] = False
    keep = np.cumsum(below, axis=-1) == 0
    out = np.zeros(f.shape[:-1] + (Rr,))
    out[..., :R] = np.where(keep, val, 0.0)
    if corners:
        out[..., R:] = out[..., R - 1:R]
    return out


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def _planes(images, what):
    CL.require_f32(images, what, 'images')
    if images.dim() not in (3, 4) or images.shape[-1] != images.shape[-2]:
        raise TvaeHipError(f'{what}: images must be [N][n][n] or [N][C][n][n] (square), got {tuple(images.shape)}')
    n = images.shape[-1]
    B = images.numel() // (n * n) if n else 0
    if not (2 <= n <= CL.MAX_SIDE and 1 <= B <= CL.MAX_PLANES):
        raise TvaeHipError(f'{what}: n={n} with {B} planes outside the supported range (2 <= n <= 1024, 1 .. 2^24 planes)')
    return B, n


def _step(query, B, n, chunk):
    per = CL.query(query, 1, n)
    step = CL.slice_step(B, CL.MAX_PLANES, WS_FLOATS // per if chunk is None else chunk)
    return step, CL.query(query, step, n)


def _mask(mask_radius, mask_edge, what):
    radius = 0.0 if mask_radius is None else float(mask_radius)
    edge = 0.0 if mask_edge is None else float(mask_edge)
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'{what}: mask_radius = {mask_radius} and mask_edge = {mask_edge} must be finite, the edge not negative')
    return radius, edge


def raw_ring_power(images, mask_radius=None, mask_edge=None, background=True, demean=True, chunk=None):
    """tvae_ring_power over the planes of `images` in slices that bound the workspace -> fp64 [planes][Rr] on the device, the
    raw ring sums of |F|^2 (a plane's row does not depend on the slice it is in)."""
    B, n = _planes(images, 'ring_power')
    radius, edge = _mask(mask_radius, mask_edge, 'ring_power')
    Rr = radial_rings(n)
    step, wsf = _step('tvae_ring_power_ws_floats', B, n, chunk)
    ws = CL.workspace(wsf, images.device)
    x = images.reshape(-1)
    out = torch.empty(B, Rr, dtype=torch.float64, device=images.device)
    with torch.cuda.device(images.device):
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            CL.call('tvae_ring_power', x[b0 * n * n:b1 * n * n], n * n, out[b0:b1], ws, wsf, b1 - b0, n, radius, edge,
                    int(bool(background)), int(bool(demean)))
    return out


def power_scale(n, mask_radius=None, mask_edge=None, background=True):
    """fp64 [Rr]: what turns the raw ring sums into the mean power per coefficient over sum w^2."""
    radius, edge = _mask(mask_radius, mask_edge, 'ring_power')
    w = window(n, radius, edge, background)
    return 1.0 / (ring_counts(n) * (w * w).sum())


def ring_power(images, mask_radius=None, mask_edge=None, background=True, demean=True, chunk=None):
    """images [N][n][n] or [N][C][n][n] (contiguous CUDA fp32) -> fp64 [N][Rr] or [N][C][Rr] on the device: per ring of the
    full plane the mean of |DFT(w (x - mu))|^2 over the ring's coefficients, divided by sum w^2, so that white noise of
    variance s^2 reads s^2 on every ring.  w is the outside of the soft disc (mask_radius, mask_edge) for background=True and
    its inside otherwise; mask_radius None or <= 0: no window.  demean removes the window-weighted mean first."""
    raw = raw_ring_power(images, mask_radius, mask_edge, background, demean, chunk)
    n = images.shape[-1]
    scale = torch.from_numpy(power_scale(n, mask_radius, mask_edge, background)).to(raw.device)
    return (raw * scale).reshape(tuple(images.shape[:-2]) + (raw.shape[-1],))


def group_power(power, labels=None, n_groups=None, mean=True):
    """power fp64 [N][Rr] (CUDA), labels [N] integers (None: one group) -> (fp64 [G][Rr], counts int32 [G]): per group the
    mean (mean=False: the sum) of its members' rows, added in fp64 in ascending image index; an empty group gives zeros."""
    from . import align
    if not (torch.is_tensor(power) and power.is_cuda and power.dtype == torch.float64 and power.dim() == 2
            and power.is_contiguous()):
        raise TvaeHipError('group_power: power must be a contiguous CUDA fp64 [N][Rr] tensor (no CPU fallback)')
    N, Rr = power.shape
    lab = torch.zeros(N, dtype=torch.int64) if labels is None else torch.as_tensor(labels)
    if lab.dim() != 1 or lab.numel() != N:
        raise TvaeHipError(f'group_power: labels must hold N = {N} entries, got {tuple(lab.shape)}')
    lab = lab.to(power.device)
    G = int(n_groups) if n_groups is not None else int(lab.max()) + 1
    if not (1 <= G <= CL.MAX_CLASSES and 1 <= N <= CL.MAX_PLANES):
        raise TvaeHipError(f'group_power: N={N}, G={G} outside the supported range')
    order, seg, _ = align.segments(lab, G)
    sums = torch.empty(G, Rr, dtype=torch.float64, device=power.device)
    counts = torch.empty(G, dtype=torch.int32, device=power.device)
    with torch.cuda.device(power.device):
        CL.call('tvae_ring_power_groups', power, order, seg, sums, counts, N, G, Rr)
    if mean:
        sums = sums / counts.clamp(min=1).to(torch.float64)[:, None]
    return sums, counts


def _interp(interp):
    try:
        return INTERP[interp]
    except (KeyError, TypeError):
        raise TvaeHipError(f"interp must be 'nearest' (0) or 'linear' (1), got {interp!r}") from None


def radial_filter(images, profile, groups=None, interp='linear', inplace=False, chunk=None):
    """images [N][n][n] or [N][C][n][n] (contiguous CUDA fp32) -> Re IDFT(H_g DFT(image)), same shape, H_g(ky, kx) the radial
    profile of the image's group at |k|.  profile [G][Rr] or [Rr] (host or device; rounded to fp32), groups [N] integers or
    None (group 0 for all); an image whose group is outside [0, G) comes back as zeros.  interp 'nearest' takes the value
    of the coefficient's ring, 'linear' interpolates between the rings at sqrt(ky^2 + kx^2).  The channels of an image share
    its group.  inplace overwrites `images`."""
    B, n = _planes(images, 'radial_filter')
    Rr = radial_rings(n)
    it = _interp(interp)
    prof = torch.as_tensor(profile) if torch.is_tensor(profile) else torch.from_numpy(np.asarray(profile, dtype=np.float64))
    if prof.dim() == 1:
        prof = prof[None]
    if prof.dim() != 2 or prof.shape[1] != Rr or not 1 <= prof.shape[0] <= CL.MAX_CLASSES:
        raise TvaeHipError(f'radial_filter: profile must be [G][{Rr}] or [{Rr}] for n = {n}, got {tuple(prof.shape)}')
    prof = prof.to(device=images.device, dtype=torch.float32).contiguous()
    G = prof.shape[0]
    N = images.shape[0]
    C = B // N
    grp = None
    if groups is not None:
        g = torch.as_tensor(groups)
        if g.dim() != 1 or g.numel() != N or g.dtype.is_floating_point or g.dtype == torch.bool:
            raise TvaeHipError(f'radial_filter: groups must be an integer array of N = {N} entries')
        grp = g.to(images.device).clamp(-1, 2 ** 31 - 1).to(torch.int32)
        if C > 1:
            grp = grp.repeat_interleave(C)
        grp = grp.contiguous()
    out = images if inplace else torch.empty_like(images)
    step, wsf = _step('tvae_radial_filter_ws_floats', B, n, chunk)
    ws = CL.workspace(wsf, images.device)
    xf, of = images.reshape(-1), out.reshape(-1)
    with torch.cuda.device(images.device):
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            CL.call('tvae_radial_filter', xf[b0 * n * n:b1 * n * n], n * n, prof, None if grp is None else grp[b0:b1],
                    of[b0 * n * n:b1 * n * n], ws, wsf, b1 - b0, n, G, it)
    return out


def whiten(images, groups=None, n_groups=None, mask_radius=None, mask_edge=None, floor=FLOOR, interp='linear', inplace=False,
           chunk=None):
    """-> (whitened images, spectra fp64 numpy [G][Rr], counts numpy [G]).  The noise spectrum of every group is the mean of
    its images' background ring power (outside the disc of `default_background` unless a mask is given; an [N][C] stack
    counts every channel); every image is filtered with `whitening_profile` of its group's spectrum.  An image whose group
    is outside [0, G) comes back as zeros; an empty group's profile is never used."""
    B, n = _planes(images, 'whiten')
    radius, edge = default_background(n, mask_radius, mask_edge)
    N, C = images.shape[0], B // images.shape[0]
    power = ring_power(images, radius, edge, True, True, chunk).reshape(B, -1)
    lab = None if groups is None else torch.as_tensor(groups).repeat_interleave(C)
    spec, counts = group_power(power, lab, n_groups)
    spec, counts = spec.cpu().numpy(), counts.cpu().numpy()
    prof = _profiles(spec, counts, floor, n)
    return radial_filter(images, prof, groups, interp, inplace, chunk), spec, counts


def _profiles(spec, counts, floor, n):
    """whitening_profile of the groups that have members; zeros for an empty group (no image reads them)."""
    prof = np.zeros_like(spec)
    has = np.asarray(counts) > 0
    if has.any():
        prof[has] = whitening_profile(spec[has], floor, n)
    return prof


def filter_averages(avg, frc, kind='cref', threshold=0.143, interp='linear', corners=False):
    """avg [K][C][n][n] or [K][n][n] (CUDA fp32) and the FRC curves of its planes, [K][C][R], [K][n // 2 + 1] (one per class,
    shared by its channels) -> the averages filtered with `frc_profile` of their curve, same shape."""
    B, n = _planes(avg, 'filter_averages')
    f = np.asarray(frc.cpu() if torch.is_tensor(frc) else frc, dtype=np.float64)
    K = avg.shape[0]
    C = B // K
    if f.ndim == 2 and avg.dim() == 4:
        f = np.repeat(f[:, None], C, 1)
    if f.shape[:-1] != tuple(avg.shape[:-2]):
        raise TvaeHipError(f'filter_averages: frc {f.shape} does not belong to averages {tuple(avg.shape)}')
    try:
        prof = frc_profile(f, n, kind, threshold, corners).reshape(B, -1)
    except ValueError as e:
        raise TvaeHipError('filter_averages: ' + str(e).split(': ', 1)[-1]) from None
    flat = radial_filter(avg.reshape(B, n, n), prof, np.arange(B), interp)
    return flat.reshape(avg.shape)


# ---- whiten_particles.py: two streamed passes over a stack ------------------------------------------------------------------
def whiten_stack(path_or_array, out_path, groups=None, mask_radius=None, mask_edge=None, floor=FLOOR, interp='linear',
                 chunk=4096, device=None):
    """Stream a particle stack through the GPU twice in chunks of `chunk` images, as tvae.image.preprocess_stack streams:
    pass one estimates the background ring power of every image, pass two filters every image with its group's whitening
    profile; the fp32 result goes to `out_path` (.mrcs, the input's pixel size kept).  -> (spectra fp64 [G][Rr], counts [G]).
    The result does not depend on `chunk`."""
    from src import mrc
    from . import image
    header = None
    if isinstance(path_or_array, (str, os.PathLike)):
        stack, header = mrc.open_stack(os.fspath(path_or_array))
    else:
        stack = np.asarray(path_or_array)
    if stack.ndim != 3 or stack.shape[1] != stack.shape[2]:
        raise TvaeHipError(f'whiten_stack: a [B][n][n] stack of square images is expected, got {stack.shape}')
    if not torch.cuda.is_available():
        raise TvaeHipError('whiten_stack: no GPU is visible and there is no CPU fallback')
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    B, n = stack.shape[0], stack.shape[-1]
    lab = np.zeros(B, dtype=np.int64) if groups is None else np.asarray(groups).reshape(-1)
    if lab.size != B or lab.dtype.kind not in 'iu':
        raise TvaeHipError(f'whiten_stack: groups must hold one integer per image ({B}), got {lab.shape} of {lab.dtype}')
    chunk = max(1, int(chunk))
    radius, edge = default_background(n, mask_radius, mask_edge)
    power = torch.empty(B, radial_rings(n), dtype=torch.float64, device=device)
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        power[b0:b1] = ring_power(image._upload(stack[b0:b1], device), radius, edge, True, True)
    spec, counts = group_power(power, lab)
    spec, counts = spec.cpu().numpy(), counts.cpu().numpy()
    prof = _profiles(spec, counts, floor, n)
    out = np.empty((B, n, n), dtype=np.float32)
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        out[b0:b1] = radial_filter(image._upload(stack[b0:b1], device), prof, lab[b0:b1], interp, inplace=True).cpu().numpy()
    apix = image._pixel_size(header) if header is not None else None
    ax, ay, az = apix if apix is not None else (1, 1, 1)
    with open(out_path, 'wb') as f:
        mrc.write(f, out, ax=ax, ay=ay, az=az)
    return spec, counts


def build_parser(tool='whiten') -> argparse.ArgumentParser:
    """The parser of whiten_particles.py ('whiten') or of filter_class_averages.py ('filter')."""
    if tool == 'whiten':
        p = argparse.ArgumentParser('Whiten a particle stack with the radial noise spectrum of its background, per group')
        p.add_argument('--stack', required=True, help='the particles (.mrc or .mrcs), square images')
        p.add_argument('--out', required=True, help='the fp32 .mrcs to write; noise_spectrum.npy and noise_counts.npy go beside it')
        p.add_argument('--groups', default=None, help='groups.npy: one integer per image (micrograph or defocus group); '
                                                      'default: one group')
        stack_cli.add_mask_flags(p, None, 'the particle disc whose outside is the background; default 0.375 n '
                                          '(edge: default n / 16)')
        p.add_argument('--floor', default=FLOOR, type=float, help='lower bound of the spectrum, as a fraction of its median')
        p.add_argument('--chunk', default=4096, type=int, help='images per trip through the GPU')
        p.add_argument('--interp', default='linear', choices=['linear', 'nearest'], help='profile lookup between the rings')
    elif tool == 'filter':
        p = argparse.ArgumentParser('Filter the class averages to their FRC: the weight sqrt(2 FRC / (1 + FRC)) or a low-pass')
        p.add_argument('--averages', required=True, help='class_averages.npy, [K][C][n][n]')
        p.add_argument('--frc', required=True, help='class_frc.npy of class_resolution.py, [K][C][R] or [K][R]')
        p.add_argument('--kind', default='cref', choices=['cref', 'hard'], help='FRC weight or hard low-pass at the crossing')
        p.add_argument('--threshold', default=0.143, type=float, help='FRC threshold of the cut')
        p.add_argument('--apix', default=None, type=float, help='Angstrom per pixel: the cut is reported in Angstrom')
        p.add_argument('--out-dir', default='.', help='where class_averages_filtered.npy, .mrcs and .jpg go')
    else:
        raise ValueError(f"build_parser: tool must be 'whiten' or 'filter', got {tool!r}")
    p.add_argument('-d', '--device', type=int, default=0)
    return p


def save_outputs(out_dir, filtered):
    """class_averages_filtered.npy, .mrcs and (with matplotlib) .jpg."""
    from . import align
    a = stack_cli.host(filtered)
    align.save_outputs(out_dir, a, np.zeros(a.shape[0], dtype=np.int64), True, 'class_averages_filtered')


def run(argv=None, tool='whiten'):
    args = build_parser(tool).parse_args(argv)
    if tool == 'whiten':
        groups = None
        if args.groups is not None:
            groups = np.load(args.groups)
            if groups.dtype.kind not in 'iu':
                raise SystemExit(f'--groups must hold integers, got {groups.dtype}')
        if not args.floor > 0:
            raise SystemExit(f'--floor = {args.floor} must be positive')
        if args.chunk < 1:
            raise SystemExit(f'--chunk = {args.chunk} must be positive')
        device = stack_cli.make_device(args)
        with stack_cli.hip_errors():
            spec, counts = whiten_stack(args.stack, args.out, groups, args.mask_radius, args.mask_edge, args.floor, args.interp,
                                        args.chunk, device)
        where = os.path.dirname(os.path.abspath(args.out))
        np.save(os.path.join(where, 'noise_spectrum.npy'), spec)
        np.save(os.path.join(where, 'noise_counts.npy'), counts)
        print('# whitened {} in {} groups: {}'.format(args.stack, len(counts), args.out), file=sys.stderr)
        return spec, counts
    avg = np.asarray(np.load(args.averages), dtype=np.float32)
    frc = np.asarray(np.load(args.frc), dtype=np.float64)
    if avg.ndim == 3:
        avg = avg[:, None]
    if avg.ndim != 4 or avg.shape[-1] != avg.shape[-2]:
        raise SystemExit(f'--averages must hold [K][C][n][n] or [K][n][n], got {avg.shape}')
    n = avg.shape[-1]
    if frc.shape[-1] != n // 2 + 1 or frc.shape[0] != avg.shape[0] or frc.ndim not in (2, 3):
        raise SystemExit(f'--frc {frc.shape} does not belong to --averages {avg.shape}')
    device = stack_cli.make_device(args)
    with stack_cli.hip_errors():
        out = filter_averages(torch.from_numpy(np.ascontiguousarray(avg)).to(device), frc, args.kind, args.threshold)
    os.makedirs(args.out_dir, exist_ok=True)
    save_outputs(args.out_dir, out)
    from . import resolution
    curve = frc if frc.ndim == 2 else frc.mean(1)
    cut = resolution.resolution(curve, n, args.threshold, args.apix)
    print('# class  cut[{}]@{:g}'.format('A' if args.apix is not None else 'px', args.threshold))
    for k, c in enumerate(cut):
        print('{} {:.4f}'.format(k, c))
    return out
