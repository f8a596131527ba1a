"""Particle preprocessing on the GPU: Fourier downsample, central crop and background-ring normalisation, the reference's
src/image.py, and `preprocess_stack`, which streams a raw .mrcs stack through them.

A Fourier crop to a fixed size is a fixed real linear map, out = (Ar x Br - Ai x Bi) / (M N) with four tables that depend
on the shapes alone (tvae.tables.resample_tables; include/tvae_cluster.h states the definition, the reference's row rule
included).  tvae_image_resample computes that product for a whole stack in one launch on the fp32 matrix pipe, reads
every pixel of the window once per output tile and keeps the intermediate on the chip; a crop is the window it reads, no
copy.  tvae_image_normalize is a second launch over the (much smaller) result: mean and two-pass standard deviation of the
pixels at or beyond `radius` from (n / 2, m / 2), in fp64.

Results are bitwise reproducible and an image's result does not depend on the images processed with it, so the chunk
size of `preprocess_stack` cannot change a bit of its output.  There is no CPU fallback.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _cluster_lib as CL
from . import tables
from ._lib import TvaeHipError

MAX_IMAGES = CL.MAX_PLANES
MAX_SIDE = CL.MAX_SIDE

_DEVICE_TABLES = {}


def device_tables(M, N, m, n, device):
    """The four fp32 tables of tvae.tables.resample_tables on `device`, uploaded once per (shape, device); the imaginary
    pair is (None, None) where the second term of the product vanishes (m == M)."""
    device = torch.device(device)
    key = (int(M), int(N), int(m), int(n), device.type, device.index if device.index is not None else torch.cuda.current_device())
    got = _DEVICE_TABLES.get(key)
    if got is None:
        Ar, Ai, Br, Bi = tables.resample_tables(*key[:4])
        imag = bool(Ai.any()) and bool(Bi.any())
        got = tuple(torch.from_numpy(np.array(t)).to(device) if t is not None else None
                    for t in (Ar, Ai if imag else None, Br, Bi if imag else None))
        _DEVICE_TABLES[key] = got
    return got


def output_shape(M, N, factor=1, shape=None):
    """(m, n) of a downsample of an M x N image: `shape`, or int(M / factor), int(N / factor) as the reference."""
    if shape is None:
        return int(M / factor), int(N / factor)
    m, n = shape
    return int(m), int(n)


def _check(x, what):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise TvaeHipError(f'{what}: a CUDA tensor is expected (no CPU fallback)')
    if x.dim() < 2:
        raise TvaeHipError(f'{what}: [..., rows, columns] expected, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    return x.contiguous()


def resample_window(frames, r0, c0, M, N, m, n):
    """frames [B][H][W] (contiguous CUDA fp32) -> [B][m][n]: the Fourier downsample of the M x N window at (r0, c0)."""
    B, H, W = frames.shape
    if not (1 <= B <= MAX_IMAGES and 1 <= m <= M <= MAX_SIDE and 1 <= n <= N <= MAX_SIDE):
        raise TvaeHipError(f'downsample: B={B}, ({M}, {N}) -> ({m}, {n}) outside the supported range (1 <= B <= 2^24, '
                           f'1 <= m <= M <= {MAX_SIDE}, 1 <= n <= N <= {MAX_SIDE})')
    if not (0 <= r0 and r0 + M <= H and 0 <= c0 and c0 + N <= W):
        raise TvaeHipError(f'downsample: the window ({r0}, {c0}, {M}, {N}) leaves the {H} x {W} frame')
    Ar, Ai, Br, Bi = device_tables(M, N, m, n, frames.device)
    out = torch.empty(B, m, n, dtype=torch.float32, device=frames.device)
    with torch.cuda.device(frames.device):
        CL.call('tvae_image_resample', frames, Ar, Ai, Br, Bi, out, B, H, W, r0, c0, M, N, m, n, 1.0 / (M * N))
    return out


def downsample(x, factor=1, shape=None):
    """x [..., M, N] (CUDA) -> fp32 [..., m, n]: the reference's Fourier downsample, m = int(M / factor) unless `shape`."""
    x = _check(x, 'downsample')
    M, N = x.shape[-2:]
    m, n = output_shape(M, N, factor, shape)
    out = resample_window(x.reshape(-1, M, N), 0, 0, M, N, m, n)
    return out.reshape(tuple(x.shape[:-2]) + (m, n))


def crop_window(n, m, size):
    """(first row, first column) of the reference's central crop of an n x m image to size x size."""
    return (n - size) // 2, (m - size) // 2


def crop(stack, size):
    """The central size x size window of [..., n, m]: a view, as the reference's; no kernel runs."""
    n, m = stack.shape[-2:]
    si, sj = crop_window(n, m, size)
    return stack[..., si:si + size, sj:sj + size]


def normalize(stack, radius=None, return_stats=False, out=None):
    """stack [..., n, m] (CUDA) -> fp32 of the same shape: every image minus the mean, over the standard deviation, of its
    pixels at distance >= radius from (n / 2, m / 2) (default min(n, m) / 2), in fp64 (two passes).  return_stats: also
    the fp64 [..., 2] tensor of (mean, standard deviation).  out: the input itself for an in-place run."""
    x = _check(stack, 'normalize')
    n, m = x.shape[-2:]
    B = x.numel() // max(n * m, 1)
    if radius is None:
        r = 0.0
    else:
        r = float(radius)
        if not (math.isfinite(r) and r > 0):
            raise TvaeHipError(f'normalize: radius = {radius} must be positive and finite (None: min(n, m) / 2)')
    wsf = CL.query('tvae_image_normalize_ws_floats', B, n, m) if n * m else 0
    if wsf <= 0:
        raise TvaeHipError(f'normalize: B={B}, n={n}, m={m} outside the supported range (1 <= B <= 2^24, sides <= {MAX_SIDE})')
    if out is None:
        out = torch.empty_like(x)
    elif not (CL.is_f32(out) and out.shape == x.shape):
        raise TvaeHipError('normalize: out must be a contiguous CUDA fp32 tensor of the input\'s shape')
    stats = torch.empty(B, 2, dtype=torch.float64, device=x.device)
    ws = CL.workspace(wsf, x.device)
    with torch.cuda.device(x.device):
        CL.call('tvae_image_normalize', x.reshape(B, n, m), out.reshape(B, n, m), stats, ws, wsf, B, n, m, r)
    if return_stats:
        return out, stats.reshape(tuple(x.shape[:-2]) + (2,))
    return out


# ---- a whole stack ---------------------------------------------------------------------------------------------------------
def _upload(block, device):
    """A host block of the stack -> contiguous fp32 on the device; integer modes are converted there."""
    a = np.ascontiguousarray(block)
    if a.dtype == np.uint16:
        a = a.astype(np.int32)                                # torch has no arithmetic on uint16
    if a.dtype not in (np.float32, np.int8, np.int16, np.int32):
        raise TvaeHipError(f'preprocess_stack: pixel type {a.dtype} is not supported (modes 0, 1, 2 and 6)')
    return torch.from_numpy(a).to(device).to(torch.float32)


def _pixel_size(header):
    """(x, y, z) pixel size of an MRC header, or None where it carries none."""
    try:
        cell = (header.xlen, header.ylen, header.zlen)
        grid = (header.mx, header.my, header.mz)
    except (AttributeError, KeyError, ValueError):
        return None
    if grid[0] > 0 and grid[1] > 0 and cell[0] > 0 and cell[1] > 0:
        return (cell[0] / grid[0], cell[1] / grid[1], cell[2] / grid[2] if grid[2] > 0 and cell[2] > 0 else 1.0)
    return None


def preprocess_stack(path_or_array, out_path, crop=0, factor=1, shape=None, normalize=False, radius=None, chunk=4096,
                     device=None):
    """Stream a particle stack through the GPU in chunks of `chunk` images: central crop (as the resampler's window, no copy),
    Fourier downsample, normalisation; write the fp32 result to `out_path` (.mrcs).  path_or_array: an .mrc / .mrcs file
    (memory-mapped; integer modes are converted to fp32 on upload) or a [B][H][W] array.  The pixel size of the input's
    header, where it has one, is multiplied by M / m (rows) and N / n (columns).  Returns the fp64 [B][2] array of the
    per-image (mean, standard deviation) the normalisation removed, None without `normalize`."""
    from src import mrc
    this = sys.modules[__name__]
    header = None
    if isinstance(path_or_array, (str, os.PathLike)):
        stack, header = mrc.open_stack(os.fspath(path_or_array))
    else:
        stack = np.asarray(path_or_array)
    if stack.ndim != 3:
        raise TvaeHipError(f'preprocess_stack: a [B][H][W] stack is expected, got {stack.shape}')
    if not torch.cuda.is_available():
        raise TvaeHipError('preprocess_stack: no GPU is visible and there is no CPU fallback')
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    B, H, W = stack.shape
    if crop and crop > 0:
        if crop > min(H, W):
            raise TvaeHipError(f'preprocess_stack: crop = {crop} exceeds the {H} x {W} images')
        (r0, c0), M, N = crop_window(H, W, crop), crop, crop
    else:
        r0, c0, M, N = 0, 0, H, W
    resample = shape is not None or factor != 1
    m, n = output_shape(M, N, factor, shape) if resample else (M, N)
    chunk = max(1, int(chunk))
    out = np.empty((B, m, n), dtype=np.float32)
    stats = np.empty((B, 2), dtype=np.float64) if normalize else None
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        x = _upload(stack[b0:b1], device)
        y = resample_window(x, r0, c0, M, N, m, n) if resample else x[:, r0:r0 + M, c0:c0 + N].contiguous()
        if normalize:
            y, st = this.normalize(y, radius, return_stats=True, out=y)
            stats[b0:b1] = st.cpu().numpy()
        out[b0:b1] = y.cpu().numpy()
    apix = _pixel_size(header) if header is not None else None
    ax, ay, az = (apix[0] * N / n, apix[1] * M / m, apix[2]) if apix is not None else (1, 1, 1)
    with open(out_path, 'wb') as f:
        mrc.write(f, out, ax=ax, ay=ay, az=az)
    return stats


# ---- preprocess_particles.py -----------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser('Crop, Fourier-downsample and normalize a particle stack on the GPU')
    p.add_argument('--stack', required=True, help='the raw particles (.mrc or .mrcs)')
    p.add_argument('--out', required=True, help='the fp32 .mrcs to write; with --normalize also <out>.stats.npy')
    p.add_argument('--crop', default=0, type=int, help='central crop to this size before anything else (0: none)')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--downsample', default=1, type=float, help='downsampling factor: m = int(M / factor)')
    g.add_argument('--shape', default=None, type=int, nargs=2, metavar=('m', 'n'), help='output size instead of a factor')
    p.add_argument('--normalize', action='store_true', help='background ring of every image to mean 0, std 1')
    p.add_argument('--radius', default=None, type=float, help='inner radius of the background ring (default: min(m, n) / 2)')
    p.add_argument('--chunk', default=4096, type=int, help='images per trip through the GPU')
    p.add_argument('-d', dest='device', type=int, default=0)
    return p


def run(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available() or args.device == -1:
        raise SystemExit('the MI355X build has no CPU compute path')
    torch.cuda.set_device(args.device)
    try:
        stats = preprocess_stack(args.stack, args.out, crop=args.crop, factor=args.downsample,
                                 shape=tuple(args.shape) if args.shape else None, normalize=args.normalize,
                                 radius=args.radius, chunk=args.chunk, device=torch.device('cuda', args.device))
    except TvaeHipError as e:
        raise SystemExit(str(e)) from e
    if stats is not None:
        np.save(args.out + '.stats.npy', stats)
    print('# preprocessed {}: {}'.format(args.stack, args.out), file=sys.stderr)
    return stats
