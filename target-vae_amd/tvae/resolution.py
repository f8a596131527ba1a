"""Resolution of the aligned 2-D class averages: the step after class_averages.py.  In one pass over the stack the two
half-set averages and the variance map of every class (tvae.align.class_halves), the Fourier ring correlation of the two
halves under a soft circular mask (tvae.align.frc), and from it a resolution per class: where the curve first falls below
a threshold (0.143 by default, 0.5 beside it).

Both halves share ONE encoder and ONE set of poses: the members of a class are dealt out alternately after they were
aligned by the same network.  This is not a gold-standard FRC (two independently refined half sets); noise that the shared
poses aligned correlates between the halves, so the numbers read optimistic.  They rank the classes of one run -- sharp,
blurred by mis-alignment, mixed views -- and should not be quoted as the resolution of a map.

`resolution` is host-only numpy; the kernels are tvae_class_halves and tvae_class_frc of libtvae_cluster.so, with no CPU
fallback.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import align, stack_cli

NOTE = ('both halves share one encoder and one set of poses: this is not a gold-standard FRC and the resolutions read '
        'optimistic')
THRESHOLDS = (0.143, 0.5)
MASK_MARGIN, MASK_EDGE = 4.0, 4.0


def resolution(frc, n, threshold=0.143, apix=None):
    """frc [...][R] (ring 0 first, R = n // 2 + 1) and the side n of the images (R alone does not tell an odd n from the
    even one below it) -> [...] fp64: n / r* pixels, or n apix / r* Angstrom, where r* is the ring at which the curve
    first falls below `threshold`: the first ring r in 1 .. R - 1 whose value is below it, interpolated linearly between
    the rings r - 1 and r and never below 1; R - 1 when no ring is below it (the curve never crosses: Nyquist)."""
    f = np.asarray(frc, dtype=np.float64)
    R = f.shape[-1]
    if R != int(n) // 2 + 1 or R < 2:
        raise ValueError(f'resolution: {R} rings do not belong to n = {n}')
    flat = f.reshape(-1, R)
    out = np.empty(flat.shape[0])
    for p, c in enumerate(flat):
        below = np.flatnonzero(c[1:] < threshold)
        if below.size == 0:
            star = float(R - 1)
        else:
            r = int(below[0]) + 1
            hi, lo = c[r - 1], c[r]
            star = (r - 1) + (hi - threshold) / (hi - lo) if hi >= threshold else float(r - 1)
            star = max(star, 1.0)
        out[p] = n / star
    out = out.reshape(f.shape[:-1])
    return out * float(apix) if apix is not None else out


def default_mask(n, mask_radius=None, mask_edge=None):
    """(radius, edge) of the soft mask: (n - 1) / 2 - 4 and 4 pixels unless given."""
    return (float((n - 1) / 2 - MASK_MARGIN) if mask_radius is None else float(mask_radius),
            MASK_EDGE if mask_edge is None else float(mask_edge))


def combined(sums):
    """sums fp64 [K][C][R][3] -> the curve of a class over all its channels, [K][R]: the ring sums added over the channels
    before the ratio (0 where either power is 0)."""
    s = np.asarray(sums, dtype=np.float64).sum(axis=1)
    den = np.sqrt(s[..., 1] * s[..., 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where((s[..., 1] == 0) | (s[..., 2] == 0), 0.0, s[..., 0] / np.where(den == 0, 1.0, den))


def class_resolution(images, theta, dx, labels, n_clusters=None, t_scale=1.0, mask_radius=None, mask_edge=None):
    """-> dict of device tensors: avg, halves, var, counts (tvae.align.class_halves), frc [K][C][R] and sums [K][C][R][3]
    of the two halves (tvae.align.frc), and the mask that was used."""
    avg, halves, var, counts = align.class_halves(images, theta, dx, labels, n_clusters, t_scale)
    radius, edge = default_mask(images.shape[-1], mask_radius, mask_edge)
    curve, sums = align.frc(halves[0], halves[1], radius, edge)
    return dict(avg=avg, halves=halves, var=var, counts=counts, frc=curve, sums=sums, mask_radius=radius, mask_edge=edge)


def save_outputs(out_dir, res, threshold=0.143, apix=None):
    """class_halves.npy ([2][K][C][n][n]), class_variance.npy, class_frc.npy ([K][C][R]), class_counts.npy ([K][2]) and
    class_resolution.txt (one line per class: both half counts and the resolution at `threshold` and at 0.5, from the
    curve over all channels); class_frc.jpg and class_variance.jpg when matplotlib is present (stderr says so when it is
    not).  -> the resolutions [K][2]."""
    from . import figures
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}
    halves, var, counts = host['halves'], host['var'], host['counts']
    n = halves.shape[-1]
    np.save(os.path.join(out_dir, 'class_halves.npy'), halves)
    np.save(os.path.join(out_dir, 'class_variance.npy'), var)
    np.save(os.path.join(out_dir, 'class_frc.npy'), host['frc'])
    np.save(os.path.join(out_dir, 'class_counts.npy'), counts)
    curve = combined(host['sums'])
    levels = (float(threshold), 0.5)
    values = np.stack([resolution(curve, n, t, apix) for t in levels], 1)
    unit = 'A' if apix is not None else 'px'
    with open(os.path.join(out_dir, 'class_resolution.txt'), 'w') as f:
        f.write('# {}\n'.format(NOTE))
        f.write('# n = {}, mask radius {:g} and edge {:g} pixels, apix {}\n'.format(
            n, host['mask_radius'], host['mask_edge'], 'none' if apix is None else '{:g}'.format(float(apix))))
        f.write('# class  half0  half1  resolution[{u}]@{:g}  resolution[{u}]@{:g}\n'.format(*levels, u=unit))
        for k in range(counts.shape[0]):
            f.write('{} {} {} {:.4f} {:.4f}\n'.format(k, int(counts[k, 0]), int(counts[k, 1]), values[k, 0], values[k, 1]))
    try:
        figures._plt()
    except ImportError as e:
        print('# matplotlib is not available ({}): class_frc.jpg and class_variance.jpg are skipped'.format(e),
              file=sys.stderr)
        return values
    figures.save_class_frc(out_dir, curve, levels, n, apix)
    figures.save_class_variance(out_dir, var, counts.sum(1))
    return values


# ---- class_resolution.py: the same from the files a clustering run wrote --------------------------------------------------
def build_parser(ctf=False) -> argparse.ArgumentParser:
    """ctf=True adds --ctf, --ctf-correct flip and --scale (what class_resolution.py parses); the default is the parser without
    them."""
    p = argparse.ArgumentParser('Half-set averages, variance maps and FRC resolution of the aligned 2-D class averages')

    def own(q):
        q.add_argument('--apix', default=None, type=float, help='Angstrom per pixel; default: resolutions in pixels')
        q.add_argument('--threshold', default=0.143, type=float, help='FRC threshold (0.5 is reported beside it)')
        stack_cli.add_mask_flags(q, MASK_EDGE, 'default (n - 1) / 2 - 4')

    stack_cli.add_stack_flags(p, 'where the .npy files, class_resolution.txt and the figures go', own)
    if ctf:
        align.add_ctf_flags(p, ('flip',), wiener=False)
    return p


def run(argv=None):
    args = build_parser(ctf=True).parse_args(argv)
    inp = stack_cli.open_inputs(args, stack_cli.make_device(args))
    images, theta, dx, clusters = inp.images, inp.theta, inp.dx, inp.clusters
    with stack_cli.hip_errors():
        if args.ctf:
            # phase-flipped in place, in the chunks of tvae.ctf.filter_stack, before the one pass over the stack
            from . import ctf
            coef = align.load_ctf_coefficients(args.ctf, images.shape[0], args.scale)
            ctf.filter_stack(images, coef=coef, mode='flip', inplace=True)
        res = class_resolution(images, theta, dx, clusters, args.n_clusters, inp.t_scale, args.mask_radius, args.mask_edge)
    os.makedirs(args.out_dir, exist_ok=True)
    values = save_outputs(args.out_dir, res, args.threshold, args.apix)
    print('# class resolution of {} images in {} classes ({}): {}'.format(images.shape[0], values.shape[0], NOTE,
                                                                         args.out_dir), file=sys.stderr)
    return res, values
