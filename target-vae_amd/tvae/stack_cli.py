"""What the scripts share that work from the files a clustering run wrote (class_averages.py, class_resolution.py,
class_eigenimages.py, refine_poses.py, polish_poses.py, reclassify_particles.py, ml_class_averages.py): the flag groups
their parsers are composed of, the opening of the inputs, the saving of a pose family's poses and averages, the resolution
table and the exit on a TvaeHipError.  Host-only: numpy, torch and argparse; nothing here needs a GPU at import, and
`open_inputs` takes its device so that it runs on the CPU.
"""
from __future__ import annotations

import contextlib
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import TvaeHipError


# ---- flag groups: functions that add to a parser ------------------------------------------------------------------------------
def add_stack_flags(p, out_dir_help='where class_averages.npy, class_counts.npy and the figure go', own=None):
    """The nine flags --stack .. -d/--device; `own` adds the flags of the script that stand before -d/--device.  The default
    --out-dir help is that of class_averages.py, which the four pose tools have always shown as well."""
    p.add_argument('--stack', required=True, help='the images (.npy, .mrc or .mrcs): [N][n][n] or [N][C][n][n]')
    p.add_argument('--rotations', required=True, help='rotations.npy of the clustering run')
    p.add_argument('--translations', required=True, help='translations.npy of the clustering run')
    p.add_argument('--clusters', required=True, help='clusters.npy of the clustering run')
    p.add_argument('--t-inf', default='attention', choices=['unimodal', 'attention'],
                   help='translation inference of the run: chooses the scale of the translations (1 or 0.1)')
    p.add_argument('--crop', default=0, type=int, help='central crop, as the clustering run applied it')
    p.add_argument('--n-clusters', default=None, type=int, help='default: the largest label + 1')
    p.add_argument('--out-dir', default='.', help=out_dir_help)
    if own is not None:
        own(p)
    p.add_argument('-d', '--device', type=int, default=0)


def add_mask_flags(p, edge_default, radius_default, cross_halves=False):
    """--mask-radius and --mask-edge (`radius_default`: what the help says an absent radius means), and --cross-halves
    behind them for the pose tools."""
    p.add_argument('--mask-radius', default=None, type=float, help='soft mask radius in pixels; ' + radius_default)
    p.add_argument('--mask-edge', default=edge_default, type=float, help='width of the raised-cosine edge in pixels')
    if cross_halves:
        p.add_argument('--cross-halves', action='store_true',
                       help='score every image against the half-set average it is not a member of')


def add_grid_flags(p):
    """The grid search of refine_poses.py, reclassify_particles.py and ml_class_averages.py, with its mask."""
    p.add_argument('--rounds', default=3, type=int, help='rounds of averaging and refining; the angle step halves every round')
    p.add_argument('--angle-range', default=22.5, type=float, help='degrees searched to each side in the first round')
    p.add_argument('--angle-steps', default=8, type=int, help='angle steps to each side (at most 32)')
    p.add_argument('--shift', default=2, type=int, help='shift radius in whole pixels (at most 8)')
    add_mask_flags(p, 0.0, 'default: no mask', cross_halves=True)


def add_candidate_flags(p):
    p.add_argument('--latents', default=None, help='latents.npy of the run: the candidates of an image are the classes '
                                                    'whose centroid is nearest to it')
    p.add_argument('--candidates', default=None, type=int, help='candidate classes per image, the current one among them '
                                                                '(at most 64); default: all classes')


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
class Inputs(NamedTuple):
    images: torch.Tensor              # fp32 [N][C][n][m], contiguous, on the device
    theta: torch.Tensor               # fp32 [N]
    dx: torch.Tensor                  # fp32 [N][2]
    clusters: np.ndarray              # [N], the dtype of the file
    latents: Optional[np.ndarray]     # fp64 [N][d], or None without --latents
    particles: bool                   # --stack is an .mrc / .mrcs file: the averages are written as .mrcs too
    rot_shape: tuple                  # the shape of the rotations file, [N] or [N][1]: the new rotations are saved in it
    t_scale: float


def make_device(args) -> torch.device:
    if not torch.cuda.is_available() or args.device == -1:
        raise SystemExit('the MI355X build has no CPU compute path')
    torch.cuda.set_device(args.device)
    return torch.device('cuda', args.device)


def open_inputs(args, device) -> Inputs:
    """The files the stack flags (and --latents, where the parser has it) name, on `device`."""
    from . import align
    images = torch.from_numpy(align.load_stack(args.stack, args.crop)).to(device)
    rot = np.asarray(np.load(args.rotations), dtype=np.float32)
    theta = torch.from_numpy(rot.reshape(-1)).to(device)
    dx = torch.from_numpy(np.ascontiguousarray(np.asarray(np.load(args.translations), dtype=np.float32))).to(device)
    clusters = np.asarray(np.load(args.clusters)).reshape(-1)
    path = getattr(args, 'latents', None)
    latents = None if path is None else np.asarray(np.load(path), dtype=np.float64)
    particles = args.stack.endswith('mrc') or args.stack.endswith('mrcs')
    return Inputs(images, theta, dx, clusters, latents, particles, rot.shape, align.translation_scale(args.t_inf))


@contextlib.contextmanager
def hip_errors():
    """A TvaeHipError ends the script with its message."""
    try:
        yield
    except TvaeHipError as e:
        raise SystemExit(str(e)) from e


# ---- the outputs --------------------------------------------------------------------------------------------------------------
def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def save_poses(out_dir, suffix, theta, dx, avg, counts, particles, rot_shape):
    """rotations_<suffix>.npy (in the shape of the rotations that came in), translations_<suffix>.npy and the averages of
    those poses under class_averages_<suffix> (tvae.align.save_outputs)."""
    from . import align
    np.save(os.path.join(out_dir, f'rotations_{suffix}.npy'), host(theta).reshape(tuple(rot_shape)))
    np.save(os.path.join(out_dir, f'translations_{suffix}.npy'), host(dx))
    align.save_outputs(out_dir, host(avg), host(counts), particles, 'class_averages_' + suffix)


def print_resolution_table(before, after, members, members_after=None):
    """before, after [K][2] (tvae.refine._resolutions) -> stdout, one line per class; `members_after` where the tool moves
    images between the classes."""
    moved = members_after is not None
    print('# class  members{}  resolution[px]@0.143 before -> after  resolution[px]@0.5 before -> after'.format(
        ' before -> after' if moved else ''))
    for k in range(len(before)):
        count = '{} -> {}'.format(int(members[k]), int(members_after[k])) if moved else str(int(members[k]))
        print('{} {} {:.4f} -> {:.4f} {:.4f} -> {:.4f}'.format(k, count, before[k, 0], after[k, 0], before[k, 1], after[k, 1]))
