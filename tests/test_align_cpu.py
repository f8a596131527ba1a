"""Aligned class averages, the part that needs no GPU: the pose convention of tests/align_ref.py against the reference's
own formula (train_*.py: eval_minibatch), tvae.align.segments on CPU tensors, the new parsers, the argument checks and
the host queries of libtvae_cluster.so."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import align_ref
from conftest import PKG, ROOT

# ---- the convention --------------------------------------------------------------------------------------------------------
N_SIDE = 65
SIGMA_PX = (4.0, 5.0, 6.0)
AMP = (1.0, 0.7, 0.5)
MEAN = ((0.2, 0.1), (-0.15, 0.25), (0.05, -0.2))              # coordinate units, off-centre and asymmetric
# bilinear interpolation of f on a unit grid: |error| <= h^2 / 8 (|f_xx| + |f_yy|), |f''| <= a / sigma^2 for a Gaussian
# (pixel units, h = 1; a rotation and a shift of the argument change neither)
BOUND = sum(a / (4 * s * s) for a, s in zip(AMP, SIGMA_PX))


def template(u):
    """T(u): u [..., 2] in coordinate units."""
    to_px = (N_SIDE - 1) / 2
    out = 0.0
    for a, s, m in zip(AMP, SIGMA_PX, MEAN):
        d2 = ((u[..., 0] - m[0]) ** 2 + (u[..., 1] - m[1]) ** 2) * to_px ** 2
        out = out + a * np.exp(-d2 / (2 * s * s))
    return out


def rendered_images(theta, dx, t):
    """y_i(x_p) = T((x_p - t dx_i) R(theta_i)), written as eval_minibatch writes it."""
    from tvae import tables
    x_coord = tables.image_coords(N_SIDE).astype(np.float64)            # (n * n, 2): x0 along columns, x1 along rows, y up
    b = theta.shape[0]
    x = np.broadcast_to(x_coord, (b,) + x_coord.shape)
    x = x - (dx * t)[:, None, :]                                        # x = x - dx              (translate coordinates)
    rot = np.zeros((b, 2, 2))
    rot[:, 0, 0] = np.cos(theta)
    rot[:, 0, 1] = np.sin(theta)
    rot[:, 1, 0] = -np.sin(theta)
    rot[:, 1, 1] = np.cos(theta)
    x = np.einsum('bpi,bij->bpj', x, rot)                               # x = torch.bmm(x, rot)   (rotate coordinates)
    return template(x).reshape(b, 1, N_SIDE, N_SIDE)


def interior_error(images, theta, dx, t):
    """Per image: the largest |aligned - T| over the pixels whose four taps are in frame."""
    n = N_SIDE
    from tvae import tables
    want = template(tables.image_coords(n).astype(np.float64)).reshape(n, n)
    col, row = align_ref.positions(n, theta, dx, t)
    inside = (col >= 0) & (col <= n - 1) & (row >= 0) & (row <= n - 1)
    assert (inside.reshape(len(theta), -1).sum(1) > n * n // 4).all()
    err = np.abs(align_ref.sample(images, col, row)[:, 0] - want)
    return np.array([e[m].max() for e, m in zip(err, inside)])


@pytest.mark.parametrize('t,dx_factor', [(1.0, 1.0), (0.1, 10.0)])
def test_restatement_follows_the_reference_convention(t, dx_factor):
    rng = np.random.default_rng(11)
    b = 12
    theta = rng.uniform(0.4, 2.7, b) * rng.choice([-1.0, 1.0], b)
    ang, rad = rng.uniform(0, 2 * np.pi, b), rng.uniform(0.1, 0.3, b)
    dx = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    assert (np.abs(dx) <= 0.3).all()
    dx = dx * dx_factor                                                 # what the encoder would report under this t
    y = rendered_images(theta, dx, t)
    good = interior_error(y, theta, dx, t)
    print(f't = {t}: interior error {good.max():.3e}, bound {BOUND:.3e}')
    assert (good <= BOUND).all()
    wrong_theta = interior_error(y, -theta, dx, t)
    wrong_dx = interior_error(y, theta, -dx, t)
    print(f'wrong sign of theta: least error {wrong_theta.min():.3e}; of dx: {wrong_dx.min():.3e}')
    assert (wrong_theta > BOUND).all() and (wrong_dx > BOUND).all()


def test_restatement_zero_border_and_out_of_frame():
    y = np.arange(1.0, 17.0).reshape(1, 1, 4, 4)
    ident = align_ref.align_stack(y, [0.0], [[0.0, 0.0]])
    assert np.array_equal(ident, y)
    # one pixel spacing to the right in x0: the aligned image reads one column further right; the last column reads 0
    shifted = align_ref.align_stack(y, [0.0], [[2.0 / 3.0, 0.0]])
    assert np.allclose(shifted[0, 0, :, :3], y[0, 0, :, 1:], atol=1e-12) and np.allclose(shifted[0, 0, :, 3], 0, atol=1e-12)
    for bad in ([3.0, 0.0], [np.nan, 0.0], [0.0, np.inf], [1e30, 0.0]):
        assert not align_ref.align_stack(y, [0.3], [bad]).any()
    assert not align_ref.align_stack(y, [np.nan], [[0.0, 0.0]]).any()
    # quarter turn: u = x R(theta) with theta = pi / 2 sends x = (1, 0) to u = (0, 1)
    q = align_ref.align_stack(y, [np.pi / 2], [[0.0, 0.0]])
    assert np.allclose(q[0, 0], np.rot90(y[0, 0], 1), atol=1e-9) or np.allclose(q[0, 0], np.rot90(y[0, 0], -1), atol=1e-9)


# ---- segments --------------------------------------------------------------------------------------------------------------
def test_segments_on_cpu_tensors():
    from tvae import align
    labels = torch.tensor([2, 0, 5, 2, -1, 0, 2, 4, 7, 0])
    order, seg, counts = align.segments(labels, 5)
    assert order.dtype == seg.dtype == counts.dtype == torch.int32
    assert seg.tolist() == [0, 3, 3, 6, 6, 7] and counts.tolist() == [3, 0, 3, 0, 1]       # classes 1 and 3 are empty
    assert order.tolist()[:7] == [1, 5, 9, 0, 3, 6, 7]                                     # ascending index within a class
    assert sorted(order.tolist()[7:]) == [2, 4, 8]                                         # out-of-range labels: no class
    ro, rs, rc = align_ref.segments(labels.numpy(), 5)
    assert ro.tolist() == order.tolist() and rs.tolist() == seg.tolist() and rc.tolist() == counts.tolist()
    rng = np.random.default_rng(3)
    lab = rng.integers(-2, 9, 1000)
    order, seg, counts = align.segments(lab, 7)
    ro, rs, rc = align_ref.segments(lab, 7)
    assert ro.tolist() == order.tolist() and rs.tolist() == seg.tolist() and rc.tolist() == counts.tolist()
    for k in range(7):
        members = order[seg[k]:seg[k + 1]].numpy()
        assert (np.diff(members) > 0).all() and (lab[members] == k).all() and len(members) == (lab == k).sum()
    with pytest.raises(align.TvaeHipError):
        align.segments(torch.zeros(3, 2, dtype=torch.int64), 2)
    with pytest.raises(align.TvaeHipError):
        align.segments(torch.zeros(3), 2)
    with pytest.raises(align.TvaeHipError):
        align.segments(labels, 0)


def test_translation_scale():
    from tvae import align
    assert align.translation_scale('attention') == 1.0 and align.translation_scale('unimodal') == 0.1
    with pytest.raises(ValueError):
        align.translation_scale('other')


# ---- parsers ---------------------------------------------------------------------------------------------------------------
def _flags(parser):
    return sorted(s for a in parser._actions for s in a.option_strings if s not in ('-h', '--help'))


def test_class_averages_parser():
    from tvae import align
    p = align.build_parser()
    assert _flags(p) == sorted(['--stack', '--rotations', '--translations', '--clusters', '--t-inf', '--crop', '--n-clusters',
                                '--out-dir', '--write-aligned', '-d', '--device'])
    a = p.parse_args(['--stack', 's.mrcs', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy'])
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir, a.write_aligned, a.device) == ('attention', 0, None, '.', False, 0)
    a = p.parse_args(['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy',
                      '--t-inf', 'unimodal', '--crop', '40', '--n-clusters', '7', '--out-dir', 'o', '--write-aligned', '-d', '1'])
    assert (a.t_inf, a.crop, a.n_clusters, a.out_dir, a.write_aligned, a.device) == ('unimodal', 40, 7, 'o', True, 1)
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's.npy'])
    with pytest.raises(SystemExit):
        p.parse_args(['--stack', 's', '--rotations', 'r', '--translations', 't', '--clusters', 'c', '--t-inf', 'other'])
    # the script is a thin wrapper over tvae.align.run
    spec = importlib.util.spec_from_file_location('class_averages_script', os.path.join(PKG, 'class_averages.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.run is align.run and callable(mod.main)


def test_align_bench_parser():
    spec = importlib.util.spec_from_file_location('align_bench', os.path.join(ROOT, 'profiles', 'tools', 'align_bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    assert _flags(p) == sorted(['--shapes', '--clusters', '--channels', '--reps', '--warmup', '--out', '--skip-aten', '--tag'])
    a = p.parse_args([])
    assert a.shapes == ['20000x64', '100000x128'] and a.clusters == [10, 100] and a.channels == 1
    assert mod.parse_shape('20000x64') == (20000, 64)


def test_the_clustering_parsers_gained_no_flag():
    from tvae import cluster_driver
    flags = _flags(cluster_driver.build_parser('particles'))
    assert not [f for f in flags if 'average' in f or 'align' in f]


# ---- argument checks and host queries --------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from tvae import align
    y, th, dx = torch.zeros(4, 1, 8, 8), torch.zeros(4), torch.zeros(4, 2)
    with pytest.raises(align.TvaeHipError):
        align.align_stack(y, th, dx)
    with pytest.raises(align.TvaeHipError):
        align.class_averages(y, th, dx, torch.zeros(4, dtype=torch.int64), 2)


def test_queries_return_zero_for_bad_arguments():
    from tvae import _cluster_lib as CL
    from tvae import align
    for N, K, C, n in [(400, 5, 3, 33), (20000, 100, 1, 64), (100000, 10, 1, 128), (1, 1, 1, 2), (7, 3, 2, 1024)]:
        chunk = CL.query('tvae_class_average_chunk', N, K, C, n)
        assert chunk == align.chunk_members(N, K, C, n) and 1 <= chunk <= 256
        slots = N // chunk + K
        ints = (K + 1 + slots + 3) // 4 * 4
        assert CL.query('tvae_class_average_ws_floats', N, K, C, n) == ints + slots * C * n * n
        # the chunking is a function of the sizes alone, and the same for every K
        assert chunk == CL.query('tvae_class_average_chunk', N, K + 1, C, n)
    for bad in [(400, 5, 1, 1), (400, 5, 1, 1025), (400, 0, 1, 16), (400, 5, 0, 16), (0, 5, 1, 16), (-1, 5, 1, 16),
                (400, 65536, 1, 16), (400, 5, 1025, 16), ((1 << 24) + 1, 5, 1, 16), (1 << 24, 5, 64, 1024)]:
        assert CL.query('tvae_class_average_ws_floats', *bad) == 0, bad
        assert CL.query('tvae_class_average_chunk', *bad) == 0, bad
