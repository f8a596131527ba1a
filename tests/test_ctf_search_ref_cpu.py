"""The CTF-aware hard search without the kernel: the selection rule of tests/ctf_search_ref.py in its two statements, the claim
that the CTF score recovers planted shifts that the plain score loses (fp64 numpy throughout), the parsers of refine_poses.py
and reclassify_particles.py, and the argument rules of tvae.ctf.select_poses."""
import json
import os

import numpy as np
import pytest
import torch

import classify_ref
import ctf_pose_ref as R
import ctf_search_ref as SR
from conftest import GOLDEN

F32 = np.float32


# ---- 1. the rule of a slot: the serial loop and the order-free arg-max ------------------------------------------------------------
def _tied_tables(rng, rows, cnd, ci):
    """Random score rows drawn from a handful of values, so that maxima repeat, with the special rows planted: everything equal,
    equal maxima off centre and on both sides of index 64, a non-finite centre, nothing finite, +0 against -0."""
    flat = rng.choice(np.array([-1.0, -0.0, 0.0, 0.25, 0.5, 0.75, np.nan, np.inf, -np.inf], dtype=F32), (rows, cnd))
    flat[0] = 0.5
    if cnd > 2:
        flat[1] = -1.0
        flat[1, [cnd - 1, 1]] = 0.75
    flat[2] = 0.25
    flat[2, ci] = np.nan
    flat[3] = np.nan
    flat[3, 0] = np.inf
    flat[4] = -0.0
    flat[4, cnd - 1] = 0.0
    if cnd > 70:
        flat[5] = -1.0
        flat[5, [3, 67]] = 0.5
        flat[6] = -1.0
        flat[6, [ci, 2]] = 0.5
    return flat


@pytest.mark.parametrize('A,S', [(0, 0), (1, 0), (2, 1), (3, 2), (0, 8)])
def test_serial_and_order_free_rules_agree(A, S):
    NS = 2 * S + 1
    cnd, ci = (2 * A + 1) * NS * NS, (A * NS + S) * NS + S
    flat = _tied_tables(np.random.default_rng(cnd), 200, cnd, ci)
    for row in flat:
        a, b = SR.slot_serial(row, ci), SR.slot_order_free(row, ci)
        assert a[0] == b[0] and np.array_equal(np.array(a[1:]).view(np.int32), np.array(b[1:]).view(np.int32)), row
    assert SR.slot_serial(flat[0], ci)[0] == ci                  # all equal: the centre
    assert SR.slot_serial(flat[3], ci) == (ci, 0, 0)             # nothing finite
    if cnd > 2:
        assert SR.slot_serial(flat[1], ci)[0] == (ci if ci in (1, cnd - 1) else 1)
        got = SR.slot_serial(flat[2], ci)
        assert got[0] == (1 if ci == 0 else 0) and got[1] == -np.inf and got[2] == F32(0.25)
    if cnd > 70:
        assert SR.slot_serial(flat[5], ci)[0] == (ci if ci in (3, 67) else 3)       # across the lane passes: the lower index
        assert SR.slot_serial(flat[6], ci)[0] == ci


def test_select_ref_with_either_rule_and_either_power():
    rng = np.random.default_rng(4)
    N, M, A, S, K, n = 9, 3, 2, 1, 4, 12
    NA, NS = 2 * A + 1, 2 * S + 1
    num = rng.choice(np.array([-1.0, 0.5, 1.0, 2.0], dtype=F32), (N, M, NA, NS, NS))
    ppc = rng.choice(np.array([0.0, 1.0, 4.0], dtype=F32), (N, M, NA))
    yy = rng.choice(np.array([0.0, 1.0, 4.0], dtype=F32), N)
    cand = rng.integers(-1, K + 1, (N, M))
    cand[0] = -1
    theta, dx = rng.standard_normal(N).astype(F32), rng.standard_normal((N, 2)).astype(F32)
    a = SR.select_ref(num, ppc, yy, cand, theta, dx, n, K, A, S, 1.5, 0.05)
    b = SR.select_ref(num, ppc, yy, cand, theta, dx, n, K, A, S, 1.5, 0.05, SR.slot_order_free)
    c = SR.select_ref(num, np.broadcast_to(ppc[..., None, None], num.shape), yy, cand, theta, dx, n, K, A, S, 1.5, 0.05)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) and np.array_equal(a[k].view(np.int32), c[k].view(np.int32)), k
    # an image with no valid slot: its pose bit for bit, slot 0's value, zeros
    assert a['cls'][0] == -1 and not a['best'][0].any() and not a['score'][0].any()
    assert a['theta'][0].view(np.int32) == theta[0].view(np.int32) and np.array_equal(a['dx'][0].view(np.int32), dx[0].view(np.int32))


# ---- 2. the planted stack -------------------------------------------------------------------------------------------------------------
PLANTED = dict(seed=11, noise=0.5, defoci=4, N=48, n=24, K=2)


def test_ctf_score_recovers_planted_shifts_the_plain_score_loses():
    """48 images of 24 x 24 in two classes, each displaced by a whole-pixel shift in [-1, 1]^2 from the start pose, seen through
    four defoci whose first zero lies between a quarter and a half of Nyquist, white noise of 0.5 added.  One hard search
    (A = 0, S = 1, both classes as candidates) with the plain score on the raw images and one with the CTF score."""
    q = PLANTED
    p = R.planted_ctf(q['noise'], q['defoci'], q['seed'], N=q['N'], n=q['n'], K=q['K'], A=0, S=1)
    cand = np.stack([p['cls'], 1 - p['cls']], 1)
    t, A, S, n, K = p['t'], 0, 1, q['n'], q['K']
    f32 = lambda a: np.asarray(a).astype(F32)
    plain = classify_ref.classify(p['Y'], p['theta'], p['dx'], cand, p['refs'], t, A, 0.05, S)
    num, pp, yy, _ = R.ctf_tables(p['Y'], R.filtered(p['Y'], p['coef']), p['theta'], p['dx'], cand, p['refs'], p['coef'], t, A, 0.05, S)
    a = SR.select_ref(f32(plain['num']), f32(plain['pp']), f32(plain['yy']), cand, p['theta'], p['dx'], n, K, A, S, t, 0.05)
    b = SR.select_ref(f32(num), f32(pp[..., 0, 0]), f32(yy), cand, p['theta'], p['dx'], n, K, A, S, t, 0.05)
    want = p['want'][:, 1:]
    hit_plain, hit_ctf = int((a['best'][:, 2:] == want).all(1).sum()), int((b['best'][:, 2:] == want).all(1).sum())
    print(f'planted shifts recovered: plain {hit_plain} / {q["N"]}, ctf {hit_ctf} / {q["N"]}')
    assert hit_ctf > hit_plain                                # the fp64 reference gave 28 / 48 plain and 43 / 48 with the CTF score


# ---- 3. the parsers -------------------------------------------------------------------------------------------------------------------
def _flags(parser):
    return [list(a.option_strings) for a in parser._actions if a.dest != 'help']


def test_default_parsers_are_unchanged_and_ctf_adds_three_flags():
    from tvae import classify, refine
    want = json.load(open(os.path.join(GOLDEN, 'cli_flags_class_tools.json')))
    for name, mod in (('refine', refine), ('classify', classify)):
        plain, ctf = mod.build_parser(), mod.build_parser(ctf=True)
        assert _flags(plain) == [a['flags'] for a in want[name]['actions']], name
        assert plain.prog == ctf.prog == want[name]['prog']
        assert _flags(ctf)[:len(_flags(plain))] == _flags(plain)
        assert _flags(ctf)[len(_flags(plain)):] == [['--ctf'], ['--wiener-tau'], ['--scale']], name
        args = ctf.parse_args(['--stack', 's.npy', '--rotations', 'r.npy', '--translations', 't.npy', '--clusters', 'c.npy'])
        assert args.ctf is None and args.wiener_tau == 0.1 and args.scale == 1


# ---- 4. the argument rules of select_poses --------------------------------------------------------------------------------------------
def test_select_poses_checks_its_arguments_before_any_library_call(monkeypatch):
    from tvae import _cluster_lib as CL
    from tvae import ctf
    from tvae._lib import TvaeHipError

    def never(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(CL, 'call', never)
    monkeypatch.setattr(CL, 'lib', never)
    N, M, A, S, K, n = 4, 2, 1, 1, 3, 8
    NA, NS = 2 * A + 1, 2 * S + 1
    ok = dict(num=torch.zeros(N, M, NA, NS, NS), pp=torch.zeros(N, M, NA), yy=torch.ones(N), candidates=torch.zeros(N, M, dtype=torch.int64),
              theta=torch.zeros(N), dx=torch.zeros(N, 2), n=n, n_clusters=K, t_scale=1.0, angle_steps=A, angle_step=0.1, shift=S)
    with pytest.raises(TvaeHipError, match='select_poses: num must be a contiguous CUDA fp32 tensor'):
        ctf.select_poses(**ok)                                # no CPU fallback
    monkeypatch.setattr(CL, 'is_f32', lambda t, contiguous=True: torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous())
    bad = [dict(num=ok['num'].double()), dict(pp=ok['pp'].double()), dict(yy=ok['yy'].to(torch.float16)), dict(theta=ok['theta'].double()),
           dict(dx=ok['dx'].to(torch.int32)), dict(num=ok['num'].transpose(3, 4)[..., :2]), dict(candidates=torch.zeros(N, M)),
           dict(candidates=torch.zeros(N, M, dtype=torch.bool)), dict(candidates=torch.zeros(N + 1, M, dtype=torch.int64)),
           dict(candidates=torch.zeros(N, 65, dtype=torch.int64)), dict(candidates=torch.zeros(N, dtype=torch.int64)),
           dict(num=torch.zeros(N, M, NA, NS, NS + 1)), dict(num=torch.zeros(N, M, NA + 1, NS, NS)), dict(pp=torch.zeros(N, M, NA + 1)),
           dict(pp=torch.zeros(N, M, NA, NS)), dict(pp=torch.zeros(N, M, NA, NS, NS + 2)), dict(yy=torch.ones(N, 1)),
           dict(theta=torch.zeros(N + 1)), dict(dx=torch.zeros(N, 3)), dict(n=1), dict(n=129), dict(n_clusters=0), dict(n_clusters=65536),
           dict(t_scale=0.0), dict(t_scale=float('nan')), dict(angle_step=float('inf')),
           dict(angle_steps=33, num=torch.zeros(N, M, 67, NS, NS), pp=torch.zeros(N, M, 67)),
           dict(shift=9, num=torch.zeros(N, M, NA, 19, 19))]
    for kw in bad:
        with pytest.raises(TvaeHipError, match='select_poses'):
            ctf.select_poses(**dict(ok, **kw))
    import contextlib
    monkeypatch.setattr(torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    for shape in ((N, M, NA), (N, M, NA, NS, NS)):            # both shapes of pp pass the checks and reach the library
        with pytest.raises(AssertionError, match='the library was called'):
            ctf.select_poses(**dict(ok, pp=torch.zeros(shape)))
