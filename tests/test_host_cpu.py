"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol of include/tvae_hip.h,
host tables equal the oracle's, the drop-in classes reproduce the reference's parameter names / shapes /
default initialisation, checkpoints pickle as `src.models.*`, and the product path refuses CPU tensors."""
import io
import itertools
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_err, tdict
from oracle import tvae_oracle as O


def test_library_exports_every_declared_symbol():
    from tvae import _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_hip.h')).read()
    declared = sorted(set(re.findall(r'\b(?:int|long)\s+(tvae_\w+)\s*\(', hdr)))
    assert declared == sorted(_lib.exported_symbols())
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert L.tvae_abi_version() == _lib.ABI_VERSION == 7


def _declared_args(hdr, name):
    """The parameter declarators of entry point `name` in the header text, the trailing stream included."""
    m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', hdr, re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(',')]


def test_signature_arity_matches_header():
    from tvae import _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_hip.h')).read()
    for name, sig in _lib.SIGNATURES.items():
        args = _declared_args(hdr, name)
        assert args[-1].startswith('tvae_stream_t'), name
        assert len(args) - 1 == len(sig), (name, len(args) - 1, len(sig))
        for a, c in zip(args[:-1], sig):
            if c == 'p':
                assert '*' in a, (name, a)
            elif c == 'f':
                assert a.startswith('float ') and '*' not in a, (name, a)
            elif c == 'l':
                assert a.startswith('long '), (name, a)
            else:
                assert a.startswith('int ') and '*' not in a, (name, a)


def test_arg_names_match_header():
    """ARG_NAMES spells the header's parameter names (the last identifier of each declarator), in order, one per code."""
    from tvae import _lib
    hdr = open(os.path.join(ROOT, 'include', 'tvae_hip.h')).read()
    assert set(_lib.ARG_NAMES) == {'tvae_linear_fwd_x6', 'tvae_linear_dgrad_x6', 'tvae_linear_wgrad_x6'}
    for name in _lib.ARG_NAMES:
        declared = [re.findall(r'[A-Za-z_]\w*', a)[-1] for a in _declared_args(hdr, name)[:-1]]
        rest, required = _lib._BINDINGS[name]
        names, defaults = list(rest[0]), list(rest[0].values())
        assert names == declared and len(names) == len(_lib.SIGNATURES[name]), name
        for n in range(len(names) + 1):                # behind n positional arguments: the remaining defaults, the required names
            assert list(rest[n].items()) == list(zip(names, defaults))[n:]
            assert required[n] == tuple(k for k, d in rest[n].items() if d is _lib._REQUIRED)
        # required: the leading run up to slope (wgrad: accumulate), parts, and every float; the others default to NULL / 0
        lead = names.index('accumulate' if 'wgrad' in name else 'slope') + 1
        for i, (n, c, d) in enumerate(zip(names, _lib.SIGNATURES[name], defaults)):
            if i < lead or n == 'parts' or c == 'f':
                assert d is _lib._REQUIRED, (name, n)
            else:
                assert d is None if c == 'p' else (d == 0 and isinstance(d, int)), (name, n)


def test_bind_args_binds_like_the_positional_calls():
    """Keyword calls of the three dense entry points against the complete positional tuples they replaced (sentinels in
    place of tensors: bind_args looks at no argument), and the refusals."""
    from tvae._lib import TvaeHipError, bind_args

    class S:
        def __init__(self, n):
            self.n = n

        def __repr__(self):
            return self.n
    w3t, d, dfeat, d_bnd, F_, Nt, Ff, ldn, p_f, SL = S('w3t'), S('d'), S('dfeat'), S('d_bnd'), 512, 6272, 1026, 6336, 2, 0.01
    # the Fourier data gradient of DecoderFn.backward
    full = (w3t, d, None, None, dfeat, F_, Nt, Ff, ldn, ldn, 0, SL,
            None, None, None, None, 0, None, None, None, None, None, 0, None, 0, None, None, None, None, p_f,
            None, None, None, d_bnd, None)
    assert bind_args('tvae_linear_dgrad_x6', (w3t, d, None, None, dfeat, F_, Nt, Ff, ldn, ldn, 0, SL),
                     dict(parts=p_f, x_amax=d_bnd)) == full
    assert bind_args('tvae_linear_dgrad_x6', full, {}) == full                 # a complete positional tuple: unchanged
    # the data gradient with the row sums of the layer behind (rs_*)
    w3r, Hr, aux, dXb, gy, csr, rs_part, wor, gys, rs_db, rs_dwo = (S(n) for n in 'w3r Hr aux dXb gy csr rs_part wor gys rs_db rs_dwo'.split())
    Mr, N, K = 160, 384, 128
    full = (w3r, Hr, None, aux, dXb, Mr, N, K, N, N, 1, SL, None, None, None,
            None, 0, None, gy, csr, None, None, 0, rs_part, 98304, wor, gys, rs_db, rs_dwo, 3, None, None, None, None, None)
    assert bind_args('tvae_linear_dgrad_x6', (w3r, Hr, None, aux, dXb, Mr, N, K, N, N, 1, SL),
                     dict(vg_gy=gy, vg_csum=csr, rs_part=rs_part, rs_part_floats=98304, rs_wo=wor, rs_gysum=gys, rs_db=rs_db,
                          rs_dwo=rs_dwo, parts=3)) == full
    # a forward with the recomputed first layer (*va), sign bits and parts
    w3, b, Y, xr, Wc, bc, LB, bits = (S(n) for n in 'w3 b Y xr Wc bc LB bits'.split())
    va = dict(va_xr=xr, va_wc=Wc, va_bc=bc, va_lb=LB, va_np=196)
    full = (w3, None, b, None, Y, 512, Nt, 512, Nt, Nt, 1, SL, None, None, None, xr, Wc, bc, LB, 196, bits, 2, None, None)
    assert bind_args('tvae_linear_fwd_x6', (w3, None, b, None, Y, 512, Nt, 512, Nt, Nt, 1, SL),
                     dict(**va, sign_bits=bits, parts=2)) == full
    assert bind_args('tvae_linear_fwd_x6', full[:22], {}) == full             # ... and the all-pointer tail left off
    # a weight gradient with rd_* and the bounds
    dW, ws, W, rowdot, am, xm = (S(n) for n in 'dW ws W rowdot am xm'.split())
    full = (d, None, dW, ws, 1 << 24, 512, Nt, 512, ldn, ldn, 0, None, None, 1, SL, None, None, None, None, 0, bits, 2,
            W, 512, rowdot, am, xm, 1)
    assert bind_args('tvae_linear_wgrad_x6', (d, None, dW, ws, 1 << 24, 512, Nt, 512, ldn, ldn, 0),
                     dict(vg_act=1, vg_slope=SL, vg_bits=bits, parts=2, rd_w=W, rd_ldw=512, rd_rowdot=rowdot, a_amax=am,
                          x_amax=xm, x_amax_rows=1)) == full
    lead = (w3, None, b, None, Y, 512, Nt, 512, Nt, Nt, 1, SL)
    for name, args, kwargs, word in (
            ('tvae_linear_fwd_x6', lead, dict(parts=2, col_z=Y), 'col_z'),                    # an unknown keyword
            ('tvae_linear_fwd_x6', lead, dict(parts=2, slope=SL), 'slope'),                   # given twice
            ('tvae_linear_fwd_x6', lead, dict(x_amax=xm), 'parts'),                           # a required one missing
            ('tvae_linear_fwd_x6', lead[:-1], dict(parts=2), 'slope'),
            ('tvae_linear_wgrad_x6', (d, None, dW, ws, 1 << 24, 512, Nt, 512, ldn, ldn, 0), dict(parts=2), 'vg_slope'),
            ('tvae_linear_fwd_x6', full, {}, '28'),                                           # too many positional arguments
            ('tvae_act_bwd', (d, d, d, 4, 1), dict(slope=SL), 'slope')):                      # a keyword without ARG_NAMES
        with pytest.raises(TvaeHipError, match=name + '.*' + word):
            bind_args(name, args, kwargs)


def test_product_path_refuses_cpu_tensors():
    import src.models as M
    from tvae import _lib
    gc = M.GroupConv(1, 2, 5, output_rot_dim=4)
    with pytest.raises(RuntimeError):
        gc(torch.rand(1, 1, 8, 8), 'cpu')
    with pytest.raises(_lib.TvaeHipError):
        _lib.call('tvae_act_bwd', torch.zeros(4), torch.zeros(4), torch.zeros(4), 4, 1, 0.01)
    gen = M.SpatialGenerator(2, 8)
    with pytest.raises(RuntimeError):
        gen(torch.zeros(1, 4, 2), torch.zeros(1, 2))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'target-vae_amd')
    for d, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith('.py'):
                src = open(os.path.join(d, f)).read()
                assert 'oracle' not in src.replace('no CPU fallback; use oracle', ''), os.path.join(d, f)


@pytest.mark.parametrize('k,R', [(5, 4), (28, 8), (9, 16), (64, 8)])
def test_tap_tables_match_oracle(k, R):
    from tvae import tables
    i1, w1 = tables.rotation_taps(k, R)
    i2, w2 = O.rotation_taps(k, R)
    assert np.array_equal(i1, i2.astype(np.int32)) and np.array_equal(w1, w2)
    if k > 28:
        return                                   # dense check below is O(R k^4) memory
    ptr, er, ed, ew = tables.rotation_taps_csr(k, R)
    dense = np.zeros((R, k * k, k * k), dtype=np.float64)          # [r][dst][src]
    for t in range(4):
        ok = i1[:, :, t] >= 0
        rr, dd = np.nonzero(ok)
        np.add.at(dense, (rr, dd, i1[rr, dd, t]), w1[rr, dd, t])
    dense2 = np.zeros_like(dense)
    for s in range(k * k):
        for e in range(ptr[s], ptr[s + 1]):
            dense2[er[e], ed[e], s] += ew[e]
    assert np.allclose(dense, dense2, atol=1e-7)


@pytest.mark.parametrize('R,refine,normal,tp', [(8, True, False, np.pi), (16, True, True, np.pi / 4),
                                                (4, False, False, np.pi)])
def test_prior_tables_match_oracle(R, refine, normal, tp):
    from tvae import tables
    assert np.allclose(tables.rotation_log_prior(R, refine, tp, normal), O.rotation_log_prior(R, refine, tp, normal),
                       rtol=1e-6, atol=1e-6)
    off = O.rotation_offsets(R) if refine else np.zeros(R, np.float32)
    assert np.array_equal(tables.rotation_offsets(R, refine), off)
    for Ho in (17, 33, 8):
        s = 2.0 / 27
        assert np.array_equal(tables.translation_grid(Ho, s), O.translation_grid(Ho, s))
        G = torch.from_numpy(O.translation_grid(Ho, s))
        p_t = torch.distributions.Normal(torch.tensor([0.0]), torch.tensor([0.1])).log_prob(G).sum(1)
        p_r = torch.from_numpy(O.rotation_log_prior(R, refine, tp, normal))
        ref = torch.log_softmax((p_t.view(1, -1) + p_r.view(R, 1)).reshape(-1), 0)
        got = tables.joint_log_prior(Ho, s, tables.rotation_log_prior(R, refine, tp, normal))
        assert np.allclose(got, ref.numpy(), rtol=1e-5, atol=1e-4)
    assert np.array_equal(tables.image_coords(28), O.image_coords(28).numpy())


def test_default_init_and_names_match_reference():
    """Same seed + same construction order (generator first, train_mnist.py:522,551) => identical parameters to
    the reference-generated fixture; state_dict names / shapes are the reference's."""
    import src.models as M
    fx = load_golden('step_mnist28_P8_init')
    torch.manual_seed(0)
    gen = M.SpatialGenerator(2, 512, n_out=1, num_layers=2, resid=False, fourier_expansion=False, sigma=2.0 / 27)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        28, 1, 2, kernels_num=128, kernels_size=28, padding=8, groupconv=8, rot_refinement=True, theta_prior=np.pi,
        normal_prior_over_r=False)
    e_ref, d_ref = tdict(fx, 'e.'), tdict(fx, 'd.')
    assert sorted(enc.state_dict()) == sorted(e_ref) and sorted(gen.state_dict()) == sorted(d_ref)
    for k_, v in enc.state_dict().items():
        assert tuple(v.shape) == tuple(e_ref[k_].shape) and torch.equal(v, e_ref[k_]), k_
    for k_, v in gen.state_dict().items():
        assert tuple(v.shape) == tuple(d_ref[k_].shape) and torch.equal(v, d_ref[k_]), k_


def test_fourier_generator_names():
    import src.models as M
    fx = load_golden('step_mnist28_P16_fourier_normal')
    gen = M.SpatialGenerator(2, 64, num_layers=2, fourier_expansion=True, sigma=2.0 / 27)
    assert sorted(gen.state_dict()) == sorted(tdict(fx, 'd.'))
    fx = load_golden('decoder_resid')
    gen = M.SpatialGenerator(3, 64, num_layers=3, resid=True)
    assert sorted(gen.state_dict()) == sorted(tdict(fx, 'p.'))


def test_whole_module_pickle_roundtrip(tmp_path):
    """Checkpoints are whole-module pickles (reference train_mnist.py:672-681, src/utils.py:37-48) with classes at
    src.models.*; device tables must not leak into them."""
    import src.models as M
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(28, 1, 2, kernels_num=8, kernels_size=28,
                                                                    padding=8, groupconv=8, rot_refinement=True)
    enc.__dict__['_tb_cache'] = {'x': object()}
    p = tmp_path / 'inference.sav'
    torch.save(enc, p)
    raw = open(p, 'rb').read()
    assert b'src.models' in raw and b'InferenceNetwork_AttentionTranslation_AttentionRotation' in raw
    enc2 = torch.load(p, weights_only=False)
    assert '_tb_cache' not in enc2.__dict__
    for (k1, v1), (k2, v2) in zip(enc.state_dict().items(), enc2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    gen = M.SpatialGenerator(2, 16, num_layers=2, fourier_expansion=True, sigma=0.1)
    buf = io.BytesIO()
    torch.save(gen, buf)
    buf.seek(0)
    gen2 = torch.load(buf, weights_only=False)
    assert float(gen2.embed_latent.sigma) == pytest.approx(0.1)


def test_flat_adam_views_and_update_cpu():
    """FlatAdam bookkeeping (flat views, zero_grad, step counting) with a torch update function on CPU; the default
    update function is the HIP kernel (checked on the GPU in test_hip_primitives.py::test_adam_flat)."""
    from tvae import optim
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    calls = []

    def upd(p, g, m, v, step, lr, b1, b2, eps, scale):
        calls.append(step)
        O.adam_update([p], [g * scale], [m], [v], step, lr, b1, b2, eps)

    opt = optim.FlatAdam(ps, lr=1e-2, update_fn=upd)
    ropt = torch.optim.Adam(ref, lr=1e-2)
    assert ps[0].data_ptr() == opt.flat_p.data_ptr() and ps[1].grad.data_ptr() == opt.flat_g[64:].data_ptr()
    assert all(p.data_ptr() % 256 == opt.flat_p.data_ptr() % 256 for p in ps)
    for it in range(3):
        loss = sum(((p * (i + 1 + it)) ** 2).sum() for i, p in enumerate(ps))
        loss.backward()
        rl = sum(((p * (i + 1 + it)) ** 2).sum() for i, p in enumerate(ref))
        rl.backward()
        opt.step(); opt.zero_grad()
        ropt.step(); ropt.zero_grad()
        assert float(opt.flat_g.abs().sum()) == 0.0
    assert calls == [1, 2, 3]
    for p, r in zip(ps, ref):
        assert rel_err(p.detach(), r.detach()) < 1e-6
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='max', factor=0.5, patience=0)
    sched.step(1.0); sched.step(0.0)
    assert opt.param_groups[0]['lr'] == pytest.approx(5e-3)


def test_flat_adam_takes_gradients_over_when_grads_are_none():
    """zero_grad(set_to_none=True), the training loops' form (round 4): the backward's AccumulateGrad nodes keep the gradient
    tensors (no add into a zeroed buffer); step() -- or the early bucket's hook, before it posts its all-reduce -- gathers them
    into the flat buffer.  Same trajectory as torch.optim.Adam; a parameter without a gradient gets a zero slice; the early
    bucket is posted with the gathered values."""
    from tvae import optim
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 2))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]

    def upd(p, g, m, v, step, lr, b1, b2, eps, scale):
        O.adam_update([p], [g * scale], [m], [v], step, lr, b1, b2, eps)

    class Reducer:
        active = True

        def __init__(self):
            self.begun = []

        def begin(self, seg):
            self.begun.append(seg.clone())

        def __call__(self, flat_g, start=0):
            return 1.0

    red = Reducer()
    opt = optim.FlatAdam(ps, lr=1e-2, update_fn=upd, reducer=red, early_params=2)
    ropt = torch.optim.Adam(ref, lr=1e-2)
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in ps)
    for it in range(3):
        use = ps if it != 1 else ps[:2]                  # step 1: the last parameter gets no gradient
        ruse = ref if it != 1 else ref[:2]
        sum(((p * (i + 1 + it)) ** 2).sum() for i, p in enumerate(use)).backward()
        sum(((p * (i + 1 + it)) ** 2).sum() for i, p in enumerate(ruse)).backward()
        assert len(red.begun) == it + 1                  # the early bucket (two parameters) was posted from inside the backward
        assert torch.equal(red.begun[-1][:12], ref[0].grad.reshape(-1)) and torch.equal(red.begun[-1][64:69], ref[1].grad)
        assert ps[0].grad.data_ptr() == opt.flat_g.data_ptr()
        opt.step()
        for p, r in zip(ps, ref):
            if r.grad is None:
                assert float(p.grad.abs().sum()) == 0.0
                r.grad = torch.zeros_like(r)             # (FlatAdam steps every parameter, with a zero gradient if it got none)
            else:
                assert torch.equal(p.grad, r.grad) and p.grad.data_ptr() >= opt.flat_g.data_ptr()
        assert float(opt.flat_g[12:64].abs().sum()) == 0.0           # padding never written
        ropt.step()
        opt.zero_grad(set_to_none=True)
        ropt.zero_grad(set_to_none=True)
    for p, r in zip(ps, ref):
        assert rel_err(p.detach(), r.detach()) < 1e-6


def test_resident_shard_plan_visits_every_image_once():
    """Shard-resident batches: every image exactly once per epoch, each rank only its own rows, global minibatch sizes
    known to every rank without communication."""
    from tvae import dp
    for n, gb, world in ((37, 16, 2), (100, 32, 8), (5, 6, 4), (64, 16, 1), (13, 6, 2), (60000, 100, 8),
                         (60000, 100, 3), (7, 2, 4), (1003, 100, 8), (9, 1, 4), (0, 4, 2)):
        plan = dp.shard_plan(n, gb, world)
        assert sum(sum(c) for c in plan) == n
        # the reference's loop: ceil(N / gb) minibatches, batch i holds min(gb, N - i*gb) images (train_mnist.py:586);
        # also when gb % world != 0 (driver default 100 over 8 ranks) and when gb < world
        assert len(plan) == (n + gb - 1) // gb
        for i, c in enumerate(plan):
            g = min(gb, n - i * gb)
            assert sum(c) == g
            assert max(c) - min(c) <= 1 or n - i * gb < gb + world      # even shares (the very tail may be ragged)
        for r in range(world):
            r0, r1 = dp.shard_bounds(n, r, world)
            assert sum(c[r] for c in plan) == r1 - r0
        glob = dp.resident_global_batches(n, gb, world, 3, 1)
        if n == 0:
            assert glob == []
            continue
        assert sorted(torch.cat(glob).tolist()) == list(range(n))
        assert [len(g) for g in glob] == [sum(c) for c in plan]
        assert all(len(g) <= gb for g in glob)
    assert dp.shard_bounds(10, 3, 4) == (8, 10) and dp.shard_bounds(10, 0, 4) == (0, 3)


def test_shard_slices_cover_every_minibatch():
    from tvae import dp
    for n, gb, world in ((10, 4, 2), (37, 8, 4), (5, 8, 2), (256, 256, 8)):
        per_rank = [list(dp.shard_slices(n, gb, r, world)) for r in range(world)]
        nb = (n + gb - 1) // gb
        assert all(len(p) == nb for p in per_rank)
        for b in range(nb):
            g = per_rank[0][b][2]
            idx = sorted(i for r in range(world) for i in range(per_rank[r][b][0], per_rank[r][b][1]))
            assert idx == list(range(b * gb, b * gb + g))
    assert torch.equal(dp.epoch_permutation(50, 3, 7), dp.epoch_permutation(50, 3, 7))
    assert not torch.equal(dp.epoch_permutation(50, 3, 7), dp.epoch_permutation(50, 3, 8))


def test_cli_flags_match_reference():
    """Every flag of the four reference scripts exists with the same option strings, default, choices and type
    (tests/golden/cli_flags.json is generated from the reference's own argparse objects)."""
    import json
    from tvae import driver
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'cli_flags.json')))
    for script, flags in ref.items():
        parser = driver.build_parser(script.replace('train_', ''))
        mine = {a.dest: a for a in parser._actions if a.dest != 'help'}
        for dest, spec in flags.items():
            assert dest in mine, (script, dest)
            a = mine[dest]
            assert list(a.option_strings) == spec['flags'], (script, dest)
            assert a.default == spec['default'], (script, dest, a.default, spec['default'])
            assert (list(a.choices) if a.choices else None) == spec['choices'], (script, dest)
            assert getattr(a.type, '__name__', None) == spec['type'], (script, dest)
            assert (a.nargs == 0) == spec['nargs0'], (script, dest)
        assert set(mine) - set(flags) == {'seed', 'synthetic', 'graph', 'no_graph'}, script      # this framework's own additions


def test_ctf_filter_matches_reference_golden():
    """src/ctf.py (product, host preprocessing) against filters generated by the reference's src/ctf.py."""
    import pandas as pd
    import src.ctf as C
    fx = load_golden('ctf_filters')
    cols = ['defocus', 'cs', 'voltage', 'apix', 'bfactor', 'ampcont', 'dfdiff', 'dfang']
    params = pd.DataFrame({c: fx[c] for c in cols})
    n = int(fx['n'])
    assert rel_err(C.ctf_filter(params, n, n), fx['filters']) < 1e-6


def test_mrc_codec_against_reference_written_files(tmp_path):
    """src/mrc.py reads stacks written by the reference codec (tests/golden/stack_ref*.mrc[s]) and writes
    byte-identical files; memory-mapped rank shards cover the stack exactly."""
    import src.mrc as mrc
    fx = load_golden('mrc_arrays')
    gdir = os.path.join(ROOT, 'tests', 'golden')
    raw = open(os.path.join(gdir, 'stack_ref.mrcs'), 'rb').read()
    arr, hdr, ext = mrc.parse(raw)
    assert (hdr.nx, hdr.ny, hdr.nz, hdr.mode, hdr.next) == (7, 6, 5, 2, 0) and ext == b''
    assert np.array_equal(arr, fx['stack']) and abs(hdr.xlen - 1.5) < 1e-6 and abs(hdr.rms - fx['stack'].std()) < 1e-6
    out = tmp_path / 'w.mrcs'
    with open(out, 'wb') as f:
        mrc.write(f, fx['stack'], ax=1.5, ay=2.5, az=3.5)
    assert open(out, 'rb').read() == raw                                   # byte-identical to the reference writer
    raw2 = open(os.path.join(gdir, 'stack_ref_ext.mrc'), 'rb').read()
    a2, h2, e2 = mrc.parse(raw2)
    assert h2.mode == 1 and h2.next == 16 and e2 == b'0123456789abcdef' and np.array_equal(a2, fx['single'])
    mm, h = mrc.open_stack(os.path.join(gdir, 'stack_ref.mrcs'))
    assert mm.shape == (5, 6, 7) and np.array_equal(np.asarray(mm), fx['stack'])
    parts = [mrc.read_shard(os.path.join(gdir, 'stack_ref.mrcs'), r, 2) for r in range(2)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), fx['stack'])
    assert [p[1][:2] for p in parts] == [(0, 3), (3, 5)]


def test_driver_loads_only_its_shard_from_mrc_and_npy(tmp_path):
    """The particles driver opens MRC / .npy stacks lazily and reads, crops and normalises only the rows of its rank
    (dp.shard_bounds); the shards of two ranks tile what a single process loads, for both file formats."""
    import src.mrc as mrc
    from tvae import dp, driver
    g = np.random.default_rng(0)
    stack = g.normal(size=(11, 24, 24)).astype(np.float32)
    with open(tmp_path / 's.mrcs', 'wb') as f:
        mrc.write(f, stack)
    np.save(tmp_path / 's.npy', stack)
    for path in ('s.mrcs', 's.npy'):
        args = driver.build_parser('particles').parse_args(['--train-path', str(tmp_path / path), '--train-portion', '0.75',
                                                            '--crop', '20', '--normalize'])
        tr, te, name, n_raw, n_tr, n_te = driver._load_arrays('particles', args)
        assert (n_tr, n_te, n_raw) == (8, 3, 24) and tuple(tr.shape) == (8, 1, 20, 20) and tuple(te.shape) == (3, 1, 20, 20)
        ref = stack[:8, 2:22, 2:22]
        ref = (ref - ref.reshape(8, -1).mean(1)[:, None, None]) / ref.reshape(8, -1).std(1)[:, None, None]
        assert np.allclose(tr[:, 0].numpy(), ref, atol=1e-6)
        parts = [driver._load_arrays('particles', args, (r, 2)) for r in range(2)]
        assert torch.equal(torch.cat([p[0] for p in parts]), tr) and torch.equal(torch.cat([p[1] for p in parts]), te)
        assert [tuple(p[0].shape)[0] for p in parts] == [b - a for a, b in (dp.shard_bounds(8, r, 2) for r in range(2))]
        assert all(p[4:] == (8, 3) for p in parts)


def test_shape_validation_happens_before_any_launch():
    """Mis-shaped operands raise on the host (ValueError) without touching the GPU library."""
    from tvae import ops
    with pytest.raises(ValueError):
        ops.EncoderFn.apply(torch.zeros(2, 1, 8, 9), torch.zeros(4, 1, 1, 5, 5), torch.zeros(4), torch.zeros(4, 4),
                            torch.zeros(4), torch.zeros(7, 4), torch.zeros(7), 8, 1, 1)
    with pytest.raises(ValueError):
        ops.EncoderFn.apply(torch.zeros(2, 1, 8, 8), torch.zeros(4, 1, 1, 5, 5), torch.zeros(4), torch.zeros(4, 4),
                            torch.zeros(4), torch.zeros(7, 4), torch.zeros(7), 5, 1, 1)       # R not in {4,8,16}
    tb = type('T', (), dict(R=4, P=9))()
    with pytest.raises(ValueError):
        ops.HeadFn.apply(torch.zeros(7, 10), torch.zeros(2, 36), torch.zeros(2, 2), torch.zeros(2), tb, 2, 2)


# (B, Np, hidden units, hidden layers, outputs, LeakyReLU, resid, Fourier features) -> the route fields that hold in the split
# arithmetics (x6 / h3 / bf16; 'h3' in h3 only) and the row padding there; in f32 none holds.  bench.py's decoders at their
# bench batch, then one each of resid / tanh / 128 / 1024 hidden units.  The GPU tests' path sets follow from these:
# virt_act -> dec.virt_act + dec.fuse_in, sign_bits -> dec.sign_bits + dec.virt_grad_2val, no_h -> dec.no_h +
# dec.row_sums_in_dgrad (test_step_hot_widths_golden, test_decoder_kink_free_probe_at_bench_size).  The same rows name the
# per-layer plans (DECODER_LAYERS: parts and bound source of every launch, ops.decoder_plan) and, as small stand-ins, the
# launch sequences (DECODER_LAUNCHES) further down.
_S64 = {'split', 'virt_act', 'fused_out', 'virt_grad', 'sign_bits', 'no_h'}
DECODER_ROUTES = {
    'S64': ((256, 4096, 512, 1, 1, True, False, 0), _S64, 0),
    'S28': ((256, 784, 512, 1, 1, True, False, 0), _S64, 0),                  # 784 pixels padded to 896 (split arithmetics)
    'S28F': ((256, 784, 512, 1, 1, True, False, 1024), {'split', 'four_x6', 'four_dgrad_x6', 'fused_out', 'virt_grad',
                                                        'sign_bits', 'no_h'}, 0),
    'S128G': ((8, 16384, 512, 3, 3, True, False, 1024), {'split', 'four_x6', 'four_dgrad_x6'}, 64),
    'resid': ((4, 4096, 512, 3, 1, True, True, 0), {'split', 'fused_out'}, 64),
    'tanh': ((64, 4096, 512, 1, 1, False, False, 0), {'split', 'virt_act', 'fused_out', 'virt_grad'}, 0),
    'F128': ((8, 16384, 128, 1, 1, True, False, 1024), {'four_dgrad_x6'}, 0),        # too narrow for the split-pipe layers
    'F1024': ((64, 4096, 1024, 2, 1, True, False, 0), {'split', 'virt_grad', 'sign_bits'}, 64),
}


@pytest.mark.parametrize('mode', ['f32', 'x6', 'h3', 'bf16'])
@pytest.mark.parametrize('name', sorted(DECODER_ROUTES))
def test_decoder_route_of_named_configurations(name, mode):
    """ops.decoder_route -- every structural decision of the decoder, taken once in the forward and kept for the backward --
    for named configurations in each arithmetic, in training and in inference (host only: no library, no GPU)."""
    from tvae import ops
    from tvae._lib import arithmetic
    (B, Np, F_, nh, n_out, lrelu, resid, Ff), fields, pad = DECODER_ROUTES[name]
    act = ops.ACT_LRELU if lrelu else ops.ACT_TANH
    split = mode != 'f32'
    with arithmetic(mode):
        Np_p = ops.decoder_padded_pixels(Np, B, F_, nh, n_out, resid, Ff > 0, act)
        assert Np_p == (896 if (name == 'S28' and split) else 0), Np_p
        Np = Np_p or Np
        for infer in (False, True):
            want = {f: split and f in fields for f in ops.DecoderRoute._fields}
            want.update(ldn=B * Np + (pad if split else 0), h3=split and mode == 'h3' and 'split' in fields, infer=infer)
            assert ops.decoder_route(B, Np, F_, nh, n_out, act, resid, Ff, infer)._asdict() == want


def _layer(p, x='', y=False, fused=False, h=True, bits=False, vg=False, two=False, fb=False, wp=None, wb='', wr=False,
           dp=None, db='', dm=False, fi=False):
    """One ops.DecoderLayer, written short: the defaults are a stored layer in parts `p` with no bound and no fusion."""
    return dict(parts=p, x_bound=x, y_max=y, fused_out=fused, store_h=h, store_bits=bits, virt_grad=vg, two_val=two,
                from_bits=fb, wgrad_parts=p if wp is None else wp, wgrad_bound=wb, wgrad_x_rows=wr,
                dgrad_parts=p if dp is None else dp, d_bound=db, dgrad_max=dm, fuse_in=fi)


def _no_bounds(p):
    """The plan-wide fields where nothing runs h3: (first_parts, four_bound, four_wgrad_parts, four_dgrad_parts, chain,
    h_words, top_bound, d_words)."""
    return (p, '', p, p, False, False, False, False)


_BITS = dict(vg=True, two=True, fb=True, fused=True, h=False, bits=True)        # last layer of S64 / S28 / S28F (no_h)
_H3_MID = dict(wb='plain', wr=True, db='meas', dm=True)                         # backward of an h3 layer between stored tensors
# name of DECODER_ROUTES -> arithmetic -> (hidden layers, plan-wide fields) of ops.decoder_plan in training; 'p': the x6 (p = 3)
# and bf16 (p = 1) plans, which differ in nothing else; f32 has _layer(3) for every layer and _no_bounds(3).  In inference
# only store_bits changes (False everywhere).
DECODER_LAYERS = {
    'S64': {'p': lambda p: ([_layer(p, 'virt', fi=True, **_BITS)], _no_bounds(p)),
            'h3': ([_layer(2, 'virt', fi=True, **_BITS)], (2, '', 3, 3, False, False, False, False))},
    'S28F': {'p': lambda p: ([_layer(p, **_BITS)], _no_bounds(p)),
             'h3': ([_layer(2, 'rows', wb='two_val', wr=True, dm=True, **_BITS)],
                    (2, 'two_val', 2, 2, True, False, False, True))},
    'S128G': {'p': lambda p: ([_layer(p)] * 3, _no_bounds(p)),
              'h3': ([_layer(2, 'rows', y=True, **_H3_MID), _layer(2, 'meas', y=True, **_H3_MID),
                      _layer(2, 'meas', wb='plain', wr=True, db='top', dm=True)], (2, 'meas', 2, 2, True, True, True, True))},
    # a residual first hidden layer runs three-part forward (its stored input has a bound, the launch does not take it)
    'resid': {'p': lambda p: ([_layer(p), _layer(p), _layer(p, fused=True)], _no_bounds(p)),
              'h3': ([_layer(3, y=True, wp=2, dp=2, **_H3_MID), _layer(2, 'meas', y=True, **_H3_MID),
                      _layer(2, 'meas', fused=True, wb='plain', wr=True, db='top', dm=True)],
                     (2, '', 3, 3, True, True, True, True))},
    # tanh: implicit gradient in its general form, three-part in h3 too (the activation is stored: no bits)
    'tanh': {'p': lambda p: ([_layer(p, 'virt', fused=True, vg=True, fi=True)], _no_bounds(p)),
             'h3': ([_layer(2, 'virt', fused=True, vg=True, fi=True, wp=3, dp=3)], (2, '', 3, 3, False, False, False, False))},
    'F128': {'p': lambda p: ([_layer(p)], _no_bounds(p)),
             'h3': ([_layer(3)], (2, '', 3, 3, False, False, False, False))},       # (no split-pipe layer: nothing runs h3)
    'F1024': {'p': lambda p: ([_layer(p), _layer(p, vg=True, two=True, bits=True)], _no_bounds(p)),
              'h3': ([_layer(2, 'rows', y=True, **_H3_MID),
                      _layer(2, 'meas', vg=True, two=True, bits=True, wb='two_val', wr=True, dm=True)],
                     (2, '', 3, 3, True, True, False, True))},
}
DECODER_LAYERS['S28'] = DECODER_LAYERS['S64']            # (padded to 896 pixels: the same plan)


@pytest.mark.parametrize('mode', ['f32', 'x6', 'h3', 'bf16'])
@pytest.mark.parametrize('name', sorted(DECODER_ROUTES))
def test_decoder_layers_of_named_configurations(name, mode):
    """ops.decoder_plan -- parts and bound source of every DecoderFn launch, decided once from the route -- for the named
    configurations in each arithmetic, in training and in inference (host only: no library, no GPU)."""
    from tvae import ops
    from tvae._lib import arithmetic
    (B, Np, F_, nh, n_out, lrelu, resid, Ff), _, _ = DECODER_ROUTES[name]
    act = ops.ACT_LRELU if lrelu else ops.ACT_TANH
    if mode == 'f32':
        layers, wide = [_layer(3)] * nh, _no_bounds(3)
    elif mode == 'h3':
        layers, wide = DECODER_LAYERS[name]['h3']
    else:
        layers, wide = DECODER_LAYERS[name]['p']({'x6': 3, 'bf16': 1}[mode])
    with arithmetic(mode):
        Np = ops.decoder_padded_pixels(Np, B, F_, nh, n_out, resid, Ff > 0, act) or Np
        for infer in (False, True):
            plan = ops.decoder_plan(ops.decoder_route(B, Np, F_, nh, n_out, act, resid, Ff, infer), nh, resid, Ff > 0)
            assert [lp._asdict() for lp in plan.layers] == [dict(lp, store_bits=lp['store_bits'] and not infer) for lp in layers]
            assert tuple(plan[1:]) == wide


# (arithmetic, B, Np, hidden units, hidden layers, outputs, LeakyReLU, resid, Fourier features, zd, inference) -> entry points
# of DecoderFn's forward + backward in order, `tvae_` dropped, and PARTS_LOG's (parts, MFMAs per block) lists of
# linear_fwd_x6, linear_dgrad_x6, linear_wgrad_x6; small stand-ins of the DECODER_ROUTES rows with every route predicate on
# the same side.  Recorded on the tree BEFORE decoder_plan existed (DecoderFn deciding inline from the tensors at hand).
_S64_LIKE = (2, 128, 512, 1, 1, True, False, 0, 2, False)
_S64_X6 = 'latent_bias dense_split3 linear_fwd_x6 rowdot_seg seg_sum linear_wgrad_x6 dense_split3 linear_dgrad_x6 ' \
    'dec_in_total latent_bwd'
_PLAIN_1 = 'latent_bias dec_l0_fwd linear_fwd coldot rowdot_seg seg_sum dec_out_bwd linear_wgrad linear_dgrad dec_in_bwd ' \
    'latent_bwd'
_S28F_X6 = 'fourier_fwd dense_split3 linear_fwd_x6 dense_split3 linear_fwd_x6 rowdot_seg seg_sum linear_wgrad_x6 ' \
    'dense_split3 linear_dgrad_x6 rowdot_seg seg_sum latent_bwd linear_wgrad_x6 dense_split3 linear_dgrad_x6 fourier_bwd'
_BWD_STORED = ' linear_wgrad_x6 rowdot_seg seg_sum dense_split2h linear_dgrad_x6'        # a hidden layer below the top one
DECODER_LAUNCHES = {
    ('f32',) + _S64_LIKE: (_PLAIN_1, ([], [], [])),
    ('x6',) + _S64_LIKE: (_S64_X6, ([(3, 6)], [(3, 3)], [(3, 3)])),
    ('h3',) + _S64_LIKE: (_S64_X6.replace('split3', 'split2h'), ([(2, 3)], [(2, 2)], [(2, 2)])),
    ('bf16',) + _S64_LIKE: (_S64_X6, ([(1, 1)], [(1, 1)], [(1, 1)])),
    ('x6', 2, 128, 512, 1, 1, True, False, 256, 2, False):                                        # S28F-like
        (_S28F_X6, ([(3, 6), (3, 6)], [(3, 3), (3, 6)], [(3, 3), (3, 6)])),
    ('h3', 2, 128, 512, 1, 1, True, False, 256, 2, False):
        (_S28F_X6.replace('split3', 'split2h'), ([(2, 3), (2, 3)], [(2, 2), (2, 3)], [(2, 2), (2, 3)])),
    ('h3', 1, 16384, 256, 3, 3, True, False, 256, 3, False):                                      # S128G-like (dec.ld_pad)
        ('fourier_fwd' + 4 * ' dense_split2h linear_fwd_x6' + ' coldot rowdot_seg seg_sum dec_out_bwd linear_wgrad_x6 '
         'dense_split2h linear_dgrad_x6' + 2 * _BWD_STORED + ' rowdot_seg seg_sum latent_bwd linear_wgrad_x6 dense_split2h '
         'linear_dgrad_x6 fourier_bwd', ([(2, 3)] * 4, [(2, 3)] * 4, [(2, 3)] * 4)),
    ('h3', 2, 128, 512, 3, 1, True, True, 0, 2, False):                                           # resid
        ('latent_bias dec_l0_fwd dense_split3 linear_fwd_x6 dense_split2h linear_fwd_x6 dense_split2h linear_fwd_x6 '
         'rowdot_seg seg_sum dec_out_bwd linear_wgrad_x6 dense_split2h linear_dgrad_x6' + 2 * _BWD_STORED +
         ' dec_in_bwd latent_bwd', ([(3, 6), (2, 3), (2, 3)], [(2, 3)] * 3, [(2, 3)] * 3)),
    ('h3', 2, 128, 512, 1, 1, False, False, 0, 2, False):                                         # tanh
        ('latent_bias dense_split2h linear_fwd_x6 rowdot_seg seg_sum dec_out_bwd linear_wgrad_x6 dense_split3 '
         'linear_dgrad_x6 dec_in_total latent_bwd', ([(2, 3)], [(3, 6)], [(3, 6)])),
    ('h3', 2, 128, 1024, 2, 1, True, False, 0, 2, False):                                         # F1024
        ('latent_bias dec_l0_fwd dense_split2h linear_fwd_x6 dense_split2h linear_fwd_x6 coldot rowdot_seg seg_sum '
         'dec_out_bwd linear_wgrad_x6 dense_split2h linear_dgrad_x6' + _BWD_STORED + ' dec_in_bwd latent_bwd',
         ([(2, 3), (2, 3)], [(2, 2), (2, 3)], [(2, 2), (2, 3)])),
    ('h3', 2, 128, 128, 1, 1, True, False, 256, 2, False):         # F128 with Fourier: split pipe in its data gradient only
        ('latent_bias fourier_fwd linear_fwd linear_fwd coldot rowdot_seg seg_sum dec_out_bwd linear_wgrad linear_dgrad '
         'rowdot_seg seg_sum latent_bwd linear_wgrad dense_split3 linear_dgrad_x6 fourier_bwd', ([], [(3, 6)], [])),
    ('h3', 2, 100, 512, 1, 1, True, False, 0, 2, False): (_PLAIN_1, ([], [], [])),                # Np = 100: plain first layer
    ('h3',) + _S64_LIKE[:-1] + (True,): ('latent_bias dense_split2h linear_fwd_x6', ([(2, 3)], [], [])),      # inference
    ('h3', 2, 128, 256, 2, 1, True, False, 0, 3, False):
        ('latent_bias dense_split2h linear_fwd_x6 dense_split2h linear_fwd_x6 rowdot_seg seg_sum linear_wgrad_x6 '
         'dense_split2h linear_dgrad_x6' + _BWD_STORED + ' dec_in_total latent_bwd',
         ([(2, 3), (2, 3)], [(2, 2), (2, 3)], [(2, 2), (3, 6)])),
}


@pytest.mark.parametrize('row', sorted(DECODER_LAUNCHES), ids=lambda r: '-'.join(str(v) for v in r))
def test_decoder_launches_of_named_configurations(row):
    """The entry points DecoderFn launches, forward then backward, and the arithmetic of its split-pipe launches, for
    stand-ins of the route table's rows: run on CPU tensors with `ops.call` recorded and `ops.query` stubbed
    (profiles/tools/launch_trace.py; host only: no library, no GPU)."""
    import importlib.util
    from tvae import ops
    spec = importlib.util.spec_from_file_location(
        'launch_trace', os.path.join(ROOT, 'profiles', 'tools', 'launch_trace.py'))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    mode, B, Np, F_, nh, n_out, lrelu, resid, Ff, zd, infer = row
    rec = lt.trace_decoder(mode, B, Np, F_, nh, n_out, ops.ACT_LRELU if lrelu else ops.ACT_TANH, resid, Ff, zd, infer)
    want, want_parts = DECODER_LAUNCHES[row]
    assert lt.names(rec) == ['tvae_' + e for e in want.split()]
    assert tuple(rec.parts.get('tvae_linear_%s_x6' % k, []) for k in ('fwd', 'dgrad', 'wgrad')) == want_parts


def test_wgrad_two_parts_need_their_bounds():
    """ops._wgrad takes its arithmetic from the caller: two parts without the bounds of the streamed operands raise on the
    host, before any launch (host only: no library, no GPU)."""
    import importlib.util
    from tvae import ops
    from tvae._lib import arithmetic
    spec = importlib.util.spec_from_file_location(
        'launch_trace', os.path.join(ROOT, 'profiles', 'tools', 'launch_trace.py'))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    d, X, one = torch.zeros(256, 128), torch.zeros(256, 128), torch.ones(1)
    with arithmetic('h3'), lt.traced() as rec:
        for bounds in ({}, dict(a_amax=one), dict(x_amax=one)):
            with pytest.raises(ValueError):
                ops._wgrad(d, X, 256, 128, 256, nparts=2, **bounds)
        assert rec.launches == []
        ops._wgrad(d, X, 256, 128, 256, nparts=2, a_amax=one, x_amax=one)
        ops._wgrad(d, X, 256, 128, 256)
    assert lt.names(rec) == ['tvae_linear_wgrad_x6'] * 2 and rec.parts['tvae_linear_wgrad_x6'] == [(2, 3), (3, 6)]


# (arithmetic, head rows, LeakyReLU, N % 32 == 0, conv1 left max |A1|) -> (tail, parts, h3, bits, wgrad) of ops.encoder_route
# in training, C = C2 = 128, N < 2^25; None = whatever.  In inference: the same tail / parts / h3, no bits, wgrad 'plain'.
_PLAIN = ('plain', 0, False, False, 'plain')
ENCODER_ROUTES = [
    (('f32', None, None, None, None), _PLAIN),
    (('x6', 7, True, True, None), ('fused', 3, False, True, 'x6')),
    (('x6', 7, True, False, None), ('fused', 3, False, True, 'plain')),
    (('x6', 7, False, None, None), ('fused', 3, False, False, 'plain')),
    (('x6', (8, 23, 103, 128), None, None, None), _PLAIN),
    (('h3', 7, True, True, True), ('fused', 2, True, True, 'x6')),
    (('h3', 7, True, True, False), ('fused', 3, False, True, 'x6')),
    (('h3', (8, 23, 128), True, True, True), ('wide', 2, True, True, 'wide')),
    (('h3', 23, True, False, True), ('wide', 2, True, True, 'plain')),
    (('h3', 23, False, None, True), ('wide', 2, True, False, 'plain')),
    (('h3', 23, None, None, False), _PLAIN),
    (('h3', 129, None, None, None), _PLAIN),
    (('bf16', 7, True, True, None), ('fused', 1, False, True, 'x6')),
    (('bf16', 23, True, None, None), ('wide', 1, False, True, 'plain')),
]


def _encoder_route_cases():
    """ENCODER_ROUTES with every None expanded: (mode, nh, act, N, out_max, expected training route)."""
    from tvae import ops
    for (mode, nh, lrelu, n32, out_max), want in ENCODER_ROUTES:
        for nh_, lrelu_, n32_, out_max_ in itertools.product(
                (3, 7, 8, 23, 128, 129) if nh is None else nh if isinstance(nh, tuple) else (nh,),
                (True, False) if lrelu is None else (lrelu,), (True, False) if n32 is None else (n32,),
                (True, False) if out_max is None else (out_max,)):
            yield (mode, nh_, ops.ACT_LRELU if lrelu_ else ops.ACT_TANH, 8 * 8 * 29 * 29 if n32_ else 6 * 8 * 29 * 29, out_max_,
                   dict(zip(('tail', 'parts', 'h3', 'bits', 'wgrad'), want)))


def test_encoder_route_of_named_configurations():
    """ops.encoder_route -- every structural decision of the encoder tail, taken once in the forward and kept for the
    backward -- against the table of configurations in each arithmetic, in training and in inference; the limits (128
    channels, 2^25 columns, 7 | 8 and 128 | 129 head rows) and the FUSE_ENC_TAIL switch (host only: no library, no GPU)."""
    from tvae import ops
    from tvae._lib import arithmetic
    L = ops.ACT_LRELU
    cases = list(_encoder_route_cases())
    assert {c[0] for c in cases} == {'f32', 'x6', 'h3', 'bf16'} and len(cases) > 60
    for mode, nh, act, N, out_max, want in cases:
        with arithmetic(mode):
            assert ops.encoder_route(128, 128, nh, N, act, out_max, False)._asdict() == dict(want, infer=False), (mode, nh)
            assert ops.encoder_route(128, 128, nh, N, act, out_max, True)._asdict() == \
                dict(want, bits=False, wgrad='plain', infer=True), (mode, nh)
    plain = dict(zip(('tail', 'parts', 'h3', 'bits', 'wgrad'), _PLAIN), infer=False)
    N = 8 * 8 * 29 * 29
    for mode in ('x6', 'h3', 'bf16'):
        with arithmetic(mode):
            for nh in (7, 23) if mode != 'x6' else (7,):         # fused / wide; each of the one-offs changes one thing
                assert ops.encoder_route(128, 128, nh, (1 << 25) - 32, L, True, False).tail == ('fused' if nh == 7 else 'wide')
                assert ops.encoder_route(128, 128, nh, 1 << 25, L, True, False)._asdict() == plain
                for C, C2 in ((64, 128), (128, 64), (64, 64)):
                    assert ops.encoder_route(C, C2, nh, N, L, True, False)._asdict() == plain
            wide = 'plain' if mode == 'x6' else 'wide'
            tails = [ops.encoder_route(128, 128, nh, N, L, True, False).tail for nh in (7, 8, 128, 129)]
            assert tails == ['fused', wide, wide, 'plain']
    old, ops.FUSE_ENC_TAIL = ops.FUSE_ENC_TAIL, False
    try:
        for mode, nh, act, N, out_max, _ in cases:
            with arithmetic(mode):
                for infer in (False, True):
                    assert ops.encoder_route(128, 128, nh, N, act, out_max, infer)._asdict() == dict(plain, infer=infer)
    finally:
        ops.FUSE_ENC_TAIL = old


# (arithmetic, head rows, LeakyReLU, image side = Ho of launch_trace: N = 512 | 392, conv1 path, inference) -> entry points of
# EncoderFn's forward + backward in order, `tvae_` dropped; recorded on the tree BEFORE EncoderRoute existed
ENCODER_LAUNCHES = {
    ('f32', 7, True, 8, 'dft', False):
        'rotate_bank_fwd conv1_fwd linear_fwd heads_fwd rowdot_seg seg_sum heads_bwd linear_wgrad linear_dgrad rowdot_seg '
        'seg_sum conv1_wgrad rotate_bank_bwd',
    ('x6', 7, True, 8, 'dft', False):
        'rotate_bank_fwd conv1_fwd_dft dense_split3 enc_tail_fwd_x6 rowdot_seg seg_sum dense_split3 dense_split3 '
        'enc_tail_dgrad_x6 heads_bwd enc_tail_wgrad_x6 conv1_wgrad_dft rotate_bank_bwd',
    ('x6', 7, False, 7, 'x6', False):
        'rotate_bank_fwd bank_split3 conv1_fwd_x6 dense_split3 enc_tail_fwd_x6 rowdot_seg seg_sum heads_bwd linear_wgrad '
        'linear_dgrad rowdot_seg seg_sum dy_split3 conv1_wgrad_x6 rotate_bank_bwd',
    ('h3', 7, True, 8, 'dft', False):
        'rotate_bank_fwd conv1_fwd_dft dense_split2h enc_tail_fwd_x6 rowdot_seg seg_sum dense_split2h dense_split3 '
        'enc_tail_dgrad_x6 heads_bwd enc_tail_wgrad_x6 conv1_wgrad_dft rotate_bank_bwd',
    ('h3', 23, True, 8, 'dft', False):
        'rotate_bank_fwd conv1_fwd_dft dense_split2h dense_split2h enc_tail_fwd_wide rowdot_seg seg_sum dense_split2h '
        'dense_split2h enc_tail_dgrad_wide enc_tail_wgrad_wide rowdot_seg seg_sum enc_tail_wgrad_wide conv1_wgrad_dft '
        'rotate_bank_bwd',
    ('h3', 23, True, 7, 'dft', False):
        'rotate_bank_fwd conv1_fwd_dft dense_split2h dense_split2h enc_tail_fwd_wide rowdot_seg seg_sum dense_split2h '
        'dense_split2h enc_tail_dgrad_wide linear_wgrad rowdot_seg seg_sum linear_wgrad conv1_wgrad_dft rotate_bank_bwd',
    ('h3', 23, True, 8, 'x6', False):
        'rotate_bank_fwd bank_split3 conv1_fwd_x6 linear_fwd linear_fwd rowdot_seg seg_sum linear_wgrad linear_dgrad '
        'rowdot_seg seg_sum linear_wgrad linear_dgrad rowdot_seg seg_sum dy_split3 conv1_wgrad_x6 rotate_bank_bwd',
    ('bf16', 23, True, 8, 'dft', False):
        'rotate_bank_fwd conv1_fwd_dft dense_split3 dense_split3 enc_tail_fwd_wide rowdot_seg seg_sum dense_split3 '
        'dense_split3 enc_tail_dgrad_wide linear_wgrad rowdot_seg seg_sum linear_wgrad conv1_wgrad_dft rotate_bank_bwd',
    ('h3', 7, True, 8, 'dft', True): 'rotate_bank_fwd conv1_fwd_dft dense_split2h enc_tail_fwd_x6',
}


@pytest.mark.parametrize('row', sorted(ENCODER_LAUNCHES), ids=lambda r: '-'.join(str(v) for v in r))
def test_encoder_launches_of_named_configurations(row):
    """The entry points EncoderFn launches, forward then backward, for rows of the route table: run on CPU tensors with
    `ops.call` recorded and `ops.query` stubbed (profiles/tools/launch_trace.py; host only: no library, no GPU)."""
    import importlib.util
    from tvae import ops
    spec = importlib.util.spec_from_file_location(
        'launch_trace', os.path.join(ROOT, 'profiles', 'tools', 'launch_trace.py'))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    mode, nh, lrelu, n, conv, infer = row
    rec = lt.trace('encoder', mode, nh, ops.ACT_LRELU if lrelu else ops.ACT_TANH, n, conv, 128, infer)
    assert lt.names(rec) == ['tvae_' + e for e in ENCODER_LAUNCHES[row].split()]


def test_scratch_buffers_outlive_a_captured_graph():
    """once a hipGraph has been captured (tvae/graph.py -> ops.pin_scratch), growing a scratch buffer
    or the shared workspace must not free the block the graph still points to.  ADVICE r04: the pin belongs to the graph
    (a token), and releasing it (GraphedStep.close) lets the outgrown blocks go."""
    import torch
    from tvae import ops
    cpu = torch.device('cpu')
    saved = dict(ops._WS), dict(ops._PINNED)
    try:
        ops._WS.clear()
        ops._PINNED.clear()
        a = ops._scratch(cpu, 'k', 16)
        w = ops.workspace(cpu, 8)
        ops._scratch(cpu, 'k', 32)                       # before pinning: plain replacement
        assert not ops._PINNED
        b = ops._scratch(cpu, 'k', 32)
        tok = ops.pin_scratch()
        c = ops._scratch(cpu, 'k', 64)
        w2 = ops.workspace(cpu, 64)
        assert c.numel() >= 64 and w2.numel() == 64
        kept = {t.data_ptr() for t in ops._PINNED[tok]}
        assert b.data_ptr() in kept and w.data_ptr() in kept and a.data_ptr() not in kept
        assert ops._scratch(cpu, 'k', 8) is c            # no growth: same buffer, nothing new pinned
        assert len(ops._PINNED[tok]) == 2
        tok2 = ops.pin_scratch()                         # a second graph: both keep what is outgrown from now on
        ops._scratch(cpu, 'k', 128)
        assert len(ops._PINNED[tok]) == 3 and len(ops._PINNED[tok2]) == 1
        ops.unpin_scratch(tok)
        assert tok not in ops._PINNED and tok2 in ops._PINNED
        ops.unpin_scratch(tok2)
        assert not ops._PINNED
    finally:
        ops._WS.clear()
        ops._WS.update(saved[0])
        ops._PINNED.clear()
        ops._PINNED.update(saved[1])


@pytest.mark.parametrize('t_inf,r_inf,has_ctf,mask_radius,want', [
    # the TARGET-VAE branch, both spellings of --r-inf; mask_radius: None (datasets without a mask), 0 (particles, none asked)
    ('attention', 'attention+offsets', False, None, True),
    ('attention', 'attention', False, None, True),
    ('attention', 'attention+offsets', False, 0, True),
    ('attention', 'attention', False, 0, True),
    # a circular mask or per-image CTF filters: the step runs eagerly
    ('attention', 'attention+offsets', False, 7, False),
    ('attention', 'attention', False, 7, False),
    ('attention', 'attention+offsets', True, None, False),
    ('attention', 'attention+offsets', True, 0, False),
    ('attention', 'attention', True, 7, False),
    # the secondary inference branches are never captured
    ('attention', 'unimodal', False, None, False),
    ('attention', 'unimodal', False, 0, False),
    ('unimodal', 'unimodal', False, None, False),
    ('unimodal', 'attention', False, None, False),
    ('unimodal', 'attention+offsets', False, 0, False),
    ('unimodal', 'unimodal', True, 7, False),
])
def test_graph_supported_table(t_inf, r_inf, has_ctf, mask_radius, want):
    """tvae.driver.graph_supported: which runs the drivers capture into a hipGraph by default."""
    from tvae import driver
    got = driver.graph_supported(t_inf, r_inf, has_ctf, mask_radius)
    assert got is want


def test_graph_case_table_and_exclusions_are_current():
    """CPU twin of tests/test_graph_gpu.py::test_every_capturable_route_was_replayed: every excluded route still exists in
    tvae/ops.py and carries a reason, the route scan finds the names ops.py is known to record (both names of a conditional
    expression included), and the case table only names configurations, fixtures and builders that exist."""
    import step_cases as S
    routes = S.noted_routes()
    assert {'conv1.dft_ring', 'conv1.x6', 'conv1.f32', 'enc.tail_fwd_wide', 'enc.tail_fwd_x6', 'dec.hidden_h3_mem',
            'dec.hidden_h3_meas', 'dec.no_h_inference', 'dec.no_h', 'dec.fused_out', 'dec.hidden_x6', 'dec.ld_pad',
            'trans_attn.plain', 'trans_attn.rot_pool'} <= routes
    assert all(re.fullmatch(r'[a-z0-9_]+\.[a-z0-9_]+', r) for r in routes), sorted(routes)
    for name, reason in S.GRAPH_EXCLUDED_ROUTES.items():
        assert name in routes, f'{name} is excluded but tvae/ops.py no longer records it'
        assert isinstance(reason, str) and len(reason.split()) >= 4, name
    assert {'enc.inference', 'dec.no_h_inference', 'trans_attn.plain', 'mlp_encoder.kernels'} <= set(S.GRAPH_EXCLUDED_ROUTES)
    for case, c in S.GRAPH_CASES.items():
        assert len([k_ for k_ in ('cfg', 'golden', 'encoder') if k_ in c]) == 1, case
        assert c['lik'] in ('bce', 'bce3', 'gauss', 'gauss_var'), case
        if 'cfg' in c:
            assert c['cfg'] in S.OOB_CONFIGS, case
        elif 'golden' in c:
            assert os.path.exists(os.path.join(ROOT, 'tests', 'golden', c['golden'] + '.npz')), case
        else:
            assert c['encoder'] in set(S.HEADS103_GEOM) | {'cin3_direct'}, case
    assert set(S.GRAPH_ARITHMETIC_CASES) <= set(S.GRAPH_CASES)
    from tvae import _lib
    assert set(S.GRAPH_ARITHMETIC_MODES) | {'h3'} == set(_lib.GEMM_MODES)


def test_flat_adam_second_backward_raises():
    """with the two-bucket reducer active exactly one backward per step() is supported -- a second one reaching the
    early bucket after it was posted raises; after disable_early_bucket() (captured-graph path) the hooks are inert."""
    import pytest
    from tvae import optim

    class Reducer:
        active = True

        def begin(self, seg):
            pass

        def __call__(self, flat_g, start=0):
            return 1.0

    ps = [torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(2))]
    opt = optim.FlatAdam(ps, lr=1e-2, update_fn=lambda *a: None, reducer=Reducer(), early_params=1)
    opt.zero_grad(set_to_none=True)
    sum((p ** 2).sum() for p in ps).backward()
    with pytest.raises(RuntimeError, match='second backward'):
        sum((p ** 2).sum() for p in ps).backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    opt.disable_early_bucket()
    for _ in range(2):                                   # hooks inert: gradient accumulation is allowed again
        sum((p ** 2).sum() for p in ps).backward()
    assert opt._early_seen == 0 and not opt._early_posted
    opt.step()


def test_hand_counted_kernels_use_no_scratch_and_no_packed_fp32():
    """the LDS-DMA ring kernels wait with hand-counted `s_waitcnt vmcnt(N)`; a compiler-emitted scratch spill (or
    any other vector-memory instruction it adds) would inflate the count and let a wave read LDS before its DMA has landed.
    Gate on the BUILT library: those kernels, and the lean epilogue instances whose point is a register budget, must have a
    private segment of 0 bytes; and no code object may contain packed-fp32 vector instructions (csrc/Makefile NOPK:
    profiles/README.md, rounds 3-4).  Reads the code objects embedded in libtvae_hip.so with llvm-readelf / llvm-objdump."""
    import re
    import subprocess
    import tempfile
    from tvae import _lib
    readelf, objdump = '/opt/rocm/lib/llvm/bin/llvm-readelf', '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not (os.path.exists(readelf) and os.path.exists(objdump) and os.path.exists(_lib.LIB_PATH)):
        import pytest
        pytest.skip('needs the ROCm llvm tools and the built library')
    data = open(_lib.LIB_PATH, 'rb').read()
    offs = [m.start() for m in re.finditer(b'\x7fELF\x02\x01\x01\x40', data)]
    assert len(offs) >= 20
    must_be_zero = re.compile(r'dft_out_ring_kernel|dft_dy_ring_kernel|dense_wgrad_x6_dma_kernel|dense_wgrad_x6_wide_kernel|enc_tail_wgrad_x6_kernel|'
                              r'dense_x6_kernelILi2ELi\dELi1E|dense_x6_kernelILi5ELi\dELi2E|dense_x6_plain4_kernelILi\dELi1E')
    seen, npk = 0, 0
    for o in offs:
        with tempfile.NamedTemporaryFile(suffix='.co') as f:
            f.write(data[o:])
            f.flush()
            notes = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
            dis = subprocess.run([objdump, '-d', f.name], capture_output=True, text=True).stdout
        npk += len(re.findall(r'\bv_pk_(?:fma|mul|add)_f32\b', dis))
        for blk in re.split(r'\n\s+- ', notes):
            n = re.search(r'\.name:\s+(\S+)', blk)
            p = re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk)
            if n and p and must_be_zero.search(n.group(1)):
                seen += 1
                assert int(p.group(1)) == 0, (n.group(1), int(p.group(1)))
    assert seen >= 23, seen
    assert npk == 0, npk


def test_every_kernel_is_built_once():
    """A non-template `static __global__` function is emitted by every translation unit that sees its definition, and a template
    kernel by every unit that instantiates it: the kernel headers are split so that each kernel reaches exactly ONE unit, and
    kernels that several units launch go through a launcher in the unit that owns them (csrc/abi_common.hpp).  Gate on the BUILT
    libraries: every kernel name of the notes metadata occurs in exactly one of the embedded code objects.  Names and counts
    only."""
    import re
    import subprocess
    import tempfile
    from tvae import _cluster_lib, _lib
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    if not (os.path.exists(readelf) and os.path.exists(_lib.LIB_PATH) and os.path.exists(_cluster_lib.LIB_PATH)):
        import pytest
        pytest.skip('needs the ROCm llvm tools and the built libraries')
    allowed = set()          # names that may be built more than once: none
    for path, least in ((_lib.LIB_PATH, 200), (_cluster_lib.LIB_PATH, 10)):
        data = open(path, 'rb').read()
        offs = [m.start() for m in re.finditer(b'\x7fELF\x02\x01\x01\x40', data)]
        count = {}
        for o, end in zip(offs, offs[1:] + [len(data)]):
            with tempfile.NamedTemporaryFile(suffix='.co') as f:
                f.write(data[o:end])
                f.flush()
                notes = subprocess.run([readelf, '--notes', f.name], capture_output=True, text=True).stdout
            for n in set(re.findall(r'\.symbol:\s+(\S+)\.kd\b', notes)):      # (.name is also what arguments have)
                count[n] = count.get(n, 0) + 1
        assert len(count) >= least, (path, len(count))      # (the walk found the kernels at all)
        dup = {n: c for n, c in count.items() if c != 1 and n not in allowed}
        assert not dup, (path, dup)


# ---- frequency-domain lifting convolution: which kernel instance every step takes (tvae_conv1_dft_route) -----------------
# Capacities of the instances, written from their header comments (csrc/conv_dft_kernels.hpp, conv_dft_h3_kernels.hpp,
# abi_dense_x6.hpp, dense_x6_kernels.hpp) and NOT from the plan that routes to them.  Frame: L (tvae_conv1_dft_frame),
# Lh = L // 2 + 1 frequencies, Ho outputs per side; K2 = 2 k Cin (reduction of the spectral GEMMs), M = C R filter rows.
DFT_RING_FRAMES = {1: (36, 17), 2: (80, 33), 3: (60, 39), 4: (44, 17), 5: (96, 33), 6: (66, 39)}   # (L, Ho) of ring 1 .. 6
DFT_STEPS = ('out', 'dy', 'fwd_gemm', 'wgrad_gemm')                                             # `which` 0 .. 3


def _cdiv(a, b):
    return -(-a // b)


def dft_instance_fits(which, rid, L, Ho, K2, M, parts):
    Lh = L // 2 + 1
    if which in (0, 1) and 1 <= rid <= 6:      # ring instances: compiled for one frame each
        return (L, Ho) == DFT_RING_FRAMES[rid]
    if which == 0:
        if rid == 10:       # dft_out_h3_kernel<KS 11, NWT 5, NLD 5>: 2 Lh <= 16 KS, Ho <= 32 NWT, 16 Lh <= NLD 64 NWT; h3 only
            return parts == 2 and 2 * Lh <= 16 * 11 and Ho <= 32 * 5 and 16 * Lh <= 5 * 64 * 5
        if rid in (11, 12):  # dft_out_wide_kernel<LHR, NLD>: Lh <= LHR; NTW waves of 32 columns (the last column of
            LHR, NLD = (82, 6) if rid == 11 else (96, 8)      # Ho = 32 NTW + 1 on the vector ALU), 64 NTW <= 512 threads,
            NTW = Ho // 32 if (Ho % 32 == 1 and Ho > 32) else _cdiv(Ho, 32)                 # 16 Lh <= NLD 64 NTW
            return Lh <= LHR and NTW <= 8 and 16 * Lh <= NLD * 64 * NTW and Ho <= 32 * NTW + 1
        if 21 <= rid <= 25:  # dft_out_gen_kernel<NT>: NT whole 32-row output tiles
            return Ho <= 32 * (rid - 20)
        if 31 <= rid <= 39:  # dft_out_mf_kernel<LHP, NT, REM1>: Lh <= LHP; NT tiles of 32 rows; REM1: the one extra row w = 32 NT
            LHP = (23, 49, 64)[(rid - 31) // 3]
            NT, REM1 = ((1, False), (1, True), (2, False))[(rid - 31) % 3]
            return Lh <= LHP and (Ho == 32 * NT + 1 if REM1 else Ho <= 32 * NT)
    if which == 1:
        if rid == 10:       # dft_dy_h3_kernel<WS 9, NKT 6, NLD 11>: Ho <= 16 WS, 2 Lh <= 32 NKT, 32 Ho <= NLD 64 NKT; h3 only
            return parts == 2 and Ho <= 16 * 9 and 2 * Lh <= 32 * 6 and 32 * Ho <= 11 * 64 * 6
        if rid in (11, 12, 13):   # dft_dy_wide_kernel<NSR, NLD 16, 2>: ceil(Ho / 2) k-steps <= NSR, NRT = ceil(2 Lh / 32) waves
            NSR, NRT = {11: 50, 12: 66, 13: 80}[rid], _cdiv(2 * Lh, 32)            # of 64 <= 512 threads, 32 Ho <= NLD 64 NRT
            return _cdiv(Ho, 2) <= NSR and NRT <= 8 and 32 * Ho <= 16 * 64 * NRT
        if rid == 20:       # dft_dy_gen_kernel: sized at run time
            return True
        if 31 <= rid <= 35:  # dft_dy_mf_kernel<NS, NRT, LH2, AREG>: ceil(32 Ho / 64) <= NS, 2 Lh <= 32 NRT, LH2 = 0 or 2 Lh
            NS, NRT, LH2 = ((9, 2, 46), (9, 2, 0), (17, 4, 98), (17, 4, 0), (32, 4, 0))[rid - 31]
            return _cdiv(32 * Ho, 64) <= NS and 2 * Lh <= 32 * NRT and LH2 in (0, 2 * Lh)
    if which == 2:
        if rid == 1:        # dense_x6_xres_kernel<NP, NK>: 2 or 3 parts, NK = 8 / 10 / 12 k-steps of 16, whole 512-row problems,
            nk, Mb = _cdiv(K2, 16), _cdiv(2 * M, 512) * 512    # the cells of a k-step and the row scales in 160 KB of LDS
            return parts in (2, 3) and nk in (8, 10, 12) and (2 * M) % 512 == 0 and \
                nk * parts * 256 * 16 + (Mb + 128) * 4 <= 160 * 1024
        if rid == 2:        # dense_x6_plain4_kernel: the 256-row tile of short reductions
            return K2 <= 256
        return rid == 3     # dense_x6_kernel: the 512-row tile, any reduction
    if which == 3:
        if rid == 2:        # dense_wgrad_x6_wide_kernel: 256-row tiles, 2 L Cin > 128 columns, split arithmetics only
            return parts != 1 and (2 * M) % 256 == 0 and K2 > 128
        return rid == 1     # dense_wgrad_x6 512 x 128 tile, any shape
    return False


def dft_sweep_geometries():
    """One (n, k, pad) per distinct frame (L, Ho) with 8 <= n <= 256 (k <= 256, pad < 200, Ho <= 192: the plan takes at most
    five 32-row output tiles, so a margin of unsupported frames is included): the smallest filter that makes the frame and
    the largest.  L as documented in include/tvae_hip.h: max(n + pad, k) rounded up to a multiple of 4, at most n + 2 pad."""
    n = np.arange(8, 257)[:, None, None]
    k = np.arange(1, 257)[None, :, None]
    p = np.arange(0, 200)[None, None, :]
    Ho = n + 2 * p - k + 1
    Lmin = (np.maximum(n + p, k) + 3) & ~3
    L = np.where(Lmin > n + 2 * p, n + 2 * p, Lmin)
    sel = (Ho >= 1) & (Ho <= 192)
    N, K, P = np.broadcast_arrays(n, k, p)
    Lv, Hv, Nv, Kv, Pv = L[sel], Ho[sel], N[sel], K[sel], P[sel]
    key = Lv.astype(np.int64) * 1000 + Hv
    o = np.lexsort((Nv, Kv, key))
    ks = key[o]
    edge = ks[1:] != ks[:-1]
    pick = np.unique(np.concatenate([o[np.r_[True, edge]], o[np.r_[edge, True]]]))
    return [(int(a), int(b), int(c), int(d), int(e)) for a, b, c, d, e in zip(Nv[pick], Kv[pick], Pv[pick], Lv[pick], Hv[pick])]


DFT_SWEEP_CR = ((5, 4), (32, 8))     # 2 M = 40: no whole tile; 512: whole 256-row (weight gradient) and 512-row (forward) tiles
DFT_SWEEP_B = 2


def test_conv1_dft_routes_fit_their_instances_and_are_covered_on_the_gpu():
    """Every frame reachable with 8 <= n <= 256, one and three input channels, three filter counts, parts 1 / 2 / 3: the
    instance each step takes (tvae_conv1_dft_route) is one whose capacity, as its header states it, holds for the geometry;
    unsupported geometries route nowhere; the transforms take the ring instance exactly when tvae_conv1_dft_ring says so.
    Every (step, instance, parts) seen here must be reached by a geometry of the GPU boundary test
    (tests/test_hip_primitives.py::DFT_ROUTE_GEOMETRIES), so a new route fails here until a GPU test covers it."""
    from test_hip_primitives import DFT_EDGE_GEOMETRIES, DFT_ROUTE_GEOMETRIES
    from tvae import _lib
    L_ = _lib.lib()
    route, supported, frame, ring = (L_.tvae_conv1_dft_route, L_.tvae_conv1_dft_supported, L_.tvae_conv1_dft_frame,
                                     L_.tvae_conv1_dft_ring)
    seen, bad, checked, n_ok = {}, [], {}, 0
    for n, k, pad, L, Ho in dft_sweep_geometries():
        assert frame(DFT_SWEEP_B, 1, n, k, pad, 4, 4) == L, (n, k, pad, L)
        rg = ring(DFT_SWEEP_B, 1, n, k, pad, 4, 4)
        for Cin in (1, 3):
            K2 = 2 * k * Cin
            for C, R in DFT_SWEEP_CR:
                ok = supported(DFT_SWEEP_B, Cin, n, k, pad, C, R)
                n_ok += ok
                if not ok:
                    for which in range(4):
                        if route(DFT_SWEEP_B, Cin, n, k, pad, C, R, 2, which) != -1:
                            bad.append(('unsupported but routed', DFT_STEPS[which], (n, k, pad, Cin, C, R)))
                    continue
                for parts in (1, 2, 3):
                    for which in range(4):
                        rid = route(DFT_SWEEP_B, Cin, n, k, pad, C, R, parts, which)
                        if which < 2 and (rid if 1 <= rid <= 6 else 0) != rg:
                            bad.append(('ring', DFT_STEPS[which], rid, rg, (n, k, pad)))
                        ck = (which, rid, L, Ho, parts) if which < 2 else (which, rid, K2, C * R, parts)
                        fits = checked.get(ck)
                        if fits is None:
                            fits = checked[ck] = dft_instance_fits(which, rid, L, Ho, K2, C * R, parts)
                        if not fits:
                            bad.append(('over capacity', DFT_STEPS[which], rid, parts,
                                        dict(n=n, k=k, pad=pad, Cin=Cin, C=C, R=R, L=L, Ho=Ho)))
                        seen.setdefault((which, rid, parts), (n, k, pad, Cin, C, R))
    assert n_ok > 10000
    assert not bad, '%d geometries routed beyond an instance (Ho %s), e.g.:\n%s' % (
        len(bad), sorted({b[-1]['Ho'] for b in bad if b[0] == 'over capacity'}), '\n'.join(map(str, bad[:40])))
    gpu = set()
    for B, Cin, n, k, pad, C, R, act in DFT_ROUTE_GEOMETRIES:
        assert supported(B, Cin, n, k, pad, C, R), (B, Cin, n, k, pad, C, R)
        for parts in (1, 2, 3):
            for which in range(4):
                gpu.add((which, route(B, Cin, n, k, pad, C, R, parts, which), parts))
    missing = sorted(set(seen) - gpu)
    assert not missing, 'routes without a GPU test (step, id, parts) -> an example (n, k, pad, Cin, C, R):\n%s' % '\n'.join(
        '%s %s parts %d: %s' % (DFT_STEPS[w], r, p, seen[(w, r, p)]) for w, r, p in missing)
    # ... and every transform instance that h3 reaches has its edge-placed maxima test (test_conv1_dft_h3_edge_placed_maxima)
    edge = {(w, route(B, Cin, n, k, pad, C, R, 2, w)) for B, Cin, n, k, pad, C, R, act in DFT_EDGE_GEOMETRIES for w in (0, 1)}
    assert {(w, r) for w, r, p in seen if w < 2 and p == 2} <= edge
