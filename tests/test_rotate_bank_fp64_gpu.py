"""Rotated filter bank (tvae_rotate_bank_fwd / _bwd, csrc/rotate_bank_kernels.hpp) against tests/bank_ref.py, the float64 sparse
operator built from the DENSE tap table and, for the backward, its transpose -- per element, with derived bounds (bank_ref's
docstring: (n + 1) u sum |w x|, n = 4 forward, the source pixel's list length backward, one more under accumulate; u = 2^-24;
nothing is measured or tuned).  The shapes reach what test_hip_primitives.py::test_rotate_bank leaves out:

  (9, 32, 1, 3), (28, 32, 1, 4)   an 8 x 8 patch stages more than RBB_CAP = 4096 CSR entries: the second staging round
  (17, 17, 2, 3)                  3 997 entries, just under it
  (33, 8, 1, 5), (64, 8, 1, 8)    k > 32: the forward's second patch column, ragged and full
  (9, 4, 3, 683)                  C Cin = 2 049: the NPT = 4 instance of the backward, ragged over its 16 pairs
  (9, 4, 1, 2032)                 the last size of NPT = 2
  (5, 4, 1, 1)                    the smallest

The backward runs with accumulate = 0 and with accumulate = 1 on a random initial dweight (through the C ABI: tvae.ops never
accumulates).  Every call is made twice and has to give the same bits."""
import numpy as np
import pytest
import torch

import bank_ref
import guardband

pytestmark = pytest.mark.gpu
RBB_CAP = 4096
U = bank_ref.U


@pytest.fixture(autouse=True)
def guarded_calls():
    """As in test_hip_primitives.py: every C-ABI call on relocated tensors between guard bands, twice from the same inputs."""
    with guardband.GuardedCalls(replay=True):
        yield


def dev():
    return torch.device('cuda:0')


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def patch_totals(k, R):
    """CSR entries that the 8 x 8 patches of the source filter stage (what rotate_bank_bwd_kernel adds up from csr_ptr)."""
    from tvae import tables
    ptr = tables.rotation_taps_csr(k, R)[0].astype(np.int64)
    per = (ptr[1:] - ptr[:-1]).reshape(k, k)
    npx = (k + 7) // 8
    return [int(per[8 * py:8 * py + 8, 8 * px:8 * px + 8].sum()) for py in range(npx) for px in range(npx)]


def npt(k, Cin, C):
    """pairs per thread of the backward (csrc/abi_small.hip: tvae_rotate_bank_bwd)"""
    npx = (k + 7) // 8
    return 4 if npx * npx * ((C * Cin + 15) // 16) >= 512 else 2


def same_bits(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


SHAPES = [  # (k, R, Cin, C, staging rounds, forward patch columns, NPT)
    (9, 32, 1, 3, 2, 1, 2), (28, 32, 1, 4, 2, 1, 2), (17, 17, 2, 3, 1, 1, 2), (33, 8, 1, 5, 1, 2, 2), (64, 8, 1, 8, 1, 2, 2),
    (9, 4, 3, 683, 1, 1, 4), (9, 4, 1, 2032, 1, 1, 2), (5, 4, 1, 1, 1, 1, 2)]


@pytest.mark.parametrize('k,R,Cin,C,rounds,cols,want_npt', SHAPES)
def test_rotate_bank_fp64(k, R, Cin, C, rounds, cols, want_npt):
    from tvae import ops
    from tvae._lib import call
    tot = max(patch_totals(k, R))
    assert (tot + RBB_CAP - 1) // RBB_CAP == rounds, tot
    if (k, R) == (17, 17):
        assert 3900 < tot <= RBB_CAP, tot                                 # (3 997: just under one round)
    assert (k + 31) // 32 == cols and npt(k, Cin, C) == want_npt
    if want_npt == 4:
        assert (C * Cin) % 16 != 0
    k2 = k * k
    w = rnd(C, Cin, 1, k, k, seed=k)
    wg = w.to(dev())
    # forward
    bank = ops.rotate_bank(wg, R)
    bank2 = ops.rotate_bank(wg, R)
    assert tuple(bank.shape) == (C * R, Cin * k2) and same_bits(bank, bank2)
    ref, cond = bank_ref.forward(w, k, R)
    err = (bank.double().cpu() - ref).abs()
    bound = 5 * U * cond
    assert bool((err <= bound).all()), ('forward', float((err / bound.clamp_min(1e-300)).max()))
    # backward, overwriting and accumulating
    g = rnd(C * R, Cin * k2, seed=9)
    gg = g.to(dev())
    ptr, er, ed, ew = ops.tap_tables_csr(k, R, dev())
    init = rnd(C, Cin, 1, k, k, seed=10)
    for accumulate in (0, 1):
        res = []
        for _ in range(2):
            dW = init.clone().to(dev()) if accumulate else torch.full((C, Cin, 1, k, k), float('nan'), device=dev())
            call('tvae_rotate_bank_bwd', gg, ptr, er, ed, ew, dW, C, Cin, k, R, accumulate)
            res.append(dW)
        torch.cuda.synchronize()
        assert same_bits(res[0], res[1]), ('backward', accumulate)
        ref, cond, n = bank_ref.backward(g, C, Cin, k, R, init=init if accumulate else None)
        err = (res[0].double().cpu().reshape(C * Cin, k2) - ref).abs()
        bound = (n.double() + 1) * U * cond
        worst = float((err / bound.clamp_min(1e-300)).max())
        assert bool((err <= bound).all()), ('backward', accumulate, worst)
        if not accumulate:                               # (tvae.ops' own backward is this call)
            assert same_bits(ops.rotate_bank_bwd(gg, C, Cin, k, R), res[0])
