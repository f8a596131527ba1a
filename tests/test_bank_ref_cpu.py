"""tests/bank_ref.py (the sparse float64 operator of the rotated bank) against oracle.rotated_bank and its autograd, on the CPU,
at R = 32, k = 9: the tap tables beyond the rotations the command lines use."""
import torch

import bank_ref
from oracle import tvae_oracle as O


def test_operator_matches_the_oracle_beyond_16_rotations():
    k, R, Cin, C = 9, 32, 2, 3
    g = torch.Generator().manual_seed(5)
    w = torch.randn(C, Cin, 1, k, k, generator=g)
    wr = w.double().requires_grad_(True)
    ref = O.rotated_bank(wr, R)                                          # (C, R, Cin, 1, k, k) float64
    bank, cond = bank_ref.forward(w, k, R)
    r0 = ref.detach().reshape(C, R, Cin, k * k)
    assert (bank.reshape(C, R, Cin, k * k) - r0).abs().max() <= 1e-14 * float(r0.abs().max())
    assert bool((cond + 1e-300 >= bank.abs()).all())
    gb = torch.randn(C * R, Cin * k * k, generator=g)
    (ref.reshape(C * R, Cin * k * k) * gb.double()).sum().backward()
    dW, cond, n = bank_ref.backward(gb, C, Cin, k, R)
    assert (dW - wr.grad.reshape(C * Cin, k * k)).abs().max() <= 1e-13 * float(wr.grad.abs().max())
    assert bool((cond + 1e-300 >= dW.abs()).all()) and int(n.sum()) > 0
    # with an initial value: one more term
    init = torch.randn(C, Cin, 1, k, k, generator=g)
    dW1, cond1, n1 = bank_ref.backward(gb, C, Cin, k, R, init=init)
    assert torch.equal(dW1, dW + init.double().reshape(C * Cin, k * k)) and torch.equal(n1, n + 1)
