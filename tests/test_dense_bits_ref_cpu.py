"""tests/dense_bits_ref.py against autograd: a real two-layer decoder tail in float64 (first layer from coordinates and a
per-image latent term, one hidden layer, the single-output Linear, loss = gy . y), its sign bits packed into words, and every
quantity the helper states -- data gradient, fused first-layer outputs, row sums, dWo from the weight-gradient identity --
compared with what torch.autograd gives for the same graph.  Also: pack / unpack are inverses of each other."""
import torch

import dense_bits_ref as R

M, K, N, Np = 24, 20, 64, 32
RTOL = 1e-12


def close(a, b):
    return (a - b).abs().max().item() <= RTOL * b.abs().max().item()


def test_pack_unpack_identity():
    words, mask = R.random_bits(7, 96, seed=3)
    words[0, 0], words[1, 1], words[2, 2] = -2 ** 31, 1, -1      # only the top bit; only bit 0; every bit
    words[3, 0] = 2 ** 31 - 1                                    # every bit but the top one
    mask = R.unpack(words)
    assert mask.shape == (7, 96) and mask.dtype == torch.bool
    assert mask[0, 31] and int(mask[0, :32].sum()) == 1          # column 31 of a word <-> its top bit (a negative int32)
    assert mask[1, 32] and int(mask[1, 32:64].sum()) == 1
    assert bool(mask[2, 64:96].all())
    assert not mask[3, 31] and int(mask[3, :32].sum()) == 31
    assert torch.equal(R.pack(mask), words)
    m2 = torch.zeros(2, 64, dtype=torch.bool)
    m2[0, 31] = m2[1, 63] = m2[1, 32] = True
    w2 = R.pack(m2)
    assert w2.dtype == torch.int32 and w2.tolist() == [[-2 ** 31, 0], [0, -2 ** 31 + 1]]
    assert torch.equal(R.unpack(w2), m2)
    words_r, mask_r = R.random_bits(5, 64, seed=1)
    assert torch.equal(R.unpack(words_r), mask_r) and torch.equal(R.pack(mask_r), words_r)


def test_reference_against_autograd():
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B = N // Np
    xr, wc, bc, lb = rn(N, 2).requires_grad_(), rn(K, 2).requires_grad_(), rn(K).requires_grad_(), rn(B, K).requires_grad_()
    W, b, wo, gy = (rn(M, K) * K ** -0.5).requires_grad_(), rn(M).requires_grad_(), rn(M).requires_grad_(), rn(N)
    act = torch.nn.LeakyReLU(R.SLOPE)
    pre0 = wc @ xr.t() + bc[:, None] + lb[torch.arange(N) // Np].t()
    pre0.retain_grad()
    H0 = act(pre0)
    H = act(W @ H0 + b[:, None])
    (gy * (wo @ H)).sum().backward()

    words = R.pack(H.detach() > 0)
    bits = R.unpack(words)
    assert torch.equal(bits, H.detach() > 0) and 0 < int(bits.sum()) < bits.numel()
    a = R.act_factor(bits)
    Wd, wod, H0d = W.detach(), wo.detach(), H0.detach()
    assert torch.equal(R.first_layer_pre(xr.detach(), wc.detach(), bc.detach(), lb.detach(), Np) > 0, pre0.detach() > 0)
    mask = R.lrelu_mask(H0d)
    assert 0 < int((mask == 1).sum()) < mask.numel()
    dX = R.dgrad(Wd, wod, gy, a, mask=mask)
    assert close(dX, pre0.grad)
    # the same with the recomputed mask, and the two other mask sources against their definition
    pre = R.first_layer_pre(xr.detach(), wc.detach(), bc.detach(), lb.detach(), Np)
    assert torch.equal(R.dgrad(Wd, wod, gy, a, mask=R.lrelu_mask(pre)), dX)
    add = rn(K, N)
    assert close(R.dgrad(Wd, wod, gy, a, mask=mask, add=add), dX + mask * add)
    assert close(R.dgrad(Wd, wod, gy, a) * mask, dX)
    assert close(R.csum(Wd, wod), (wod @ Wd))
    # row sums and the identity dWo[m] = sum_k W[m][k] G[m][k] + b[m] g0[m]
    G = (gy[None, :] * a) @ H0d.t()
    assert close(wod[:, None] * G, W.grad)
    g0, rs_db, rs_dwo = R.row_sums(a, gy, wod, (Wd * G).sum(1), b.detach())
    assert close(rs_db, b.grad) and close(rs_dwo, wo.grad)
    assert close(R.tile_sums(bits, gy, panel=16).sum(1), bits.double() @ gy)
    # fused first-layer backward
    gxr, part, Simg, dbc, dWc = R.in_tail(dX, xr.detach(), wc.detach(), Np, panel=16)
    assert close(gxr, xr.grad) and close(dbc, bc.grad) and close(dWc, wc.grad) and close(Simg, lb.grad)
    assert part.shape == (N // 16, K, 3)
    x = xr.detach()
    assert close(part[3, :, 0], dX[:, 48:64].sum(1)) and close(part[1, :, 2], dX[:, 16:32] @ x[16:32, 1])
