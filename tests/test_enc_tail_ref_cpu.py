"""tests/enc_tail_ref.py checked on the CPU: its gradient restatements against torch autograd of the forward expression in float64
(masks taken from the same H and A1), the sign-word layout and the k permutation against include/tvae_hip.h and tvae.ops, the
restated h3 scale, its case lists against the branch conditions they are meant to reach (the grid arithmetic of the kernels,
for 256 and 304 CUs), and its K table against CPU arithmetic on the cases test_enc_tail_fp64_gpu.py runs
(K = max(16, 8 x worst ratio); printed by test_budget_constants)."""
import math

import pytest
import torch

import enc_tail_ref as R

F64 = torch.float64
CUS = (256, 304)
BY_PARTS = {}                 # (output, parts) -> worst CPU ratio, filled by cpu_ratios()


def close(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('nh,N', [(1, 33), (7, 70), (23, 40), (128, 33)])
def test_gradients_against_autograd(nh, N):
    """dgrad / wgrad are d/d(pre-activation of A1), d/dW2 and d/dWh of sum(dheads . heads), heads = Wh lrelu(W2 lrelu(P) + b2) + bh."""
    W2, b2, Wh, bh = R.weights(nh)
    dheads = R.rnd(nh, N, seed=11)
    P = R.rnd(R.C, N, seed=12).double().requires_grad_(True)
    w2, wh = W2.double().requires_grad_(True), Wh.double().requires_grad_(True)
    A1 = R.act_apply(P, 1)
    out = R.fwd(w2, A1, b2, wh, bh, 1)
    assert close(out['heads'].detach(), R.heads_of(Wh, out['H'].detach(), bh))
    (out['heads'] * dheads.double()).sum().backward()
    g = R.dgrad(W2, Wh, dheads, out['H'].detach() > 0, A1.detach() > 0)
    assert close(g['dA1'], P.grad)
    assert close(R.wgrad(g['dH'], A1.detach()), w2.grad)                 # tvae_enc_tail_wgrad_x6, and _wide with D = dH
    assert close(R.wgrad(dheads, out['H'].detach()), wh.grad)            # tvae_enc_tail_wgrad_wide with D = dheads, A = H
    c = R.dgrad(W2, Wh, dheads, out['H'].detach() > 0, A1.detach() > 0, cond=True)
    assert (c['dA1'] >= g['dA1'].abs() * (1 - 1e-12)).all() and (c['dH'] >= g['dH'].abs() * (1 - 1e-12)).all()


def test_sign_word_layout_and_round_trip():
    bits = R.bit_pattern('random', 70, 3)
    words = R.pack(bits)
    assert words.shape == (70, 4) and words.dtype == torch.int32 and torch.equal(R.unpack(words), bits)
    for r, n in ((0, 0), (31, 5), (32, 5), (77, 69), (127, 1)):          # bit (r & 31) of word r >> 5 of column n is row r
        one = torch.zeros(R.C, 70, dtype=torch.bool)
        one[r, n] = True
        w = R.pack(one).to(torch.int64) & 0xffffffff
        assert int(w[n, r >> 5]) == 1 << (r & 31) and int(w.sum()) == 1 << (r & 31)
    walk, co = R.bit_pattern('walk', 300, 0), R.bit_pattern('cowalk', 300, 0)
    assert (walk.sum(0) == 1).all() and all(bool(walk[n % 128, n]) for n in range(300)) and torch.equal(co, ~walk)
    assert not R.bit_pattern('zeros', 5, 0).any() and R.bit_pattern('ones', 5, 0).all()
    pre = torch.full((3, 4), R.BITS_PREFILL, dtype=torch.int32)
    assert int(pre[0, 0]) & 0xffffffff == 0xA5A5A5A5


def test_permutation_is_the_products():
    from tvae.ops import _enc_tail_perm
    p = R.perm()
    assert torch.equal(p, torch.as_tensor(_enc_tail_perm(torch.device('cpu'))).long().cpu())
    assert sorted(p.tolist()) == list(range(128))


def test_h3_scale_restated():
    a = torch.tensor([0.0, 1e-45, 1.0, 1.5, 2.0, 0.3, 1e-20, 1e20, 3e38, 2.0 ** -126])
    s = R.h3_scale(a)
    assert s[0] == 2.0 ** 14 and s[1] == 2.0 ** 14 and s[2] == 2.0 ** 14 and s[3] == 2.0 ** 14 and s[4] == 2.0 ** 13
    for x, sv in zip(a[2:8].tolist(), s[2:8].tolist()):
        assert 2.0 ** 14 <= x * sv < 2.0 ** 15 and math.frexp(sv)[0] == 0.5
    assert s[8] == 2.0 ** -113 and s[9] == 2.0 ** 125                    # (the scale's biased exponent is clamped to 2 .. 252)
    assert float(R.delta(torch.tensor(1.0))) == 2.0 ** -39


def test_case_lists_reach_their_branches():
    """The grid arithmetic of abi_enc_tail_x6.hip / abi_enc_tail_wide.hip and of the kernels' chunk loops on the case lists."""
    for cus in CUS:
        my = {N: R.et_waves(N, cus) for N in R.NS_SMALL + R.ns_big(cus)}
        assert my[1] == [1] + [0] * 7 and my[31] == my[1] and my[32] == my[1]           # fewer chunks than waves
        assert my[33] == [1, 1] + [0] * 6 and my[255] == [1] * 8 and my[256] == [1] * 8  # exactly one workgroup's worth
        assert my[257] == [1] * 9 + [0] * 7                                              # a second workgroup with one busy wave
        assert all(N % 32 for N in (1, 31, 33, 255, 257)) and all(N % 32 == 0 for N in (32, 256))
        n1, n2 = R.ns_big(cus)
        assert len(my[n1]) == 8 * cus and my[n1] == [2] * 4 + [1] * (8 * cus - 4) and n1 % 32 == 5
        assert ((n1 + 31) // 32 - 1) % (8 * cus) == 3                  # the ragged chunk is wave 3's SECOND: ci = 1 of my = 2
        assert my[n2] == [3] * 8 + [2] * (8 * cus - 8) and n2 % 32 == 0
        # the clamped reload (ci >= my) is met by every wave in its last chunk; the hand-over wAsn -> wAs / load_bits(ci + 1)
        # between DIFFERENT chunks only where my >= 2; two-ahead loads all distinct where my == 3
        for N in (n1, n2):
            sp = R.special_chunks(N, cus)
            nch = (N + 31) // 32
            assert all(ch < nch for ch in sp) and {0.0, 2.0 ** 20, 2.0 ** -20} <= set(sp.values())
            assert any(ch >= 8 * cus and f == 2.0 ** 20 for ch, f in sp.items())        # a stale chunk scale would overflow
        assert any(ch >= 16 * cus for ch in R.special_chunks(n2, cus))
        counts = {n: R.ew_counts(n, cus) for n in R.wgrad_chunks(cus)}
        assert counts[1] == [1] and counts[2] == [1, 1] and counts[3] == [1, 1, 1]
        c = counts[cus + 1]
        assert len(c) == cus and c[:cus // 2] == [2] * (cus // 2) and c[cus // 2] == 1 and set(c[cus // 2 + 1:]) == {0}
        c = counts[2 * cus + 1]
        busy = [x for x in c if x]
        assert set(busy[:-1]) == {3} and 0 in c and sum(c) == 2 * cus + 1
        c = counts[3 * cus + 2]
        busy = [x for x in c if x]
        assert set(busy[:-1]) == {4} and busy[-1] == 2 and 0 in c and sum(c) == 3 * cus + 2
    # wide data gradient: rem of the k-steps
    rems = {nh: R.wide_rems(nh) for nh in R.WIDE_DGRAD_NH}
    part = {nh: [r for r in rems[nh] if 0 < r < 16] for nh in R.WIDE_DGRAD_NH}
    assert part[1] == [1] and part[7] == [7] and part[8] == [8]                      # upper lane half fully clamped
    assert part[9] == [9] and part[12] == [12] and part[15] == [15] and part[31] == [15]      # ... partly clamped
    assert part[16] == [] and part[128] == [] and part[17] == [1] and part[113] == [1]
    assert all(r >= 16 for r in rems[128]) and rems[16][1:] == [0, -16, -32, -48, -64, -80, -96]     # rem >= 16 | rem <= 0
    assert {r for nh in R.WIDE_DGRAD_NH for r in part[nh]} >= {1, 7, 8, 9, 12, 15}
    # wide forward: halves and row tiles of the second GEMM, the store mask row < m2 in both lane halves
    tiles = {nh: R.wide_tiles(nh) for nh in R.WIDE_FWD_NH}
    assert all(tiles[nh][0] == [True, False] for nh in (1, 4, 7, 8, 9, 32, 33, 64))
    assert all(tiles[nh][0] == [True, True] for nh in (65, 96, 97, 127, 128))
    assert [sum(tiles[nh][1]) for nh in R.WIDE_FWD_NH] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4]
    # et_row(i, r, kh) = 32 i + 8 (r >> 2) + (r & 3) + 4 kh: nh = 1 .. 4 end inside half 0's rows of a group of 8, 5 .. 7 in half 1's
    assert {nh % 8 for nh in R.WIDE_FWD_NH} >= {1, 4, 7, 0}
    assert {c[1] for c in R.x6_fwd_cases()} == set(range(1, 8)) and {c[2] for c in R.x6_fwd_cases()} == {0, 1, 2}
    assert {c[0] for c in R.x6_fwd_cases()} >= set(R.NS_SMALL) and any(not c[3] for c in R.x6_fwd_cases())
    assert {(c[1], c[2]) for c in R.x6_fwd_cases() if c[2] == 1} >= {(nh, 1) for nh in (1, 4, 7)}
    assert {c[1] for c in R.x6_dgrad_cases()} == set(range(1, 8)) and {c[2] for c in R.x6_dgrad_cases()} == set(R.BIT_PATTERNS)
    assert {c[0] for c in R.x6_dgrad_cases()} >= set(R.NS_SMALL)
    assert [c[1] for c in R.wide_fwd_cases()[:13]] == R.WIDE_FWD_NH and {c[2] for c in R.wide_fwd_cases()} == {0, 1, 2}
    assert [c[1] for c in R.wide_dgrad_cases()[:11]] == R.WIDE_DGRAD_NH and {c[3] for c in R.wide_dgrad_cases()} == {1.0, 64.0}
    assert len(set(R.PADS)) == 4
    # planted columns: first and last of a chunk, the last valid column of a ragged chunk
    assert R.plant_columns(257) == [0, 31, 32, 63, 256] and R.plant_columns(33) == [0, 31, 32] and R.plant_columns(1) == [0]
    A1 = R.a1_case(257)
    assert (A1[:, R.zero_column(257)] == 0).all() and float(A1[0, 0]) == 0.0 and math.copysign(1.0, float(A1[3, 0])) == -1.0
    assert float(A1[8, 0]) == 1e-40 or float(A1[8, 0]) > 0               # (a denormal survives in the tensor)
    W2, b2, _, _ = R.weights(7)
    assert int((W2[R.ONE_HOT_ROW] != 0).sum()) == 1 and int((W2[:, R.ONE_HOT_COL] != 0).sum()) == 1 and float(b2[R.ONE_HOT_ROW]) == 0


def cpu_ratios(cus=256):
    """name -> worst ratio of the CPU arithmetic of `parts` against the reference, over the cases of the GPU file"""
    worst = {n_: 0.0 for n_ in R.K}
    BY_PARTS.clear()

    def take(fam, parts, got, ref, cond, floor):
        for n_ in ref:
            r = R.ratio(got[n_], ref[n_], cond[n_], R.UNIT[parts], None if floor is None else floor[n_])
            assert math.isfinite(r), (fam, n_, parts)
            worst[f'{fam}_{n_}'] = max(worst[f'{fam}_{n_}'], r)
            BY_PARTS[f'{fam}_{n_}', parts] = max(BY_PARTS.get((f'{fam}_{n_}', parts), 0.0), r)

    memo = {}

    def once(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    def fwd_case(wide, N, nh, act, has_b2, parts, scale=1.0, slack=1.0, dyn=False):
        W2, b2, Wh, bh = R.weights(nh, dyn)
        b2 = b2 if has_b2 else None
        A1 = R.a1_case(N, scale, dyn)
        amax = A1.abs().amax(1) * slack
        ref, cond = once(('fwd', N, nh, act, has_b2, scale, dyn), lambda: R.both(R.fwd, W2, A1, b2, Wh, bh, act))
        got = R.emu_fwd(parts, wide, W2, A1, b2, Wh, bh, act, amax)
        floor = R.fwd_floor(wide, W2, A1, Wh, amax, ref['H']) if parts == 2 else None
        take('wide' if wide else 'x6', parts, got, ref, cond, floor)

    def dgrad_case(wide, N, nh, pat, parts, slack=1.0, cus_=None):
        W2, _, Wh, _ = R.weights(nh)
        d = R.dheads_case(nh, N, cus_)
        bh_, ba_ = R.bit_pattern(pat, N, 1), R.bit_pattern(pat, N, 2)
        amax = d.abs().max() * slack
        ref, cond = once(('dgrad', N, nh, pat), lambda: R.both(R.dgrad, W2, Wh, d, bh_, ba_))
        got = R.emu_dgrad(parts, wide, W2, Wh, d, bh_, ba_, amax)
        floor = R.dgrad_floor(wide, W2, Wh, d, bh_, ba_, amax, ref) if parts == 2 else None
        if not wide:
            ref, cond, got = ({'dA1': x['dA1']} for x in (ref, cond, got))
            floor = None if floor is None else {'dA1': floor['dA1']}
        take('wide' if wide else 'x6', parts, got, ref, cond, floor)

    def wgrad_x6_case(N, nh, pat, parts, dyn=False, slack=1.0, zero_col=None):
        Wh = R.wgrad_wh(nh, dyn)
        if zero_col is not None:
            Wh[:, zero_col] = 0.0
        A, _ = R.wgrad_case(N, dyn)
        d, bits = R.dheads_case(nh, N, plain=True), R.bit_pattern(pat, N, 1)
        dH = R.mask(bits) * (Wh.double().t() @ d.double())
        cH = R.mask(bits) * (Wh.double().abs().t() @ d.double().abs())
        sd, sa = R.wgrad_x6_scale_d(Wh, d), A.abs().amax(1) * slack
        got = R.emu_wgrad(parts, R.mask(bits, torch.float32) * (Wh.t() @ d), A, sd, sa)
        floor = {'dW2': R.wgrad_floor(dH, A, sd, sa)} if parts == 2 else None
        take('x6', parts, {'dW2': got}, {'dW2': R.wgrad(dH, A)}, {'dW2': R.wgrad(cH, A, cond=True)}, floor)

    big = R.ns_big(cus)
    for parts in (3, 2, 1):
        for N, nh, act, has_b2 in R.x6_fwd_cases() + [(N, 7, 1, True) for N in big]:
            fwd_case(False, N, nh, act, has_b2, parts)
        for N, nh, pat in R.x6_dgrad_cases() + [(N, 7, 'random') for N in big]:
            dgrad_case(False, N, nh, pat, parts, cus_=cus if N in big else None)
        for ci, nch in enumerate(R.wgrad_chunks(cus)):
            for nh in R.WGRAD_X6_NH:
                wgrad_x6_case(32 * nch, nh, R.BIT_PATTERNS[(ci + nh) % 5], parts)
    wgrad_x6_case(96, 7, 'random', 2, True, 64.0, 50)
    for scale, slack, dyn, act in R.h3_fwd_variants():
        fwd_case(False, 257, 7, act, True, 2, scale, slack, dyn)
    for parts in (2, 1):
        for N, nh, act, has_b2 in R.wide_fwd_cases() + [(N, 103, 1, True) for N in big]:
            fwd_case(True, N, nh, act, has_b2, parts)
        for N, nh, pat, slack in R.wide_dgrad_cases() + [(N, 103, 'random', 1.0) for N in big]:
            dgrad_case(True, N, nh, pat, parts, slack, cus_=cus if N in big else None)
    for ci, nch in enumerate(R.wgrad_chunks(cus)):
        for rows in R.WGRAD_WIDE_ROWS:
            A, D = R.wgrad_case(32 * nch, (ci + rows) % 2 == 1)
            D = D[:rows]
            slack = (1.0, 64.0)[ci % 2]
            am_d, am_a = D.abs().max() * slack, A.abs().amax(1) * slack
            ref, cond = R.both(R.wgrad, D, A)
            take('wide', 2, {'dW': R.emu_wgrad(2, D, A, am_d, am_a)}, {'dW': ref}, {'dW': cond}, {'dW': R.wgrad_floor(D, A, am_d, am_a)})
    return worst


def test_budget_constants(capsys):
    """K of enc_tail_ref: every operation in CPU arithmetic (fp32; fp16 / bf16 operand rounding under the kernels' scales) against
    its float64 restatement.  Printed; enc_tail_ref.K has to cover it, and not by more than a quarter."""
    worst = cpu_ratios()
    with capsys.disabled():
        print('\nencoder-tail budgets: worst ratio (error - floor) / (UNIT cond), CPU arithmetic against enc_tail_ref, and K = max(16, 8 x ratio)')
        for n_, w in worst.items():
            by = '  '.join(f'parts {p}: {BY_PARTS[n_, p]:6.3f}' for p in (3, 2, 1) if (n_, p) in BY_PARTS)
            print(f'  {n_:12s} ratio {w:8.3f}   K measured {max(16.0, 8 * w):8.2f}   K used {R.K[n_]:8.2f}   ({by})')
    for n_, w in worst.items():
        assert w > 0, n_                                     # (every output was measured)
        assert max(16.0, 8 * w) <= R.K[n_] <= max(16.0, 8 * w) * 1.25, (n_, w, R.K[n_])


def test_ratio_helper_is_strict():
    ref, cond = torch.tensor([1.0, 2.0, 0.0], dtype=F64), torch.tensor([1.0, 2.0, 0.0], dtype=F64)
    u = R.UNIT[3]
    assert R.ratio(ref.float(), ref, cond, u) == 0.0
    assert R.ratio(torch.tensor([1.0, 2.0, 1e-30]), ref, cond, u) == math.inf              # exact where the condition is zero
    assert R.ratio(torch.tensor([1.0, 2.0, 1e-30]), ref, cond, u, floor=torch.ones(3, dtype=F64)) == math.inf     # ... floor or not
    assert R.ratio(torch.tensor([1.0, float('nan'), 0.0]), ref, cond, u) == math.inf
    assert R.ratio(torch.tensor([1.0, 2.0, -0.0]), ref, cond, u) == 0.0
    assert abs(R.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond, u) - 16.0) < 1e-6
    assert R.ratio(torch.tensor([1.0 + 2.0 ** -20, 2.0, 0.0]), ref, cond, u, floor=torch.full((3,), 1.0, dtype=F64)) == 0.0
