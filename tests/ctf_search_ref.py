"""numpy restatement of the section "Selection of a hard pose search from its tables" of include/tvae_cluster.h (a plain helper
module, used by test_ctf_search_ref_cpu.py and test_ctf_search_gpu.py): the score of a candidate from the three fp32 words, the
selection rule of a slot as the serial loop of tvae_pose_refine and as the order-free arg-max the kernel reduces with, the rule
across slots and the pose update (pose_ref.update_pose: fp32 steps in the order of the device function).

The score is np.float32(np.float64(num) / np.sqrt(np.float64(p) * np.float64(y))) and exactly 0 where p or y is 0.  Each numpy
fp64 operation is correctly rounded, like the device intrinsics, and so is the conversion to fp32: equality with the kernel is
bit for bit, for NaN and the infinities too (IEEE gives both sides the same special values)."""
import numpy as np

import pose_ref

F32 = np.float32
NINF = F32(-np.inf)


def scores(num, p, y):
    """fp32 arrays that broadcast against each other -> fp32 scores."""
    num, p, y = (np.asarray(a, dtype=F32).astype(np.float64) for a in (num, p, y))
    with np.errstate(all='ignore'):
        zero = (p == 0) | (y == 0)
        return np.where(zero, 0.0, num / np.sqrt(p * y)).astype(F32)


def slot_serial(flat, ci):
    """The rule of tvae_pose_refine as it visits the candidates: flat fp32 [cnd], ci the centre -> (bi, sc, sb)."""
    centre = flat[ci]
    bi = ci
    found = bool(np.isfinite(centre))
    bv = centre if found else NINF
    for e in range(flat.size):
        v = flat[e]
        if np.isfinite(v) and v > bv:
            bv, bi, found = v, e, True
    if not found:
        return ci, F32(0), F32(0)
    return bi, (centre if np.isfinite(centre) else NINF), bv


def slot_order_free(flat, ci):
    """The same rule without an order of visits: among the finite scores the largest; among equal largest the centre if it is
    one of them, otherwise the lowest flat index."""
    finite = np.isfinite(flat)
    if not finite.any():
        return ci, F32(0), F32(0)
    top = flat[finite].max()
    winners = np.flatnonzero(finite & (flat == top))
    bi = ci if ci in winners else int(winners.min())
    return bi, (flat[ci] if finite[ci] else NINF), flat[bi]


def select_ref(num, pp, yy, cand, theta, dx, n, K, A, S, t_scale, dtheta, slot_rule=slot_serial):
    """num fp32 [N][M][NA][NS][NS], pp [N][M][NA] or the shape of num, yy [N], cand int [N][M], theta [N], dx [N][2] ->
    dict(cls int32 [N], best int32 [N][4], theta fp32 [N], dx fp32 [N][2], score fp32 [N][M][2]): tvae_pose_select."""
    num = np.asarray(num, dtype=F32)
    pp = np.asarray(pp, dtype=F32)
    cand = np.asarray(cand).astype(np.int64)
    N, M = cand.shape
    NA, NS = 2 * A + 1, 2 * S + 1
    assert num.shape == (N, M, NA, NS, NS) and pp.shape in ((N, M, NA), num.shape)
    p = pp if pp.ndim == 5 else pp[:, :, :, None, None]
    sc = scores(num, p, np.asarray(yy, dtype=F32).reshape(N, 1, 1, 1, 1)).reshape(N, M, -1)
    ci = (A * NS + S) * NS + S
    score = np.zeros((N, M, 2), dtype=F32)
    cls, best = np.zeros(N, dtype=np.int32), np.zeros((N, 4), dtype=np.int32)
    for i in range(N):
        wm, wbi, wsb = -1, ci, F32(0)
        for m in range(M):
            if not 0 <= cand[i, m] < K:
                continue
            bi, c, b = slot_rule(sc[i, m], ci)
            score[i, m] = (c, b)
            if wm < 0 or b > wsb:                            # ties stay with the lower slot
                wm, wbi, wsb = m, bi, b
        cls[i] = np.clip(cand[i, max(wm, 0)], -2 ** 31, 2 ** 31 - 1)
        best[i] = (max(wm, 0), wbi // (NS * NS) - A, (wbi // NS) % NS - S, wbi % NS - S)
    th, d = pose_ref.update_pose(theta, dx, best[:, 1:].astype(np.int64), n, t_scale, dtheta)
    return dict(cls=cls, best=best, theta=th, dx=d, score=score)
