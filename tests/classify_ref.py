"""fp64 numpy restatement of the reassignment against the class averages of include/tvae_cluster.h (a plain helper module,
used by test_classify_cpu.py and test_classify_gpu.py), built on pose_ref: every slot IS pose_ref.refine with
cls = cand[:, m]; on top of it the rule across slots, the pose update of the winner, the candidate lists and the cross-half
slot rule of tvae.classify, and rounds(), the loop of classify_rounds on align_ref.align_stack / class_averages."""
import numpy as np

import align_ref
import frc_ref
import pose_ref

F32 = np.float32


def choose(slot_out, slot_best, cand, K):
    """The rule across slots.  slot_out [N][M][2] = (centre, best) and slot_best [N][M][3] = (a, sy, sx) of every slot,
    cand [N][M] -> (cls_out int64 [N], best int64 [N][4] = (m*, a, sy, sx)): the valid slots in ascending m, the first is the
    start and a later one replaces it only if its best score is strictly greater; no valid slot: cand[i][0] and zeros."""
    slot_out, slot_best = np.asarray(slot_out), np.asarray(slot_best)
    cand = np.asarray(cand).astype(np.int64)
    N, M = cand.shape
    cls_out, best = cand[:, 0].copy(), np.zeros((N, 4), dtype=np.int64)
    for i in range(N):
        win = -1
        for m in range(M):
            if not 0 <= cand[i, m] < K:
                continue
            if win < 0 or slot_out[i, m, 1] > slot_out[i, win, 1]:
                win = m
        if win >= 0:
            cls_out[i] = cand[i, win]
            best[i] = (win,) + tuple(slot_best[i, win])
    return cls_out, best


def classify(Y, theta, dx, cand, refs, t_scale, A, dtheta, S, mask_radius=None, mask_edge=0.0):
    """The whole definition -> dict(T [N][M].., num, pp [N][M][NA][NS][NS], yy [N], score [N][M][2], slot_best [N][M][3],
    cls, best [N][4], theta, dx)."""
    refs = np.asarray(refs)
    K, n = refs.shape[0], refs.shape[-1]
    cand = np.asarray(cand).astype(np.int64)
    N, M = cand.shape
    slots = [pose_ref.refine(Y, theta, dx, cand[:, m], refs, t_scale, A, dtheta, S, mask_radius, mask_edge) for m in range(M)]
    stack = lambda key: np.stack([s[key] for s in slots], 1)
    yy = np.stack([s['yy'] for s in slots], 1).max(1)        # the same sum in every valid slot, 0 in a skipped one
    cls_out, best = choose(stack('out'), stack('best'), cand, K)
    th, d = pose_ref.update_pose(theta, dx, best[:, 1:], n, t_scale, dtheta)
    return dict(T=stack('T'), num=stack('num'), pp=stack('pp'), yy=yy, score=stack('out'), slot_best=stack('best'),
                cls=cls_out, best=best, theta=th, dx=d)


def candidate_lists(labels, n_clusters, latents=None, m=None):
    """-> int64 [N][M] as tvae.classify.candidate_lists defines it, one image at a time."""
    lab = np.asarray(labels).astype(np.int64)
    K = int(n_clusters)
    if m is None:
        if K > 64:
            raise ValueError('more than 64 classes need m')
        m = K
    N = lab.size
    member = (lab >= 0) & (lab < K)
    if latents is not None:
        z = np.asarray(latents, dtype=np.float64)
        counts = np.array([(lab == k).sum() for k in range(K)])
        cen = np.stack([z[lab == k].sum(0) / max(counts[k], 1) for k in range(K)])
    out = np.zeros((N, m), dtype=np.int64)
    for i in range(N):
        if latents is None:
            dist = np.arange(K, dtype=np.float64)
        else:
            dist = np.where(counts == 0, np.inf, ((z[i][None, :] - cen) ** 2).sum(-1))
        others = [k for k in sorted(range(K), key=lambda k: (dist[k], k)) if not (member[i] and k == lab[i])]
        out[i] = ([lab[i]] if member[i] else [-1]) + others[:m - 1]
    return out


def cross_half_candidates(labels, cand, n_clusters):
    """The slot for class k among the 2K references [half 0 of class 0 .. K - 1, half 1 of ...]: K + k for an image at an
    even position of its own class (and for an image outside every class), k at an odd one; -1 for a slot outside [0, K)."""
    K = int(n_clusters)
    cand = np.asarray(cand).astype(np.int64)
    own = pose_ref.cross_half_labels(labels, K)
    odd = (own >= 0) & (own < K)
    valid = (cand >= 0) & (cand < K)
    return np.where(valid, np.where(odd[:, None], cand, cand + K), -1)


def averages(Y, theta, dx, labels, K, t_scale, halves=False):
    """fp64 class averages [K][C][n][n] of the labels and poses, or the 2K half-set averages [half 0 | half 1]."""
    aligned = align_ref.align_stack(Y, theta, dx, t_scale)
    order, seg, _ = align_ref.segments(labels, K)
    if not halves:
        return align_ref.class_averages(aligned, order, seg)[0]
    out = np.zeros((2, K) + aligned.shape[1:])
    for k, (even, odd) in enumerate(frc_ref.half_lists(order, seg, aligned.shape[0])):
        for h, mem in enumerate((even, odd)):
            if len(mem):
                out[h, k] = aligned[np.asarray(mem, dtype=np.int64)].sum(0) / len(mem)
    return out.reshape((2 * K,) + aligned.shape[1:])


def rounds(Y, theta, dx, labels, K, t_scale=1.0, rounds=3, angle_range=np.pi / 8, A=8, S=2, mask_radius=None, mask_edge=0.0,
           cross_halves=False, latents=None, m=None):
    """The loop of tvae.classify.classify_rounds in fp64 -> (labels, theta, dx, history) with history['steps'], ['scores']
    [rounds][2], ['moved'] [rounds], ['counts'] [rounds + 1][K] and the last round's ['candidates'] and ['slot_scores']."""
    lab = np.asarray(labels).astype(np.int64)
    th, d = np.asarray(theta, dtype=F32).reshape(-1), np.asarray(dx, dtype=F32)
    count = lambda l: np.bincount(l[(l >= 0) & (l < K)], minlength=K)
    steps, scores, moved, counts = [], [], [], [count(lab)]
    cand = res = None
    for j in range(rounds):
        step = float(angle_range) / max(A, 1) / 2 ** j
        cand = candidate_lists(lab, K, latents, m)
        refs = averages(Y, th, d, lab, K, t_scale, cross_halves)
        slots = cross_half_candidates(lab, cand, K) if cross_halves else cand
        res = classify(Y, th, d, slots, refs, t_scale, A, step, S, mask_radius, mask_edge)
        new = res['cls']
        if cross_halves:
            new = np.where(new >= 0, new % K, new)
        member = (lab >= 0) & (lab < K)
        win = res['score'][np.arange(lab.size), res['best'][:, 0], 1]
        pair = np.stack([res['score'][:, 0, 0], win], 1)[member].astype(np.float64)
        scores.append(pair.mean(0) if pair.size else np.zeros(2))
        moved.append(int((new != lab).sum()))
        lab, th, d = new, res['theta'], res['dx']
        steps.append(step)
        counts.append(count(lab))
    return lab, th, d, dict(steps=steps, scores=np.stack(scores), moved=np.asarray(moved), counts=np.stack(counts),
                            candidates=cand, slot_scores=res['score'])
