"""fp64 numpy restatement of the maximum-likelihood class averages of include/tvae_cluster.h (a plain helper module, used by
test_ml2d_cpu.py and test_ml2d_gpu.py), built on align_ref and pose_ref: the posterior over the candidates of the tables
num / pp / yy, the entries it keeps, the weighted aligned average over a list of entries with its error bound, the updates
of a round and rounds(), the loop of tvae.ml2d.ml_rounds on classify_ref.classify and align_ref.

What the definition fixes in fp32 is taken in fp32 here as well: sigma2 as the fp32 value the kernel gets, the poses of the
kept candidates (pose_ref.update_pose) and the weights an entry carries into the average.  Everything else is fp64."""
import functools

import numpy as np

import align_ref
import classify_ref
import pose_ref

F32 = np.float32
EPS = 2.0 ** -24


# ---- the posterior ---------------------------------------------------------------------------------------------------------------
def log_weights(num, pp, yy, cand, logprior, K, sigma2):
    """-> (l, r) fp64 [N][J], J = M NA NS^2: l = logprior - r / (2 sigma2) with NaN for a candidate that is not live, and
    r = (yy - 2 num) + pp, each operation rounded on its own."""
    num, pp = np.asarray(num, dtype=np.float64), np.asarray(pp, dtype=np.float64)
    N, M = num.shape[:2]
    cand = np.asarray(cand).astype(np.int64).reshape(N, M)
    yy = np.asarray(yy, dtype=np.float64).reshape(N, 1, 1, 1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        r = (yy - 2.0 * num) + pp
        valid = (cand >= 0) & (cand < K)
        lp = np.zeros(K) if logprior is None else np.asarray(logprior, dtype=np.float64)
        slot = np.where(valid, lp[np.where(valid, cand, 0)], np.nan)
        h = 0.5 / float(F32(sigma2))
        l = slot[:, :, None, None, None] - r * h
    l = np.where(np.isfinite(l), l, np.nan)
    return l.reshape(N, -1), r.reshape(N, -1)


def posterior(num, pp, yy, cand, logprior, theta, dx, n, K, A, S, P, t_scale, dtheta, sigma2):
    """The whole definition of tvae_pose_posterior -> dict(l, r [N][J], idx, cls int64 [N][P], theta fp32 [N][P], dx fp32
    [N][P][2], w fp64 [N][P] (= w_j / W), wj fp64 [N][P] (= w_j), resp fp64 [N][M], lse, r2, kept fp64 [N], live bool [N])."""
    l, r = log_weights(num, pp, yy, cand, logprior, K, sigma2)
    N, J = l.shape
    cand = np.asarray(cand).astype(np.int64).reshape(N, -1)
    M = cand.shape[1]
    NS = 2 * S + 1
    cnd = (2 * A + 1) * NS * NS
    theta = np.asarray(theta, dtype=F32).reshape(-1)
    dx = np.asarray(dx, dtype=F32).reshape(-1, 2)
    out = dict(l=l, r=r, idx=np.full((N, P), -1, dtype=np.int64), cls=np.full((N, P), -1, dtype=np.int64),
               theta=np.repeat(theta[:, None], P, 1).copy(), dx=np.repeat(dx[:, None, :], P, 1).copy(), w=np.zeros((N, P)),
               wj=np.zeros((N, P)), resp=np.zeros((N, M)), lse=np.zeros(N), r2=np.zeros(N), kept=np.zeros(N),
               live=np.zeros(N, dtype=bool))
    for i in range(N):
        live = np.flatnonzero(~np.isnan(l[i]))
        if live.size == 0:
            continue
        out['live'][i] = True
        L = l[i, live].max()
        e = np.zeros(J)
        e[live] = np.exp(l[i, live] - L)
        Z = e.sum()
        w = e / Z
        out['lse'][i] = L + np.log(Z)
        out['r2'][i] = (w[live] * r[i, live]).sum()
        out['resp'][i] = w.reshape(M, cnd).sum(1)
        rank = live[np.lexsort((live, -l[i, live]))][:P]      # l descending, then j ascending
        W = w[rank].sum()
        q = rank.size
        m, c = rank // cnd, rank % cnd
        best = np.stack([c // (NS * NS) - A, (c // NS) % NS - S, c % NS - S], 1)
        th, d = pose_ref.update_pose(np.repeat(theta[i], q), np.repeat(dx[i][None], q, 0), best, n, t_scale, dtheta)
        out['idx'][i, :q], out['cls'][i, :q] = rank, cand[i, m]
        out['theta'][i, :q], out['dx'][i, :q] = th, d
        out['wj'][i, :q], out['w'][i, :q], out['kept'][i] = w[rank], w[rank] / W, W
    return out


def separation(l):
    """The least |l_a - l_b| / max(|l_a|, |l_b|) over the pairs of distinct live values of every image (inf where an image has
    fewer than two), and whether any two live values of an image are equal -> (fp64 [N], bool [N])."""
    l = np.asarray(l)
    sep, tie = np.full(l.shape[0], np.inf), np.zeros(l.shape[0], dtype=bool)
    for i in range(l.shape[0]):
        v = np.sort(l[i][~np.isnan(l[i])])
        if v.size < 2:
            continue
        d = np.diff(v)
        tie[i] = bool((d == 0).any())
        rel = d[d > 0] / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))[d > 0]
        if rel.size:
            sep[i] = rel.min()
    return sep, tie


# ---- entries and the weighted average ------------------------------------------------------------------------------------------------
def entries_by_class(ent_cls, ent_w, ent_theta, ent_dx, K):
    """tvae.ml2d.entries_by_class one entry at a time -> dict(img, theta, dx, w, seg)."""
    ent_cls = np.asarray(ent_cls)
    N, P = ent_cls.shape
    rows = [[] for _ in range(K)]
    for i in range(N):
        for p in range(P):
            k = int(ent_cls[i, p])
            if 0 <= k < K:
                rows[k].append((i, p))
    flat = [ip for row in rows for ip in row]
    ii = np.array([i for i, _ in flat], dtype=np.int64)
    pp_ = np.array([p for _, p in flat], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum([len(row) for row in rows])]).astype(np.int64)
    return dict(img=ii, theta=np.asarray(ent_theta)[ii, pp_], dx=np.asarray(ent_dx)[ii, pp_].reshape(-1, 2),
                w=np.asarray(ent_w)[ii, pp_], seg=seg)


def clean_seg(seg, E):
    """min(max(0, seg[0], ..., seg[k]), E)"""
    return np.minimum(np.maximum.accumulate(np.maximum(np.asarray(seg, dtype=np.int64), 0)), E)


def live_entries(img, w, N):
    img, w = np.asarray(img).astype(np.int64), np.asarray(w, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return (img >= 0) & (img < N) & np.isfinite(w) & (w > 0)


def adjacent_step(Y):
    """g_i of test_align_gpu.py: the largest difference between adjacent pixels of the zero-bordered image i (every channel)."""
    P = np.pad(np.asarray(Y, dtype=np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    return np.maximum(np.abs(np.diff(P, axis=3)).max(axis=(1, 2, 3)), np.abs(np.diff(P, axis=2)).max(axis=(1, 2, 3)))


def image_bounds(Y, dx, t):
    """The per-image bound of test_align_gpu.py (image_bounds), restated: the fp32 position is about a dozen roundings from the
    exact one, each relative to a quantity of at most 2 + t |dx|_inf coordinate units,
        delta = 16 2^-24 (2 + t |dx|_inf) (n - 1) / 2 pixels,      |A - ref| <= 2 g delta + 4 2^-24 max |y|.
    Y [E][C][n][n] the image of every entry, dx [E][2] the entry's own translation.  A pose that is not finite gives NaN here:
    the caller puts 0 where the definition requires exact zeros."""
    n = Y.shape[-1]
    with np.errstate(invalid='ignore', over='ignore'):
        delta = 16 * EPS * (2 + np.float64(F32(t)) * np.abs(np.asarray(dx, dtype=np.float64)).max(1)) * (n - 1) / 2
        return 2 * adjacent_step(Y) * delta + 4 * EPS * np.abs(Y).max(axis=(1, 2, 3))


def weighted_averages(Y, img, theta_e, dx_e, w, seg, t_scale, chunk):
    """The whole definition of tvae_class_average_weighted in fp64 -> dict(avg [K][C][n][n], wsum [K], counts [K], bound
    [K][C][n][n], aligned [E][C][n][n] (zeros for a dead entry), live [E], b [E])."""
    Y = np.asarray(Y)
    N, C, n, _ = Y.shape
    img = np.asarray(img).astype(np.int64)
    E = img.size
    w64 = np.asarray(w, dtype=F32).astype(np.float64)
    live = live_entries(img, w64, N)
    seg = clean_seg(seg, E)
    K = seg.size - 1
    th, d = np.asarray(theta_e, dtype=F32), np.asarray(dx_e, dtype=F32).reshape(-1, 2)
    aligned, b = np.zeros((E, C, n, n)), np.zeros(E)
    ok = np.flatnonzero(live)
    if ok.size:
        aligned[ok] = align_ref.align_stack(Y[img[ok]], th[ok], d[ok], float(F32(t_scale)))
        bb = image_bounds(Y[img[ok]], d[ok], t_scale)
        with np.errstate(invalid='ignore'):
            hostile = ~np.isfinite(th[ok]) | ~np.isfinite(d[ok]).all(1) | (np.abs(np.float64(F32(t_scale)) * d[ok]).max(1) > 4)
        assert not aligned[ok][hostile].any()                 # wholly out of frame: exact zeros are required
        b[ok] = np.where(hostile, 0.0, bb)
        assert np.isfinite(b).all()
    out = dict(avg=np.zeros((K, C, n, n)), wsum=np.zeros(K), counts=np.zeros(K, dtype=np.int64), bound=np.zeros((K, C, n, n)),
               aligned=aligned, live=live, b=b, seg=seg)
    for k in range(K):
        e = np.arange(seg[k], seg[k + 1])
        e = e[live[e]]
        out['counts'][k] = e.size
        W = w64[e].sum()
        out['wsum'][k] = W
        if W > 0:
            ww = w64[e][:, None, None, None]
            out['avg'][k] = (ww * aligned[e]).sum(0) / W
            Ek = int(seg[k + 1] - seg[k])
            out['bound'][k] = (w64[e] * b[e]).sum() / W + (min(Ek, chunk) + 2) * EPS * (ww * np.abs(aligned[e])).sum(0) / W
    return out


# ---- the updates of a round ----------------------------------------------------------------------------------------------------------
def update_sigma2(r2, live, C, n):
    r2, live = np.asarray(r2, dtype=np.float64), np.asarray(live, dtype=bool)
    return r2[live].sum() / (live.sum() * C * n * n)


def update_priors(wsum):
    w = np.asarray(wsum, dtype=np.float64)
    pi = w / w.sum()
    with np.errstate(divide='ignore'):
        return pi, np.where(pi > 0, np.log(np.where(pi > 0, pi, 1.0)), -np.inf)


def log_likelihood(lse, live, C, n, sigma2, A, S):
    lse, live = np.asarray(lse, dtype=np.float64), np.asarray(live, dtype=bool)
    nl = int(live.sum())
    return lse[live].sum() - nl * (C * n * n / 2.0) * np.log(2 * np.pi * sigma2) - nl * np.log((2 * A + 1) * (2 * S + 1) ** 2)


def rounds(Y, theta, dx, labels, K, t_scale=1.0, rounds=2, angle_range=np.pi / 8, A=8, S=2, keep=8, sigma2=None):
    """The loop of tvae.ml2d.ml_rounds in fp64 (all classes are candidates, no mask, no cross halves) -> dict(avg, wsum,
    labels, theta, dx, log_likelihood, sigma2 [rounds], pi [rounds][K], kept [rounds], post: the last round's posterior,
    gaps [rounds]: the least difference in weight w_j between a kept candidate and the best one not kept)."""
    Y = np.asarray(Y)
    N, C, n, _ = Y.shape
    lab = np.asarray(labels).astype(np.int64)
    th0, d0 = np.asarray(theta, dtype=F32).reshape(-1), np.asarray(dx, dtype=F32)
    step = float(angle_range) / max(A, 1)
    refs = classify_ref.averages(Y, th0, d0, lab, K, t_scale)
    logprior, s2 = None, None if sigma2 is None else float(F32(sigma2))
    hist = dict(log_likelihood=[], sigma2=[], pi=[], kept=[], gaps=[])
    cur, post, res = lab, None, None
    for _ in range(rounds):
        cand = classify_ref.candidate_lists(cur, K)
        res = classify_ref.classify(Y, th0, d0, cand, refs, t_scale, A, step, S)
        if s2 is None:
            l0, r0 = log_weights(res['num'], res['pp'], res['yy'], cand, None, K, 1.0)
            rmin = np.where(np.isnan(l0), np.inf, r0).min(1)
            s2 = float(F32(rmin[np.isfinite(rmin)].mean() / (C * n * n)))
        post = posterior(res['num'], res['pp'], res['yy'], cand, logprior, th0, d0, n, K, A, S, keep, t_scale, step, s2)
        gap = np.inf
        for i in np.flatnonzero(post['live']):
            kept = post['idx'][i][post['idx'][i] >= 0]
            rest = np.setdiff1d(np.flatnonzero(~np.isnan(post['l'][i])), kept)
            if rest.size:
                e = np.exp(post['l'][i] - post['lse'][i])
                gap = min(gap, e[kept].min() - e[rest].max())
        ent = entries_by_class(post['cls'], post['w'].astype(F32), post['theta'], post['dx'], K)
        avg = weighted_averages(Y, ent['img'], ent['theta'], ent['dx'], ent['w'], ent['seg'], t_scale, 128)
        refs = avg['avg']
        live = post['live']
        hist['log_likelihood'].append(log_likelihood(post['lse'], live, C, n, s2, A, S))
        hist['sigma2'].append(s2)
        hist['kept'].append(post['kept'][live].mean())
        hist['gaps'].append(gap)
        pi, logprior = update_priors(avg['wsum'])
        hist['pi'].append(pi)
        s2 = float(F32(update_sigma2(post['r2'], live, C, n)))
        cur = np.where(live, cand[np.arange(N), post['resp'].argmax(1)], cur)
    return dict(avg=refs, wsum=avg['wsum'], labels=cur, theta=post['theta'][:, 0], dx=post['dx'][:, 0], post=post,
                sigma2_next=s2, **{k: np.asarray(v) for k, v in hist.items()})


# ---- the start of the GPU test of the loop -----------------------------------------------------------------------------------------
def loop_case():
    """The start of the GPU test of the loop: pose_ref.planted at its smallest size (tests/test_classify_cpu.py: N = 24, K = 4,
    n = 17, A = 2, S = 3) with white noise added, LOOP['keep'] entries per image, two rounds."""
    p = pose_ref.planted(seed=LOOP['seed'], N=24, K=4, n=17, A=2, S=3)
    rng = np.random.default_rng(LOOP['seed'] + 100)
    p['Y'] = (p['Y'] + LOOP['noise'] * rng.standard_normal(p['Y'].shape)).astype(F32)
    return p


# Chosen by running the reference alone over seeds 1 .. 40, noise 0.3 .. 1 and keep 8, 4, 2.  With 24 images the hard averages
# the loop starts from carry a sixth of each member's own noise, so the posteriors are peaked: at keep = 8 the cut falls among
# weights far below 1e-6 for every seed, and two such weights are within 1e-6 of each other by being small.  At keep = 2 the
# second and third weights differ by 1.5e-2 at least in both rounds of this seed, and the two kept entries carry 84 % and 90 %
# of the posterior mass, so the truncation is not idle either.
LOOP = dict(seed=30, noise=1.0, keep=2)


@functools.lru_cache(maxsize=None)
def loop_reference():
    p = loop_case()
    return p, rounds(p['Y'], p['theta'], p['dx'], p['cls'], p['K'], p['t'], rounds=2, angle_range=p['A'] * p['dtheta'],
                     A=p['A'], S=p['S'], keep=LOOP['keep'])
