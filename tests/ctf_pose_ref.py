"""fp64 numpy restatement of the section "CTF in the template" of include/tvae_cluster.h (a plain helper module, used by
test_ctf_pose_ref_cpu.py and test_ctf_pose_gpu.py), built on pose_ref, ctf_ref and ml_ref: the norm of the CTF-filtered template
per (image, slot, angle), the weighted per-class power of the CTF, the round of tvae.ml2d.ml_rounds(ctf=...) on ml_ref.rounds'
parts with the three substituted tables and the Wiener M-step, an fp32 emulation of the two DFT stages and the a-priori bound.

The bound of template_power, per (image, slot, angle), no constant chosen by hand.  u = 2^-24, g_L = (L + 2) u.
  input      the kernel's template is the fp32 one of tvae_pose_refine: per sample within b_i of the fp64 template, b_i the
             bound of test_refine_gpu.py at S = 0 (position error delta_i = 16 u (1 + 2 (1 + t |dx_i|_inf)) (n - 1) / 2 pixels,
             b_i = 2 g_k delta_i + 4 u max |ref_k|, and under a soft mask + max |ref_k| (pi / (2 edge) sqrt(2) delta_i + 2 u)).
             By Parseval the spectrum of a channel moves by |dF_in|_2 = n |dT|_F <= n^2 b_i (full plane).
  stages     in the Frobenius norm, as ctf_ref.filter_bound takes them (the per-coefficient bounds are those of
             spectrum_ref.power_bound): stage 1 (real rows, L = n) |E1(r, kx)| <= g_n sqrt(n) |T_r|_2, so over the half spectrum
             |E1|_F <= g_n sqrt(n R) |T|_F, and stage 2 carries it on with norm sqrt(n); stage 2 (complex, L = 2 n)
             |E2(ky, kx)| <= sqrt(2) g_2n sqrt(n) |G'_kx|_2 for the computed column, so |E2|_F <= sqrt(2) g_2n n (|G|_F + |E1|_F).
             On the full plane (at most sqrt(2) times the half): |dF|_2 <= n^2 b_i + sqrt(2) (sqrt(n) |E1|_F + |E2|_F), and
             sum ||F + dF|^2 - |F|^2| <= d = 2 |F|_2 |dF|_2 + |dF|_2^2 per channel (Cauchy-Schwarz).
  H          |H_gpu - H| <= dH = 8 u (|c0| + |c1|), the contract of tvae_ctf_eval (c4 q >= 0), so
             |H_gpu^2 - H^2| <= 2 |H| dH + dH^2 and H_gpu^2 <= (max |H| + dH)^2.
  sum        n^2 |ppc_gpu - ppc| <= ((max |H| + dH)^2 + max (2 |H| dH + dH^2)) sum_ch d + sum (2 |H| dH + dH^2) |F|^2 over
             the full plane and the channels, plus (C n^2 + 2) 2^-52 of the reference for the fp64 sums and u of it for the
             final rounding to fp32.
A template that is zero throughout in fp64 (out of frame, an invalid slot) gets the bound 0: exact zeros are required."""
import math

import numpy as np

import align_ref
import classify_ref
import ctf_ref
import ml_ref
import pose_ref

F32 = np.float32
EPS = 2.0 ** -24


# ---- the norm of the CTF-filtered template -----------------------------------------------------------------------------------------
def slot_templates(refs, cand, theta, dx, t_scale, A, dtheta, mask_radius=None, mask_edge=0.0):
    """-> T fp64 [N][M][NA][C][n][n]: pose_ref.templates at S = 0 of every slot (zeros for a slot outside [0, K))."""
    cand = np.asarray(cand).astype(np.int64)
    return np.stack([pose_ref.templates(refs, cand[:, m], theta, dx, t_scale, A, dtheta, 0, mask_radius, mask_edge)
                     for m in range(cand.shape[1])], 1)


def h_full(coef, n):
    """coef [N][5] -> H fp64 [N][n][n] on the full plane."""
    return ctf_ref.full_plane(ctf_ref.H(coef, n), n)


def power_of(T, Hf):
    """T [N][..][C][n][n], Hf [N][n][n] -> [N][..]: (1 / n^2) sum_ch sum_k Hf^2 |fft2(T)|^2."""
    n = T.shape[-1]
    F2 = np.abs(np.fft.fft2(T)) ** 2
    H2 = (Hf ** 2).reshape((T.shape[0],) + (1,) * (T.ndim - 3) + (n, n))
    with np.errstate(invalid='ignore', over='ignore'):
        return (F2 * H2).sum(axis=(-3, -2, -1)) / float(n * n)


def template_power(refs, cand, theta, dx, coef, t_scale, A, dtheta, mask_radius=None, mask_edge=0.0):
    """The whole definition of tvae_template_ctf_power in fp64 -> (ppc [N][M][NA], T [N][M][NA][C][n][n])."""
    T = slot_templates(refs, cand, theta, dx, t_scale, A, dtheta, mask_radius, mask_edge)
    return power_of(T, h_full(coef, T.shape[-1])), T


def filtered(x, coef):
    """x [N][C][n][n] -> H_i (*) x_i, fp64."""
    n = np.asarray(x).shape[-1]
    return ctf_ref.filter(x, ctf_ref.H(coef, n)[:, None])


def template_power_f32(T, coef):
    """Stages 1 and 2 in float32 numpy on the fp32 rounding of T, H the fp32 rounding of the fp64 value, the products and
    sums in fp64 as the kernel forms them -> [N][M][NA]."""
    T32 = np.asarray(T).astype(F32)
    n = T32.shape[-1]
    R = n // 2 + 1
    C, S = ctf_ref.twiddle_tables(n, F32)
    Gr, Gi = T32 @ C[:, :R], -(T32 @ S[:, :R])
    Fr, Fi = C @ Gr + S @ Gi, C @ Gi - S @ Gr
    p = Fr.astype(np.float64) ** 2 + Fi.astype(np.float64) ** 2
    h = ctf_ref.H(coef, n).astype(F32).astype(np.float64)
    hw = (h * h * ctf_ref.weights(n)).reshape((T32.shape[0],) + (1,) * (T32.ndim - 3) + (n, R))
    return (p * hw).sum(axis=(-3, -2, -1)) / float(n * n)


def sample_bound(refs, cand, dx, t_scale, mask_radius=None, mask_edge=0.0, S=0):
    """b [N][M]: the per-sample bound of the kernel's template against the fp64 one (module docstring, `input`); S > 0: on the
    grid extended by S pixels, whose half width is 1 + 2 S / (n - 1) coordinate units (test_refine_gpu.py)."""
    refs = np.asarray(refs, dtype=np.float64)
    K, n = refs.shape[0], refs.shape[-1]
    cand = np.asarray(cand).astype(np.int64)
    valid = (cand >= 0) & (cand < K)
    kk = np.where(valid, cand, 0)
    with np.errstate(invalid='ignore', over='ignore'):
        Mg = 1 + 2 * (1 + 2 * S / (n - 1) + np.float64(F32(t_scale)) * np.abs(np.asarray(dx, dtype=np.float64)).max(1))
        delta = (16 * EPS * Mg * (n - 1) / 2)[:, None]
        rmax = np.abs(refs).max(axis=(1, 2, 3))[kk]
        b = 2 * ml_ref.adjacent_step(refs)[kk] * delta + 4 * EPS * rmax
        if mask_radius is not None and float(F32(mask_radius)) > 0:
            b = b + rmax * (np.pi / (2 * float(F32(mask_edge))) * np.sqrt(2) * delta + 2 * EPS)
    return b


def template_power_bound(T, coef, b):
    """The a-priori absolute bound [N][M][NA] on |kernel - template_power| (module docstring); T the fp64 templates, b [N][M]."""
    T = np.asarray(T, dtype=np.float64)
    N, M, NA, C, n, _ = T.shape
    R = n // 2 + 1
    coef = np.asarray(coef, dtype=np.float64).reshape(N, 5)
    Hf = np.abs(h_full(coef, n))[:, None, None, None]                     # [N][1][1][1][n][n]
    dH = (8 * EPS * (np.abs(coef[:, 0]) + np.abs(coef[:, 1])))[:, None, None, None, None, None]
    g1, g2 = (n + 2) * EPS, (2 * n + 2) * EPS
    G = np.fft.fft(T, axis=-1)[..., :R]
    F = np.fft.fft2(T)
    dead = ~np.abs(T).reshape(N, M, NA, -1).any(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        bb = np.where(dead, 0.0, b[:, :, None])[..., None]                                          # [N][M][NA][1]
        nT = np.sqrt((T ** 2).sum((-2, -1)))                                                        # [N][M][NA][C]
        nF = np.sqrt((np.abs(F) ** 2).sum((-2, -1)))
        E1 = g1 * math.sqrt(n * R) * nT
        E2 = math.sqrt(2) * g2 * n * (np.sqrt((np.abs(G) ** 2).sum((-2, -1))) + E1)
        dF = n * n * bb + math.sqrt(2) * (math.sqrt(n) * E1 + E2)
        d = (2 * nF * dF + dF * dF).sum(-1)                                                         # [N][M][NA]
        dH2 = 2 * Hf * dH + dH * dH
        hmax = (Hf.max(axis=(-2, -1), keepdims=True) + dH) ** 2
        ref = power_of(T, h_full(coef, n))
        moved = (hmax + dH2.max(axis=(-2, -1), keepdims=True)).reshape(N, 1, 1) * d
        out = (moved + (dH2 * np.abs(F) ** 2).sum((-3, -2, -1))) / float(n * n)
        out = out + ((C * n * n + 2) * 2.0 ** -52 + EPS) * ref
    return np.where(dead, 0.0, out)


# ---- the weighted per-class power of the CTF ----------------------------------------------------------------------------------------
def power_weighted(coef, img, w, seg, n, N=None):
    """The whole definition of tvae_ctf_power_entries in fp64 -> (D [K][n][R], wsum [K], counts [K]): the live entries
    (ml_ref.live_entries) of the cleaned seg (ml_ref.clean_seg) in ascending e."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    N = coef.shape[0] if N is None else N
    img = np.asarray(img).astype(np.int64)
    E = img.size
    w64 = np.asarray(w, dtype=F32).astype(np.float64)
    live = ml_ref.live_entries(img, w64, N)
    clean = ml_ref.clean_seg(seg, E)
    K = clean.size - 1
    h2 = ctf_ref.H(coef, n) ** 2
    D, wsum, counts = np.zeros((K, n, n // 2 + 1)), np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        e = np.arange(clean[k], clean[k + 1])
        e = e[live[e]]
        counts[k] = e.size
        for q in e:
            D[k] += w64[q] * h2[img[q]]
            wsum[k] += w64[q]
    return D, wsum, counts


def power_weighted_bound(coef, img, w, seg, n, N=None):
    """|kernel - power_weighted| <= 1e-15 D + sum w (2 |H| dH + dH^2): the fp64 sums and the contract of tvae_ctf_eval."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    dH = (8 * EPS * (np.abs(coef[:, 0]) + np.abs(coef[:, 1])))[:, None, None]
    h = np.abs(ctf_ref.H(coef, n))
    slack = 2 * h * dH + dH * dH
    N = coef.shape[0] if N is None else N
    img = np.asarray(img).astype(np.int64)
    w64 = np.asarray(w, dtype=F32).astype(np.float64)
    live = ml_ref.live_entries(img, w64, N)
    clean = ml_ref.clean_seg(seg, img.size)
    D = power_weighted(coef, img, w, seg, n, N)[0]
    out = 1e-15 * D
    for k in range(clean.size - 1):
        e = np.arange(clean[k], clean[k + 1])
        for q in e[live[e]]:
            out[k] += w64[q] * slack[img[q]]
    return out


# ---- the round of ml_rounds(ctf=...) -------------------------------------------------------------------------------------------------
def wiener(mean, D, W, tau):
    """mean [K][C][n][n], D [K][n][R], W [K] -> the filter of mean_k with G_k = 1 / (D_k / W_k + tau) (zeros where W_k = 0)."""
    Wc = np.asarray(W, dtype=np.float64)[:, None, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        G = np.where(Wc > 0, 1.0 / (D / np.where(Wc > 0, Wc, 1.0) + tau), 0.0)
    return ctf_ref.filter(mean, G[:, None]), G


def ctf_tables(Y, Yf, theta, dx, cand, refs, coef, t_scale, A, step, S):
    """The three tables of |Y_i - H_i (*) P_j|^2: num of the filtered stack (classify_ref.classify), pp = template_power
    expanded over the NS^2 shifts, yy of the raw images -> (num, pp [N][M][NA][NS][NS], yy [N], the dict of classify)."""
    NS = 2 * S + 1
    res = classify_ref.classify(Yf, theta, dx, cand, refs, t_scale, A, step, S)
    ppc, _ = template_power(refs, cand, theta, dx, coef, t_scale, A, step)
    pp = np.broadcast_to(ppc[:, :, :, None, None], ppc.shape + (NS, NS)).copy()
    yy = (np.asarray(Y, dtype=np.float64) ** 2).sum(axis=(1, 2, 3))
    return res['num'], pp, yy, res


def rounds(Y, theta, dx, labels, K, coef, t_scale=1.0, rounds=2, angle_range=np.pi / 8, A=8, S=2, keep=8, sigma2=None, tau=0.1,
           emulate=False):
    """ml_ref.rounds under the model Y_i = H_i (*) P_j + noise (all classes are candidates, no mask, no cross halves): the start
    references are ctf_ref.class_averages_ctf ('wiener'), the E-step takes ctf_tables, the M-step is the Wiener form with the
    posterior weights -> the dict of ml_ref.rounds, D (that of the returned averages) and per round `tables` = (num, pp, yy, cand),
    `refs` (what the round scored against) and `posts` (its posterior).  emulate: the float32 restatement (further down)."""
    Y = np.asarray(Y)
    N, C, n, _ = Y.shape
    lab = np.asarray(labels).astype(np.int64)
    th0, d0 = np.asarray(theta, dtype=F32).reshape(-1), np.asarray(dx, dtype=F32)
    step = float(angle_range) / max(A, 1)
    Yf, wien, tabs = filtered(Y, coef), wiener, ctf_tables
    if emulate:
        Yf, wien, t32 = _rounds_f32_parts(np.asarray(Y, dtype=F32), coef, n)
        tabs = lambda Yraw, Yf_, *a: t32(Yraw, *a[:4], *a[5:])           # (the float32 tables need no coef: it is bound)
    order, seg, _ = align_ref.segments(lab, K)
    D0, m0 = ctf_ref.power(coef, order, seg, n)
    ent0 = dict(img=order, theta=th0[order], dx=d0[order], w=np.ones(N, dtype=F32), seg=seg)
    mean0 = weighted_mean_f32(Yf, ent0, K, t_scale) if emulate else \
        align_ref.class_averages(align_ref.align_stack(Yf, th0, d0, t_scale), order, seg)[0]
    refs = wien(mean0, D0, np.maximum(m0, 1).astype(np.float64), tau)[0]                # ctf_ref.class_averages_ctf, 'wiener'
    logprior, s2 = None, None if sigma2 is None else float(F32(sigma2))
    hist = dict(log_likelihood=[], sigma2=[], pi=[], kept=[], gaps=[], tables=[], refs=[], posts=[])
    cur, post, avg, D = lab, None, None, None
    for _ in range(rounds):
        cand = classify_ref.candidate_lists(cur, K)
        num, pp, yy, _ = tabs(Y, Yf, th0, d0, cand, refs, coef, t_scale, A, step, S)
        hist['tables'].append((num, pp, yy, cand))
        hist['refs'].append(refs)
        if s2 is None:
            l0, r0 = ml_ref.log_weights(num, pp, yy, cand, None, K, 1.0)
            rmin = np.where(np.isnan(l0), np.inf, r0).min(1)
            s2 = float(F32(rmin[np.isfinite(rmin)].mean() / (C * n * n)))
        post = ml_ref.posterior(num, pp, yy, cand, logprior, th0, d0, n, K, A, S, keep, t_scale, step, s2)
        hist['posts'].append(post)
        gap = np.inf
        for i in np.flatnonzero(post['live']):
            kept = post['idx'][i][post['idx'][i] >= 0]
            rest = np.setdiff1d(np.flatnonzero(~np.isnan(post['l'][i])), kept)
            if rest.size:
                e = np.exp(post['l'][i] - post['lse'][i])
                gap = min(gap, e[kept].min() - e[rest].max())
        ent = ml_ref.entries_by_class(post['cls'], post['w'].astype(F32), post['theta'], post['dx'], K)
        avg = ml_ref.weighted_averages(Yf, ent['img'], ent['theta'], ent['dx'], ent['w'], ent['seg'], t_scale, 128)
        D, W, _ = power_weighted(coef, ent['img'], ent['w'], ent['seg'], n)
        refs, _ = wien(weighted_mean_f32(Yf, ent, K, t_scale) if emulate else avg['avg'], D, W, tau)
        live = post['live']
        hist['log_likelihood'].append(ml_ref.log_likelihood(post['lse'], live, C, n, s2, A, S))
        hist['sigma2'].append(s2)
        hist['kept'].append(post['kept'][live].mean())
        hist['gaps'].append(gap)
        pi, logprior = ml_ref.update_priors(avg['wsum'])
        hist['pi'].append(pi)
        s2 = float(F32(ml_ref.update_sigma2(post['r2'], live, C, n)))
        cur = np.where(live, cand[np.arange(N), post['resp'].argmax(1)], cur)
    tables, refs_used, posts = hist.pop('tables'), hist.pop('refs'), hist.pop('posts')
    return dict(avg=refs, wsum=avg['wsum'], D=D, labels=cur, theta=post['theta'][:, 0], dx=post['dx'][:, 0], post=post,
                sigma2_next=s2, tables=tables, refs=refs_used, posts=posts, **{k: np.asarray(v) for k, v in hist.items()})


# ---- the planted stack seen through its CTFs ------------------------------------------------------------------------------------------
def defocus_rows(n, count, w=0.07):
    """`count` coefficient rows (c0, c1, c2, c3, c4) of a weak-phase CTF, H = -(sqrt(1 - w^2) sin + w cos)(2 pi t), t = c2 q, with
    the defoci spread so that the first zero of H beyond the one next to the origin runs from about a quarter to about half
    of the Nyquist radius: in the sum over the rows every ring beyond the first of those zeros has members of both signs, which
    is what a plain average cancels.  w is the amplitude contrast, H(0) = -w."""
    q0 = np.linspace(0.25, 0.5, count) ** 2 / 4.0            # q at that zero: (radius / n)^2, Nyquist is 1 / 2
    phase = math.atan2(w, math.sqrt(1 - w * w)) / (2 * math.pi)           # H = -sin(2 pi (t + phase)): zeros at t = -phase - j / 2
    c2 = -(0.5 + phase) / q0
    out = np.zeros((count, 5))
    out[:, 0], out[:, 1], out[:, 2], out[:, 4] = -math.sqrt(1 - w * w), -w, c2, 2.0
    return out


def planted_ctf(noise=0.5, defoci=8, seed=11, **over):
    """pose_ref.planted seen through `defoci` CTFs (image i has row i mod defoci), white noise added -> the dict of planted with
    Y the CTF-filtered noisy stack (fp32), clean = the planted images before the CTF, and coef [N][5]."""
    p = pose_ref.planted(seed=seed, **over)
    N, n = p['N'], p['n']
    coef = defocus_rows(n, defoci)[np.arange(N) % defoci]
    rng = np.random.default_rng(seed + 100)
    clean = p['Y'].astype(np.float64)
    p['clean'] = clean
    p['Y'] = (filtered(clean, coef) + noise * rng.standard_normal(clean.shape)).astype(F32)
    p['coef'] = coef
    return p


LOOP = dict(seed=3, noise=0.3, keep=4, N=64, n=16, K=2, A=2, S=1, tau=0.1, rounds=2)


def loop_case():
    """The loop case of test_ctf_pose_ref_cpu.py and test_ctf_pose_gpu.py: N = 64, n = 16, K = 2 (so M = 2), A = 2, S = 1."""
    return planted_ctf(LOOP['noise'], 8, LOOP['seed'], N=LOOP['N'], n=LOOP['n'], K=LOOP['K'], A=LOOP['A'], S=LOOP['S'])


# ---- the cases of test_ctf_pose_gpu.py (built without the kernel: test_ctf_pose_ref_cpu.py runs them too) ---------------------------
K_CLS, N_IMG = 3, 5
# (n, C, M, A, masked): n = 9 odd, 16, 33 one past a tile, 64, 128 the LDS limit; C 1 and 2; M 1 and 3; A 0 and 2; both masks
GPU_CASES = [(9, 1, 1, 0, False), (9, 2, 3, 2, True), (16, 1, 3, 2, False), (16, 2, 1, 0, True), (33, 1, 3, 2, True),
             (33, 2, 1, 2, False), (64, 1, 3, 0, True), (64, 2, 1, 2, False), (128, 1, 3, 2, False), (128, 1, 1, 0, True)]


def gpu_case(n, C, M, A, masked):
    """Inputs of one geometry and the fp64 reference with its bound.  Smooth references, poses inside the frame, five defoci
    at an amplitude contrast of 0.6 (the bound is relative to max H^2 |T|^2: H must not be small where the references have their
    power, or the bound says little);
    with M = 3 one row holds a duplicate and an invalid slot and another a slot beyond K.  Every second size runs at t = 0.1
    with the translations scaled by 10."""
    rng = np.random.default_rng([n, C, M, A, int(masked)])
    t = 1.0 if n in (9, 33, 128) else 0.1
    dtheta = 0.05
    radius, edge = (0.3 * n, max(2.0, 0.15 * n)) if masked else (0.0, 0.0)
    refs = pose_ref.smooth_refs(n, K_CLS, C, seed=n + C)
    theta = rng.uniform(-np.pi, np.pi, N_IMG).astype(F32)
    dx = (rng.uniform(-0.1, 0.1, (N_IMG, 2)) / t).astype(F32)
    cand = rng.integers(0, K_CLS, (N_IMG, M))
    if M == 3:
        cand[1] = (2, 2, -1)
        cand[3] = (K_CLS + 3, 0, 1)
    coef = defocus_rows(n, N_IMG, 0.6)
    ref, T = template_power(refs, cand, theta, dx, coef, float(F32(t)), A, dtheta, radius if masked else None, edge)
    b = sample_bound(refs, cand, dx, t, radius if masked else None, edge)
    bound = template_power_bound(T, coef, b)
    c = dict(n=n, C=C, M=M, A=A, t=t, dtheta=dtheta, radius=radius, edge=edge, refs=refs, theta=theta, dx=dx, cand=cand, coef=coef,
             ref=ref, T=T, bound=bound)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pp_bound(T, b):
    """|pp_kernel - sum T^2| of tvae_pose_classify's centre shift (test_refine_gpu.py): 2 b sum |T| + m b^2 + gamma sum T^2 with
    m = C n^2 terms and gamma = m u / (1 - m u); T [N][M][NA][C][n][n], b [N][M] -> [N][M][NA]."""
    m = T.shape[-3] * T.shape[-2] * T.shape[-1]
    gamma = m * EPS / (1 - m * EPS)
    dead = ~np.abs(T).reshape(T.shape[:3] + (-1,)).any(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        bb = np.where(dead, 0.0, b[:, :, None])
        return 2 * bb * np.abs(T).sum((-3, -2, -1)) + m * bb * bb + gamma * (T ** 2).sum((-3, -2, -1))


# ---- the float32 restatement of the loop and the tolerance of its GPU test ------------------------------------------------------------
# An a-priori bound carried through two rounds (filter, average, Wiener filter, three tables, posterior, weighted average, Wiener
# filter again) is worst case upon worst case: for the loop case it allows the log-weights to move by more than their spacing and
# decides nothing.  The loop is therefore held to the rule of test_ctf_gpu.py and test_spectrum_gpu.py, tolerance (b): 8 x the
# error of a float32 numpy restatement of the same steps against fp64, rounds(emulate=True) below.  It rounds where the GPU rounds:
# the filter in float32 (ctf_ref.filter_f32), the position arithmetic of the templates and their bilinear samples in float32
# (templates_f32, the operations of refine_position one rounding each), num as a float32 sum, pp by template_power_f32, yy rounded
# once, the entry weights in float32, the weighted sums in float32, G rounded once.  The posterior is fp64 on both sides.
def templates_f32(refs, cls, theta, dx, t_scale, A, dtheta, S):
    """pose_ref.templates without a mask, every operation of the position and of the bilinear sample in float32 -> float32
    [N][NA][C][ne][ne]."""
    refs = np.asarray(refs, dtype=F32)
    K, C, n, _ = refs.shape
    cls = np.asarray(cls).astype(np.int64)
    N, NA, ne = cls.size, 2 * A + 1, n + 2 * S
    th = pose_ref.angles(theta, A, dtheta)                                 # float32 [N][NA]
    d = np.asarray(dx, dtype=F32).reshape(-1, 2)
    t = F32(t_scale)
    step, half = F32(2) / F32(n - 1), F32(0.5) * F32(n - 1)
    g = np.arange(-S, n + S).astype(F32)
    x0 = (g * step - F32(1))[None, None, None, :]
    x1 = (-g * step + F32(1))[None, None, :, None]
    c, s = np.cos(th)[:, :, None, None], np.sin(th)[:, :, None, None]
    v0, v1 = x0 - (t * d[:, 0])[:, None, None, None], x1 - (t * d[:, 1])[:, None, None, None]
    u0, u1 = v0 * c - v1 * s, v0 * s + v1 * c
    col, row = (u0 + F32(1)) * half, (F32(1) - u1) * half                  # float32 [N][NA][ne][ne]
    assert col.dtype == F32 and row.dtype == F32
    ok = (cls >= 0) & (cls < K)
    planes = np.zeros((N, C, n, n), dtype=F32)
    planes[ok] = refs[cls[ok]]
    return bilinear_f32(planes, col, row)


def bilinear_f32(planes, col, row):
    """bilinear_zero_border in float32: planes float32 [N][C][n][n], col, row float32 [N][A][h][w] -> float32 [N][A][C][h][w]."""
    N, C, n, _ = planes.shape
    assert col.dtype == F32 and row.dtype == F32
    inside = (col > -1) & (col < n) & (row > -1) & (row < n)
    colc, rowc = np.where(inside, col, F32(0)), np.where(inside, row, F32(0))
    fc, fr = np.floor(colc), np.floor(rowc)
    c0, r0 = fc.astype(np.int64), fr.astype(np.int64)
    wc, wr = colc - fc, rowc - fr
    out = np.zeros(col.shape[:2] + (C,) + col.shape[2:], dtype=F32)
    pad = np.zeros((N, C, n + 2, n + 2), dtype=F32)                        # a zero border of one pixel: taps -1 and n
    pad[:, :, 1:-1, 1:-1] = planes
    ii = np.arange(N)[:, None, None, None]
    for ch in range(C):
        tap = lambda dr, dc: pad[ii, ch, r0 + 1 + dr, c0 + 1 + dc]
        top = wc * (tap(0, 1) - tap(0, 0)) + tap(0, 0)
        bot = wc * (tap(1, 1) - tap(1, 0)) + tap(1, 0)
        out[:, :, ch] = np.where(inside, wr * (bot - top) + top, F32(0))
    return out


def align_f32(Y, theta, dx, t_scale):
    """align_ref.align_stack with the position arithmetic of align_sample and the bilinear sample in float32 -> float32."""
    Y = np.asarray(Y, dtype=F32)
    n = Y.shape[-1]
    th, d, t = np.asarray(theta, dtype=F32).reshape(-1), np.asarray(dx, dtype=F32).reshape(-1, 2), F32(t_scale)
    step, half = F32(2) / F32(n - 1), F32(0.5) * F32(n - 1)
    g = np.arange(n).astype(F32)
    u0, u1 = (g * step - F32(1))[None, None, :], (-g * step + F32(1))[None, :, None]
    c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    x0 = u0 * c + (u1 * s + (t * d[:, 0])[:, None, None])
    x1 = -u0 * s + (u1 * c + (t * d[:, 1])[:, None, None])
    return bilinear_f32(Y, ((x0 + F32(1)) * half)[:, None], ((F32(1) - x1) * half)[:, None])[:, 0]


def tables_f32(Yf, T, S):
    """pose_ref.tables' num as float32 sums: Yf float32 [N][C][n][n], T float32 [N][NA][C][ne][ne] -> float32 [N][NA][NS][NS]."""
    n, NS = Yf.shape[-1], 2 * S + 1
    num = np.zeros(T.shape[:2] + (NS, NS), dtype=F32)
    for syi in range(NS):
        for sxi in range(NS):
            P = T[:, :, :, 2 * S - syi:2 * S - syi + n, 2 * S - sxi:2 * S - sxi + n]
            num[:, :, syi, sxi] = (P * Yf[:, None]).sum(axis=(2, 3, 4), dtype=F32)
    return num


def _rounds_f32_parts(Y, coef, n):
    """What rounds(emulate=True) puts in the place of the fp64 steps -> (Yf fp64 values of the float32 filter, wiener32, tables32)."""
    H32 = ctf_ref.H(coef, n).astype(F32)
    Yf = np.stack([ctf_ref.filter_f32(Y[:, ch], H32) for ch in range(Y.shape[1])], 1).astype(np.float64)

    def wiener32(mean, D, W, tau):
        _, G = wiener(mean, D, W, tau)
        m32 = np.asarray(mean).astype(F32)
        out = np.stack([ctf_ref.filter_f32(m32[:, ch], G.astype(F32)) for ch in range(m32.shape[1])], 1)
        return out.astype(np.float64), G

    def tables32(Yraw, theta, dx, cand, refs, t, A, step, S):
        NS = 2 * S + 1
        T = np.stack([templates_f32(refs, cand[:, m], theta, dx, t, A, step, S) for m in range(cand.shape[1])], 1)
        num = np.stack([tables_f32(Yf.astype(F32), T[:, m], S) for m in range(cand.shape[1])], 1)
        ppc = template_power_f32(T[..., S:S + n, S:S + n], coef).astype(F32)
        pp = np.broadcast_to(ppc[:, :, :, None, None], ppc.shape + (NS, NS)).copy()
        yy = (np.asarray(Yraw, dtype=np.float64) ** 2).sum(axis=(1, 2, 3)).astype(F32)
        return num.astype(np.float64), pp.astype(np.float64), yy.astype(np.float64), None
    return Yf, wiener32, tables32


def weighted_mean_f32(Yf, ent, K, t_scale):
    """The weighted aligned mean with float32 samples (align_f32), products and sums."""
    al = align_f32(Yf[ent['img']], ent['theta'], ent['dx'], t_scale)
    w = np.asarray(ent['w'], dtype=F32)
    out = np.zeros((K,) + Yf.shape[1:])
    for k in range(K):
        e = np.arange(ent['seg'][k], ent['seg'][k + 1])
        if e.size:
            out[k] = (w[e][:, None, None, None] * al[e]).sum(0, dtype=F32).astype(np.float64) / w[e].astype(np.float64).sum()
    return out


def loop_reference(emulate=False):
    """rounds() of loop_case() with sigma2 given (the planted noise variance), in fp64 or as the float32 restatement."""
    p, L = loop_case(), LOOP
    return p, rounds(p['Y'], p['theta'], p['dx'], p['cls'], p['K'], p['coef'], p['t'], rounds=L['rounds'],
                     angle_range=p['A'] * p['dtheta'], A=p['A'], S=p['S'], keep=L['keep'], sigma2=L['noise'] ** 2, tau=L['tau'],
                     emulate=emulate)


def top_two(l):
    """l [N][J] with NaN for a candidate that is not live -> the two largest live values of every image, [N][2]."""
    return -np.sort(-np.where(np.isnan(l), -np.inf, l), 1)[:, :2]


def loop_tolerance():
    """-> (p, ref, tol): ref the fp64 rounds of the loop case and tol = dict(dl, avg [K], left_out bool [N], cut_clear):
    dl = 8 max |l_f32 - l_fp64| over the live candidates of the last round, avg_k = 8 |avg_f32 - avg_fp64|_F, and the images left
    out of the comparison of labels and poses: those whose runner-up margin in the reference (ml_ref.separation of the two
    largest log-weights) is within 2 dl, or whose two largest slot posteriors are within the factor exp(4 dl) (every log-weight
    may move by dl, so a slot sum by the factor exp(+-dl) against the common maximum, twice for a ratio of two)."""
    p, ref = loop_reference()
    _, emu = loop_reference(True)
    l64, l32 = ref['post']['l'], emu['post']['l']
    assert np.array_equal(np.isnan(l64), np.isnan(l32))
    dl = 8 * float(np.nanmax(np.abs(l32 - l64)))
    avg = 8 * np.sqrt(((emu['avg'] - ref['avg']) ** 2).sum((1, 2, 3)))
    top = top_two(l64)
    sep, _ = ml_ref.separation(top)
    resp = np.sort(ref['post']['resp'], 1)
    with np.errstate(divide='ignore'):
        margin = np.log(resp[:, -1]) - np.log(resp[:, -2])
    left_out = (sep <= 2 * dl / np.abs(top).min(1)) | (margin <= 4 * dl)
    # the kept SET of every image is the reference's while the log-weights at the cut are more than 2 dl apart, in every round
    cut_clear = True
    for post in ref['posts']:
        for i in range(l64.shape[0]):
            kept = post['idx'][i][post['idx'][i] >= 0]
            rest = np.setdiff1d(np.flatnonzero(~np.isnan(post['l'][i])), kept)
            cut_clear &= bool(rest.size == 0 or post['l'][i][kept].min() - post['l'][i][rest].max() > 2 * dl)
    return p, ref, dict(dl=dl, avg=avg, left_out=left_out, cut_clear=cut_clear)
