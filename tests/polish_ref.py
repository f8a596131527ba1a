"""fp64 numpy restatement of the sub-pixel pose polish of include/tvae_cluster.h (a plain helper module, used by
test_polish_cpu.py and test_polish_gpu.py), built on pose_ref and align_ref: the basis functions P, Dtheta, G0, G1 of
tvae_pose_moments, their 15 sums, and tvae_pose_polish_step operation for operation.

What the definition fixes in fp32 is taken in fp32 here as well: theta and dx as the fp32 values the kernel gets, c and s of the
step as fp32 values, the trial pose rounded to fp32 once per component.  The positions of the samples are pose_ref's (fp64 on
those values).  The step is written with Python floats: IEEE doubles, every operation rounded on its own, never fused."""
import math

import numpy as np

import pose_ref

F32 = np.float32
NAMES = ('PP', 'PD', 'PG0', 'PG1', 'DD', 'DG0', 'DG1', 'G0G0', 'G0G1', 'G1G1', 'PY', 'DY', 'G0Y', 'G1Y', 'YY')
IDX = {k: i for i, k in enumerate(NAMES)}
LAMBDA0 = 1e-3


def positions(n, theta, dx, t_scale):
    """theta [N] fp32, dx [N][2] fp32 -> dict(u0, u1, col, row, d, inside) [N][n][n] fp64: the template positions of
    pose_ref.template_positions at S = 0 together with the canonical coordinates they come from."""
    th = np.asarray(theta, dtype=F32).reshape(-1).astype(np.float64)
    dx = np.asarray(dx, dtype=F32).reshape(-1, 2).astype(np.float64)
    t = float(F32(t_scale))
    g = np.arange(n, dtype=np.float64)
    x0 = (2 * g / (n - 1) - 1)[None, None, :]
    x1 = (1 - 2 * g / (n - 1))[None, :, None]
    with np.errstate(invalid='ignore', over='ignore'):
        c, s = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
        v0 = x0 - t * dx[:, 0, None, None]
        v1 = x1 - t * dx[:, 1, None, None]
        u0 = v0 * c - v1 * s
        u1 = v0 * s + v1 * c
        col, row = (u0 + 1) * (n - 1) / 2, (1 - u1) * (n - 1) / 2
        d = np.sqrt(u0 * u0 + u1 * u1) * (n - 1) / 2
        inside = (col > -1) & (col < n) & (row > -1) & (row < n)
    return dict(u0=u0, u1=u1, col=col, row=row, d=d, inside=inside)


def basis(refs, cls, theta, dx, t_scale, mask_radius=None, mask_edge=0.0):
    """-> dict(P, D, G0, G1 [N][C][n][n] fp64 (zeros for a skipped image and out of frame), valid [N], pos): the basis functions
    of tvae_pose_moments, the derivatives those of the bilinear cell that produced the sample, the mask held constant."""
    refs = np.asarray(refs, dtype=np.float64)
    K, C, n, _ = refs.shape
    cls = np.asarray(cls).astype(np.int64).reshape(-1)
    N = cls.size
    valid = (cls >= 0) & (cls < K)
    pos = positions(n, theta, dx, t_scale)
    inside = pos['inside'] & valid[:, None, None]
    col, row = np.where(inside, pos['col'], 0.0), np.where(inside, pos['row'], 0.0)
    c0, r0 = np.floor(col).astype(np.int64), np.floor(row).astype(np.int64)
    wc, wr = (col - c0)[:, None], (row - r0)[:, None]
    pad = np.zeros((N, C, n + 2, n + 2))                                  # the zero border, taps -1 .. n
    pad[valid, :, 1:-1, 1:-1] = refs[cls[valid]]
    ii = np.arange(N)[:, None, None]

    def tap(r, c):
        return np.moveaxis(pad[ii, :, r + 1, c + 1], -1, 1)

    a00, a01, a10, a11 = tap(r0, c0), tap(r0, c0 + 1), tap(r0 + 1, c0), tap(r0 + 1, c0 + 1)
    top = (1 - wc) * a00 + wc * a01                                        # (the operations of align_ref.sample: P is
    bot = (1 - wc) * a10 + wc * a11                                        # pose_ref's template to the last bit)
    B = (1 - wr) * top + wr * bot
    Bc = (1 - wr) * (a01 - a00) + wr * (a11 - a10)
    Br = bot - top
    m = np.where(inside, pose_ref.mask_at(np.where(inside, pos['d'], 0.0), mask_radius, mask_edge), 0.0)[:, None]
    h = (n - 1) / 2
    on = inside[:, None]
    u0, u1 = np.where(inside, pos['u0'], 0.0)[:, None], np.where(inside, pos['u1'], 0.0)[:, None]
    P = np.where(on, m * B, 0.0)
    G0 = np.where(on, m * h * Bc, 0.0)
    G1 = np.where(on, -m * h * Br, 0.0)
    D = -u1 * G0 + u0 * G1
    return dict(P=P, D=D, G0=G0, G1=G1, valid=valid, pos=pos, c0=c0, r0=r0, inside=inside)


def moments(Y, b):
    """Y [N][C][n][n], b = basis(...) -> mom [N][15] fp64 in the order NAMES; 15 zeros for a skipped image."""
    Y = np.asarray(Y, dtype=np.float64)
    f = dict(P=b['P'], D=b['D'], G0=b['G0'], G1=b['G1'], Y=Y)
    pairs = (('P', 'P'), ('P', 'D'), ('P', 'G0'), ('P', 'G1'), ('D', 'D'), ('D', 'G0'), ('D', 'G1'), ('G0', 'G0'), ('G0', 'G1'),
             ('G1', 'G1'), ('P', 'Y'), ('D', 'Y'), ('G0', 'Y'), ('G1', 'Y'), ('Y', 'Y'))
    mom = np.stack([(f[a] * f[c]).sum(axis=(1, 2, 3)) for a, c in pairs], 1)
    return np.where(b['valid'][:, None], mom, 0.0)


def translation_basis(b, theta):
    """(Dtx, Dty) = (-c G0 - s G1, s G0 - c G1): the derivatives of P along t dx0 and t dx1 (fp64 c and s of the fp32 angle)."""
    th = np.asarray(theta, dtype=F32).reshape(-1).astype(np.float64)
    with np.errstate(invalid='ignore'):
        c, s = np.cos(th)[:, None, None, None], np.sin(th)[:, None, None, None]
    return -c * b['G0'] - s * b['G1'], s * b['G0'] - c * b['G1']


def score(m):
    """The score of one row of moments (any float type) -> a Python float: fp64, exactly 0 where PP or YY is 0."""
    pp, py, yy = float(m[IDX['PP']]), float(m[IDX['PY']]), float(m[IDX['YY']])
    if pp == 0.0 or yy == 0.0:
        return 0.0
    prod = pp * yy
    if not prod >= 0.0:                                                  # NaN (or a negative sum: never from the kernel)
        return math.nan
    return _div(py, math.sqrt(prod))


def _div(a, b):
    """IEEE division of Python floats, where Python raises instead."""
    return float(np.float64(a) / np.float64(b)) if b == 0.0 or not math.isfinite(a) or not math.isfinite(b) else a / b


def _cos_sin_f32(th):
    """c and s as the step takes them: the fp32 cosine and sine of the fp32 angle (correctly rounded here), as doubles."""
    x = float(F32(th))
    if not math.isfinite(x):
        return math.nan, math.nan
    return float(F32(math.cos(x))), float(F32(math.sin(x)))


def solve(m, th, lam):
    """The normal equations of the header from one row of moments -> (dtheta, dtx, dty) or None for "no step"."""
    g = lambda k: float(m[IDX[k]])
    pp, py = g('PP'), g('PY')
    if pp == 0.0 or g('YY') == 0.0:
        return None
    c, s = _cos_sin_f32(th)
    al = _div(py, pp)
    pd, pg0, pg1, dd, dg0, dg1 = g('PD'), g('PG0'), g('PG1'), g('DD'), g('DG0'), g('DG1')
    g00, g01, g11, dy, g0y, g1y = g('G0G0'), g('G0G1'), g('G1G1'), g('DY'), g('G0Y'), g('G1Y')
    px, pyy = -(c * pg0) - s * pg1, s * pg0 - c * pg1
    dxm, dym = -(c * dg0) - s * dg1, s * dg0 - c * dg1
    cc, ss, cs = c * c, s * s, c * s
    xx = (cc * g00 + (2.0 * cs) * g01) + ss * g11
    xy = ((cc - ss) * g01 - cs * g00) + cs * g11
    yyv = (ss * g00 - (2.0 * cs) * g01) + cc * g11
    xyv, yyy = -(c * g0y) - s * g1y, s * g0y - c * g1y
    a2 = al * al
    A = [[a2 * dd, a2 * dxm, a2 * dym, al * pd],
         [a2 * dxm, a2 * xx, a2 * xy, al * px],
         [a2 * dym, a2 * xy, a2 * yyv, al * pyy],
         [al * pd, al * px, al * pyy, pp]]
    b = [al * (dy - al * pd), al * (xyv - al * px), al * (yyy - al * pyy), py - al * pp]
    for i in range(4):
        A[i][i] = A[i][i] + lam * A[i][i]
    for k in range(4):
        piv, big = k, abs(A[k][k])
        for r in range(k + 1, 4):
            if abs(A[r][k]) > big:
                big, piv = abs(A[r][k]), r
        if piv != k:
            A[k], A[piv] = A[piv], A[k]
            b[k], b[piv] = b[piv], b[k]
        pv = A[k][k]
        if pv == 0.0 or not math.isfinite(pv):
            return None
        for r in range(k + 1, 4):
            f = _div(A[r][k], pv)
            for j in range(k + 1, 4):
                A[r][j] = A[r][j] - f * A[k][j]
            b[r] = b[r] - f * b[k]
    x = [0.0] * 4
    for i in range(3, -1, -1):
        a = b[i]
        for j in range(i + 1, 4):
            a = a - A[i][j] * x[j]
        x[i] = _div(a, A[i][i])
    if not all(math.isfinite(v) for v in x[:3]):
        return None
    return x[0], x[1], x[2]


def radii(n, t_scale, max_shift, max_angle):
    """The trust region's radius per component (theta, dx0, dx1), as the header forms it."""
    t = float(F32(t_scale))
    rd = ((float(F32(max_shift)) * 2.0) / float(n - 1)) / t
    return float(F32(max_angle)), rd, rd


def trial(m, cur, start, lam, n, t_scale, max_shift, max_angle):
    """cur, start = (theta, dx0, dx1) fp32 -> (the trial as three fp32 scalars, the clamped fp64 values before rounding or None)."""
    sol = solve(m, cur[0], lam)
    if sol is None:
        return tuple(F32(v) for v in cur), None
    t = float(F32(t_scale))
    want = (float(cur[0]) + sol[0], float(cur[1]) + _div(sol[1], t), float(cur[2]) + _div(sol[2], t))
    out, exact = [], []
    for w, cen, rad in zip(want, start, radii(n, t_scale, max_shift, max_angle)):
        c = float(cen)
        lo, hi = c - rad, c + rad
        w = lo if w < lo else w
        w = hi if w > hi else w
        with np.errstate(over='ignore'):
            f = F32(w)
        if abs(float(f) - c) > rad:
            f = np.nextafter(f, F32(cen))
        out.append(f)
        exact.append(w)
    if not all(np.isfinite(v) for v in out):
        return tuple(F32(v) for v in cur), None
    return tuple(out), tuple(exact)


def same_bits(a, b):
    return all(F32(x).view(np.int32) == F32(y).view(np.int32) for x, y in zip(a, b))


def new_state(N):
    return dict(theta=np.zeros(N, F32), dx=np.zeros((N, 2), F32), mom=np.zeros((N, 15)), score=np.zeros((N, 2), F32),
                lam=np.zeros(N), steps=np.zeros(N, np.int32), ended=np.zeros(N, np.int32), theta_try=np.zeros(N, F32),
                dx_try=np.zeros((N, 2), F32), exact=[None] * N)


def step(st, mom_try, cls, K, theta0, dx0, n, t_scale, max_shift, max_angle, first):
    """tvae_pose_polish_step on the state dict `st` (changed in place; st['mom'] takes the dtype of mom_try's values as
    doubles).  st['exact'][i]: the clamped fp64 trial before its rounding, None where there was no step."""
    theta0 = np.asarray(theta0, dtype=F32).reshape(-1)
    dx0 = np.asarray(dx0, dtype=F32).reshape(-1, 2)
    cls = np.asarray(cls).astype(np.int64).reshape(-1)
    mom_try = np.asarray(mom_try)
    for i in range(cls.size):
        start = (theta0[i], dx0[i, 0], dx0[i, 1])
        if first:
            sd = score(mom_try[i])
            live = 0 <= cls[i] < K and math.isfinite(sd)
            st['theta'][i], st['dx'][i] = theta0[i], dx0[i]
            st['mom'][i] = mom_try[i]
            st['score'][i] = F32(sd) if live else F32(0)
            st['lam'][i], st['steps'][i], st['exact'][i] = LAMBDA0, 0, None
            if not live:
                st['theta_try'][i], st['dx_try'][i], st['ended'][i] = theta0[i], dx0[i], 1
                continue
        else:
            if st['ended'][i]:
                continue
            sd = score(mom_try[i])
            if math.isfinite(sd) and sd > score(st['mom'][i]):
                st['theta'][i], st['dx'][i] = st['theta_try'][i], st['dx_try'][i]
                st['mom'][i] = mom_try[i]
                st['score'][i, 1] = F32(sd)
                st['lam'][i] = st['lam'][i] / 4.0
                st['steps'][i] += 1
            else:
                st['lam'][i] = st['lam'][i] * 8.0
        cur = (st['theta'][i], st['dx'][i, 0], st['dx'][i, 1])
        tr, exact = trial(st['mom'][i], cur, start, float(st['lam'][i]), n, t_scale, max_shift, max_angle)
        st['theta_try'][i], st['dx_try'][i, 0], st['dx_try'][i, 1] = tr
        st['exact'][i] = exact
        st['ended'][i] = 1 if same_bits(tr, cur) else 0
    return st


def polish(Y, theta, dx, cls, refs, t_scale=1.0, iterations=8, max_shift=1.0, max_angle=0.05, mask_radius=None, mask_edge=0.0):
    """The whole loop in fp64: moments(start) -> step -> [moments(trial) -> step] x iterations.
    -> dict(theta, dx, score [N][2], steps)."""
    refs = np.asarray(refs)
    K, n = refs.shape[0], refs.shape[-1]
    theta0 = np.array(np.asarray(theta, dtype=F32).reshape(-1))
    dx0 = np.array(np.asarray(dx, dtype=F32).reshape(-1, 2))
    st = new_state(theta0.size)
    ev = lambda th, d: moments(Y, basis(refs, cls, th, d, t_scale, mask_radius, mask_edge))
    step(st, ev(theta0, dx0), cls, K, theta0, dx0, n, t_scale, max_shift, max_angle, True)
    for _ in range(int(iterations)):
        step(st, ev(st['theta_try'], st['dx_try']), cls, K, theta0, dx0, n, t_scale, max_shift, max_angle, False)
    return dict(theta=st['theta'].copy(), dx=st['dx'].copy(), score=st['score'].copy(), steps=st['steps'].copy())
