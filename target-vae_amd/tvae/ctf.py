"""CTF correction on the GPU: the contrast transfer function of every particle from five fp64 coefficients, the per-image
Fourier filter of a stack (multiply by H, or by its sign: phase flipping), the reference's real-space filter bank, and
CTF-corrected (phase-flipped or Wiener-weighted) aligned class averages.

Training models a particle as y = h_i * y_mu with a per-image CTF kernel h_i, so the particles of one class, which sit
at different defoci, partly cancel in a plain average beyond the first CTF zero.  `class_averages_ctf` undoes that:
  flip     every particle is multiplied by sign(H_i) in Fourier space before it is aligned and averaged;
  wiener   avg_k = IDFT( (1 / m_k) sum_i H_i X_i  /  ((1 / m_k) sum_i H_i^2 + tau) ), tau = 1 / SNR.
H is isotropic (astigmatism is ignored, as the reference ignores it), so the filter commutes with the in-plane rotation
of the alignment and may be applied before it (up to the bilinear resampling).

include/tvae_cluster.h (last section) states the definitions; the kernels are tvae_ctf_eval, tvae_fourier_filter and
tvae_ctf_power of libtvae_cluster.so.  No FFT library: a direct DFT on the fp32 matrix pipe for any n, odd and prime
sizes included, bitwise reproducible and independent of the batch.  There is no CPU fallback; `coefficients` is host
arithmetic in fp64.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _cluster_lib as CL
from ._lib import TvaeHipError

COLUMNS = ('defocus', 'cs', 'voltage', 'apix', 'bfactor', 'ampcont', 'dfdiff', 'dfang')
MODES = {'multiply': 0, 'flip': 1, 0: 0, 1: 1}
WS_FLOATS = 1 << 26               # bound of the workspace of one tvae_fourier_filter call: 256 MB
MAX_PLANES = CL.MAX_PLANES


def _column(params, name):
    if isinstance(params, np.ndarray):
        if params.ndim != 2 or params.shape[1] != len(COLUMNS):
            raise ValueError(f'coefficients: an array must be [N][8] ({" ".join(COLUMNS)}), got {params.shape}')
        return np.asarray(params[:, COLUMNS.index(name)], dtype=np.float64)
    return np.asarray(params[name], dtype=np.float64).reshape(-1)


def coefficients(params, scale=1, sign=-1):
    """The reference's eight-column table (a DataFrame of src.ctf.parse_ctf, a mapping of columns or an [N][8] array) ->
    coef fp64 [N][5] = (c0, c1, c2, c3, c4) with H = (c0 sin 2 pi t + c1 cos 2 pi t) exp(-c4 q), t = c2 q + c3 q^2 and
    q = |k|^2 / n^2: exactly src.ctf.compute_2d_ctf as src.ctf.ctf_filter calls it, times `sign`.  sign = -1 is the model's
    convention (the filter the reference trains with is -fftshift(Re ifft2(c))).  dfdiff and dfang are ignored."""
    if sign not in (-1, 1):
        raise ValueError(f'coefficients: sign must be -1 or 1, got {sign!r}')
    df = _column(params, 'defocus') * 10000.0
    volt = _column(params, 'voltage') * 1000.0
    cs = _column(params, 'cs') * 10 ** 7
    lam = 12.2639 / np.sqrt(volt + 0.97845e-6 * volt ** 2)
    w = _column(params, 'ampcont') / 100
    a = _column(params, 'apix') * scale
    out = np.empty((df.shape[0], 5), dtype=np.float64)
    out[:, 0] = sign * np.sqrt(1 - w ** 2)
    out[:, 1] = -sign * w
    out[:, 2] = -0.5 * df * lam / a ** 2
    out[:, 3] = 0.25 * cs * lam ** 3 / a ** 4
    out[:, 4] = _column(params, 'bfactor') / (4 * a ** 2)
    return out


def _mode(mode):
    try:
        return MODES[mode]
    except (KeyError, TypeError):
        raise TvaeHipError(f"mode must be 'multiply' (0) or 'flip' (1), got {mode!r}") from None


def _coef_tensor(coef, device, what):
    t = torch.as_tensor(np.asarray(coef, dtype=np.float64) if not torch.is_tensor(coef) else coef)
    if t.dim() != 2 or t.shape[1] != 5 or t.shape[0] < 1:
        raise TvaeHipError(f'{what}: coef must be [N][5], got {tuple(t.shape)}')
    return t.to(device=device, dtype=torch.float64).contiguous()


def _device(device):
    if not torch.cuda.is_available():
        raise TvaeHipError('tvae.ctf needs a GPU (no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def transfer(coef, n, mode='multiply', device=None):
    """coef [N][5] -> H fp32 [N][n][n // 2 + 1] on the GPU: the transfer function (or, mode 'flip', its sign) at the
    frequencies of numpy's rfft2 layout."""
    dev = _device(device)
    c = _coef_tensor(coef, dev, 'transfer')
    N, n = c.shape[0], int(n)
    if not (2 <= n <= CL.MAX_SIDE and N <= MAX_PLANES):
        raise TvaeHipError(f'transfer: N={N}, n={n} outside the supported range (N <= 2^24, 2 <= n <= 1024)')
    H = torch.empty(N, n, n // 2 + 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        CL.call('tvae_ctf_eval', c, H, N, n, _mode(mode))
    return H


def _filter(x, x_stride, coef, planes, h_stride, out, n, mode, chunk=None):
    """tvae_fourier_filter over the B planes of `out` in slices that bound the workspace (a plane's result does not depend
    on the slice it is in)."""
    B = out.numel() // (n * n)
    per = CL.query('tvae_fourier_filter_ws_floats', 1, n)
    if per <= 0 or B < 1:
        raise TvaeHipError(f'fourier filter: n={n} with {B} planes outside the supported range (2 <= n <= 1024)')
    step = CL.slice_step(B, MAX_PLANES, WS_FLOATS // per if chunk is None else chunk)
    wsf = CL.query('tvae_fourier_filter_ws_floats', step, n)
    ws = CL.workspace(wsf, out.device)
    xf, of = x.reshape(-1), out.reshape(-1)
    with torch.cuda.device(out.device):
        for b0 in range(0, B, step):
            b1 = min(b0 + step, B)
            xs = xf[b0 * x_stride:b1 * x_stride] if x_stride else xf
            cs = coef[b0:b1] if coef is not None else None
            hs = None
            if planes is not None:
                hs = planes.reshape(-1)[b0 * h_stride:b1 * h_stride] if h_stride else planes.reshape(-1)
            CL.call('tvae_fourier_filter', xs, x_stride, cs, hs, h_stride, of[b0 * n * n:b1 * n * n], ws, wsf, b1 - b0, n,
                    mode)
    return out


def filter_stack(images, coef=None, planes=None, mode='multiply', inplace=False, chunk=None):
    """images [N][n][n] or [N][C][n][n] (contiguous CUDA fp32) -> Re IDFT(H_i DFT(image_i)), same shape.  Exactly one of
    coef ([N][5] fp64, host or device: H is formed in registers, never stored) and planes ([N][n][R] or one shared [n][R],
    CUDA fp32, R = n // 2 + 1).  The channels of an image share its row.  mode 'flip' multiplies by sign(H) instead.
    inplace overwrites `images`.  chunk: planes per launch (default: what keeps the workspace within 256 MB)."""
    CL.require_f32(images, 'filter_stack', 'images')
    if images.dim() not in (3, 4) or images.shape[-1] != images.shape[-2]:
        raise TvaeHipError(f'filter_stack: images must be [N][n][n] or [N][C][n][n] (square), got {tuple(images.shape)}')
    if (coef is None) == (planes is None):
        raise TvaeHipError('filter_stack: exactly one of coef and planes')
    N, n = images.shape[0], images.shape[-1]
    C = images.shape[1] if images.dim() == 4 else 1
    R = n // 2 + 1
    m = _mode(mode)
    c = p = None
    h_stride = 0
    if coef is not None:
        c = _coef_tensor(coef, images.device, 'filter_stack')
        if c.shape[0] != N:
            raise TvaeHipError(f'filter_stack: coef must hold N = {N} rows, got {c.shape[0]}')
        if C > 1:
            c = c.repeat_interleave(C, 0).contiguous()
    else:
        p = planes
        if not (CL.is_f32(p) and p.device == images.device):
            raise TvaeHipError('filter_stack: planes must be a contiguous CUDA fp32 tensor on the device of images')
        if tuple(p.shape) == (N, n, R):
            h_stride = n * R
            if C > 1:
                p = p.repeat_interleave(C, 0).contiguous()
        elif tuple(p.shape) != (n, R):
            raise TvaeHipError(f'filter_stack: planes must be [{N}][{n}][{R}] or [{n}][{R}], got {tuple(p.shape)}')
    out = images if inplace else torch.empty_like(images)
    return _filter(images, n * n, c, p, h_stride, out, n, m, chunk)


def filter_bank(params, n, scale=1, device=None, chunk=None):
    """src.ctf.ctf_filter(params, n, n, scale) on the device: fp32 [N][n][n], the real-space kernels the model convolves
    with, -fftshift(Re ifft2(c)) for odd and even n -- the filter (sign = -1) of ONE shared plane, a delta at
    (n // 2, n // 2)."""
    dev = _device(device)
    n = int(n)
    rows = coefficients(params, scale, -1)
    if rows.shape[0] == 0:
        return torch.zeros(0, n, n, dtype=torch.float32, device=dev)
    c = _coef_tensor(rows, dev, 'filter_bank')
    delta = torch.zeros(n, n, dtype=torch.float32, device=dev)
    delta[n // 2, n // 2] = 1.0
    out = torch.empty(c.shape[0], n, n, dtype=torch.float32, device=dev)
    return _filter(delta, 0, c, None, 0, out, n, 0, chunk)


def power(coef, labels, n, n_clusters=None, device=None):
    """-> (D fp64 [K][n][R], counts int32 [K]): D[k] = sum of H_i^2 over the images with label k (tvae_ctf_power)."""
    from . import align
    dev = _device(device)
    c = _coef_tensor(coef, dev, 'power')
    N, n = c.shape[0], int(n)
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.numel() != N:
        raise TvaeHipError(f'power: labels must hold N = {N} entries, got {tuple(lab.shape)}')
    lab = lab.to(dev)
    K = int(n_clusters) if n_clusters is not None else int(lab.max()) + 1
    if not (1 <= K <= CL.MAX_CLASSES and 2 <= n <= CL.MAX_SIDE and N <= MAX_PLANES):
        raise TvaeHipError(f'power: N={N}, K={K}, n={n} outside the supported range')
    order, seg, _ = align.segments(lab, K)
    D = torch.empty(K, n, n // 2 + 1, dtype=torch.float64, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        CL.call('tvae_ctf_power', c, order, seg, D, counts, N, K, n)
    return D, counts


def template_power(theta, dx, slots, refs, coef, t_scale=1.0, angle_steps=8, angle_step=None, mask_radius=None, mask_edge=0.0):
    """|H_i (*) T|^2 of every (image, slot, angle): theta [N] or [N][1], dx [N][2], refs [K][C][n][n] (CUDA fp32), slots [N][M]
    integers (a value outside [0, K) gives zeros), coef [N][5] -> ppc fp32 [N][M][NA], NA = 2 angle_steps + 1.  T is the template
    of tvae.classify.classify_poses of the slot's reference at the angle theta + a angle_step, a = -A .. A, H_i the transfer
    function of coef[i] (tvae_template_ctf_power).  The shift of a candidate does not enter: it is a phase factor."""
    from . import classify, refine
    what = 'template_power'
    CL.require_f32(refs, what, 'refs')
    CL.require_f32(theta, what, 'theta')
    CL.require_f32(dx, what, 'dx')
    if refs.dim() != 4 or refs.shape[-1] != refs.shape[-2]:
        raise TvaeHipError(f'{what}: refs must be [K][C][n][n] (square), got {tuple(refs.shape)}')
    K, C, n, _ = refs.shape
    dev = refs.device
    N = theta.numel()
    if tuple(dx.shape) != (N, 2) or theta.device != dev or dx.device != dev:
        raise TvaeHipError(f'{what}: theta must hold N = {N} angles and dx must be [N][2], on the device of refs')
    cand, M = classify._as_table(slots, N, dev, what)
    c = _coef_tensor(coef, dev, what)
    if c.shape[0] != N:
        raise TvaeHipError(f'{what}: coef must hold N = {N} rows, got {c.shape[0]}')
    A = int(angle_steps)
    step, t = refine.angle_step_of(A, angle_step), float(t_scale)
    radius, edge = 0.0 if mask_radius is None else float(mask_radius), float(mask_edge)
    if not (np.isfinite(t) and t > 0 and np.isfinite(step)):
        raise TvaeHipError(f'{what}: t_scale = {t_scale} must be finite and positive and angle_step = {angle_step} finite')
    if not (np.isfinite(radius) and np.isfinite(edge) and edge >= 0):
        raise TvaeHipError(f'{what}: mask_radius = {mask_radius} and mask_edge = {mask_edge} must be finite, the edge not negative')
    if not (1 <= K <= CL.MAX_CLASSES and CL.query('tvae_template_ctf_power_ws_floats', 1, C, n, M, A) > 0):
        raise TvaeHipError(f'{what}: K={K}, C={C}, n={n}, M={M}, angle_steps={A} outside the supported range (2 <= n <= '
                           f'{refine.MAX_SIDE}, C <= {refine.MAX_CHANNELS}, M <= {classify.MAX_CANDIDATES}, 0 <= angle_steps <= '
                           f'{refine.MAX_ANGLE_STEPS})')
    NA = 2 * A + 1
    th = theta.reshape(N)
    ppc = torch.empty(N, M, NA, dtype=torch.float32, device=dev)
    stepN = CL.slice_step(N, MAX_PLANES, (2 ** 31 - 1) // (M * NA))       # one workgroup per (image, slot, angle)
    wsf = CL.query('tvae_template_ctf_power_ws_floats', stepN, C, n, M, A)
    ws = CL.workspace(wsf, dev)
    with torch.cuda.device(dev):
        for i0 in range(0, N, stepN):
            i1 = min(i0 + stepN, N)
            sl = slice(i0, i1)
            CL.call('tvae_template_ctf_power', th[sl], dx[sl], cand[sl], refs, c[sl], ppc[sl], ws, wsf, i1 - i0, C, n, K, M, A,
                    t, step, radius, edge)
    return ppc


def select_poses(num, pp, yy, candidates, theta, dx, n, n_clusters, t_scale=1.0, angle_steps=8, angle_step=None, shift=2):
    """The hard selection from the three tables of a pose search (tvae_pose_select): num [N][M][NA][NS][NS], yy [N], and pp
    either [N][M][NA] -- tvae.ctf.template_power, the template power per angle -- or [N][M][NA][NS][NS] (CUDA fp32), with the
    candidates [N][M] the tables were made for, the poses theta [N] or [N][1] and dx [N][2] the grid is centred on and the side n
    of the images -> the tuple of tvae.classify.classify_poses: (labels' int64 [N], theta' [N], dx' [N][2], scores [N][M][2],
    best int32 [N][4]).  angle_steps, angle_step and shift as they were given to the search that wrote num."""
    from . import classify, refine
    what = 'select_poses'
    for nm, t in (('num', num), ('pp', pp), ('yy', yy), ('theta', theta), ('dx', dx)):
        CL.require_f32(t, what, nm)
    N = yy.numel()
    dev = yy.device
    cand, M = classify._as_table(candidates, N, dev, what)
    A, S, K, n = int(angle_steps), int(shift), int(n_clusters), int(n)
    NA, NS = 2 * A + 1, 2 * S + 1
    if yy.dim() != 1 or tuple(num.shape) != (N, M, NA, NS, NS):
        raise TvaeHipError(f'{what}: yy must be [N] and num [N][M][NA][NS][NS] = {(N, M, NA, NS, NS)}, got {tuple(yy.shape)} and '
                           f'{tuple(num.shape)}')
    if tuple(pp.shape) not in ((N, M, NA), (N, M, NA, NS, NS)):
        raise TvaeHipError(f'{what}: pp must be [N][M][NA] = {(N, M, NA)} or [N][M][NA][NS][NS], got {tuple(pp.shape)}')
    if theta.numel() != N or theta.dim() > 2 or tuple(dx.shape) != (N, 2):
        raise TvaeHipError(f'{what}: theta must hold N = {N} angles and dx must be [N][2]')
    if any(t.device != dev for t in (num, pp, theta, dx)):
        raise TvaeHipError(f'{what}: num, pp, yy, theta and dx must live on one device')
    if not (1 <= K <= CL.MAX_CLASSES and 2 <= n <= refine.MAX_SIDE and 0 <= A <= refine.MAX_ANGLE_STEPS
            and 0 <= S <= refine.MAX_SHIFT and 1 <= N <= MAX_PLANES and num.numel() < 2 ** 40):
        raise TvaeHipError(f'{what}: N={N}, n={n}, K={K}, angle_steps={A}, shift={S} outside the supported range')
    step, t = refine.angle_step_of(A, angle_step), float(t_scale)
    if not (np.isfinite(t) and t > 0 and np.isfinite(step)):
        raise TvaeHipError(f'{what}: t_scale = {t_scale} must be finite and positive and angle_step = {angle_step} finite')
    cls_out = torch.empty(N, dtype=torch.int32, device=dev)
    best = torch.empty(N, 4, dtype=torch.int32, device=dev)
    th_out = torch.empty(N, dtype=torch.float32, device=dev)
    dx_out = torch.empty(N, 2, dtype=torch.float32, device=dev)
    score = torch.empty(N, M, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        CL.call('tvae_pose_select', theta.reshape(N), dx, cand, num, pp, yy, cls_out, best, th_out, dx_out, score, N, n, K, M, A, S,
                int(pp.dim() == 5), t, step)
    return cls_out.to(torch.int64), th_out, dx_out, score, best


def search_record(what, images, ctf, wiener_tau):
    """What the rounds of a hard search form once from the coef rows `ctf` [N][5]: -> (coef fp64 on the device, tau, the stack
    filtered with H_i, (coef, yy of the raw images)), the last the `ctf` record of refine_poses and classify_poses."""
    from . import ml2d
    coef, tau = _coef_tensor(ctf, images.device, what), float(wiener_tau)
    if coef.shape[0] != images.shape[0]:
        raise TvaeHipError(f'{what}: ctf must hold N = {images.shape[0]} rows, got {coef.shape[0]}')
    if not tau > 0:
        raise TvaeHipError(f'{what}: wiener_tau = {wiener_tau} must be positive')
    return coef, tau, filter_stack(images, coef=coef, mode='multiply'), (coef, ml2d.raw_sum_squares(images))


def search_poses(what, tables_of, theta, dx, slots, refs, ctf, n, t_scale, A, step, S, mask_radius, mask_edge, tables=False):
    """The hard pose search under Y_i = H_i (*) P_j + noise, slice by slice so that the tables never exceed the workspace bound
    of tvae.refine (tvae.ml2d._slices): num = tables_of(slice) [N'][M][NA][NS][NS], the num table of the plain search on the
    stack filtered with H_i already; template_power; select_poses with the power per angle.  ctf = (coef [N][5], yy fp32 [N] of
    the RAW images), theta [N], slots [N][M] on the device.
    -> (labels' int64 [N], theta' [N], dx' [N][2], scores [N][M][2], best int32 [N][4]) and with tables=True also
    (num, ppc [N][M][NA], yy)."""
    from . import ml2d
    N, M, K = theta.numel(), slots.shape[1], refs.shape[0]
    if not (isinstance(ctf, (tuple, list)) and len(ctf) == 2):
        raise TvaeHipError(f'{what}: ctf must be (coef [N][5], yy [N] of the raw images)')
    coef = _coef_tensor(ctf[0], refs.device, what)
    yy_raw = ctf[1]
    CL.require_f32(yy_raw, what, 'ctf[1]')
    if coef.shape[0] != N or tuple(yy_raw.shape) != (N,) or yy_raw.device != refs.device:
        raise TvaeHipError(f'{what}: ctf must hold N = {N} rows of coefficients and N sums of squares on the device of the images')
    stepN = ml2d._slices(N, M, A, S)
    parts = []
    for i0 in range(0, N, stepN):
        sl = slice(i0, min(i0 + stepN, N))
        num = tables_of(sl)
        ppc = template_power(theta[sl], dx[sl], slots[sl], refs, coef[sl], t_scale, A, step, mask_radius, mask_edge)
        yy = yy_raw[sl].contiguous()
        out = select_poses(num, ppc, yy, slots[sl], theta[sl], dx[sl], n, K, t_scale, A, step, S)
        parts.append(out + (num, ppc, yy) if tables else out)
        del num, ppc, yy
    return tuple(torch.cat([p[j] for p in parts]) for j in range(len(parts[0])))


def power_weighted(coef, entries, n, n_clusters):
    """coef [N][5], entries as tvae.ml2d.entries_by_class returns them (img, w, seg on one CUDA device) -> (D fp64 [K][n][R],
    wsum fp64 [K], counts int32 [K]): D[k] = sum w_e H_img[e]^2 over the live entries of class k (tvae_ctf_power_entries), the
    denominator of the Wiener M-step beside tvae.ml2d.weighted_class_averages of the filtered stack."""
    what = 'power_weighted'
    img, w, seg = (entries[k] for k in ('img', 'w', 'seg'))
    K, n = int(n_clusters), int(n)
    if not (torch.is_tensor(img) and img.is_cuda):
        raise TvaeHipError(f'{what}: entries must be CUDA tensors (no CPU fallback)')
    dev = img.device
    E = img.numel()
    for nm, t, dt, shape in (('img', img, torch.int32, (E,)), ('w', w, torch.float32, (E,)), ('seg', seg, torch.int32, (K + 1,))):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
            raise TvaeHipError(f'{what}: entries[{nm!r}] must be a contiguous {dt} tensor of shape {shape} on one device')
    c = _coef_tensor(coef, dev, what)
    N = c.shape[0]
    if not (1 <= K <= CL.MAX_CLASSES and 2 <= n <= CL.MAX_SIDE and N <= MAX_PLANES and E <= 1 << 30):
        raise TvaeHipError(f'{what}: N={N}, E={E}, K={K}, n={n} outside the supported range')
    D = torch.zeros(K, n, n // 2 + 1, dtype=torch.float64, device=dev)
    wsum = torch.zeros(K, dtype=torch.float64, device=dev)
    counts = torch.zeros(K, dtype=torch.int32, device=dev)
    if E == 0:                                                # nothing to add: every class is empty
        return D, wsum, counts
    with torch.cuda.device(dev):
        CL.call('tvae_ctf_power_entries', c, img, w, seg, D, wsum, counts, N, E, K, n)
    return D, wsum, counts


def class_averages_ctf(images, theta, dx, labels, coef, n_clusters=None, t_scale=1.0, correct='wiener', tau=0.1):
    """CTF-corrected aligned class averages -> (avg fp32 [K][C][n][n], counts int32 [K], D fp64 [K][n][R]).
    images [N][C][n][n], theta, dx, labels, n_clusters, t_scale as tvae.align.class_averages; coef [N][5].
      'flip'    align.class_averages of the phase-flipped stack;
      'wiener'  x' = H_i x_i;  N_k = the aligned mean of x' over the m_k members;  G_k = 1 / (D_k / max(m_k, 1) + tau) formed in
                fp64 and rounded once;  avg_k = the filter of N_k with the plane G_k.  tau is 1 / SNR.
    An empty class gives zeros.  D[k] = sum of H_i^2 over the class (both corrections return it)."""
    from . import align
    if correct not in ('wiener', 'flip'):
        raise TvaeHipError(f"class_averages_ctf: correct must be 'wiener' or 'flip', got {correct!r}")
    N, C, n, K, lab = align._check_labels(images, theta, dx, labels, n_clusters, 'class_averages_ctf')
    c = _coef_tensor(coef, images.device, 'class_averages_ctf')
    if c.shape[0] != N:
        raise TvaeHipError(f'class_averages_ctf: coef must hold N = {N} rows, got {c.shape[0]}')
    if not float(tau) > 0:
        raise TvaeHipError(f'class_averages_ctf: tau = {tau} must be positive')
    D, m = power(c, lab, n, K, images.device)
    if correct == 'flip':
        avg, counts = align.class_averages(filter_stack(images, coef=c, mode='flip'), theta, dx, lab, K, t_scale)
        return avg, counts, D
    mean, counts = align.class_averages(filter_stack(images, coef=c, mode='multiply'), theta, dx, lab, K, t_scale)
    G = (1.0 / (D / m.clamp(min=1).to(torch.float64)[:, None, None] + float(tau))).to(torch.float32).contiguous()
    return filter_stack(mean, planes=G), counts, D
