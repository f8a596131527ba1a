"""Inference-time latent extraction (reference clustering_mnist.py:45-164).

attention/attention(+offsets) branch (:121-161): encoder forward on the HIP kernels, then ONE epilogue kernel (argmax
over (r,h,w), gather, softmax-expected translation) instead of the reference's ~20 ATen launches and per-call host grid
rebuild (the attention/unimodal branch keeps its grid on the device too).  The two secondary branches (:64-119) run their encoders on the HIP kernels too (ops.MlpFn,
ops.TransAttnEncoderFn); their small epilogue is generic torch, the policy of tvae/secondary.py.
`extract_latents` is the dataset-level loop of the clustering scripts, kept on the device."""
from __future__ import annotations

import torch

from . import step, tables
from ._lib import call


def _attention_attention(x, y, enc, out=None):
    B, R, Ho, zd = y.shape[0], enc.groupconv, enc.output_size(), enc.latent_dim
    heads = enc.encode_heads(y)
    tb = enc.head_tables(y.device, step.pixel_spacing(x))
    if out is None:
        zc = torch.empty(B, 2 * zd, dtype=torch.float32, device=y.device)
        th = torch.empty(B, 1, dtype=torch.float32, device=y.device)
        dx = torch.empty(B, 2, dtype=torch.float32, device=y.device)
    else:
        zc, th, dx = out
    call('tvae_get_latent', heads, heads.shape[1], tb.p_r, tb.off, tb.grid, B, R, Ho * Ho, zd, tb.theta_off_scale,
         zc, th, dx)
    return zc, th, dx


def _unimodal_unimodal(y, enc):
    """clustering_mnist.py:64-78: the first latent is the rotation, the next two the translation."""
    z_mu, z_logstd = enc(y.reshape(y.shape[0], -1))
    z_std = torch.exp(z_logstd)
    return torch.cat((z_mu[:, 3:], z_std[:, 3:]), dim=1), z_mu[:, 0:1], z_mu[:, 1:3]


_GRID = {}


def _translation_grid(Ho, spacing, device):
    """Candidate translations (Ho*Ho, 2) on the device, cached per (Ho, spacing, device) as enc.head_tables caches the
    main branch's tables: built and copied once, not per minibatch."""
    key = (int(Ho), float(spacing), str(device))
    G = _GRID.get(key)
    if G is None:
        G = _GRID[key] = torch.from_numpy(tables.translation_grid(Ho, spacing)).to(device).float()
    return G


def _attention_unimodal(x, y, enc):
    """clustering_mnist.py:81-119: z and theta at the most probable translation, dx = E_softmax(attn)[grid]."""
    b = y.shape[0]
    attn, _, theta_vals, z_vals = enc(y, y.device)
    logits = attn.reshape(b, -1)
    ind1 = logits.max(1)[1]
    ind0 = torch.arange(b, device=y.device)
    z_vals = z_vals.reshape(b, z_vals.shape[1], -1)
    theta_vals = theta_vals.reshape(b, theta_vals.shape[1], -1)
    zd = z_vals.shape[1] // 2
    z_mu = z_vals[:, :zd][ind0, :, ind1]
    z_std = torch.exp(z_vals[:, zd:])[ind0, :, ind1]
    dx = torch.softmax(logits, dim=1) @ _translation_grid(attn.shape[3], step.pixel_spacing(x), y.device)
    return torch.cat((z_mu, z_std), dim=1), theta_vals[ind0, 0:1, ind1], dx


def _latent(x, y, enc, t_inf, r_inf, out=None):
    if t_inf == 'attention' and r_inf in ('attention', 'attention+offsets'):
        return _attention_attention(x, y, enc, out)
    if t_inf == 'unimodal' and r_inf == 'unimodal':
        res = _unimodal_unimodal(y, enc)
    elif t_inf == 'attention' and r_inf == 'unimodal':
        res = _attention_unimodal(x, y, enc)
    else:
        raise NotImplementedError(f'--t-inf {t_inf} --r-inf {r_inf} is not a combination the reference supports')
    if out is None:
        return tuple(t.contiguous() for t in res)
    for o, t in zip(out, res):
        o.copy_(t)
    return out


def get_latent(x, y, encoder_model, t_inf, r_inf, device, image_dim=None):
    """Reference signatures clustering_mnist.py:45 (7 arguments) and clustering_{particles,galaxy,dsprites}.py (6, no
    image_dim; it is not used).  Returns (z_content (B, 2z) = [z_mu, z_std], theta_mu (B,1), dx (B,2)); z_std =
    exp(logstd) without the training-time epsilon (reference :137)."""
    with torch.no_grad():
        return _latent(x.to(device), y.to(device), encoder_model, t_inf, r_inf)


def extract_latents(images, encoder_model, x_coord, t_inf, r_inf, minibatch_size=100, device=None):
    """Latents of a whole image stack (N, Cin, n, n): the loop of clustering_mnist.py:315-328 with everything resident on
    the device.  One no-grad loop over minibatches (the last one ragged); every minibatch writes straight into row
    slices of three preallocated device tensors; no host synchronisation inside the loop (the reference copies three
    tensors to the host per minibatch).

    Returns (z_content [N][2z], theta [N][1], dx [N][2]) on the device: bitwise the concatenation of get_latent over the
    slices [i, i + minibatch_size).  minibatch_size is part of the result: the encoder's h3 arithmetic scales its fp16
    operand parts per minibatch tensor, so another split of the same stack may differ in the last bits."""
    dev = torch.device(device) if device is not None else x_coord.device
    images, x = images.to(dev), x_coord.to(dev)
    N = images.shape[0]
    zd = encoder_model.latent_dim - (3 if (t_inf, r_inf) == ('unimodal', 'unimodal') else 0)
    zc = torch.empty(N, 2 * zd, dtype=torch.float32, device=dev)
    th = torch.empty(N, 1, dtype=torch.float32, device=dev)
    dx = torch.empty(N, 2, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for i in range(0, N, minibatch_size):
            j = min(i + minibatch_size, N)
            _latent(x, images[i:j], encoder_model, t_inf, r_inf, out=(zc[i:j], th[i:j], dx[i:j]))
    return zc, th, dx
