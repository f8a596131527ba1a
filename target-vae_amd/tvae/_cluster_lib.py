"""ctypes binding of libtvae_cluster.so (C ABI declared in include/tvae_cluster.h): the batched k-means, Ward
linkage, t-SNE, alignment, pose-refinement, reassignment, pose-polish, class-statistics, eigenimage and maximum-likelihood kernels.

A library of its own beside libtvae_hip.so -- the ABI of the training kernels (tvae._lib.SIGNATURES, version 7) is not
touched by the clustering half.  Same rules: no CPU fallback, tensors are checked by tvae._lib._ptr (GPU, contiguous,
fp32 / int32) and every launch goes through tvae._lib.dispatch, so it consults tvae._lib.CALL_HOOK as tvae._lib.call does.
"""
from __future__ import annotations

import functools
import os

import torch

from . import _lib
from ._lib import TvaeHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TVAE_CLUSTER_LIB') or os.path.join(os.path.dirname(_HERE), 'csrc', 'build', 'libtvae_cluster.so')
ABI_VERSION = 1

# p = device pointer, i = int, l = long, f = float; the trailing stream argument is appended automatically
SIGNATURES = {
    'tvae_kmeans_assign': 'plppppppliiii',    # Xt, ldx, C, done, labels, mind2, changed, ws, ws_floats, N, d, k, R
    'tvae_kmeans_update': 'plppppiiii',       # ws, ws_floats, done, C, inertia, shift, N, d, k, R
    'tvae_kmeans_mindist': 'plppiii',         # Xt, ldx, cnew, D, N, d, R
    'tvae_ward_nn': 'plpppplii',              # Ct, ldc, cnt, nn, nd, ws, ws_floats, M, d
    # C_in (fp64), ld_in, cnt_in, id_in, hmax_in (fp64), nn, C_out (fp64), Ct_out, ld_out, cnt_out, id_out,
    # hmax_out (fp64), rec_ids, rec_hs (fp64), m_out, ws, ws_ints, M, d, N, base, cap
    'tvae_ward_merge': 'plpppp' 'pplppp' 'pppp' 'l' 'iiiii',
    'tvae_knn': 'plppiii',                    # Xt, ldx, idx, d2, N, d, K
    'tvae_tsne_repulsion': 'plpppli',         # Yt, ldy, rep, Z (fp64), ws, ws_floats, N
    # rowptr, col, val, nnz, Yt, rep, Z (fp64), gains, update, Yt_out, grad (or None), gnorm2 (fp64), ldy, N,
    # exaggeration, momentum, learning_rate
    'tvae_tsne_step': 'ppplpppppppplifff',
    'tvae_tsne_kl': 'ppplplpppli',            # rowptr, col, val, nnz, Yt, ldy, Z, kl, ws (fp64 all three), ws_doubles, N
    'tvae_align_stack': 'ppppiiif',           # Y, theta, dx, out, N, C, n, t_scale
    # Y, theta, dx, order (int32), seg (int32), avg, ws, ws_floats, N, C, n, K, t_scale
    'tvae_class_average': 'pppppppliiiif',
    # Y, theta, dx, order (int32), seg (int32), avg, half, var, counts (int32), ws, ws_floats, N, C, n, K, t_scale
    'tvae_class_halves': 'pppppppppp' 'l' 'iiiif',
    'tvae_class_frc': 'pppppliiff',           # a, b, frc, sums (fp64), ws, ws_floats, P, n, mask_radius, mask_edge
    # X, Ar, Ai (or None), Br, Bi (or None), out, B, H, W, r0, c0, M, N, m, n, scale
    'tvae_image_resample': 'pppppp' 'iiiiiiiii' 'f',
    'tvae_image_normalize': 'ppppliiif',      # X, out, stats (fp64), ws, ws_floats, B, n, m, radius
    'tvae_ctf_eval': 'ppiii',                 # coef (fp64), H, N, n, mode
    # X, x_stride, coef (fp64, or None), Hp (or None), h_stride, out, ws, ws_floats, B, n, mode
    'tvae_fourier_filter': 'plpplppliii',
    'tvae_ctf_power': 'pppppiii',             # coef (fp64), order, seg, D (fp64), counts (int32), N, K, n
    # X, x_stride, power (fp64), ws, ws_floats, B, n, mask_radius, mask_edge, background, demean
    'tvae_ring_power': 'plppliiffii',
    'tvae_ring_power_groups': 'pppppiii',     # power (fp64), order, seg, sums (fp64), counts (int32), N, K, Rr
    # X, x_stride, prof, group (int32, or None), out, ws, ws_floats, B, n, G, interp
    'tvae_radial_filter': 'plpppp' 'l' 'iiii',
    # Y, theta, dx, cls (int32), ref, theta_out, dx_out, score, best (int32), num, pp, yy (or None all three), ws, ws_floats,
    # N, C, n, K, A, S, t_scale, dtheta, mask_radius, mask_edge
    'tvae_pose_refine': 'ppppp' 'pppp' 'ppp' 'p' 'l' 'iiiiii' 'ffff',
    # Y, theta, dx, cand (int32), ref, cls_out (int32), best (int32), theta_out, dx_out, score, num, pp, yy (or None all three),
    # ws, ws_floats, N, C, n, K, M, A, S, t_scale, dtheta, mask_radius, mask_edge
    'tvae_pose_classify': 'ppppp' 'ppppp' 'ppp' 'p' 'l' 'iiiiiii' 'ffff',
    # Y, theta, dx, cls (int32), ref, mom, N, C, n, K, t_scale, mask_radius, mask_edge
    'tvae_pose_moments': 'pppppp' 'iiii' 'fff',
    # cls (int32), theta0, dx0, mom_try, theta_try, dx_try, theta_out, dx_out, mom_cur, score, lambda (fp64), steps, ended (int32
    # both), N, n, K, first, t_scale, max_shift, max_angle
    'tvae_pose_polish_step': 'pppp' 'pp' 'ppppppp' 'iiii' 'fff',
    # Y, theta, dx, order (int32), seg (int32), mean, V, coef, norm2 (or None), ws, ws_floats, N, C, n, K, J, t_scale,
    # mask_radius, mask_edge
    'tvae_class_project': 'ppppp' 'pp' 'pp' 'p' 'l' 'iiiii' 'fff',
    # Y, theta, dx, order (int32), seg (int32), mean, coef, W, counts (int32), ws, ws_floats, N, C, n, K, J, t_scale,
    # mask_radius, mask_edge
    'tvae_class_backproject': 'ppppp' 'pp' 'pp' 'p' 'l' 'iiiii' 'fff',
    # num, pp, yy, cand (int32), logprior (fp64, or None), theta, dx, ent_idx, ent_cls (int32 both), ent_theta, ent_dx, ent_w, resp,
    # lse, r2 (fp64 both), kept, N, n, K, M, A, S, P, t_scale, dtheta, sigma2
    'tvae_pose_posterior': 'ppppp' 'pp' 'ppppp' 'pppp' 'iiiiiii' 'fff',
    # Y, img (int32), theta_e, dx_e, w, seg (int32), avg, wsum (fp64), counts (int32), ws, ws_floats, N, E, C, n, K, t_scale
    'tvae_class_average_weighted': 'pppppp' 'pppp' 'l' 'iiiii' 'f',
    # theta, dx, cand (int32), ref, coef (fp64), ppc, ws, ws_floats, N, C, n, K, M, A, t_scale, dtheta, mask_radius, mask_edge
    'tvae_template_ctf_power': 'ppppp' 'pp' 'l' 'iiiiii' 'ffff',
    # coef (fp64), img (int32), w, seg (int32), D, wsum (fp64 both), counts (int32), N, E, K, n
    'tvae_ctf_power_entries': 'pppp' 'ppp' 'iiii',
    # theta, dx, cand (int32), num, pp, yy, cls_out, best (int32 both), theta_out, dx_out, score, N, n, K, M, A, S, pp_per_shift,
    # t_scale, dtheta
    'tvae_pose_select': 'pppppp' 'ppppp' 'iiiiiii' 'ff',
}
# pure host queries: name -> (argument codes, return code)
QUERIES = {
    'tvae_kmeans_ws_floats': ('iiii', 'l'),
    'tvae_kmeans_groups': ('iii', 'i'),
    'tvae_ward_nn_ws_floats': ('ii', 'l'),
    'tvae_ward_nn_splits': ('ii', 'i'),
    'tvae_ward_merge_ws_ints': ('ii', 'l'),
    'tvae_tsne_groups': ('i', 'i'),
    'tvae_tsne_repulsion_ws_floats': ('i', 'l'),
    'tvae_class_average_ws_floats': ('iiii', 'l'),
    'tvae_class_average_chunk': ('iiii', 'i'),
    'tvae_class_halves_ws_floats': ('iiii', 'l'),
    'tvae_frc_rings': ('i', 'i'),
    'tvae_class_frc_ws_floats': ('ii', 'l'),
    'tvae_image_normalize_ws_floats': ('iii', 'l'),
    'tvae_fourier_filter_ws_floats': ('ii', 'l'),
    'tvae_radial_rings': ('i', 'i'),
    'tvae_ring_power_ws_floats': ('ii', 'l'),
    'tvae_radial_filter_ws_floats': ('ii', 'l'),
    'tvae_pose_refine_ws_floats': ('iiiii', 'l'),
    'tvae_pose_classify_ws_floats': ('iiiiii', 'l'),
    'tvae_class_project_ws_floats': ('iiiii', 'l'),
    'tvae_class_backproject_ws_floats': ('iiiii', 'l'),
    'tvae_class_eigen_chunk': ('iiiii', 'i'),
    'tvae_class_average_weighted_ws_floats': ('iiii', 'l'),
    'tvae_class_average_weighted_chunk': ('iiii', 'i'),
    'tvae_template_ctf_power_ws_floats': ('iiiii', 'l'),
}

# the shape limits every image family shares (SIDE_MAX, PLANES_MAX, CLASSES_MAX of csrc/cluster_common.hpp)
MAX_SIDE = 1024
MAX_PLANES = 1 << 24
MAX_CLASSES = 65535


def is_f32(t, contiguous=True) -> bool:
    """A CUDA fp32 tensor, contiguous unless the caller lays it out itself."""
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and (t.is_contiguous() or not contiguous)


def require_f32(t, what, name):
    """`what` (the public function) and `name` (its argument) are the caller's words: tests and CLIs match on the message."""
    if not is_f32(t):
        raise TvaeHipError(f'{what}: {name} must be a contiguous CUDA fp32 tensor (no CPU fallback)')


def workspace(floats, device):
    """At least `floats` fp32 words that start on an 8-byte boundary: the kernels keep fp64 values in them."""
    return torch.empty((int(floats) + 1) // 2, dtype=torch.float64, device=device).view(torch.float32)


def slice_step(planes, cap, fit) -> int:
    """Planes per call when a stack goes through a kernel in slices: at most `cap` (what a launch covers) and `fit` (what
    the workspace bound or the caller allows), at least one."""
    return max(1, min(int(planes), int(cap), int(fit)))


def exported_symbols():
    return ['tvae_cluster_abi_version'] + sorted(SIGNATURES) + sorted(QUERIES)


@functools.cache
def lib():
    """Load the shared library once; fail loudly when it has not been built."""
    return _lib.load_library(LIB_PATH, SIGNATURES, QUERIES, 'tvae_cluster_abi_version', ABI_VERSION,
                             'build it with `make -C target-vae_amd/csrc`.  There is no CPU fallback.')


def query(name, *args) -> int:
    return _lib.run_query(lib, QUERIES, name, args)


def call(name, *args):
    """Invoke an entry point of libtvae_cluster.so on the current torch stream."""
    return _lib.dispatch(lib, SIGNATURES, name, args)


def _launch(name, sig, args):
    _lib._launch(lib, name, sig, args)
