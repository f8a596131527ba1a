"""Drop-in for the reference's src/image.py: `downsample`, `crop` and `normalize` with the same names and signatures, numpy
in and numpy out in the input's dtype, computed on the GPU by tvae.image (fp32 kernels, fp64 statistics; the definition
is in include/tvae_cluster.h).  There is no CPU fallback: without a GPU the two computing functions raise."""
from __future__ import division, print_function

import numpy as np


def _device():
    import torch
    from tvae._lib import TvaeHipError
    if not torch.cuda.is_available():
        raise TvaeHipError('src.image: no GPU is visible and there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _to_device(x):
    import torch
    a = np.ascontiguousarray(x, dtype=np.float32)
    return torch.from_numpy(a).to(_device())


def downsample(x, factor=1, shape=None):
    """ Downsample 2d array using fourier transform """
    from tvae import image
    x = np.asarray(x)
    return image.downsample(_to_device(x), factor, shape).cpu().numpy().astype(x.dtype)


def crop(stack, size):
    from tvae import image
    return image.crop(stack, size)


def normalize(stack, radius=None):
    from tvae import image
    stack = np.asarray(stack)
    return image.normalize(_to_device(stack), radius).cpu().numpy().astype(stack.dtype)
