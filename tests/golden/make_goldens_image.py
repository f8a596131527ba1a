#!/usr/bin/env python3
"""Generate tests/golden/image_ref.npz from the REAL reference's src/image.py (downsample, crop, normalize):

    python tests/golden/make_goldens_image.py <path of the reference checkout>

Small seeded fp64 inputs and what the reference's three functions return for them; inputs and outputs only, nothing of
the reference's text is stored.  Run once; the file is committed."""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (M, N) -> (m, n): even to even, even to odd, odd to even, mixed, to a single pixel, tiny, and the identity sizes; the
# last one keeps every column and drops rows (Im Kx does not vanish at n == N, Im Ry does at m == M)
DOWNSAMPLE = [((16, 16), (8, 8)), ((16, 16), (7, 7)), ((15, 15), (6, 6)), ((15, 17), (5, 8)), ((20, 24), (7, 10)),
              ((8, 8), (1, 1)), ((8, 8), (3, 2)), ((12, 10), (12, 10)), ((13, 11), (13, 11)), ((9, 6), (4, 6))]
NORMALIZE = [((7, 9), None), ((7, 9), 3), ((16, 16), None), ((16, 16), 3)]


def main():
    ref = sys.argv[1]
    spec = importlib.util.spec_from_file_location('reference_image', os.path.join(ref, 'src', 'image.py'))
    image = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(image)
    rng = np.random.default_rng(20240611)
    out = {}
    for k, ((M, N), (m, n)) in enumerate(DOWNSAMPLE):
        x = rng.standard_normal((1, M, N)) + 3.0
        out[f'down{k}_x'] = x
        out[f'down{k}_shape'] = np.array([m, n])
        out[f'down{k}_y'] = image.downsample(x, shape=(m, n))
    x = rng.standard_normal((2, 16, 12))
    out['downf_x'], out['downf_factor'], out['downf_y'] = x, np.array(2.5), image.downsample(x, factor=2.5)
    for k, ((n, m), radius) in enumerate(NORMALIZE):
        x = 1000.0 + rng.standard_normal((2, n, m))
        out[f'norm{k}_x'] = x
        out[f'norm{k}_radius'] = np.array(np.nan if radius is None else float(radius))
        out[f'norm{k}_y'] = image.normalize(x) if radius is None else image.normalize(x, radius)
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        x = rng.standard_normal((2, 7, 9))
        out['norm_empty_x'], out['norm_empty_radius'] = x, np.array(40.0)         # no pixel that far out: NaN throughout
        out['norm_empty_y'] = image.normalize(x, 40.0)
        x = rng.standard_normal((2, 8, 8))
        far = np.hypot(*np.meshgrid(4.0 - np.arange(8), 4.0 - np.arange(8), indexing='ij')) >= 4.0
        x[:, far] = 2.5                                                           # a constant ring: sigma = 0
        out['norm_const_x'], out['norm_const_radius'] = x, np.array(np.nan)
        out['norm_const_y'] = image.normalize(x)
    x = rng.standard_normal((3, 9, 10))
    out['crop_x'], out['crop_size'], out['crop_y'] = x, np.array(4), np.ascontiguousarray(image.crop(x, 4))
    path = os.path.join(HERE, 'image_ref.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
