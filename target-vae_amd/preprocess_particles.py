#!/usr/bin/env python3
"""Crop, Fourier-downsample and normalize a raw particle stack on the GPU, the step before train_particles.py and
clustering_particles.py; writes an fp32 .mrcs and, with --normalize, <out>.stats.npy.  See tvae/image.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.image import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
