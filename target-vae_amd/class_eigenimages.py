#!/usr/bin/env python3
"""Eigenimages of the aligned 2-D classes (the leading principal components of the aligned, mean-subtracted members), the
coordinates of every particle along them and its residual norm, from the files a clustering_*.py run wrote (rotations.npy,
translations.npy, clusters.npy) and the stack it clustered; needs no encoder.  With --ctf FILE the stack is phase-flipped
first (tvae/ctf.py).  See tvae/eigen.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.eigen import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
