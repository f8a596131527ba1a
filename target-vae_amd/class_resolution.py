#!/usr/bin/env python3
"""Half-set averages, variance maps and the FRC resolution of the aligned 2-D class averages, from the files a
clustering_*.py run wrote (rotations.npy, translations.npy, clusters.npy) and the stack it clustered; needs no encoder.
Both halves share one encoder and one set of poses: not a gold-standard FRC, it reads optimistic.  With --ctf FILE the stack is
phase-flipped first (tvae/ctf.py).  See tvae/resolution.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.resolution import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
