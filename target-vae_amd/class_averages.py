#!/usr/bin/env python3
"""Aligned 2-D class averages from the files a clustering_*.py run wrote (rotations.npy, translations.npy, clusters.npy)
and the stack it clustered; needs no encoder.  With --ctf FILE (one row of CTF parameters per image) also the phase-flipped
or Wiener-weighted averages, class_averages_ctf.*.  See tvae/align.py and tvae/ctf.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.align import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
