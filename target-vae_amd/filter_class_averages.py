#!/usr/bin/env python3
"""Filter the class averages to their FRC on the GPU: the weight sqrt(2 FRC / (1 + FRC)) or a hard low-pass, cut at the
ring where the curve of class_resolution.py first falls below the threshold; writes class_averages_filtered.npy, .mrcs
and .jpg.  See tvae/spectrum.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.spectrum import run  # noqa: E402


def main():
    run(tool='filter')


if __name__ == '__main__':
    main()
