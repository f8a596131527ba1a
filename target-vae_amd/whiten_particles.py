#!/usr/bin/env python3
"""Whiten a particle stack on the GPU with the radial noise spectrum of its background, per group (micrograph or defocus
group): the step before ml_class_averages.py and refine_poses.py, whose scores assume white noise.  Two streamed passes
(estimate, then filter); writes the fp32 .mrcs and, beside it, noise_spectrum.npy and noise_counts.npy.  See tvae/spectrum.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.spectrum import run  # noqa: E402


def main():
    run(tool='whiten')


if __name__ == '__main__':
    main()
