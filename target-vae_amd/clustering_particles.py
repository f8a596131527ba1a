#!/usr/bin/env python3
"""Drop-in for the reference clustering_particles.py (same flags, results.txt wording) on the MI355X: latents of the whole
stack extracted on the device, k-means on the HIP kernels.  See tvae/cluster_driver.py for the driver."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.cluster import cluster_acc, measure_correlations  # noqa: F401,E402  (reference module-level names)
from tvae.cluster_driver import run  # noqa: E402
from tvae.latent import get_latent  # noqa: F401,E402


def main():
    run('particles')


if __name__ == '__main__':
    main()
