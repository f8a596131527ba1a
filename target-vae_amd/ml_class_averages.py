#!/usr/bin/env python3
"""Maximum-likelihood 2-D class averages of a clustered stack, from the files a clustering_*.py run wrote (rotations.npy,
translations.npy, clusters.npy, optionally latents.npy) and the stack it clustered; needs no encoder.  Every image
contributes to every class and pose it is compatible with, with its posterior weight; the noise variance and the class priors
are re-estimated every round.  Writes class_averages_ml.{npy,mrcs,jpg}, class_weights.npy, clusters_ml.npy, rotations_ml.npy,
translations_ml.npy, ml_log_likelihood.npy, ml_sigma2.npy and ml_entropy.npy; the cluster and pose files go straight into
class_averages.py, class_resolution.py and refine_poses.py.  See tvae/ml2d.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.ml2d import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
