#!/usr/bin/env python3
"""Reassign the images of a clustered stack to their best-matching aligned 2-D class average and refine their poses, from the
files a clustering_*.py run wrote (rotations.npy, translations.npy, clusters.npy, optionally latents.npy) and the stack it
clustered; needs no encoder.  Writes clusters_reclassified.npy, rotations_reclassified.npy, translations_reclassified.npy,
classify_scores.npy, classify_moved.npy, class_scores.npy and class_averages_reclassified.{npy,mrcs,jpg}; the cluster and
pose files go straight into class_averages.py, class_resolution.py and refine_poses.py.  See tvae/classify.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.classify import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
