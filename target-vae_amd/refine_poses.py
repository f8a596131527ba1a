#!/usr/bin/env python3
"""Refine the poses of a clustered stack against its aligned 2-D class averages, from the files a clustering_*.py run wrote
(rotations.npy, translations.npy, clusters.npy) and the stack it clustered; needs no encoder.  Writes rotations_refined.npy,
translations_refined.npy, refine_scores.npy and class_averages_refined.{npy,mrcs,jpg}; the refined pose files go straight
into class_averages.py and class_resolution.py.  See tvae/refine.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.refine import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
