#!/usr/bin/env python3
"""Polish the poses of a clustered stack to sub-pixel accuracy against its aligned 2-D class averages, from the pose files a
clustering_*.py, refine_poses.py or reclassify_particles.py run wrote and the stack it worked on; needs no encoder.  Writes
rotations_polished.npy, translations_polished.npy, polish_scores.npy, polish_steps.npy and
class_averages_polished.{npy,mrcs,jpg}; the polished pose files go straight into class_averages.py, class_resolution.py and
every other script that takes poses.  See tvae/polish.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tvae.polish import run  # noqa: E402


def main():
    run()


if __name__ == '__main__':
    main()
