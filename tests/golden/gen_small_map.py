"""Writes tests/golden/small_map.rvm: five voxels' records from the numpy restatement (tests/voxel_map_ref.py through
tests/map_records_ref.py), laid out field by field with struct -- not through revo_amd.mapfile, whose byte layout it pins.

    python tests/golden/gen_small_map.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import map_records_ref as mrr  # noqa: E402

VOXEL, DENSE, DROPPED, KEYFRAMES = 0.25, 1, 1, 2


def points():
    xyz = np.array([[0.1, 0.1, 1.0], [0.2, 0.05, 1.1], [-0.3, 0.4, 0.9], [-0.26, 0.45, 0.7], [1.7, -2.2, 3.1], [-5.5, 0.0, 2.0],
                    [0.15, 0.12, 1.2], [3000.0, 0.0, 1.0]], np.float32)  # the last one is out of range: dropped
    rgb = np.array([[10, 20, 30], [250, 0, 7], [1, 2, 3], [4, 5, 7], [255, 255, 255], [0, 128, 64], [9, 9, 200], [1, 1, 1]], np.uint8)
    return xyz, rgb


def main():
    rec = mrr.records_from_points(*points(), np.eye(4, dtype=np.float32), VOXEL)
    data = mrr.file_bytes(VOXEL, DENSE, rec, DROPPED, KEYFRAMES)
    with open(os.path.join(HERE, "small_map.rvm"), "wb") as f:
        f.write(data)
    print("small_map.rvm: %d records, %d bytes" % (len(rec), len(data)))


if __name__ == "__main__":
    main()
