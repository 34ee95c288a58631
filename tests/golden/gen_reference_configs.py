"""Generates tests/golden/reference_configs.json.

Runs ONLY in the authoring container, by hand: reads the reference's shipped configuration files
(config/dataset_tum1.yaml, orbbec_dataset.yaml, orbbec_normal.yaml, orbbec_pro.yaml, realsense.yaml and
revo_settings.yaml) with the port's own YAML reader and keeps the VALUES of the keys revo_amd/config.py reads --
no file text, no comments.  A key a file does not set is left out, so the test that reads the JSON also pins the
default the port falls back to (cv::read(fs[key], var, default), camerapyr.h:40-64, tracker.h:43-47).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from revo_amd.config import _load  # noqa: E402

REF = "/root/reference/config"
DATASET_KEYS = ["Camera.fx", "Camera.fy", "Camera.cx", "Camera.cy", "Camera.width", "Camera.height", "width", "height",
                "cannyThreshold1", "cannyThreshold2", "PYR_MIN_LVL", "PYR_MAX_LVL", "DEPTH_MIN", "DEPTH_MAX", "USE_EDGE_HIST",
                "nPercentage", "DEPTH_SCALE_FACTOR"]
SETTINGS_KEYS = ["CHECK_TRACKING_RESULTS", "CHECK_INIT_VALUES", "USE_EDGE_FILTER", "N_FRAMES_HIST_VOTING",
                 "DO_GENERATE_DENSE_PCL", "DO_OUTPUT_POSES"]
DATASETS = ["dataset_tum1", "orbbec_dataset", "orbbec_normal", "orbbec_pro", "realsense"]


def values(name, keys):
    d = _load(os.path.join(REF, name + ".yaml"))
    return {k: d[k] for k in keys if k in d}


def main():
    out = {"datasets": {n: values(n, DATASET_KEYS) for n in DATASETS},
           "settings": {"revo_settings": values("revo_settings", SETTINGS_KEYS)}}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_configs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
