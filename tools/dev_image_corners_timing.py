"""HIP-event ms per K10 stage (gradients + min/max, likelihood, NMS, refine + score) and wall ms of the
host structure recovery, for the six golden crops and a full 1920 x 1200 synthetic frame.  Median of
--reps runs after one warm-up.  Usage: python tools/dev_image_corners_timing.py [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lidar_camera_calibration_amd import image_corners as IC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from test_image_corners import render_board
    images = []
    for i in range(1, 7):
        z = np.load(os.path.join(ROOT, "tests", "golden", f"pointgrey{i}_crop.npz"))
        images.append((f"pointgrey{i}_crop", z["image"]))
    img, _ = render_board((1920, 1200), square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    images.append(("synthetic_1920x1200", img))
    rows = []
    for name, im in images:
        t = torch.from_numpy(im).cuda()
        IC.find_corners(t, stages=True)
        runs = []
        for _ in range(a.reps):
            corners, st = IC.find_corners(t, stages=True)
            t0 = time.perf_counter()
            try:
                IC.chessboard_from_corners(corners, (7, 5))
            except IC.BoardNotFound:
                pass
            host = (time.perf_counter() - t0) * 1e3
            runs.append([st["ms"]["gradients"], st["ms"]["likelihood"], st["ms"]["nms"], st["ms"]["refine_score"], host])
        med = np.median(np.array(runs), 0)
        row = dict(image=name, width=im.shape[1], height=im.shape[0], candidates=st["n_candidates"], corners=len(corners),
                   gradients_ms=med[0], likelihood_ms=med[1], nms_ms=med[2], refine_score_ms=med[3], structure_host_ms=med[4])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}))


if __name__ == "__main__":
    main()
