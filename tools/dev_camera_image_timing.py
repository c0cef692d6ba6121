"""HIP-event ms of K11 (ilcc_image_to_mono8_device) on a 1920 x 1200 frame in each encoding, the four Bayer ones included, with the
golden pointgrey.yaml camera (conversion + undistortion) and without one (conversion only), beside the
algorithmic byte count (source + destination, each once) and the rate that makes.  A run is --calls
back-to-back calls between two events, divided by their number (one launch alone is mostly launch gap);
the figure is the median of --reps runs after one warm-up.
Usage: python tools/dev_camera_image_timing.py [--reps 5] [--calls 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_camera_calibration_amd import camera_image as CI  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    import torch
    cam = CI.read_camera_yaml(os.path.join(ROOT, "tests", "golden", "pointgrey.yaml"))
    w, h = cam.width, cam.height
    rng = np.random.default_rng(0)
    for encoding in CI.ENCODINGS + tuple(CI.BAYER_ENCODINGS):
        bpp = CI.BYTES_PER_PIXEL[encoding]
        shape = (h, w) if encoding in CI.BAYER_ENCODINGS else (h, w, bpp)      # a Bayer frame is (rows, cols)
        src = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).cuda()
        for camera in (cam, None):
            CI.to_mono8(src, encoding, camera)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    CI.to_mono8(src, encoding, camera)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.calls)
            med = float(np.median(ms))
            nbytes = w * h * (bpp + 1)
            print(json.dumps(dict(encoding=encoding, undistort=camera is not None, width=w, height=h, ms=round(med, 4),
                                  bytes=nbytes, gb_per_s=round(nbytes / med / 1e6, 1))))


if __name__ == "__main__":
    main()
