"""HIP-event ms of the two overlay kernels on a 1920 x 1200 frame with the golden pointgrey.yaml lens:
K11c (ilcc_image_to_bgr8_device) in each encoding, with the camera (conversion + undistortion) and without
(conversion only), beside the algorithmic byte count (source + 3 bytes per output pixel, each once) and the rate
that makes; and K12 (ilcc_draw_hits_device: clear + mark + resolve) for 28 800 and 131 072 hits spread over the
frame.  A run is --calls back-to-back calls between two events, divided by their number (one launch alone is
mostly launch gap); the figure is the median of --reps runs after one warm-up.
Usage: python tools/dev_overlay_timing.py [--reps 5] [--calls 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_camera_calibration_amd import camera_image as CI  # noqa: E402
from lidar_camera_calibration_amd import project  # noqa: E402


def median_ms(fn, reps, calls):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    import torch
    cam = CI.read_camera_yaml(os.path.join(ROOT, "tests", "golden", "pointgrey.yaml"))
    w, h = cam.width, cam.height
    rng = np.random.default_rng(0)
    for encoding in CI.ENCODINGS:
        bpp = CI.BYTES_PER_PIXEL[encoding]
        src = torch.from_numpy(rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)).cuda()
        for camera in (cam, None):
            med = median_ms(lambda: CI.to_bgr8(src, encoding, camera), a.reps, a.calls)
            nbytes = w * h * (bpp + 3)
            print(json.dumps(dict(kernel="k11c", encoding=encoding, undistort=camera is not None, width=w, height=h,
                                  ms=round(med, 4), bytes=nbytes, gb_per_s=round(nbytes / med / 1e6, 1))))
    image = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    scratch = torch.empty(project.draw_hits_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for n in (28800, 131072):
        hits = np.zeros(n, project.HIT_DTYPE)
        hits["x"], hits["y"] = rng.integers(0, w, n), rng.integers(0, h, n)
        hits["r"], hits["g"], hits["b"] = rng.integers(0, 256, (3, n))
        d_hits = torch.from_numpy(np.frombuffer(hits.tobytes(), np.uint8).copy()).cuda()
        med = median_ms(lambda: project.draw_hits_device(image.data_ptr(), w, h, 3 * w, d_hits.data_ptr(), n, scratch.data_ptr(),
                                                         stream=stream), a.reps, a.calls)
        print(json.dumps(dict(kernel="k12", hits=n, width=w, height=h, ms=round(med, 4), scratch_bytes=int(scratch.numel()))))


if __name__ == "__main__":
    main()
