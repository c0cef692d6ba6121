"""Where the time of reading a JPEG frame goes (include/ilcc_jpeg.h), per stage, for the reference's pointgrey1.jpg
(1920 x 1200, one component) and for the same frame tinted and re-encoded as colour 4:2:0 (needs Pillow):

  entropy decode   host, monotonic clock, median of --reps calls
  upload           H2D of the int16 coefficients from pageable memory, HIP events
  K13              ilcc_jpeg_idct_device, HIP events
                   (a call is 1 launch for one component, 4 for three: at these sizes mostly launch gaps)
  K10              image_corners.find_corners on the decoded frame (device stages + its D2H), for scale

The HIP-event figures follow tools/dev_camera_image_timing.py: --calls back-to-back calls between two events, divided by
their number; the median of --reps runs after one warm-up.  The time of each kernel by itself comes from a kernel trace,
in a run of its own per frame, for which --trace gray|colour makes the target (50 K13 calls and nothing else):
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/dev_jpeg_timing.py --trace colour
Usage: python tools/dev_jpeg_timing.py [--reps 5] [--calls 10] [--trace gray|colour]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_camera_calibration_amd import camera_image as CI  # noqa: E402
from lidar_camera_calibration_amd import image_corners as IC  # noqa: E402
from lidar_camera_calibration_amd import jpeg  # noqa: E402


def event_ms(fn, reps, calls):
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


def clock_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def measure(name, jpg, reps, calls):
    import torch
    info = jpeg.parse(jpg)
    coef = jpeg.entropy_decode(jpg, info)
    d_coef = torch.from_numpy(coef).cuda()
    out = jpeg.idct(info, d_coef)
    row = dict(frame=name, bytes=len(jpg), width=info.width, height=info.height, components=info.n_components,
               coefficients_mb=round(coef.nbytes / 1e6, 2))
    row["entropy_ms"] = round(clock_ms(lambda: jpeg.entropy_decode(jpg, info), reps), 3)
    row["upload_ms"] = round(event_ms(lambda: d_coef.copy_(torch.from_numpy(coef)), reps, calls), 3)
    row["k13_ms"] = round(event_ms(lambda: jpeg.idct(info, d_coef, out), reps, calls), 4)
    row["decode_call_ms"] = round(clock_ms(lambda: jpeg.decode(jpg), reps), 3)   # the one-call entry: parse .. K13, its hipMalloc / hipFree
    mono = CI.to_mono8(out, info.encoding)
    torch.cuda.synchronize()
    row["k10_find_corners_ms"] = round(clock_ms(lambda: IC.find_corners(mono), reps), 3)
    print(json.dumps(row))


def trace_target(jpg, calls=50):
    import torch
    info = jpeg.parse(jpg)
    d_coef = torch.from_numpy(jpeg.entropy_decode(jpg, info)).cuda()
    out = jpeg.idct(info, d_coef)
    for _ in range(calls):
        jpeg.idct(info, d_coef, out)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--trace", choices=["gray", "colour"])
    a = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "jpeg", "pointgrey1.jpg"), "rb") as f:
        gray = f.read()
    if a.trace == "gray":
        return trace_target(gray)
    if not a.trace:
        measure("pointgrey1.jpg", gray, a.reps, a.calls)
    try:
        from PIL import Image
    except ImportError:
        print(json.dumps(dict(frame="colour 4:2:0", skipped="Pillow is not installed")))
        return
    y = np.asarray(Image.open(io.BytesIO(gray))).astype(np.float32)
    x = np.linspace(0.6, 1.0, y.shape[1], dtype=np.float32)[None, :]
    rgb = np.stack([y * x, y * 0.9, y * x[:, ::-1]], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=90, subsampling=2)
    if a.trace:
        return trace_target(buf.getvalue())
    measure("pointgrey1 tinted, 4:2:0 q90", buf.getvalue(), a.reps, a.calls)


if __name__ == "__main__":
    main()
