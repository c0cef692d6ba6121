"""Where the time of writing a JPEG frame goes (include/ilcc_jpeg_write.h), per stage, at 1920 x 1200 and quality 95:
the reference's pointgrey1.jpg decoded (one component) and the same frame tinted (three components, written 4:2:0).

  K14              ilcc_jpeg_fdct_device, HIP events: 1 launch for one component (k14_fdct_quant alone), 4 for three
                   (k14_colour_downsample, then k14_fdct_quant per component)
  download         D2H of the int16 coefficients into pageable memory, HIP events
  entropy encode   host, monotonic clock
  encode call      ilcc_jpeg_encode_device: info .. file bytes, its hipMalloc / hipFree included, monotonic clock

The HIP-event figures follow tools/dev_jpeg_timing.py: --calls back-to-back calls between two events, divided by their
number; the median of --reps runs after one warm-up.  The time of each kernel by itself comes from a kernel trace, in a
run of its own, for which --trace gray|colour makes the target (50 K14 calls and nothing else):
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/dev_jpeg_write_timing.py --trace colour
Usage: python tools/dev_jpeg_write_timing.py [--reps 7] [--calls 10] [--quality 95] [--trace gray|colour]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dev_jpeg_timing import clock_ms, event_ms  # noqa: E402
from lidar_camera_calibration_amd import jpeg  # noqa: E402
from lidar_camera_calibration_amd import jpeg_write as JW  # noqa: E402


def frames():
    """(name, device pixels, sampling) of the two frames."""
    import torch
    with open(os.path.join(ROOT, "tests", "golden", "jpeg", "pointgrey1.jpg"), "rb") as f:
        gray = jpeg.decode(f.read())
    y = gray.cpu().numpy().astype(np.float32)
    x = np.linspace(0.6, 1.0, y.shape[1], dtype=np.float32)[None, :]
    bgr = np.stack([y * x[:, ::-1], y * 0.9, y * x], axis=-1).astype(np.uint8)
    return [("pointgrey1 decoded, gray", gray, None), ("pointgrey1 tinted, 4:2:0", torch.from_numpy(bgr).cuda(), "420")]


def measure(name, px, sampling, quality, reps, calls):
    import torch
    info = JW.write_info(px.shape[1], px.shape[0], sampling, quality)
    d_coef = JW.fdct(info, px)
    coef = d_coef.cpu().numpy()
    data = JW.entropy_encode(info, coef)
    assert JW.encode(px, quality, sampling or "420") == data
    host = torch.empty(info.coef_count, dtype=torch.int16)
    row = dict(frame=name, width=info.width, height=info.height, components=info.n_components, quality=quality,
               coefficients_mb=round(coef.nbytes / 1e6, 2), file_bytes=len(data))
    row["k14_ms"] = round(event_ms(lambda: JW.fdct(info, px, d_coef), reps, calls), 4)
    row["download_ms"] = round(event_ms(lambda: host.copy_(d_coef), reps, calls), 3)
    row["entropy_ms"] = round(clock_ms(lambda: JW.entropy_encode(info, coef), reps), 3)
    row["encode_call_ms"] = round(clock_ms(lambda: JW.encode(px, quality, sampling or "420"), reps), 3)
    print(json.dumps(row))


def trace_target(px, sampling, quality, calls=50):
    import torch
    info = JW.write_info(px.shape[1], px.shape[0], sampling, quality)
    d_coef = JW.fdct(info, px)
    for _ in range(calls):
        JW.fdct(info, px, d_coef)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--trace", choices=["gray", "colour"])
    a = ap.parse_args()
    for k, (name, px, sampling) in enumerate(frames()):
        if a.trace:
            if a.trace == ("gray", "colour")[k]:
                trace_target(px, sampling, a.quality)
        else:
            measure(name, px, sampling, a.quality, a.reps, a.calls)


if __name__ == "__main__":
    main()
