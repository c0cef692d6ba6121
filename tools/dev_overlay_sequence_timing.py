"""What batching the overlay buys, on --scans scans of --points points drawn on 1920 x 1200 and 702 x 629 images (MI355X, alone on
the chip).

  loop_ms      leg (a), all the library offered before K12b: per scan a device copy of its image into its canvas,
               ilcc_project_intensity_device (two launches, a stream synchronise, a host read of a page-locked counter) and
               ilcc_draw_hits_device (three launches); the hit list lives in device memory between the two
  batch_ms     leg (b): ilcc_overlay_batch_device on ONE plan (a table upload, three launches, the counts back) and
               ilcc_overlay_plan_finish
               Both legs leave the same canvases and counts; host clock around work that ends in a synchronise, 2 warm-ups, median of
               10, the legs alternating in one process, outputs compared byte for byte

    python tools/dev_overlay_sequence_timing.py --out profiles/r20_overlay_sequence_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMAGES = 4          # distinct images of the batch, each shared by a quarter of the scans


def scene(width, height, scans, points, seed):
    """-> (camera, xyzi (scans * points, 4) float32, images [N_IMAGES] (height, 3 * width) uint8): points aimed at image coordinates
    in [-0.1, 1.1) of the image at depths of 1 .. 10 m, so that about seven in ten are drawn, neighbours in memory near each other in
    the image as along a scan line"""
    from lidar_camera_calibration_amd import project
    rng = np.random.default_rng(seed)
    cam = project.Projection()
    cam.R[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    cam.t[:] = [0.0, 0.0, 0.0]
    cam.fx, cam.cx, cam.fy, cam.cy = 0.55 * width, 0.5 * width, 0.55 * width, 0.5 * height
    cam.width, cam.height = width, height
    n = scans * points
    lines = 16                                               # a scan: 16 lines swept from left to right
    k = np.arange(n) % points
    u = (k // lines) / (points // lines) * 1.2 * width - 0.1 * width + rng.uniform(-0.5, 0.5, n)
    v = (k % lines + 0.5) / lines * 1.2 * height - 0.1 * height + rng.uniform(-0.04, 0.04, n) * height
    d = rng.uniform(1.0, 10.0, n)
    xyzi = np.stack([(u - cam.cx) / cam.fx * d, (v - cam.cy) / cam.fy * d, d, rng.uniform(0, 60, n)], 1).astype(np.float32)
    images = [rng.integers(0, 256, (height, 3 * width), dtype=np.uint8) for _ in range(N_IMAGES)]
    return cam, xyzi, images


def legs(width, height, scans, points, seed):
    import torch
    from lidar_camera_calibration_amd import overlay, project
    cam, xyzi, images = scene(width, height, scans, points, seed)
    d_xyzi = torch.from_numpy(xyzi.view(np.uint8).reshape(-1)).cuda()
    d_images = [torch.from_numpy(im).cuda() for im in images]
    image_of = np.arange(scans, dtype=np.int32) % N_IMAGES
    offsets = np.arange(scans + 1, dtype=np.uint64) * points
    pitch = 3 * width * height
    out_a = torch.zeros(scans * pitch, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros_like(out_a)
    hits = torch.empty(16 * points, dtype=torch.uint8, device="cuda")
    k12_scratch = torch.empty(project.draw_hits_scratch_bytes(width, height), dtype=torch.uint8, device="cuda")
    scratch_bytes = overlay.overlay_batch_scratch_bytes(width, height, scans)
    k12b_scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device="cuda")
    plan = overlay.OverlayPlan(scans, scans * points)
    stream = torch.cuda.current_stream().cuda_stream
    counts = {}

    def loop():
        n = []
        for s in range(scans):
            canvas = out_a[s * pitch:(s + 1) * pitch]
            canvas.copy_(d_images[image_of[s]].reshape(-1))
            m = project.project_intensity_device(d_xyzi.data_ptr() + 16 * points * s, points, cam, hits.data_ptr(), 50.0, 0.0, 60.0, stream=stream)
            project.draw_hits_device(canvas.data_ptr(), width, height, 3 * width, hits.data_ptr(), m, k12_scratch.data_ptr(), stream=stream)
            n.append(m)
        counts["loop"] = n

    def batch():
        overlay.overlay_batch_device(d_xyzi.data_ptr(), offsets, [im.data_ptr() for im in d_images], [3 * width] * N_IMAGES, image_of, cam, out_b.data_ptr(),
                                     3 * width, pitch, k12b_scratch.data_ptr(), scratch_bytes, plan, 50.0, 0.0, 60.0, stream=stream)
        counts["batch"] = plan.finish(scans).tolist()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        timed(loop), timed(batch)
    a, b = [], []
    for _ in range(10):
        out_a.zero_()
        out_b.zero_()
        a.append(timed(loop))
        b.append(timed(batch))
        assert plan.launches == 3 and counts["loop"] == counts["batch"]
        assert torch.equal(out_a, out_b)
    plan.close()
    med = statistics.median
    drawn = int(sum(counts["batch"]))
    return {"scans": scans, "points_per_scan": points, "width": width, "height": height, "distinct_images": N_IMAGES, "points_drawn": drawn,
            "loop_ms": med(a), "loop_ms_range": [min(a), max(a)], "batch_ms": med(b), "batch_ms_range": [min(b), max(b)],
            "canvas_bytes": scans * pitch, "owner_bytes": scratch_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--points", type=int, default=28800)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"method": "host clock around work that ends in a synchronise, 2 warm-ups, median of 10, legs alternating, canvases and counts equal byte for byte"}
    out["full_frame"] = legs(1920, 1200, args.scans, args.points, 21)
    out["crop"] = legs(702, 629, args.scans, args.points, 22)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
