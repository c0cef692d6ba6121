"""K8b against a loop of ilcc_colourise_device: 64 scans x 28 800 points, one 1440 x 1080 image per scan.  HIP events and a host
clock (both windows end in a device synchronise), warm-up, median of 20, the two alternating.  Also the wall time of the chain on the
test recording of tests/paired_cases.py.  On an MI355X:
    python tools/dev_k8b_timing.py --out profiles/r12_k8b_timing.json"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import paired_cases as K  # noqa: E402
from lidar_camera_calibration_amd import camera_image as CI  # noqa: E402
from lidar_camera_calibration_amd import paired, project  # noqa: E402

SCANS, POINTS, W, H, DIS, REPS, WARM = 64, 28800, 1440, 1080, 30.0, 20, 3
ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
args = ap.parse_args()

rng = np.random.default_rng(1)
T = K.T_LIDAR2CAM
cam = project.Projection.from_extrinsic(T, (1000.0, 720.0, 1000.0, 540.0), (W, H))
pts = np.stack([rng.uniform(-20, 20, SCANS * POINTS), rng.uniform(-20, 20, SCANS * POINTS), rng.uniform(-2, 3, SCANS * POINTS),
                rng.uniform(0, 255, SCANS * POINTS)], 1).astype(np.float32)
d_pts = torch.from_numpy(pts).cuda()
d_imgs = [torch.from_numpy(rng.integers(0, 256, (H, 3 * W), dtype=np.uint8)).cuda() for _ in range(SCANS)]
d_batch = torch.zeros((SCANS * POINTS, 4), dtype=torch.float32, device="cuda")
d_loop = torch.zeros((SCANS * POINTS, 4), dtype=torch.float32, device="cuda")
offsets = np.arange(SCANS + 1, dtype=np.uint64) * POINTS
plan = paired.ColourisePlan(SCANS, SCANS * POINTS)
ptrs, steps, image_of = [im.data_ptr() for im in d_imgs], [3 * W] * SCANS, np.arange(SCANS, dtype=np.int32)


def batch():
    paired.colourise_batch_device(d_pts.data_ptr(), offsets, ptrs, steps, image_of, cam, d_batch.data_ptr(), SCANS * POINTS, plan, distance_valid=DIS)
    return plan.finish(SCANS)


def loop():
    at = 0
    for s in range(SCANS):
        at += project.colourise_device(d_pts.data_ptr() + 16 * POINTS * s, POINTS, cam, ptrs[s], 3 * W, d_loop.data_ptr() + 16 * at, DIS)
    return at


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


for _ in range(WARM):
    off = batch()
    total = loop()
torch.cuda.synchronize()
assert int(off[-1]) == total and plan.launches == 3
same = bool((d_batch[:total].view(torch.uint8) == d_loop[:total].view(torch.uint8)).all().item())
times = {"k8b": [], "loop": []}
for _ in range(REPS):
    times["k8b"].append(timed(batch))
    times["loop"].append(timed(loop))

# the chain on the test bag, wall time
tmp = tempfile.mkdtemp()
bag = os.path.join(tmp, "rec.bag")
K.write_recording(bag, "lz4")
yaml = os.path.join(tmp, "cam.yaml")
open(yaml, "w").write(K.yaml_text(K.recording_camera()))
ncam = CI.read_camera_yaml(yaml)
pp = paired.default_paired_params()
chain = []
for _ in range(1 + 5):
    t0 = time.perf_counter()
    items = list(paired.bag_rgblidar_all_scans(bag, K.IMAGE_TOPIC, K.LIDAR_TOPIC, ncam, T, distance_valid=K.DISTANCE, pp=pp))
    chain.append((time.perf_counter() - t0) * 1e3)
os.remove(bag)
os.remove(yaml)
os.rmdir(tmp)

result = {
    "scans": SCANS, "points_per_scan": POINTS, "image": [W, H], "records": int(total), "bytes_equal": same, "reps": REPS,
    "k8b_event_ms_median": float(np.median([t[0] for t in times["k8b"]])), "k8b_host_ms_median": float(np.median([t[1] for t in times["k8b"]])),
    "loop_event_ms_median": float(np.median([t[0] for t in times["loop"]])), "loop_host_ms_median": float(np.median([t[1] for t in times["loop"]])),
    "k8b_event_ms_min_max": [float(min(t[0] for t in times["k8b"])), float(max(t[0] for t in times["k8b"]))],
    "loop_event_ms_min_max": [float(min(t[0] for t in times["loop"])), float(max(t[0] for t in times["loop"]))],
    "chain_test_bag_first_ms": chain[0], "chain_test_bag_ms_median_of_5": float(np.median(chain[1:])), "chain_scans": len(items),
}
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as fh:
        fh.write(json.dumps(result, indent=1) + "\n")
assert same
