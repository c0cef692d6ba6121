"""K15 and ilcc_extract_auto_batch on the bench's config-2 frames, alone on the chip (MI355X), median of 5 after a warm-up:

  k15_ms            HIP-event spans of K15's six launches on 1024 frames resident in HBM (ilcc_debug_seed_launch_ms) and their sum
  k1_count_ms       K1's count pass of the same batch -- the other kernel that reads every input point once (ilcc_timing)
  extract_batch_ms  ilcc_extract_batch on the same clouds with the true clicks: host wall clock of the synchronous call
  extract_auto_ms   ilcc_extract_auto_batch on the same clouds: host wall clock, its allocations and device copies included

    python tools/dev_seed_timing.py --frames 1024 --out profiles/r09_seed_timing.json
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _chunk(args):
    from lidar_camera_calibration_amd import synth
    lo, n = args
    return synth.make_batch(n, seed=0xC0FFEE + lo)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    F = args.frames
    with mp.get_context("spawn").Pool(args.workers) as pool:      # before the GPU is opened
        parts = pool.map(_chunk, [(lo, min(32, F - lo)) for lo in range(0, F, 32)])
    clouds = np.concatenate([p[0] for p in parts])
    clicks = np.concatenate([p[1] for p in parts])

    import torch
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    from lidar_camera_calibration_amd import seed as S
    n = clouds.shape[1]
    est = LidarCornersBatch(F, n, N.default_params())
    est.reserve(1792, 2560)
    sp = S.default_seed_params(est.params)
    offsets = np.arange(F + 1, dtype=np.uint64) * np.uint64(n)
    d_clouds = torch.from_numpy(clouds).cuda()
    scratch = torch.empty(S.scratch_bytes(F, F * n, sp), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def med(fn, reps=5):
        fn()
        return statistics.median(fn() for _ in range(reps))

    launches = []

    def k15():
        S.propose_seeds_device(est, d_clouds.data_ptr(), offsets, sp, scratch.data_ptr())
        launches.append(S.launch_ms())
        return sum(launches[-1].values())

    def batch():
        t = time.perf_counter()
        est.extract(clouds, clicks)
        return (time.perf_counter() - t) * 1e3

    def auto():
        t = time.perf_counter()
        _, _, ranks = S.extract_auto(est, clouds, None, sp)
        auto.accepted = int((ranks >= 0).sum())
        return (time.perf_counter() - t) * 1e3

    out = {"frames": F, "points_per_frame": n, "k15_ms": med(k15)}
    out["k15_launch_ms"] = {k: statistics.median(row[k] for row in launches[1:]) for k in S.LAUNCHES}
    est.reset_timing()
    out["extract_batch_ms"] = med(batch)
    t = est.timing()
    out["k1_count_ms"] = t.roi_count_ms_sum / max(t.batches, 1)
    out["extract_auto_ms"] = med(auto)
    out["auto_accepted"] = auto.accepted
    out["scratch_bytes"] = int(scratch.numel())
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    est.close()


if __name__ == "__main__":
    main()
