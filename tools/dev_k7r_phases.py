"""Where k7r_pattern_refine's wavefront cycles go: setup (staging, grid argmin, near-tie recount, first-round test), silence-test
trips, queued evaluations, row reduction + LDS atomics, the sweep's two barriers, the decision step, the basin checks -- for
1024-frame config-2 batches alone on the chip, and again inside the depth-4 pipeline.  Per frame: rounds, trips, queued points
and the life of its slowest wavefront (median / p90 / max over the batch: the launch lasts as long as the max).
Build the instrumented library first (tools/build_variant.sh k7rtiming -DILCC_K7R_TIMING) and run on the GPU box:
    ILCC_HIP_LIB=build/ab/libilcc_hip_k7rtiming.so python tools/dev_k7r_phases.py [out.json]"""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import numpy as np
import torch
from lidar_camera_calibration_amd import LidarCornersBatch
from lidar_camera_calibration_amd import _native as N

F, n_points, DEPTH = 1024, 28800, 4
WORDS, CAP = 16, 1 << 14   # k7r_pattern_refine.hip: kProfWords, kRefineProfWaves
# RefineProfSlot
WRITTEN, SETUP, TRIPS, EVALS, REDUCE, BARRIER, DECIDE, BASIN, LIFE, ROUNDS, TRIP_COUNT, QUEUED, FRAME, WAVE = range(14)
PHASES = (("setup", SETUP), ("silence_trips", TRIPS), ("queued_evaluations", EVALS), ("reduce_and_atomics", REDUCE),
          ("barriers", BARRIER), ("decision", DECIDE), ("basin_checks", BASIN))
clouds, clicks, _ = bench.generate(2, F, 0xC0FFEE, 16)
d_cloud, d_click = torch.from_numpy(clouds).cuda(), torch.from_numpy(clicks).cuda()
est = LidarCornersBatch(F, n_points, N.default_params(), device=0)
est.set_result_mode(N.RESULTS_COMPACT)
est.reserve(1792, 2560)
lib = N.lib()
lib.ilcc_debug_k7r_profile.restype = C.c_int
lib.ilcc_debug_k7r_profile.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_int]
prof = (C.c_ulonglong * (WORDS * CAP))()


def run(n, depth):
    inflight = []
    for _ in range(n):
        inflight.append(est.submit_device(d_cloud.data_ptr(), F, n_points, d_click.data_ptr()))
        if len(inflight) == depth:
            est.wait_compact(inflight.pop(0))
    while inflight:
        est.wait_compact(inflight.pop(0))


def spread(v):
    return {"median": float(np.median(v)), "p90": float(np.percentile(v, 90)), "max": float(v.max())}


def phases(depth, batches):
    run(8, depth)
    torch.cuda.synchronize()
    assert lib.ilcc_debug_k7r_profile(prof, CAP, 1) >= 0
    run(batches, depth)
    torch.cuda.synchronize()
    n = lib.ilcc_debug_k7r_profile(prof, CAP, 1)
    assert n > 0
    r = np.frombuffer(prof, dtype=np.uint64)[:n * WORDS].reshape(n, WORDS).astype(np.float64)   # one record per wavefront: the last batch's
    life = r[:, LIFE].sum()
    out = {"depth": depth, "wavefronts": n, "mean_life_cycles": life / n}
    for name, slot in PHASES:
        out[name + "_cycles"] = r[:, slot].sum() / n
        out[name + "_share"] = r[:, slot].sum() / life
    out["unattributed_share"] = 1.0 - sum(out[name + "_share"] for name, _ in PHASES)
    # per frame: its wavefronts walk the same rounds; trips and queued points add up over them; its life is its slowest wavefront's
    frames = np.unique(r[:, FRAME])
    per = np.array([(r[r[:, FRAME] == f][:, ROUNDS].max(), r[r[:, FRAME] == f][:, TRIP_COUNT].sum(), r[r[:, FRAME] == f][:, QUEUED].sum(),
                     r[r[:, FRAME] == f][:, LIFE].max()) for f in frames])
    out["frames_recorded"] = int(len(frames))
    for k, name in enumerate(("rounds", "trips", "queued_points", "life_cycles")):
        out["frame_" + name] = spread(per[:, k])
    return out


res = {"frames": F, "config": 2, "lib": os.path.basename(os.environ.get("ILCC_HIP_LIB", "(in-tree)")), "alone": phases(1, 4), "pipeline_depth4": phases(DEPTH, 24)}
for key in ("alone", "pipeline_depth4"):
    r = res[key]
    print("%-16s life %8.0f cycles/wavefront: " % (key, r["mean_life_cycles"]) + ", ".join("%s %.1f %%" % (n, 100 * r[n + "_share"]) for n, _ in PHASES))
    print("%-16s per frame: " % "" + ", ".join("%s %s" % (n, {k: round(v) for k, v in r["frame_" + n].items()}) for n in ("rounds", "trips", "queued_points", "life_cycles")))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
