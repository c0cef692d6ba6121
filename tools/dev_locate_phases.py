"""Where k6_locate's wavefront cycles go: staging, seed, refinement, the anchor's copy to LDS, the anchor's walk -- for 1024-frame
config-2 batches alone on the chip, and again inside the depth-4 pipeline.
Build the instrumented library first (tools/build_variant.sh k6timing -DILCC_K6_TIMING) and run on the GPU box:
    ILCC_HIP_LIB=build/ab/libilcc_hip_k6timing.so python tools/dev_locate_phases.py [out.json]"""
import ctypes as C
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import torch
from lidar_camera_calibration_amd import LidarCornersBatch
from lidar_camera_calibration_amd import _native as N

F, n_points, DEPTH = 1024, 28800, 4
clouds, clicks, _ = bench.generate(2, F, 0xC0FFEE, 16)
d_cloud, d_click = torch.from_numpy(clouds).cuda(), torch.from_numpy(clicks).cuda()
est = LidarCornersBatch(F, n_points, N.default_params(), device=0)
est.set_result_mode(N.RESULTS_COMPACT)
est.reserve(1792, 2560)
lib = N.lib()
prof = (C.c_ulonglong * 8)()
NAMES = ("staging", "seed", "refinement", "anchor_copy", "anchor_walk")


def run(n, depth):
    inflight = []
    for _ in range(n):
        inflight.append(est.submit_device(d_cloud.data_ptr(), F, n_points, d_click.data_ptr()))
        if len(inflight) == depth:
            est.wait_compact(inflight.pop(0))
    while inflight:
        est.wait_compact(inflight.pop(0))


def phases(depth, batches):
    run(8, depth)
    torch.cuda.synchronize()
    assert lib.ilcc_debug_k6_locate_profile(prof, 1) == 0
    run(batches, depth)
    torch.cuda.synchronize()
    assert lib.ilcc_debug_k6_locate_profile(prof, 1) == 0
    p = [float(x) for x in prof]
    waves, life = p[0], p[6]   # (one record per wavefront slot: the last batch that wrote it)
    out = {"depth": depth, "wavefronts": waves, "mean_life_cycles": life / waves}
    for k, name in enumerate(NAMES):
        out[name + "_cycles"] = p[1 + k] / waves
        out[name + "_share"] = p[1 + k] / life
    return out


res = {"frames": F, "config": 2, "lib": os.path.basename(os.environ.get("ILCC_HIP_LIB", "(in-tree)")), "alone": phases(1, 4), "pipeline_depth4": phases(DEPTH, 24)}
for key in ("alone", "pipeline_depth4"):
    r = res[key]
    print("%-16s life %8.0f cycles/wavefront: " % (key, r["mean_life_cycles"]) + ", ".join("%s %.1f %%" % (n, 100 * r[n + "_share"]) for n in NAMES))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
