"""The live (frame, theta) share of a bench-sized batch, and the full pass's HIP-event span per launch form (ilcc_debug_full_pass_launch):
the (n_th, F) grid, the rule, and the listed launch at several G around the live count.  Synchronous batches, one alone on the chip,
12 batches per figure, three rounds of all the variants in turn.
usage: python tools/dev_full_pass_forms.py [config=2|5|2c] [out.json]     (2c: every workgroup alive, for the rule's "near the full grid" threshold)"""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidar_camera_calibration_amd import LidarCornersBatch, synth
from lidar_camera_calibration_amd import _native as N
coarse = len(sys.argv) > 1 and sys.argv[1] == "2c"   # config 2's frames on 21 thetas 3 degrees apart: the common pre-pass rejects nothing, EVERY workgroup is alive
config = 2 if coarse else int(sys.argv[1]) if len(sys.argv) > 1 else 2
params = N.default_params()
if coarse:
    params.n_th, params.th_step, params.th_min = 21, np.pi / 60.0, -np.pi / 6.0
if config == 5:
    F = 128
    lidar = synth.hdl64()
    clouds, clicks, _, _ = synth.make_batch(F, lidar, synth.Board(9, 12, 0.10), seed=0xC0FFEE, range_m=(2.0, 3.0),
                                            yaw_deg=25.0, pitch_deg=15.0, roll_deg=30.0)
    params.board_w, params.board_h, params.grid_length = 9, 12, 0.10
    params.n_th = params.n_ty = params.n_tz = 129
    params.th_min, params.th_step = -16.0 * np.pi / 180.0, 0.25 * np.pi / 180.0
    params.ty_min = params.tz_min = -0.10
    params.ty_step = params.tz_step = 0.10 / 64
    n = lidar.n_points
else:
    F = 1024
    clouds, clicks, _, _ = synth.make_batch(F, seed=0xC0FFEE)
    n = 28800
d_c = torch.from_numpy(clouds).cuda(); d_k = torch.from_numpy(clicks).cuda()
est = LidarCornersBatch(F, n, params)
est.reserve(6400, 20000) if config == 5 else est.reserve(1792, 2560)
full = params.n_th * F
out = {"config": config, "coarse_theta_grid": coarse, "frames": F, "records": full, "runs": []}
for _ in range(3):
    est.extract_device(d_c.data_ptr(), F, n, d_k.data_ptr())
last = est.debug_full_pass_last()
live = last["live"]
out["live"] = live
out["live_share"] = live / full
print("config %d: %d frames, live %d of %d = %.4f; rule after warm-up: %s" % (config, F, live, full, live / full, last), flush=True)
variants = [("grid", N.FULL_PASS_GRID, 0), ("rule", N.FULL_PASS_RULE, 0), ("listed_exact", N.FULL_PASS_LISTED, live),
            ("listed_1/16", N.FULL_PASS_LISTED, live + live // 16), ("listed_1/4", N.FULL_PASS_LISTED, live + live // 4),
            ("listed_half", N.FULL_PASS_LISTED, max(1, live // 2)), ("listed_3/4", N.FULL_PASS_LISTED, max(1, 3 * live // 4)),
            ("listed_full", N.FULL_PASS_LISTED, full)]
for rep in range(3):
    for name, mode, g in variants:
        est.debug_full_pass_launch(mode, g)
        est.reset_timing()
        for _ in range(12):
            est.extract_device(d_c.data_ptr(), F, n, d_k.data_ptr())
        t = est.timing()
        last = est.debug_full_pass_last()
        row = {"variant": name, "rep": rep, "form": last["form"], "workgroups": last["workgroups"], "full_us": 1e3 * t.grid_cost_full_ms_sum / t.batches,
               "prepass_us": 1e3 * t.grid_cost_prepass_ms_sum / t.batches, "total_us": 1e3 * t.stage_ms_sum[6] / t.batches}
        out["runs"].append(row)
        print(row, flush=True)
est.close()
dst = sys.argv[2] if len(sys.argv) > 2 else "full_pass_forms_cfg%s.json" % (sys.argv[1] if len(sys.argv) > 1 else "2")
os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
json.dump(out, open(dst, "w"), indent=1)
