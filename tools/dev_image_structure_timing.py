"""What K18 buys: structure recovery of a batch of corner lists on the host thread and on the device (MI355X, alone on the chip).

  host_ms      ilcc_chessboard_from_corners image by image on one host thread: what the chains' host route spends per batch
  gpu_ms       ilcc_chessboards_from_corners_batch on ONE plan (two launches; packing, both copies and the wait included)
               both on the same corner lists (K10b's, or constructed ones); host clock around calls that are synchronous on return,
               2 warm-ups, median of 7, the two routes alternating in one process, outputs compared
  chain        the whole ilcc_bag_corners_all_images call on a --chain-images-image bag with structure="host" and "gpu" alternating,
               host wall clock, median of 5 after one warm-up each; recovery_ms is host_recovery_ms of the median run's route

    python tools/dev_image_structure_timing.py --out profiles/r21_image_structure_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # render_board, the constructed cases and the only bag WRITER of the repository
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dev_image_sequence_timing import images_of   # noqa: E402 -- the image sets of the K10b table


def legs(lists, board=(7, 5), runs=7):
    import torch
    from lidar_camera_calibration_amd import _native as N
    from lidar_camera_calibration_amd import image_corners as IC
    from lidar_camera_calibration_amd import image_sequence as IS
    n, longest = len(lists), max(len(c) for c in lists)
    plan = IS.StructurePlan(n, max(longest, 1))

    def host():
        out = []
        for c in lists:
            try:
                out.append(IC.chessboard_from_corners(c, board))
            except IC.BoardNotFound as e:
                out.append(e.status)
        return out

    def gpu():
        status, boards = IS.chessboards_from_corners_batch(lists, board, plan=plan)
        return [b if s == N.OK else int(s) for s, b in zip(status, boards)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        timed.out = fn()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        timed(host)
        timed(gpu)
    a, b = [], []
    for _ in range(runs):
        a.append(timed(host))
        want = timed.out
        b.append(timed(gpu))
        got = timed.out
        assert len(want) == len(got) and all(np.array_equal(w, g) for w, g in zip(want, got)), "the routes differ"
    res = {"images": n, "corners": int(sum(len(c) for c in lists)), "corners_max": longest, "boards_found": sum(not isinstance(w, int) for w in want),
           "host_ms": statistics.median(a), "gpu_ms": statistics.median(b), "host_ms_range": [min(a), max(a)], "gpu_ms_range": [min(b), max(b)],
           "launches": plan.launches, "fallbacks": plan.fallbacks, "plan_allocations": plan.allocations}
    plan.close()
    return res


def chain(images, runs=5):
    import camera_image_ref as CR
    import rosbag_writer as W
    from lidar_camera_calibration_amd import image_sequence as IS
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "images.bag")
    bag = W.BagWriter(path, "none")
    msgs = [("/camera/image_raw", CR.IMAGE_TYPE, CR.IMAGE_MD5, (100 + k // 10, (k % 10) * 100000000),
             CR.image_msg(im, "mono8", seq=k, stamp=(100 + k // 10, (k % 10) * 100000000))) for k, im in enumerate(images)]
    for k in range(0, len(msgs), 8):
        bag.add_chunk(msgs[k:k + 8])
    bag.write()

    def run(route):
        t0 = time.perf_counter()
        out, records = IS.bag_corners_all_images(path, "/camera/image_raw", None, (7, 5), structure=route)
        return (time.perf_counter() - t0) * 1e3, out, records

    ms = {"host": [], "gpu": []}
    for route in ms:
        run(route)
    for _ in range(runs):
        for route in ms:
            ms[route].append(run(route))
    res = {"images": len(images), "width": images[0].shape[1], "height": images[0].shape[0], "bag_bytes": os.path.getsize(path)}
    records = {}
    for route, got in ms.items():
        got.sort(key=lambda r: r[0])
        t, out, records[route] = got[len(got) // 2]
        res[route] = {"chain_ms": t, "chain_ms_range": [got[0][0], got[-1][0]], "recovery_ms": out.host_recovery_ms, "status": out.status, "n_ok": out.n_ok,
                      "n_used": out.n_used, "n_batches": out.n_batches}
    res["records_equal"] = [bytes(r) for r in records["host"]] == [bytes(r) for r in records["gpu"]]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--chain-images", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import structure_cases as S
    from lidar_camera_calibration_amd import image_sequence as IS
    full = images_of((1920, 1200), args.images, square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    crop = images_of((702, 629), max(args.images, args.chain_images), square=60.0, theta=0.2, seed=12)
    out = {"full_frame": legs(IS.find_corners_batch(full)), "crop": legs(IS.find_corners_batch(crop[:args.images])),
           "chain_lists": legs(IS.find_corners_batch(crop[:args.chain_images])),
           "cluttered": legs([S.case("J").corners] * args.images, runs=5),          # 1 200 strays + a 7 x 5 board, tests/structure_cases.py
           "lattice_16x16": legs([S.case("M").corners] * 8, board=(16, 16), runs=5),
           "chain": chain(crop[:args.chain_images]),
           "method": "host clock around calls that are synchronous on return, 2 warm-ups, median of 7 (5 on the constructed lists), routes alternating, "
                     "outputs compared; chain: host wall clock, median of 5 after one warm-up per route, routes alternating"}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
