"""What batching findCorners buys, on --images images of one size (MI355X, alone on the chip).

  loop_ms      leg (a), all the library offered before K10b: ilcc_image_corners_device image by image (per image one hipMalloc /
               hipFree, twice with candidates, three host waits, a host sort and a re-upload)
  batch_ms     leg (b): ilcc_image_corners_batch_device on ONE plan (at most eight launches, two host waits)
               both on the same device images; host clock around work that ends in a synchronise (both entries are synchronous on
               return), 2 warm-ups, median of 10, the two legs alternating in one process, outputs compared byte for byte
  chain_ms     the whole ilcc_bag_corners_all_images call on a --chain-images-image bag (bag read, staging, copies, K11, K10b, structure
               recovery, fusion), host wall clock, median of 3; recovery_ms is the share the host spends in structure recovery

    python tools/dev_image_sequence_timing.py --out profiles/r14_image_sequence_timing.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # render_board, image_msg and the only bag WRITER of the repository


def images_of(size, n, **render):
    """n images of ONE rendered board (noise-free), each with its own sensor noise"""
    from test_image_corners import render_board
    base, _ = render_board(size, noise=0.0, **render)
    out = []
    for k in range(n):
        rng = np.random.default_rng(100 + k)
        out.append(np.clip(np.rint(base + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8))
    return out


def legs(images, capacity=4096):
    import torch
    from lidar_camera_calibration_amd import image_corners as IC
    from lidar_camera_calibration_amd import image_sequence as IS
    L = IS.lib()
    IC.lib()
    n, (h, w) = len(images), images[0].shape
    t = torch.from_numpy(np.stack(images)).cuda()
    out_a, out_b = np.zeros((n, capacity), IC.CORNER_DTYPE), np.zeros((n, capacity), IC.CORNER_DTYPE)
    cnt_a, cnt_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
    i32p = C.POINTER(C.c_int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = IS.CornerPlan(n, w, h)

    def loop():
        for m in range(n):
            one = C.c_int32(0)
            st = L.ilcc_image_corners_device(C.c_void_p(t.data_ptr() + m * w * h), w, h, w, C.c_void_p(out_a.ctypes.data + m * out_a.strides[0]), capacity,
                                             C.byref(one), None, stream)
            assert st == 0
            cnt_a[m] = one.value

    def batch():
        st = L.ilcc_image_corners_batch_device(C.c_void_p(t.data_ptr()), w * h, n, w, h, w, out_b.ctypes.data_as(C.c_void_p), capacity,
                                               cnt_b.ctypes.data_as(i32p), plan._p, stream)
        assert st == 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                      # synchronous on return
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        timed(loop)
        timed(batch)
    a, b = [], []
    for _ in range(10):
        a.append(timed(loop))
        b.append(timed(batch))
    assert list(cnt_a) == list(cnt_b) and all(out_a[m, :cnt_a[m]].tobytes() == out_b[m, :cnt_b[m]].tobytes() for m in range(n))
    cand, off = plan.candidates(n)
    res = {"images": n, "width": w, "height": h, "loop_ms": statistics.median(a), "batch_ms": statistics.median(b),
           "loop_ms_range": [min(a), max(a)], "batch_ms_range": [min(b), max(b)], "candidates": int(off[-1]), "corners": int(cnt_b.sum()),
           "batch_launches": plan.launches, "plan_allocations": plan.allocations}
    plan.close()
    return res


def chain(images):
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

    def run():
        t0 = time.perf_counter()
        out, _ = IS.bag_corners_all_images(path, "/camera/image_raw", None, (7, 5))
        run.out = out
        return (time.perf_counter() - t0) * 1e3

    run()
    ms = statistics.median(run() for _ in range(3))
    out = run.out
    h, w = images[0].shape
    return {"images": len(images), "width": w, "height": h, "bag_bytes": os.path.getsize(path), "chain_ms": ms, "recovery_ms": out.host_recovery_ms,
            "status": out.status, "n_ok": out.n_ok, "n_used": out.n_used, "n_batches": out.n_batches, "spread_rms_px": out.spread_rms,
            "spread_max_px": out.spread_max}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--chain-images", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    full = images_of((1920, 1200), args.images, square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)   # test_synthetic_full_frame's render
    crop = images_of((702, 629), max(args.images, args.chain_images), square=60.0, theta=0.2, seed=12)                      # the size of the pointgrey2 crop
    out = {"full_frame": legs(full), "crop": legs(crop[:args.images]), "chain": chain(crop[:args.chain_images]),
           "method": "host clock around calls that are synchronous on return, 2 warm-ups, median of 10, legs alternating, outputs equal byte for byte; "
                     "chain: host wall clock, median of 3 after one warm-up"}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
