"""What batching the unpack buys, on a synthetic VLP-16 bag of --scans scans whose point counts differ (MI355X, alone on the chip).

  per_message_ms   leg (a), the way before K0b: per message one H2D copy of its data[] and one K0 launch
  batched_ms       leg (b): ONE H2D copy of the staged blob, then K0b
                   both from the same page-locked blob into the same device buffers, on ONE stream, HIP events around the whole
                   leg, 2 warm-ups, median of 10; the outputs of the two legs are compared byte for byte
  chain_ms         the whole ilcc_bag_corners_all_scans call, host wall clock (bag read, inflate, stage, copies, K0b, pipeline, fusion)
  read_inflate_ms  the host time to read and inflate every message of the same bag through the iterator alone

    python tools/dev_sequence_timing.py --scans 256 --out profiles/r11_sequence_timing.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))   # rosbag_writer: the only bag WRITER of the repository


def write_bag(path, scans):
    import rosbag_writer as W
    from lidar_camera_calibration_amd import synth
    board, pose = synth.Board(), synth.pose_from_fixture(0)
    base = [synth.make_frame(synth.vlp16(), board, pose, 0x5EC + k) for k in range(8)]
    w = W.BagWriter(path, "lz4")
    msgs = []
    for k in range(scans):
        cloud = base[k % len(base)]
        cloud = cloud[:len(cloud) - (k * 37) % 500]              # real scans differ in point count
        a, fields, step = W.velodyne_points(cloud)
        tm = (100 + k // 10, (k % 10) * 100000000)
        msgs.append(("/velodyne_points", "sensor_msgs/PointCloud2", W.POINTCLOUD2_MD5, tm, W.pointcloud2(a, fields, step, seq=k, stamp=tm)))
    for k in range(0, scans, 8):
        w.add_chunk(msgs[k:k + 8])
    w.write()
    return synth.make_click(pose, 0x5EC)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    bag = os.path.join(tmp, "sequence.bag")
    click = write_bag(bag, args.scans)

    import torch
    from lidar_camera_calibration_amd import LidarCornersBatch, ingest, sequence
    L = sequence.lib()

    # the host alone: every message read and inflated once, in order (what the chain does after open)
    def read_all(keep):
        t = time.perf_counter()
        with sequence.BagTopic(bag, "/velodyne_points") as it:
            buf = (C.c_uint8 * max(it.size(i) for i in range(len(it))))()
            n = C.c_uint64(0)
            for i in range(len(it)):
                st = L.ilcc_bag_topic_read(it._it, i, buf, len(buf), C.byref(n))
                assert st == 0
                if keep is not None:
                    keep.append(bytes(buf[:n.value]))
        return (time.perf_counter() - t) * 1e3

    msgs = []
    read_all(msgs)
    read_ms = statistics.median(read_all(None) for _ in range(3))

    # the staged blob, as the chain lays it out: data[] at 16-byte aligned offsets in page-locked memory
    layouts = [ingest.parse_pointcloud2(m) for m in msgs]
    src, at = [], 0
    for lay in layouts:
        at = (at + 15) // 16 * 16
        src.append(at)
        at += lay.data_bytes
    blob = torch.empty(at, dtype=torch.uint8).pin_memory()
    for m, lay, o in zip(msgs, layouts, src):
        blob[o:o + lay.data_bytes] = torch.frombuffer(bytearray(m[lay.data_offset:lay.data_offset + lay.data_bytes]), dtype=torch.uint8)
    points = sum(lay.n_points for lay in layouts)
    d_blob = torch.empty(at, dtype=torch.uint8, device="cuda")
    out_a = torch.zeros(16 * points, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros(16 * points, dtype=torch.uint8, device="cuda")
    offs = np.concatenate([[0], np.cumsum([lay.n_points for lay in layouts])])
    plan = sequence.UnpackPlan(len(msgs))
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def per_message():
        for lay, o, p in zip(layouts, src, offs):
            d_blob[o:o + lay.data_bytes].copy_(blob[o:o + lay.data_bytes], non_blocking=True)
            ingest.unpack_device(d_blob.data_ptr() + o, lay, out_a.data_ptr() + 16 * int(p), s)

    def batched():
        d_blob.copy_(blob, non_blocking=True)
        sequence.unpack_batch_device(d_blob.data_ptr(), at, layouts, src, out_b.data_ptr(), points, plan, s)

    def med(fn):
        for _ in range(2):
            timed(fn)
        return statistics.median(timed(fn) for _ in range(10))

    a_ms, b_ms = med(per_message), med(batched)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)
    launches = plan.launches
    plan.close()

    est = LidarCornersBatch(args.scans, max(lay.n_points for lay in layouts))
    est.reserve(2000, 2500)

    def chain():
        t = time.perf_counter()
        res, _ = sequence.bag_corners_all_scans(est, bag, "/velodyne_points", click, per_scan=False)
        chain.res = res
        return (time.perf_counter() - t) * 1e3

    chain()
    chain_ms = statistics.median(chain() for _ in range(3))
    res = chain.res
    out = {"scans": args.scans, "points": int(points), "blob_bytes": int(at), "bag_bytes": os.path.getsize(bag),
           "per_message_ms": a_ms, "batched_ms": b_ms, "k0b_launches": launches, "per_message_launches": len(msgs),
           "chain_ms": chain_ms, "read_inflate_ms": read_ms,
           "chain": {"status": res.status, "n_ok": res.n_ok, "n_used": res.n_used, "n_batches": res.n_batches,
                     "spread_rms_mm": res.spread_rms * 1e3, "spread_max_mm": res.spread_max * 1e3},
           "method": "HIP events on one stream around each leg, 2 warm-ups, median of 10, identical inputs; chain and read: host wall clock, median of 3"}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    est.close()


if __name__ == "__main__":
    main()
