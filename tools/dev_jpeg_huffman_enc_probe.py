"""What encoding the Huffman scans on the GPU (K17, include/ilcc_jpeg_write_sequence.h) costs and buys, on --images frames of
1920 x 1200 gray (the frames of tools/dev_image_sequence_timing.py), MI355X, alone on the chip.

  batch_ms     K14b + K17 on the frames already in device memory, by events around the two entries on the current stream, 2
               warm-ups, median of --repeats; K14b and K17 alone likewise.  Every scan is compared with ilcc_jpeg_entropy_encode's
               byte for byte once.
  single_ms    the single-image way for the same frames in the same process: per image K14, the coefficients device to host,
               ilcc_jpeg_entropy_encode on one core; host wall clock over all frames, median of 3 after one warm-up, and its parts
  d2h_bytes    what comes back from the device on either route
  chain_ms     the whole ilcc_bag_save_jpeg_all call on a bag of the frames as sensor_msgs/Image, host wall clock, median of 3 after
               one warm-up, route 0 (K17) and route 1 (the host encoder); the files are compared

    python tools/dev_jpeg_huffman_enc_probe.py --out profiles/r19_jpeg_huffman_enc_probe.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))   # render_board, the message writer and the only bag WRITER of the repository
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dev_image_sequence_timing import images_of        # noqa: E402


def events_ms(run, repeats):
    import torch
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms": statistics.median(ms), "ms_range": [min(ms), max(ms)]}


def kernels(frames, quality, repeats):
    import torch
    from lidar_camera_calibration_amd import jpeg_write
    from lidar_camera_calibration_amd import jpeg_write_sequence as S
    n, (h, w) = len(frames), frames[0].shape
    info = jpeg_write.write_info(w, h, None, quality, 0)
    count = int(info.coef_count)
    px = torch.from_numpy(np.stack(frames)).cuda()
    coef = torch.zeros((n, count), dtype=torch.int16, device="cuda")
    out_cap = n * w * h
    out = torch.zeros(out_cap, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(S.huffman_encode_scratch_bytes(info, n, out_cap), dtype=torch.uint8, device="cuda")

    def k14b():
        S.fdct_batch(info, px, coef_pitch=count, out=coef)

    def k17():
        S.huffman_encode_batch(info, coef.data_ptr(), count, n, out.data_ptr(), out_cap, rows.data_ptr(), scratch.data_ptr(), scratch.numel())

    def both():
        k14b()
        k17()

    res = {"images": n, "width": w, "height": h, "quality": quality, "k14b": events_ms(k14b, repeats), "k17": events_ms(k17, repeats),
           "k14b_k17": events_ms(both, repeats)}
    got = rows.cpu().numpy().view(S.ROW_DTYPE)
    assert not got["status"].any()
    span = int(got["offset"][-1] + got["bytes"][-1])
    scans = out[:span].cpu().numpy()
    res["d2h_bytes_route_0"] = 16 * n + span
    res["d2h_bytes_route_1"] = 2 * count * n
    res["scan_bytes"] = int(got["bytes"].sum())

    # the single-image way, and the check of every scan against it
    head = S.write_headers(info)
    one = torch.zeros(count, dtype=torch.int16, device="cuda")
    host = torch.zeros(count, dtype=torch.int16).pin_memory()
    parts = {"k14_and_d2h_ms": 0.0, "entropy_encode_ms": 0.0}

    def single(check):
        t_all = time.perf_counter()
        parts["k14_and_d2h_ms"] = parts["entropy_encode_ms"] = 0.0
        for m in range(n):
            t0 = time.perf_counter()
            jpeg_write.fdct(info, px[m], out=one)
            host.copy_(one)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            data = jpeg_write.entropy_encode(info, host.numpy())
            parts["k14_and_d2h_ms"] += (t1 - t0) * 1e3
            parts["entropy_encode_ms"] += (time.perf_counter() - t1) * 1e3
            if check:
                r = got[m]
                assert data == head + scans[int(r["offset"]):int(r["offset"]) + int(r["bytes"])].tobytes() + S.EOI, m
        return (time.perf_counter() - t_all) * 1e3

    single(True)
    ms = [single(False) for _ in range(3)]
    res["single"] = {"ms": statistics.median(ms), "ms_range": [min(ms), max(ms)], "k14_and_d2h_ms": parts["k14_and_d2h_ms"],
                     "entropy_encode_ms": parts["entropy_encode_ms"]}
    return res


def chain(frames, quality):
    import image_sequence_cases as K
    from lidar_camera_calibration_amd import jpeg_write_sequence as S
    tmp = tempfile.mkdtemp()
    msgs = [K.CR.image_msg(f, "mono8", seq=k, stamp=(100 + k // 10, (k % 10) * 100000000)) for k, f in enumerate(frames)]
    path = K.write_bag(os.path.join(tmp, "frames.bag"), msgs, per_chunk=8)
    res, files = {"images": len(frames)}, []
    for name, route in (("route_0_k17", "gpu"), ("route_1_host", "host")):
        prefix = os.path.join(tmp, name + "_")

        def run():
            t0 = time.perf_counter()
            run.got = S.bag_save_jpeg_all(path, K.TOPIC, None, prefix, quality, huffman=route)
            return (time.perf_counter() - t0) * 1e3
        run()
        ms = [run() for _ in range(3)]
        out, records = run.got
        files.append([open("%s%06d.jpg" % (prefix, r.message), "rb").read() for r in records])
        res[name] = {"chain_ms": statistics.median(ms), "chain_ms_range": [min(ms), max(ms)], "n_batches": out.n_batches, "d2h_bytes": int(out.d2h_bytes),
                     "file_bytes": int(out.file_bytes), "n_host_encoded": out.n_host_encoded}
    assert files[0] == files[1], "the routes' files differ"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    frames = images_of((1920, 1200), args.images, square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    out = {"method": "kernels: events around the entries, 2 warm-ups, median of %d, every scan equal to the host encoder's; single and chain: host "
                     "wall clock, median of 3 after one warm-up, files equal on both routes" % args.repeats}
    out["kernels"] = kernels(frames, args.quality, args.repeats)
    out["chain"] = chain(frames, args.quality)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
