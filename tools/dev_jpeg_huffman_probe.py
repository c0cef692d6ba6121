"""What decoding the Huffman scans on the GPU (K16, include/ilcc_jpeg_huffman.h) costs and buys, on the four image kinds of
tools/dev_jpeg_sequence_timing.py (1920 x 1200 and 702 x 629, gray and 4:2:0; --images frames), MI355X, alone on the chip.

  k16_ms       K16 alone on a batch already in device memory, by events around the entry on the current stream, 2 warm-ups, median
               of --repeats, at S = 256, 512, 1024, 2048; the coefficients are compared with ilcc_jpeg_entropy_decode_many's byte for
               byte once per S.  rounds: the most rounds any chunk of the batch took, and the mean per chunk.
  pointgrey    the same for the six camera frames tests/golden/jpeg/pointgrey1..6.jpg (1920 x 1200 gray) as one batch
  flat         the same for ONE flat 1920 x 1200 gray frame at quality 90: the decoder never synchronises, every chunk takes its
               bound of rounds
  chain_ms     the whole ilcc_bag_corners_all_compressed_images call, host wall clock, median of 3 after one warm-up: route 0 with 1
               and 8 decode threads against route 1, on a --chain-images bag of 702 x 629 and on a bag of --images full frames, all
               measured in this one process on this one build
  h2d_bytes    what the one H2D copy of a batch moves on either route (ilcc_jpeg_sequence_bytes / ilcc_jpeg_huffman_sequence_bytes)

    python tools/dev_jpeg_huffman_probe.py --out profiles/r18_jpeg_huffman_probe.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))   # render_board, the message writer and the only bag WRITER of the repository
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dev_image_sequence_timing import images_of        # noqa: E402
from dev_jpeg_sequence_timing import encoded           # noqa: E402


def k16_alone(jpgs, repeats, check=True):
    import torch
    from lidar_camera_calibration_amd import jpeg
    from lidar_camera_calibration_amd import jpeg_huffman as JH
    from lidar_camera_calibration_amd import jpeg_sequence as JS
    infos = [jpeg.parse(j) for j in jpgs]
    b = JH.Batch([JH.scan_prepare(j, i) for j, i in zip(jpgs, infos)])
    layout, n = infos[0], len(jpgs)
    pitch = (int(layout.coef_count) + 127) // 128 * 128
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("scans", b.scans), ("tables", b.tables), ("segments", b.segments), ("images", b.images))}
    coef = torch.zeros((n, pitch), dtype=torch.int16, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(max(JH.scratch_bytes(n), 16), dtype=torch.uint8, device="cuda")
    want = np.stack(JS.entropy_decode_many(jpgs, 8)[0]) if check else None
    out = {"images": n, "width": layout.width, "height": layout.height, "components": layout.n_components, "scan_bytes": int(b.scans_bytes)}
    for bits in JH.SUBSEQUENCE_BITS:
        def run():
            JH.huffman_batch(layout, dev["scans"].data_ptr(), b.scans_bytes, dev["tables"].data_ptr(), dev["segments"].data_ptr(), b.n_segments,
                             dev["images"].data_ptr(), n, b.max_segments, coef.data_ptr(), pitch, status.data_ptr(), scratch.data_ptr(), scratch.numel(), bits)
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
        assert not status.any().item()
        if check:
            assert np.array_equal(coef[:, :int(layout.coef_count)].cpu().numpy(), want), bits
        c = scratch.cpu().numpy()[:16 * n].view(np.uint32).reshape(n, 4)
        out["S_%d" % bits] = {"k16_ms": statistics.median(ms), "k16_ms_range": [min(ms), max(ms)], "chunks": int(c[:, 1].sum()),
                              "rounds_per_chunk_mean": float(c[:, 2].sum()) / max(int(c[:, 1].sum()), 1), "rounds_per_chunk_max": int(c[:, 3].max())}
    return out


def chain(jpgs):
    import image_sequence_cases as K
    import jpeg_ref as R
    from lidar_camera_calibration_amd import jpeg
    from lidar_camera_calibration_amd import jpeg_huffman as JH
    from lidar_camera_calibration_amd import jpeg_sequence as JS
    tmp = tempfile.mkdtemp()
    msgs = [R.compressed_image_msg(j, "jpeg", seq=k, stamp=(100 + k // 10, (k % 10) * 100000000)) for k, j in enumerate(jpgs)]
    path = K.write_bag(os.path.join(tmp, "compressed.bag"), msgs, per_chunk=8, conn=("sensor_msgs/CompressedImage", R.COMPRESSED_IMAGE_MD5))
    infos = [jpeg.parse(j) for j in jpgs]
    res = {"images": len(jpgs), "width": infos[0].width, "height": infos[0].height, "components": infos[0].n_components,
           "h2d_bytes_route_0": len(jpgs) * JS.sequence_bytes(infos[0])[0],
           "h2d_bytes_route_1": sum(JH.sequence_bytes(i, len(j), JH.scan_bound(i, len(j))[1])[0] for i, j in zip(infos, jpgs))}
    summaries = []
    for name, kw in (("route_0_1_thread", dict(decode_threads=1)), ("route_0_8_threads", dict(decode_threads=8)),
                     ("route_1_1_thread", dict(decode_threads=1, huffman="gpu")), ("route_1_8_threads", dict(decode_threads=8, huffman="gpu"))):
        def run():
            t0 = time.perf_counter()
            run.got = JS.bag_corners_all_compressed_images(path, K.TOPIC, None, (7, 5), raise_on_failure=False, **kw)
            return (time.perf_counter() - t0) * 1e3
        run()
        ms = [run() for _ in range(3)]
        out, records = run.got
        summaries.append((out.status, out.n_ok, out.n_used, out.board().tobytes(), [bytes(r) for r in records]))
        res[name] = {"chain_ms": statistics.median(ms), "chain_ms_range": [min(ms), max(ms)], "status": out.status, "n_ok": out.n_ok, "n_batches": out.n_batches}
    assert all(s == summaries[0] for s in summaries), "the routes' records differ"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--chain-images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from lidar_camera_calibration_amd import jpeg_write
    full = images_of((1920, 1200), args.images, square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    crop = images_of((702, 629), max(args.images, args.chain_images), square=60.0, theta=0.2, seed=12)
    out = {"method": "K16: events around the entry, 2 warm-ups, median of %d, coefficients equal the host decoder's; chain: host wall clock, "
                     "median of 3 after one warm-up, records equal on every route" % args.repeats}
    for name, colour in (("gray", False), ("colour_420", True)):
        big, small = encoded(full, colour), encoded(crop, colour)
        out["k16_full_frame_" + name] = k16_alone(big, args.repeats)
        out["k16_crop_" + name] = k16_alone(small[:args.images], args.repeats)
        out["chain_crop_" + name] = chain(small[:args.chain_images])
        out["chain_full_frame_" + name] = chain(big)
    golden = os.path.join(ROOT, "tests", "golden", "jpeg")
    out["k16_pointgrey"] = k16_alone([open(os.path.join(golden, "pointgrey%d.jpg" % i), "rb").read() for i in range(1, 7)], args.repeats)
    out["k16_flat_full_frame_gray"] = k16_alone([jpeg_write.encode(np.full((1200, 1920), 128, np.uint8), 90)], args.repeats)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
