"""What batching the JPEG decode buys, on --images JPEG frames of one size, gray and 4:2:0 colour (MI355X, alone on the chip).

  loop_ms      leg (a), all the library offered before K13b: ilcc_jpeg_decode_device image by image (per image a parse, a serial
               Huffman decode on the calling thread, one hipMalloc / hipFree, a pageable hipMemcpy, one or four launches, a wait)
  batch_ms     leg (b): ilcc_jpeg_entropy_decode_many into ONE page-locked buffer, one H2D copy of coefficients and tables, K13b
               (one or two launches), a wait; with 1 and with 8 decode threads.  decode_ms is the share of it spent in the pool.
               Both legs write the same device images; host clock around work that ends in a synchronise, 2 warm-ups, median of
               10, the legs alternating in one process, outputs compared byte for byte
  chain_ms     the whole ilcc_bag_corners_all_compressed_images call on a --chain-images-image bag (bag read, parse, pool, copies,
               K13b, K11, K10b, structure recovery, fusion), host wall clock, median of 3, with 1 and 8 decode threads;
               decode_ms is what ilcc_jpeg_entropy_decode_many alone takes on the same files with the same threads

    python tools/dev_jpeg_sequence_timing.py --out profiles/r17_jpeg_sequence_timing.json
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

from dev_image_sequence_timing import images_of   # noqa: E402


def encoded(images, colour):
    from lidar_camera_calibration_amd import jpeg_write
    return [jpeg_write.encode(np.repeat(im[..., None], 3, axis=2) if colour else im, 95, "420") for im in images]


class Jobs:
    """the arrays ilcc_jpeg_entropy_decode_many takes, built once: the files, their infos, and page-locked room for the
    coefficients of all of them followed by their table rows"""

    def __init__(self, jpgs):
        import torch
        from lidar_camera_calibration_amd import jpeg
        from lidar_camera_calibration_amd import jpeg_sequence as JS
        self.n = n = len(jpgs)
        self.infos = [jpeg.parse(j) for j in jpgs]
        self.layout = jpeg.make_info(self.infos[0].width, self.infos[0].height, None if self.infos[0].n_components == 1 else "420")
        self.pitch = (self.layout.coef_count + 127) // 128 * 128
        self.host = torch.empty(n * self.pitch + n * 192, dtype=torch.int16).pin_memory()
        self.host[n * self.pitch:] = torch.from_numpy(np.concatenate([JS.quant_rows(i).reshape(-1) for i in self.infos]).view(np.int16))
        self.bufs = [np.frombuffer(j, np.uint8) for j in jpgs]
        self.jp = (C.c_void_p * n)(*[b.ctypes.data for b in self.bufs])
        self.nb = (C.c_uint64 * n)(*[b.size for b in self.bufs])
        self.cp = (C.c_void_p * n)(*[self.host.data_ptr() + 2 * self.pitch * m for m in range(n)])
        self.cap = (C.c_uint64 * n)(*[self.layout.coef_count] * n)
        self.info = (jpeg.Info * n)(*self.infos)
        self.status = (C.c_int32 * n)()

    def decode(self, threads):
        from lidar_camera_calibration_amd import jpeg_sequence as JS
        st = JS.lib().ilcc_jpeg_entropy_decode_many(self.jp, self.nb, self.info, self.cp, self.cap, self.n, threads, self.status)
        assert st == 0


def legs(jpgs):
    import torch
    from lidar_camera_calibration_amd import jpeg
    from lidar_camera_calibration_amd import jpeg_sequence as JS
    J = Jobs(jpgs)
    n, lay = J.n, J.layout
    w, h, bpp = lay.width, lay.height, 1 if lay.n_components == 1 else 3
    out_a = torch.zeros((n, h, w * bpp), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros_like(out_a)
    dev = torch.empty_like(J.host, device="cuda")
    scratch = torch.empty(max(JS.batch_scratch_bytes(lay, n), 16), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arrs = [(C.c_uint8 * len(j)).from_buffer_copy(j) for j in jpgs]
    L = jpeg.lib()
    decode_ms = {}

    def loop():
        ww, hh, enc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        for m in range(n):
            st = L.ilcc_jpeg_decode_device(arrs[m], len(jpgs[m]), C.c_void_p(out_a.data_ptr() + m * w * h * bpp), w * bpp, w * h * bpp, C.byref(ww),
                                           C.byref(hh), C.byref(enc), stream)
            assert st == 0

    def batch(threads):
        def run():
            t0 = time.perf_counter()
            J.decode(threads)
            decode_ms.setdefault(threads, []).append((time.perf_counter() - t0) * 1e3)
            dev.copy_(J.host, non_blocking=True)
            st = JS.lib().ilcc_jpeg_idct_batch_device(C.byref(lay), C.c_void_p(dev.data_ptr() + 2 * n * J.pitch), C.c_void_p(dev.data_ptr()), J.pitch, n,
                                                      C.c_void_p(out_b.data_ptr()), w * h * bpp, w * bpp, C.c_void_p(scratch.data_ptr()), scratch.numel(), stream)
            assert st == 0
            torch.cuda.synchronize()
        return run

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    b1, b8 = batch(1), batch(8)
    for _ in range(2):
        timed(loop), timed(b1), timed(b8)
    decode_ms.clear()
    a, t1, t8 = [], [], []
    for _ in range(10):
        a.append(timed(loop))
        t1.append(timed(b1))
        assert torch.equal(out_a, out_b)
        out_b.zero_()
        t8.append(timed(b8))
        assert torch.equal(out_a, out_b)
        out_b.zero_()
    med = statistics.median
    return {"images": n, "width": w, "height": h, "components": lay.n_components, "jpeg_bytes": int(sum(len(j) for j in jpgs)),
            "loop_ms": med(a), "loop_ms_range": [min(a), max(a)],
            "batch_1_thread_ms": med(t1), "batch_1_thread_ms_range": [min(t1), max(t1)], "decode_1_thread_ms": med(decode_ms[1]),
            "batch_8_threads_ms": med(t8), "batch_8_threads_ms_range": [min(t8), max(t8)], "decode_8_threads_ms": med(decode_ms[8])}


def chain(jpgs):
    import image_sequence_cases as K
    import jpeg_ref as R
    from lidar_camera_calibration_amd import jpeg_sequence as JS
    tmp = tempfile.mkdtemp()
    msgs = [R.compressed_image_msg(j, "jpeg", seq=k, stamp=(100 + k // 10, (k % 10) * 100000000)) for k, j in enumerate(jpgs)]
    path = K.write_bag(os.path.join(tmp, "compressed.bag"), msgs, per_chunk=8, conn=("sensor_msgs/CompressedImage", R.COMPRESSED_IMAGE_MD5))
    J = Jobs(jpgs)
    res = {"images": len(jpgs), "width": J.layout.width, "height": J.layout.height, "components": J.layout.n_components,
           "bag_bytes": os.path.getsize(path)}
    for threads in (1, 8):
        def run():
            t0 = time.perf_counter()
            out, _ = JS.bag_corners_all_compressed_images(path, K.TOPIC, None, (7, 5), decode_threads=threads)
            run.out = out
            return (time.perf_counter() - t0) * 1e3

        def decode():
            t0 = time.perf_counter()
            J.decode(threads)
            return (time.perf_counter() - t0) * 1e3

        run()
        decode()
        out = run.out
        res["threads_%d" % threads] = {"chain_ms": statistics.median(run() for _ in range(3)), "decode_ms": statistics.median(decode() for _ in range(3)),
                                       "recovery_ms": out.host_recovery_ms, "status": out.status, "n_ok": out.n_ok, "n_used": out.n_used,
                                       "n_batches": out.n_batches}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--chain-images", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    full = images_of((1920, 1200), args.images, square=90.0, theta=0.2, centre=(1100, 540), persp=(5e-5, -4e-5), seed=11)
    crop = images_of((702, 629), max(args.images, args.chain_images), square=60.0, theta=0.2, seed=12)
    out = {"method": "host clock around work that ends in a synchronise, 2 warm-ups, median of 10, legs alternating, outputs equal byte for byte; "
                     "chain: host wall clock, median of 3 after one warm-up"}
    for name, colour in (("gray", False), ("colour_420", True)):
        out["full_frame_" + name] = legs(encoded(full, colour))
        small = encoded(crop, colour)
        out["crop_" + name] = legs(small[:args.images])
        out["chain_" + name] = chain(small[:args.chain_images])
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
