"""Every device entry that takes a `void* hip_stream` (19 declarations in 11 headers under include/), called on a side stream whose
inputs arrive late (tests/stream_contract.py).  Nearly every other GPU test here passes the null stream, which serialises with
everything and so hides a launch or copy queued on the wrong stream, a host argument read after the call returned, a plan's table
overwritten under its previous call, and scratch reused behind a launch that has not run yet.

Each case is compared exactly as the entry's own test compares it: byte equality with the same restatement, sentinels behind every
buffer untouched.  No tolerance is introduced in this file: K10's corners go through test_image_corners.py's own stage comparison
and must then equal the solo run's bytes.  The CPU tests hold the list of entries below against the headers, and every decoy that
can be built without a device against its real output."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import stream_contract as SC
from stream_contract import Buf, Case, SENTINEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = C.c_void_p
DECLARATION = re.compile(r"\b(ilcc_[a-z0-9_]+)\s*\(([^;{}()]*\bvoid\s*\*\s*hip_stream\b[^;{}()]*)\)\s*;")


def declared(include_dir=os.path.join(ROOT, "include")):
    """name -> header of every function declared with a `void* hip_stream` parameter"""
    out = {}
    for path in sorted(glob.glob(os.path.join(include_dir, "*.h"))):
        for m in DECLARATION.finditer(open(path).read()):
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = os.path.basename(path)
    return out


def sentinels(nbytes):
    return np.full(int(nbytes), SENTINEL, np.uint8)


def ok(status):
    from lidar_camera_calibration_amd import _native as N
    assert status == N.OK, (status, N.lib().ilcc_last_error(None).decode())


def overwrite(dst, src):
    """the bytes of one ctypes object over another of the same type, in place"""
    assert C.sizeof(dst) == C.sizeof(src)
    C.memmove(C.addressof(dst), C.addressof(src), C.sizeof(src))


# ---- K0 ------------------------------------------------------------------------------------------------------------------------

def _decoy_message(msg, lay, seed):
    """-> (message, layout): other bytes in data[], x and y taken from each other's offsets; every size as in the real one"""
    from lidar_camera_calibration_amd import ingest
    raw = bytearray(msg)
    rng = np.random.Generator(np.random.Philox(key=seed))
    raw[lay.data_offset:lay.data_offset + lay.data_bytes] = rng.integers(0, 256, lay.data_bytes, dtype=np.uint8).tobytes()
    other = ingest.Layout.from_buffer_copy(lay)
    other.off_x, other.off_y = lay.off_y, lay.off_x
    return bytes(raw), other


def _data(msg, lay):
    return np.frombuffer(msg, np.uint8, lay.data_bytes, lay.data_offset)


def k0_cases(ob=None):
    import rosbag_writer as W
    import test_ingest as TI
    from lidar_camera_calibration_amd import ingest
    xyzi = TI._cloud(1025, 1025)
    xyzi[::7, 0] = np.nan
    raw22 = np.random.default_rng(8).integers(0, 256, (777, 22), dtype=np.uint8)
    for name, msg in (("velodyne 1025", TI._msg(xyzi)),
                      ("22-byte generic 777", W.pointcloud2(raw22, [("z", 1, 7, 1), ("x", 9, 7, 1), ("y", 17, 7, 1)], 22))):
        lay = ingest.parse_pointcloud2(msg)
        msg2, lay2 = _decoy_message(msg, lay, 5)
        arg = ingest.Layout.from_buffer_copy(lay)

        def call(p, stream, arg=arg):
            ok(ingest._lib().ilcc_pointcloud2_unpack_device(PTR(p["data"]), C.byref(arg), PTR(p["xyzi"]), PTR(stream)))

        yield Case("K0 " + name, [Buf("data", _data(msg, lay), _data(msg2, lay2)), Buf("xyzi", nbytes=16 * lay.n_points, out=True)], call,
                   {"xyzi": TI.from_ros_msg_numpy(msg, lay)}, {"xyzi": TI.from_ros_msg_numpy(msg2, lay2)},
                   scribble=lambda arg=arg, lay2=lay2: overwrite(arg, lay2))


# ---- K0b -----------------------------------------------------------------------------------------------------------------------

LEAD = 32          # bytes in front of the first message: the decoy's messages sit 16 bytes before the real ones


class UnpackBatch:
    """A batch of messages as K0b takes it, and its decoy: other bytes, x and y exchanged, every message 16 bytes earlier in the blob
    (its alignment class, and with it the kernel it takes, stays).  Whichever layouts meet whichever offsets, every read stays
    inside the blob and every write inside the output: the sizes are the same in both."""

    def __init__(self, batch, seed):
        import sequence_ref as R
        import test_ingest as TI
        from lidar_camera_calibration_amd import ingest
        self.layouts = [ingest.parse_pointcloud2(m) for m, _ in batch]
        decoys = [_decoy_message(m, lay, seed + k) for k, ((m, _), lay) in enumerate(zip(batch, self.layouts))]
        self.decoy_layouts = [lay for _, lay in decoys]
        self.src, at = [], LEAD
        for (_, align), lay in zip(batch, self.layouts):
            at = (at + 15) // 16 * 16 + (align % 16)
            self.src.append(at)
            at += lay.data_bytes
        self.decoy_src = [s - 16 for s in self.src]
        self.blob_bytes = at
        self.blob, self.decoy_blob = np.full(at, 0x5A, np.uint8), np.full(at, 0x5A, np.uint8)
        for k, ((m, _), lay) in enumerate(zip(batch, self.layouts)):
            self.blob[self.src[k]:self.src[k] + lay.data_bytes] = _data(m, lay)
            self.decoy_blob[self.decoy_src[k]:self.decoy_src[k] + lay.data_bytes] = _data(decoys[k][0], lay)
        self.want = np.concatenate([R.unpack(m) for m, _ in batch])
        self.want_decoy = np.concatenate([TI.from_ros_msg_numpy(m, lay) for m, lay in decoys])
        self.offsets = [0] + np.cumsum([lay.n_points for lay in self.layouts]).tolist()
        self.points = len(self.want)
        assert self.want_decoy.shape == self.want.shape

    def case(self, name, plan):
        from lidar_camera_calibration_amd import ingest, sequence
        n = len(self.layouts)
        arr = (ingest.Layout * n)(*self.layouts)
        src = np.array(self.src, np.uint64)

        def call(p, stream):
            offsets = np.full(n + 1, 77, np.uint64)
            ok(sequence.lib().ilcc_pointcloud2_unpack_batch_device(PTR(p["blob"]), self.blob_bytes, arr, src.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                                   PTR(p["xyzi"]), self.points, offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                   plan._p, PTR(stream)))
            return offsets.tolist()

        def scribble():
            overwrite(arr, (ingest.Layout * n)(*self.decoy_layouts))
            src[:] = self.decoy_src

        return Case(name, [Buf("blob", self.blob, self.decoy_blob), Buf("xyzi", nbytes=16 * self.points, out=True)], call,
                    {"xyzi": self.want}, {"xyzi": self.want_decoy}, scribble=scribble, host_want=self.offsets)


def k0b_batches():
    """the every-layout batch of test_sequence.py, and another one for the second call of a plan"""
    import test_sequence as TS
    mixed = TS._mixed_batch()
    return UnpackBatch(mixed, 100), UnpackBatch(mixed[7:] + mixed[:7], 200)


def k0b_cases(ob=None):
    from lidar_camera_calibration_amd import sequence
    batch, _ = k0b_batches()
    plan = sequence.UnpackPlan(len(batch.layouts))
    yield batch.case("K0b every layout", plan)
    SC._torch().cuda.synchronize()
    plan.close()


# ---- K11, K11c, the undistortion map -------------------------------------------------------------------------------------------

def _k11_reference(px, encoding, cam, colour):
    import bayer_ref
    import camera_image_ref as R
    import overlay_ref
    if encoding.startswith("bayer"):
        return bayer_ref.to_bgr8(px, encoding, cam) if colour else bayer_ref.to_mono8(px, encoding, cam)
    return overlay_ref.convert_bgr8(px, encoding, cam) if colour else R.convert(px, encoding, cam)


K11_SHAPES = ((37, 29, "bgr8"), (37, 29, "bayer_rggb8"), (130, 67, "mono8"))


def _k11_cameras(w, h):
    """the pincushion camera of test_camera_image.py and its decoy, the barrel one"""
    import test_camera_image as TC
    return TC.cam_for(w, h, TC.D_PINCUSHION), TC.cam_for(w, h, TC.D_BARREL)


def k11_case(w, h, encoding, colour):
    import camera_image_ref as R
    import test_camera_image as TC
    from lidar_camera_calibration_amd import camera_image as CI
    bpp = 1 if encoding.startswith("bayer") else R.BPP[encoding]
    shape = (h, w) if bpp == 1 else (h, w, bpp)
    px, px2 = (np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8) for seed in (w + h, w + h + 1))
    cam, cam2 = _k11_cameras(w, h)
    arg, code, out_bpp = TC.native(cam), CI.encoding_code(encoding), 3 if colour else 1
    fn = CI.lib().ilcc_image_to_bgr8_device if colour else CI.lib().ilcc_image_to_mono8_device

    def call(p, stream):
        ok(fn(PTR(p["src"]), w, h, w * bpp, code, C.byref(arg), PTR(p["dst"]), w * out_bpp, PTR(stream)))

    return Case("%s %d x %d %s" % ("K11c" if colour else "K11", w, h, encoding),
                [Buf("src", px, px2), Buf("dst", nbytes=w * h * out_bpp, out=True)], call,
                {"dst": _k11_reference(px, encoding, cam, colour)}, {"dst": _k11_reference(px2, encoding, cam2, colour)},
                scribble=lambda: overwrite(arg, TC.native(cam2)))


def k11_mono_cases(ob=None):
    return (k11_case(w, h, e, False) for w, h, e in K11_SHAPES)


def k11_colour_cases(ob=None):
    return (k11_case(w, h, e, True) for w, h, e in K11_SHAPES)


def undistort_map_cases(ob=None):
    import camera_image_ref as R
    import test_camera_image as TC
    from lidar_camera_calibration_amd import camera_image as CI
    for w, h in ((37, 29), (130, 67)):
        cam, cam2 = _k11_cameras(w, h)
        # the codes are small int32: with the barrel lens centred two images away they are all negative, so the upper bytes differ too
        cam2 = R.camera(cam2.fx, cam2.cx + 2 * w, cam2.fy, cam2.cy + 2 * h, cam2.d, w, h)
        arg = TC.native(cam)

        def call(p, stream, arg=arg):
            ok(CI.lib().ilcc_undistort_map_device(C.byref(arg), PTR(p["iu"]), PTR(p["iv"]), PTR(stream)))

        (iu, iv), (iu2, iv2) = R.undistort_map(cam), R.undistort_map(cam2)
        yield Case("undistort map %d x %d" % (w, h), [Buf("iu", nbytes=4 * w * h, out=True), Buf("iv", nbytes=4 * w * h, out=True)], call,
                   {"iu": iu.astype("<i4"), "iv": iv.astype("<i4")}, {"iu": iu2.astype("<i4"), "iv": iv2.astype("<i4")},
                   scribble=lambda arg=arg, cam2=cam2: overwrite(arg, TC.native(cam2)))


# ---- K8 ------------------------------------------------------------------------------------------------------------------------

def _k8_inputs():
    """4097 points, all kept (two chunks, the second of one point); the decoy keeps the second half only, with other intensities, seen
    by a camera whose principal point lies 40 rows lower: its records hold other points, and half of its output is never written"""
    import project_cases as PC
    n = PC.CHUNK + 1
    i = np.arange(n)
    real, decoy = PC.keep_cloud(np.ones(n, bool)), PC.keep_cloud(i >= n // 2)
    decoy[:, 3] = (7 * i + 5) % 256
    return real, decoy, PC.keep_camera(), PC.camera(width=PC.KEEP_SIDE, height=PC.KEEP_SIDE, cy=40.0), PC.KEEP_DIS


def _records_then_sentinels(records, n):
    out = sentinels(16 * n)
    out[:records.nbytes] = SC.as_bytes(records)
    return out


def k8_intensity_cases(ob):
    from lidar_camera_calibration_amd import project
    real, decoy, cam, cam2, dis = _k8_inputs()
    n = len(real)
    want, want2 = ob.project_intensity(real, cam, dis, 0.0, 60.0), ob.project_intensity(decoy, cam2, dis, 0.0, 60.0)
    arg = project.Projection.from_buffer_copy(cam)

    def call(p, stream):
        m = C.c_uint32(0)
        ok(project._lib().ilcc_project_intensity_device(PTR(p["xyzi"]), n, C.byref(arg), dis, 0.0, 60.0, PTR(p["hits"]), C.byref(m), PTR(stream)))
        return m.value

    yield Case("K8 intensity 4097 all kept", [Buf("xyzi", real, decoy), Buf("hits", nbytes=16 * n, out=True)], call,
               {"hits": _records_then_sentinels(want, n)}, {"hits": _records_then_sentinels(want2, n)},
               scribble=lambda: overwrite(arg, cam2), host_want=len(want))


def k8_colourise_cases(ob):
    import project_cases as PC
    from lidar_camera_calibration_amd import project
    real, decoy, cam, cam2, dis = _k8_inputs()
    n = len(real)
    img, img2 = PC.keep_image(), PC.random_image(cam, 0, 77)
    want, want2 = ob.colourise(real, cam, img, dis), ob.colourise(decoy, cam2, img2, dis)
    arg = project.Projection.from_buffer_copy(cam)

    def call(p, stream):
        m = C.c_uint32(0)
        ok(project._lib().ilcc_colourise_device(PTR(p["xyzi"]), n, C.byref(arg), dis, PTR(p["image"]), img.strides[0], PTR(p["out"]), C.byref(m),
                                                PTR(stream)))
        return m.value

    yield Case("K8 colourise 4097 all kept", [Buf("xyzi", real, decoy), Buf("image", img, img2), Buf("out", nbytes=16 * n, out=True)], call,
               {"out": _records_then_sentinels(want, n)}, {"out": _records_then_sentinels(want2, n)},
               scribble=lambda: overwrite(arg, cam2), host_want=len(want))


# ---- K12 -----------------------------------------------------------------------------------------------------------------------

def _stamp_of_64():
    """the custom stamp of test_overlay.py's test_k12_custom_stamp_of_64_offsets"""
    rng = np.random.default_rng(11)
    stamp = [(127, 127), (-127, 127), (127, -127), (-127, -127), (-128, -128), (0, 0)]
    return stamp + [(int(a), int(b)) for a, b in rng.integers(-128, 128, (58, 2))]


def k12_case(custom, flip=False):
    """64 x 48, 257 hits (two workgroups of hits); flip: the decoy's image, hits and stamp as the real ones"""
    import overlay_ref as O
    import test_overlay as TO
    from lidar_camera_calibration_amd import project
    w, h, n = 64, 48, 257
    images = [TO.noise_image(w, h, "bgr8", 4), TO.noise_image(w, h, "bgr8", 5)]
    hits = [TO.random_hits(n, w, h, seed=n + w), TO.random_hits(n, w, h, seed=1)]
    stamps = [_stamp_of_64(), [(b, a) for a, b in _stamp_of_64()]] if custom else [None, None]
    if flip:
        images, hits, stamps = images[::-1], hits[::-1], stamps[::-1]
    flat = [[int(v) for pair in st for v in pair] if st is not None else None for st in stamps]
    xy = (C.c_int8 * 128)(*flat[0]) if custom else None

    def call(p, stream):
        ok(project._lib().ilcc_draw_hits_device(PTR(p["image"]), w, h, 3 * w, PTR(p["hits"]), n, xy, 64 if custom else 0, PTR(p["scratch"]),
                                                PTR(stream)))

    want = [O.draw_hits(images[k], hits[k], stamps[k] if custom else O.REFERENCE_STAMP) for k in (0, 1)]
    return Case("K12 %s%s" % ("stamp of 64 offsets" if custom else "reference stamp", ", exchanged" if flip else ""),
                [Buf("image", images[0], images[1], out=True), Buf("hits", hits[0], hits[1]),
                 Buf("scratch", nbytes=project.draw_hits_scratch_bytes(w, h), scratch=True)], call,
                {"image": want[0]}, {"image": want[1]},
                scribble=(lambda: overwrite(xy, (C.c_int8 * 128)(*flat[1]))) if custom else None)


def k12_cases(ob=None):
    return (k12_case(custom) for custom in (False, True))


# ---- K8b -----------------------------------------------------------------------------------------------------------------------

class ColouriseBatch:
    """A batch of paired_cases as K8b takes it, and its decoy: another keep pattern on the same scan lengths, other pixels in both
    images, every paired scan on the other image, a camera whose principal point lies elsewhere.  The images keep their places and
    their row steps, so whatever meets whatever, every read stays inside its buffer."""

    def __init__(self, p, p_decoy):
        import paired_cases as K
        import paired_ref as R
        import project_cases as PC
        self.b, b2 = K.keep_batch(p), K.keep_batch(p_decoy)
        assert self.b["offsets"].tolist() == b2["offsets"].tolist() and self.b["image_of_scan"].tolist() == b2["image_of_scan"].tolist()
        self.images = self.b["images"]
        self.decoy_images = [np.random.default_rng(900 + k).integers(0, 256, im.shape, dtype=np.uint8) for k, im in enumerate(self.images)]
        of = self.b["image_of_scan"]
        self.decoy_of = np.where(of >= 0, 1 - of, of).astype(np.int32)
        self.decoy_cam = PC.camera(width=PC.KEEP_SIDE, height=PC.KEEP_SIDE, cx=-1.0, cy=1.0)
        self.decoy_xyzi = b2["xyzi"]
        self.want, self.want_off = R.colourise_batch(self.b["xyzi"], self.b["offsets"], self.images, of, self.b["cam"], self.b["dis"])
        self.want_decoy, _ = R.colourise_batch(self.decoy_xyzi, self.b["offsets"], self.decoy_images, self.decoy_of, self.decoy_cam, self.b["dis"])
        n = np.diff(self.b["offsets"].astype(np.int64))
        self.cap = int(n[of >= 0].sum())
        self.n_scans = len(of)

    def case(self, name, plan):
        from lidar_camera_calibration_amd import paired, project
        b = self.b
        off = np.ascontiguousarray(b["offsets"], np.uint64)
        of = np.ascontiguousarray(b["image_of_scan"], np.int32)
        steps = np.array([im.strides[0] for im in self.images], np.uint32)
        cam = project.Projection.from_buffer_copy(b["cam"])
        ptrs = (C.c_void_p * 2)()

        def call(p, stream):
            ptrs[0], ptrs[1] = p["image0"], p["image1"]
            ok(paired.lib().ilcc_colourise_batch_device(PTR(p["xyzi"]), off.ctypes.data_as(C.POINTER(C.c_uint64)), self.n_scans, ptrs,
                                                        steps.ctypes.data_as(C.POINTER(C.c_uint32)), 2, of.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        C.byref(cam), float(b["dis"]), PTR(p["out"]), self.cap, plan._p, PTR(stream)))

        def scribble():
            of[:] = self.decoy_of
            overwrite(cam, self.decoy_cam)

        return Case(name, [Buf("xyzi", b["xyzi"], self.decoy_xyzi), Buf("image0", self.images[0], self.decoy_images[0]),
                           Buf("image1", self.images[1], self.decoy_images[1]), Buf("out", nbytes=16 * self.cap, out=True)], call,
                    {"out": _records_then_sentinels(self.want, self.cap)}, {"out": _records_then_sentinels(self.want_decoy, self.cap)},
                    scribble=scribble, finish=lambda _: plan.finish(self.n_scans).tolist(), host_want=self.want_off.tolist())


def colourise_plan():
    from lidar_camera_calibration_amd import paired
    return paired.ColourisePlan(64, 80000)


def k8b_cases(ob=None):
    plan = colourise_plan()
    yield ColouriseBatch(3, 1).case("K8b keep_batch(3)", plan)
    plan.close()


# ---- K13, K13b -----------------------------------------------------------------------------------------------------------------

def k13_idct_case(flip=False):
    """the (33, 2, 257, 9) grid at 4:2:0; the decoy: other coefficients under other tables"""
    import jpeg_cases as J
    import jpeg_ref as R
    from lidar_camera_calibration_amd import jpeg
    w, h = 257, 9
    specs = [("ones", 109), ("ramp", 1)][::-1 if flip else 1]
    built = []
    for quant, seed in specs:
        q = np.stack([J.QUANTS[quant], J.QUANTS[quant][::-1]])
        rinfo = R.make_info(w, h, jpeg.SAMPLINGS["420"], q)
        coef = J.grid_coefficients(rinfo.coef_count, seed, max(1, 1000 // int(q.max())))
        built.append((jpeg.make_info(w, h, "420", q), coef, R.pixels(rinfo, coef)))
    (info, coef, px), (info2, coef2, px2) = built
    arg = jpeg.Info.from_buffer_copy(info)
    scratch = jpeg.scratch_bytes(info)

    def call(p, stream):
        ok(jpeg.lib().ilcc_jpeg_idct_device(C.byref(arg), PTR(p["coef"]), PTR(p["dst"]), 3 * w, PTR(p["scratch"]), scratch, PTR(stream)))

    return Case("K13 idct 257 x 9 4:2:0%s" % (", exchanged" if flip else ""),
                [Buf("coef", coef, coef2), Buf("dst", nbytes=3 * w * h, out=True), Buf("scratch", nbytes=scratch, scratch=True)], call,
                {"dst": px}, {"dst": px2}, scribble=lambda: overwrite(arg, info2))


def k13_idct_cases(ob=None):
    yield k13_idct_case()


def k13_decode_cases(ob=None):
    import jpeg_cases as J
    from lidar_camera_calibration_amd import jpeg
    name, name2 = "noise_17x33_420_q50_r0.jpg", "ramp_17x33_420_q50_r0.jpg"
    jpg, jpg2 = J.data(name), J.data(name2)
    px, px2 = J.restated(name)[2], J.restated(name2)[2]
    assert px.shape == px2.shape == (33, 17, 3)
    host = (C.c_uint8 * max(len(jpg), len(jpg2)))(*jpg)

    def call(p, stream):
        w, h, enc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        ok(jpeg.lib().ilcc_jpeg_decode_device(host, len(jpg), PTR(p["dst"]), 3 * 17, px.size, C.byref(w), C.byref(h), C.byref(enc), PTR(stream)))
        return w.value, h.value, jpeg.ENCODINGS[enc.value]

    yield Case("K13 decode " + name, [Buf("dst", nbytes=px.size, out=True)], call, {"dst": px}, {"dst": px2},
               scribble=lambda: C.memmove(host, jpg2, len(jpg2)), host_want=(17, 33, "bgr8"))


def k13b_case(flip=False):
    """the ("420", 17, 33) seam case of test_jpeg_sequence.py as a batch of 3; the decoy: other coefficients under permuted tables"""
    import jpeg_ref as R
    import test_jpeg_sequence as TJ
    from lidar_camera_calibration_amd import jpeg
    from lidar_camera_calibration_amd import jpeg_sequence as JS
    w, h, n = 17, 33, 3
    tables = [("ones", "255", "ramp"), ("ramp", "ramp", "ones"), ("255", "ones", "ones")]
    sets = [[TJ._constructed(w, h, "420", 10 + m, tables[m]) for m in range(n)], [TJ._constructed(w, h, "420", 20 + m, tables[(m + 1) % n]) for m in range(n)]]
    if flip:
        sets = sets[::-1]
    layout = jpeg.make_info(w, h, "420")
    pitch = (layout.coef_count + 7) // 8 * 8
    quants, coefs, want = [], [], []
    for built in sets:
        quants.append(np.stack([b[2] for b in built]).astype(np.uint16))
        c = np.full((n, pitch), 0x7FFF, np.int16)
        for m, b in enumerate(built):
            c[m, :layout.coef_count] = b[3]
        coefs.append(c)
        want.append(np.stack([R.pixels(b[1], b[3]) for b in built]))
    scratch = JS.batch_scratch_bytes(layout, n)
    smaller = jpeg.make_info(9, 17, "420")          # a valid layout that fits every buffer of this one

    def call(p, stream):
        ok(JS.lib().ilcc_jpeg_idct_batch_device(C.byref(layout), PTR(p["quant"]), PTR(p["coef"]), pitch, n, PTR(p["dst"]), 3 * w * h, 3 * w,
                                                PTR(p["scratch"]), scratch, PTR(stream)))

    return Case("K13b 3 x (17 x 33) 4:2:0%s" % (", exchanged" if flip else ""),
                [Buf("quant", quants[0], quants[1]), Buf("coef", coefs[0], coefs[1]), Buf("dst", nbytes=n * 3 * w * h, out=True),
                 Buf("scratch", nbytes=scratch, scratch=True)], call, {"dst": want[0]}, {"dst": want[1]},
                scribble=lambda: overwrite(layout, smaller))


def k13b_cases(ob=None):
    yield k13b_case()


# ---- K14 -----------------------------------------------------------------------------------------------------------------------

def _k14_fixed(w, h, mode):
    """The coefficient bytes no pixels of this size can change at any quality: the restatement on eight unlike images, finest tables
    and coarse ones.  Most coefficients of a small 4:2:0 image belong to blocks that pad it to whole MCUs, whose samples repeat the
    last column or row: all but their first row or column of coefficients is 0 whatever the image holds."""
    import jpeg_write_ref as W
    rng = np.random.default_rng(14)
    shape = (h, w) if mode == "gray" else (h, w, 3)
    outs = []
    for k in range(4):
        px = rng.integers(0, 2, shape).astype(np.uint8) * 255 if k % 2 else rng.integers(0, 256, shape, dtype=np.uint8)
        for image in (px, 255 - px):
            info = W.make_info(w, h, W.SAMPLINGS[mode], (100, 95)[k // 2], 0)
            outs.append(SC.as_bytes(W.coefficients(info, image).astype("<i2")))
    return (np.stack(outs) == outs[0]).all(0)


def k14_fdct_case(size_mode, flip=False):
    """a case of jpeg_write_cases.py at quality 95; the decoy: its pixels inverted, under the tables of quality 50"""
    import jpeg_write_cases as JW
    import jpeg_write_ref as R
    from lidar_camera_calibration_amd import jpeg
    from lidar_camera_calibration_amd import jpeg_write as W
    name = "noise_%s_q95_r0" % size_mode
    _, w, h, mode, _, _ = JW.cases()[name]
    sampling = None if mode == "gray" else mode
    sets = [(JW.source(name), 95), (255 - JW.source(name), 50)]
    if flip:
        sets = sets[::-1]
    infos = [W.write_info(w, h, sampling, q, 0) for _, q in sets]
    want = [R.coefficients(R.make_info(w, h, R.SAMPLINGS[mode], q, 0), px).astype("<i2") for px, q in sets]
    if not flip:
        assert want[0].tobytes() == JW.restated(name)[1].astype("<i2").tobytes()
    bpp = 1 if mode == "gray" else 3
    arg = jpeg.Info.from_buffer_copy(infos[0])
    scratch = max(W.fdct_scratch_bytes(arg), 16)
    enc = W.ENCODINGS.index("mono8" if bpp == 1 else "bgr8")

    def call(p, stream):
        ok(W.lib().ilcc_jpeg_fdct_device(C.byref(arg), PTR(p["src"]), bpp * w, enc, PTR(p["coef"]), PTR(p["scratch"]), scratch, PTR(stream)))

    return Case("K14 fdct %s%s" % (name, ", exchanged" if flip else ""),
                [Buf("src", sets[0][0], sets[1][0]), Buf("coef", nbytes=2 * arg.coef_count, out=True), Buf("scratch", nbytes=scratch, scratch=True)],
                call, {"coef": want[0]}, {"coef": want[1]}, scribble=lambda: overwrite(arg, infos[1]), fixed={"coef": _k14_fixed(w, h, mode)})


def k14_fdct_cases(ob=None):
    return (k14_fdct_case(s) for s in ("17x33_420", "257x9_gray"))


def k14_encode_cases(ob=None):
    import jpeg_write_cases as JW
    from lidar_camera_calibration_amd import jpeg_write as W
    name, name2 = "noise_17x33_420_q95_r0", "noise_17x33_420_q50_r0"
    want, want2 = JW.restated(name)[2], JW.restated(name2)[2]
    bound = W.file_bound(W.write_info(17, 33, "420", 95, 0))

    def call(p, stream):
        out, size = np.empty(bound, np.uint8), C.c_uint64(0)
        ok(W.lib().ilcc_jpeg_encode_device(PTR(p["src"]), 3 * 17, 17, 33, W.ENCODINGS.index("bgr8"), 95, 2, 2, 0, out.ctypes.data_as(C.c_void_p),
                                           bound, C.byref(size), PTR(stream)))
        return out[:size.value].tobytes()

    yield Case("K14 encode " + name, [Buf("src", JW.source(name), JW.source(name2))], call, {}, {}, host_want=bytes(want),
               host_bytes=(bytes(want), bytes(want2)))


# ---- K10, K10b ------------------------------------------------------------------------------------------------------------------

def _on_stream(stream):
    torch = SC._torch()
    return torch.cuda.stream(torch.cuda.ExternalStream(stream))


def k10_corners_cases(ob=None):
    """squares_34x34, the smallest edge fixture of test_image_corners.py, held against the restatement stage by stage by that
    file's own comparison (its tolerances are its own); the decoy is the noise image of that size"""
    import test_image_corners as TI
    name, name2 = "squares_34x34", "noise_34x34"
    img, img2 = TI.fixture(name), TI.fixture(name2)

    def call(p, stream):
        with _on_stream(stream):
            corners, st = TI._assert_stages_match(img, name, TI.restated(name), image=p.t["image"][:img.size].view(img.shape))
        return corners.tobytes(), st["candidates"].tobytes(), st["refined"].tobytes()

    yield Case("K10 corners " + name, [Buf("image", img, img2)], call, {}, {}, host_key=lambda ret: ret,
               host_bytes=(TI.restated(name)["final"].tobytes(), TI.restated(name2)["final"].tobytes()))


BOARD = (5, 3)


def _board_images():
    """160 x 128 with a 5 x 3 board: no smaller fixture of test_image_corners.py holds a whole board"""
    import test_image_corners as TI
    return (TI.render_board((160, 128), board=BOARD, square=20.0, theta=0.3, seed=5),
            TI.render_board((160, 128), board=BOARD, square=20.0, theta=-0.2, centre=(86, 60), seed=6))


def _two_steps(img):
    """ilcc_find_chessboard_device is 'both steps': the corners of the first entry on the null stream, then the host's recovery"""
    from lidar_camera_calibration_amd import image_corners as IC
    corners = IC.find_corners(img)
    idx = IC.chessboard_from_corners(corners, BOARD)
    return idx.shape, np.stack([corners["u"][idx], corners["v"][idx]], -1).astype(np.float64)


def k10_chessboard_cases(ob=None):
    import test_image_corners as TI
    from lidar_camera_calibration_amd import image_corners as IC
    (img, truth), (img2, _) = _board_images()
    (shape, xy), (_, xy2) = _two_steps(img), _two_steps(img2)
    a, b = TI._match(xy, truth)
    assert a < 0.25 and b < 0.25, (a, b)                    # the bar of test_synthetic_boards
    h, w = img.shape

    def call(p, stream):
        out = np.zeros(BOARD[0] * BOARD[1] * 2)
        r, k = C.c_int32(0), C.c_int32(0)
        ok(IC.lib().ilcc_find_chessboard_device(PTR(p["image"]), w, h, w, BOARD[0], BOARD[1], C.byref(r), C.byref(k),
                                                out.ctypes.data_as(C.POINTER(C.c_double)), PTR(stream)))
        return (r.value, k.value), out.tobytes()

    yield Case("K10 chessboard 160 x 128", [Buf("image", img, img2)], call, {}, {}, host_want=(tuple(shape), xy.tobytes()),
               host_bytes=(xy.tobytes(), xy2.tobytes()))


class CornerBatch:
    """A batch of image_sequence_cases' 160 x 128 images back to back, held against the single entry image by image"""

    def __init__(self, names, decoy_names):
        import image_sequence_cases as K
        import test_image_sequence as TS
        self.images, self.decoys = K.mixed_batch(names), K.mixed_batch(decoy_names)
        self.want = [TS.single(im)[0].tobytes() for im in self.images]
        self.want_decoy = [TS.single(im)[0].tobytes() for im in self.decoys]
        self.name = " + ".join(names)

    def case(self, name, plan, capacity=8192):
        from lidar_camera_calibration_amd import image_corners as IC
        from lidar_camera_calibration_amd import image_sequence as IS
        n, (h, w) = len(self.images), self.images[0].shape

        def call(p, stream):
            out, cnt = np.zeros((n, capacity), IC.CORNER_DTYPE), np.zeros(n, np.int32)
            ok(IS.lib().ilcc_image_corners_batch_device(PTR(p["images"]), w * h, n, w, h, w, out.ctypes.data_as(C.c_void_p), capacity,
                                                        cnt.ctypes.data_as(C.POINTER(C.c_int32)), plan._p, PTR(stream)))
            return [out[m, :cnt[m]].tobytes() for m in range(n)]

        return Case(name, [Buf("images", np.stack(self.images), np.stack(self.decoys))], call, {}, {}, host_want=self.want,
                    host_bytes=(b"".join(self.want), b"".join(self.want_decoy)))


def corner_plan():
    import image_sequence_cases as K
    from lidar_camera_calibration_amd import image_sequence as IS
    return IS.CornerPlan(2, K.W0, K.H0)


def k10b_cases(ob=None):
    plan = corner_plan()
    yield CornerBatch(["squares", "board"], ["noise2", "squares2"]).case("K10b squares + board", plan)
    plan.close()


# ---- K15, K15p -----------------------------------------------------------------------------------------------------------------

def _seed_batches():
    """seed_cases' ragged batch of 0, 1, 63, 64, 65 and 257 points, which holds no seed, and behind it a board-sized plate, which is
    one; the decoy: other boxes of those sizes and another plate"""
    import seed_cases as K
    points, offsets, frames = K.ragged_batch()
    real = list(frames) + [K.board_plate(0)]
    decoy = [K.random_box(len(f), 300 + len(f), -3.0, -0.2) if len(f) else f for f in frames] + [K.board_plate(1)]
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in real])]).astype(np.uint64)
    assert offsets[:7].tolist() == [0, 0, 1, 64, 128, 193, 450]
    return real, decoy, offsets


def _seeds_as_the_tests_compare_them(lists):
    return [None if seeds is None else [(s.key, s.n, tuple(s.centroid_array().tolist())) for s in seeds] for seeds in lists]


def _seed_bytes(per_frame):
    return b"".join(np.array([key, n], np.int64).tobytes() + np.array(c, np.float32).tobytes() for seeds in per_frame for key, n, c in seeds)


def k15_cases(ob=None, planar=False):
    import seed_cases as K
    import seed_planar_cases as KP
    import seed_planar_ref as P
    import seed_ref as R
    import test_seed as TS
    import test_seed_planar as TP
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    from lidar_camera_calibration_amd import seed as S
    real, decoy, offsets = _seed_batches()
    sp = K.small_params()
    grid = R.grid(sp, TS.POINTS)

    def restated(frames):
        recs = [P.components(f, sp, KP.PP, grid) if planar else R.components(f, sp, grid) for f in frames]
        return [[(s.key, s.n, tuple(float(v) for v in s.centroid)) for s in R.finish(r, sp)] for r in recs]

    want, want2 = restated(real), restated(decoy)
    assert [len(s) for s in want] == [0] * 6 + [1]
    est = LidarCornersBatch(8, TS.POINTS // 8, N.default_params())
    if planar:
        nsp, npp = TP.native(sp)
        scratch = S.planar_scratch_bytes(len(real), int(offsets[-1]), nsp)
    else:
        nsp, npp = TS.native(sp), None
        scratch = S.scratch_bytes(len(real), int(offsets[-1]), nsp)

    def call(p, stream):
        if planar:
            got = S.propose_seeds_planar_device(est, p["xyzi"], offsets, nsp, npp, p["scratch"], stream)
        else:
            got = S.propose_seeds_device(est, p["xyzi"], offsets, nsp, p["scratch"], stream)
        return _seeds_as_the_tests_compare_them(got)

    yield Case("K15%s ragged batch + plate" % ("p" if planar else ""),
               [Buf("xyzi", np.concatenate(real), np.concatenate(decoy)), Buf("scratch", nbytes=scratch, scratch=True)], call, {}, {},
               host_want=want, host_bytes=(_seed_bytes(want), _seed_bytes(want2)))
    est.close()


def k15p_cases(ob=None):
    return k15_cases(ob, planar=True)


# ---- the list: one entry per declaration ------------------------------------------------------------------------------------------

ENTRIES = {
    "ilcc_pointcloud2_unpack_device": k0_cases,
    "ilcc_pointcloud2_unpack_batch_device": k0b_cases,
    "ilcc_image_to_mono8_device": k11_mono_cases,
    "ilcc_image_to_bgr8_device": k11_colour_cases,
    "ilcc_undistort_map_device": undistort_map_cases,
    "ilcc_project_intensity_device": k8_intensity_cases,
    "ilcc_colourise_device": k8_colourise_cases,
    "ilcc_draw_hits_device": k12_cases,
    "ilcc_colourise_batch_device": k8b_cases,
    "ilcc_jpeg_idct_device": k13_idct_cases,
    "ilcc_jpeg_decode_device": k13_decode_cases,
    "ilcc_jpeg_idct_batch_device": k13b_cases,
    "ilcc_jpeg_fdct_device": k14_fdct_cases,
    "ilcc_jpeg_encode_device": k14_encode_cases,
    "ilcc_image_corners_device": k10_corners_cases,
    "ilcc_find_chessboard_device": k10_chessboard_cases,
    "ilcc_image_corners_batch_device": k10b_cases,
    "ilcc_propose_seeds_device": k15_cases,
    "ilcc_propose_seeds_planar_device": k15p_cases,
}


def test_every_declaration_with_a_stream_has_a_stream_test():
    """A new entry that takes a hip_stream fails here until it is in ENTRIES."""
    found = declared()
    assert sorted(found) == sorted(ENTRIES), sorted(set(found) ^ set(ENTRIES))
    assert len(found) >= 19 and len(set(found.values())) >= 11          # the expression still finds what it found when it was written


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_on_a_delayed_stream(ob, entry):
    n = 0
    for case in ENTRIES[entry](ob):
        SC.check_entry(case)
        n += 1
    assert n >= 1


# ---- plans: a call waits for the plan's previous call; two plans do not meet --------------------------------------------------------

def _right(case, got, ret=None):
    """the restatement's bytes, which are also the solo run's"""
    SC.same(case, got, case.want, "the restatement")
    if case.solo_out is not None:
        SC.same(case, got, case.solo_out, "its solo run")
    if case.host_want is not None and (ret is not None or case.finish is None):
        assert ret == case.host_want, case.name


def _plan_pairs(which):
    """-> (make a plan, the first batch's case for a plan, the second batch's)"""
    if which == "K0b":
        from lidar_camera_calibration_amd import sequence
        a, b = k0b_batches()
        return (lambda: sequence.UnpackPlan(len(a.layouts))), (lambda plan: a.case("K0b every layout", plan)), (lambda plan: b.case("K0b rotated", plan))
    if which == "K8b":
        a, b = ColouriseBatch(3, 1), ColouriseBatch(5, 1)
        return colourise_plan, (lambda plan: a.case("K8b keep_batch(3)", plan)), (lambda plan: b.case("K8b keep_batch(5)", plan))
    a, b = CornerBatch(["squares", "board"], ["noise2", "squares2"]), CornerBatch(["board", "noise"], ["squares2", "range3"])
    return corner_plan, (lambda plan: a.case("K10b squares + board", plan)), (lambda plan: b.case("K10b board + noise", plan))


PLANS = ("K0b", "K8b", "K10b")


@pytest.mark.gpu
@pytest.mark.parametrize("which", PLANS)
def test_plan_serves_a_second_call_while_its_first_is_held_back(which):
    """The same plan: a call on a delayed stream and, at once, another batch on an idle stream.  K10b is synchronous on return, so
    its second call simply follows its first."""
    make, first, second = _plan_pairs(which)
    plan = make()
    first, second = first(plan), second(plan)
    for case, (out, ret) in zip((first, second), SC.plan_reuse(first, second)):
        _right(case, out, ret)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", PLANS)
def test_two_plans_on_two_delayed_streams(which):
    """Two plans, two delayed streams, both calls made before either stream is waited for (K10b waits inside each call)."""
    make, first, second = _plan_pairs(which)
    plans = [make(), make()]
    cases = [first(plans[0]), second(plans[1])]
    for case, (out, ret) in zip(cases, SC.in_flight_together(cases)):
        _right(case, out, ret)                           # K8b: each plan's finish call reports its own call
    for plan in plans:
        plan.close()


# ---- caller-owned scratch: two calls on two streams, each with its own ---------------------------------------------------------------

SCRATCH = {
    "K12": lambda: [k12_case(True), k12_case(True, flip=True)],
    "K13": lambda: [k13_idct_case(), k13_idct_case(flip=True)],
    "K13b": lambda: [k13b_case(), k13b_case(flip=True)],
    "K14": lambda: [k14_fdct_case("17x33_420"), k14_fdct_case("17x33_420", flip=True)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SCRATCH))
def test_two_calls_with_separate_scratch_on_two_delayed_streams(which):
    cases = SCRATCH[which]()
    for case, (out, ret) in zip(cases, SC.in_flight_together(cases)):
        _right(case, out, ret)


# ---- controls: the harness sees an entry that runs on another stream ----------------------------------------------------------------

@pytest.mark.gpu
def test_control_k11_on_another_stream_is_seen():
    SC.check_control(k11_case(130, 67, "mono8", False))


@pytest.mark.gpu
def test_control_k0b_on_another_stream_is_seen():
    from lidar_camera_calibration_amd import sequence
    batch, _ = k0b_batches()
    plan = sequence.UnpackPlan(len(batch.layouts))
    SC.check_control(batch.case("K0b control", plan))
    plan.close()


def test_decoys_that_need_no_gpu_differ_from_the_real_outputs():
    """What check_entry asserts first, for the cases that can be built without a device."""
    n = 0
    for make in (k0_cases, k11_mono_cases, k11_colour_cases, undistort_map_cases, k12_cases, k13_idct_cases, k13_decode_cases, k13b_cases,
                 k14_fdct_cases, k14_encode_cases):
        for case in make():
            case.assert_decoy_differs()
            n += 1
    assert n == 18
