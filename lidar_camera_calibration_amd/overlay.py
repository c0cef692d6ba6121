"""LiDAR points drawn on the undistorted colour image: ctypes mirror of ``include/ilcc_overlay.h`` -- the
reference's pcd2image node (/root/reference/ilcc2/test/pcd2image.cpp:33-89) from bags, without ROS or OpenCV.
The stages it chains are in ``camera_image`` (K11c ``to_bgr8``), ``ingest`` (K0) and ``project`` (K8, K12
``draw_hits_device``).  The camera is the lens (``camera_image.CameraModel``), the extrinsic a 4 x 4; the library
makes K8's ``project.Projection`` of the two.

``include/ilcc_overlay_sequence.h`` is mirrored here too: ``OverlayPlan`` and ``overlay_batch_device`` are K12b, a batch of scans
projected, coloured and drawn on a copy of each one's image in three launches; ``overlay_sequence_bytes`` is what a paired scan
takes on the device in the chain; ``bag_pcd2image_all_pairs`` is the chain bags -> one JPEG (and picture) per scan.
``tests/overlay_sequence_ref.py`` restates them."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import CameraImageError, CameraModel
from .project import Projection

OVERLAY_EXPORTS = ["ilcc_bag_pcd2image", "ilcc_save_ppm_bgr"]
OVERLAY_SEQUENCE_EXPORTS = ["ilcc_overlay_plan_create", "ilcc_overlay_plan_destroy", "ilcc_overlay_batch_scratch_bytes", "ilcc_overlay_batch_device",
                            "ilcc_overlay_plan_finish", "ilcc_overlay_plan_launches", "ilcc_overlay_sequence_bytes",
                            "ilcc_default_overlay_sequence_params", "ilcc_bag_pcd2image_all_pairs"]


class OverlayBatchJob(C.Structure):
    _fields_ = [
        ("d_xyzi", C.c_void_p), ("offsets", C.POINTER(C.c_uint64)), ("d_images_bgr", C.POINTER(C.c_void_p)), ("image_steps", C.POINTER(C.c_uint32)),
        ("image_of_scan", C.POINTER(C.c_int32)), ("cam", C.POINTER(Projection)), ("stamp_xy", C.POINTER(C.c_int8)),
        ("d_canvas", C.c_void_p), ("d_scratch", C.c_void_p), ("plan", C.c_void_p), ("hip_stream", C.c_void_p),
        ("canvas_pitch", C.c_uint64), ("scratch_bytes", C.c_uint64),
        ("distance_valid", C.c_double), ("inten_low", C.c_double), ("inten_high", C.c_double),
        ("n_scans", C.c_uint32), ("n_images", C.c_uint32), ("canvas_stride", C.c_int32), ("n_stamp", C.c_int32),
    ]


class OverlaySequenceParams(C.Structure):
    _fields_ = [
        ("first", C.c_uint32), ("stride", C.c_uint32), ("max_scans", C.c_uint32), ("route", C.c_uint32), ("keep_pixels", C.c_uint32), ("reserved", C.c_uint32),
        ("max_dt_ns", C.c_uint64), ("staging_bytes", C.c_uint64), ("image_bytes", C.c_uint64), ("device_bytes", C.c_uint64),
        ("out_bytes_per_image", C.c_uint64),
    ]


class OverlayRecord(C.Structure):
    _fields_ = [
        ("message", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
        ("image_message", C.c_int32),
        ("image_stamp_sec", C.c_uint32), ("image_stamp_nsec", C.c_uint32),
        ("dt_ns", C.c_int64),
        ("n_points", C.c_uint64),
        ("n_drawn", C.c_uint32), ("route", C.c_uint32),
        ("file_bytes", C.c_uint64),
    ]


OVERLAY_SINK = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(OverlayRecord), C.c_void_p, C.c_uint64, C.c_void_p)


class OverlayError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = int(status)
        msg = _native.strerror(status)
        super().__init__("%s: %s" % (msg, detail) if detail else msg)


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        i32p = C.POINTER(C.c_int32)
        L.ilcc_bag_pcd2image.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(CameraModel),
                                         C.POINTER(C.c_double), C.c_double, C.c_void_p, C.c_uint64, i32p, i32p,
                                         C.POINTER(C.c_uint32)]
        L.ilcc_bag_pcd2image.restype = C.c_int32
        L.ilcc_save_ppm_bgr.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]
        L.ilcc_save_ppm_bgr.restype = C.c_int32
        L.ilcc_overlay_plan_create.argtypes = [C.c_uint32, C.c_uint64]
        L.ilcc_overlay_plan_create.restype = C.c_void_p
        L.ilcc_overlay_plan_destroy.argtypes = [C.c_void_p]
        L.ilcc_overlay_plan_destroy.restype = None
        L.ilcc_overlay_batch_scratch_bytes.argtypes = [C.c_int32, C.c_int32, C.c_uint32]
        L.ilcc_overlay_batch_scratch_bytes.restype = C.c_uint64
        L.ilcc_overlay_batch_device.argtypes = [C.POINTER(OverlayBatchJob)]
        L.ilcc_overlay_batch_device.restype = C.c_int32
        L.ilcc_overlay_plan_finish.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.ilcc_overlay_plan_finish.restype = C.c_int32
        L.ilcc_overlay_plan_launches.argtypes = [C.c_void_p]
        L.ilcc_overlay_plan_launches.restype = C.c_uint32
        L.ilcc_overlay_sequence_bytes.argtypes = [C.c_int32, C.c_int32, C.c_uint64]
        L.ilcc_overlay_sequence_bytes.restype = C.c_uint64
        L.ilcc_default_overlay_sequence_params.argtypes = [C.POINTER(OverlaySequenceParams)]
        L.ilcc_default_overlay_sequence_params.restype = None
        L.ilcc_bag_pcd2image_all_pairs.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(CameraModel),
                                                   C.POINTER(C.c_double), C.c_double, C.c_int32, C.POINTER(OverlaySequenceParams), OVERLAY_SINK,
                                                   C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.ilcc_bag_pcd2image_all_pairs.restype = C.c_int32
        _ready = True
    return L


def _check(st):
    if st != _native.OK:
        raise CameraImageError(st)


def bag_pcd2image(image_bag, image_topic, lidar_topic, camera, T_lidar2cam, lidar_bag=None, distance_valid=5.0, device=0):
    """(image, n_drawn): the (rows, cols, 3) uint8 B,G,R picture pcd2image shows for the first Image on image_topic and
    the first PointCloud2 on lidar_topic (of lidar_bag, or of the same bag), and the number of points drawn.  Bytes 0, 1, 2
    of a drawn pixel hold (r, g, b), as in the reference."""
    L = lib()
    T = np.ascontiguousarray(T_lidar2cam, dtype=np.float64).reshape(16)
    w, h, n = C.c_int32(0), C.c_int32(0), C.c_uint32(0)
    args = (device, os.fsencode(image_bag), image_topic.encode(), os.fsencode(lidar_bag if lidar_bag is not None else image_bag),
            lidar_topic.encode(), C.byref(camera), T.ctypes.data_as(C.POINTER(C.c_double)), distance_valid)
    st = L.ilcc_bag_pcd2image(*args, None, 0, C.byref(w), C.byref(h), C.byref(n))
    if st not in (_native.OK, _native.CAPACITY):
        raise CameraImageError(st)
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(L.ilcc_bag_pcd2image(*args, out.ctypes.data_as(C.c_void_p), out.size, C.byref(w), C.byref(h), C.byref(n)))
    return out, n.value


def save_ppm_bgr(filename, bgr):
    """Binary PPM (P6) of a (rows, cols, 3) B,G,R image, written as R,G,B."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("expected (rows, cols, 3) uint8, got %s" % (a.shape,))
    _check(lib().ilcc_save_ppm_bgr(os.fsencode(filename), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))


# ------------------------------------------------------------------------------------------ include/ilcc_overlay_sequence.h

def _last_error():
    return _native.lib().ilcc_last_error(None).decode()


class OverlayPlan:
    """The table memory of K12b for batches of at most `max_scans` scans and `max_points` points (on the current device)."""

    def __init__(self, max_scans: int, max_points: int):
        self._p = lib().ilcc_overlay_plan_create(int(max_scans), int(max_points))
        if not self._p:
            raise OverlayError(_native.HIP_ERROR, _last_error())

    @property
    def launches(self) -> int:
        return int(lib().ilcc_overlay_plan_launches(self._p))

    def finish(self, n_scans: int) -> np.ndarray:
        """Waits for the plan's last call -> its n_drawn [n_scans] uint32."""
        out = np.zeros(max(1, int(n_scans)), np.uint32)
        st = lib().ilcc_overlay_plan_finish(self._p, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st != _native.OK:
            raise OverlayError(st, _last_error())
        return out[:int(n_scans)]

    def close(self):
        if self._p:
            lib().ilcc_overlay_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def overlay_batch_scratch_bytes(width: int, height: int, n_scans: int) -> int:
    return int(lib().ilcc_overlay_batch_scratch_bytes(int(width), int(height), int(n_scans)))


def overlay_batch_job(d_xyzi_ptr, offsets, image_ptrs, image_steps, image_of_scan, cam, d_canvas_ptr, canvas_stride, canvas_pitch, d_scratch_ptr,
                      scratch_bytes, plan, distance_valid=50.0, inten_low=0.0, inten_high=60.0, stamp=None, stream=0):
    """-> (OverlayBatchJob, the host arrays it points to: keep them until the call has returned)"""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_scans = len(off) - 1
    of = np.ascontiguousarray(image_of_scan, dtype=np.int32)
    assert len(of) == n_scans and len(image_ptrs) == len(image_steps)
    n_images = len(image_ptrs)
    ptrs = (C.c_void_p * max(1, n_images))(*[None if p is None else int(p) for p in image_ptrs])
    steps = np.ascontiguousarray(image_steps, dtype=np.uint32)
    xy, n_stamp = None, 0
    if stamp is not None:
        flat = [int(v) for pair in stamp for v in pair]
        xy, n_stamp = (C.c_int8 * max(1, len(flat)))(*flat), len(flat) // 2
    cam_copy = Projection.from_buffer_copy(cam)
    job = OverlayBatchJob()
    job.d_xyzi = d_xyzi_ptr
    job.offsets = off.ctypes.data_as(C.POINTER(C.c_uint64))
    job.d_images_bgr = C.cast(ptrs, C.POINTER(C.c_void_p))
    job.image_steps = steps.ctypes.data_as(C.POINTER(C.c_uint32))
    job.image_of_scan = of.ctypes.data_as(C.POINTER(C.c_int32))
    job.cam = C.pointer(cam_copy)
    job.stamp_xy = C.cast(xy, C.POINTER(C.c_int8)) if xy is not None else None
    job.d_canvas, job.d_scratch = d_canvas_ptr, d_scratch_ptr
    job.plan = plan._p if plan is not None else None
    job.hip_stream = stream
    job.canvas_pitch, job.scratch_bytes = int(canvas_pitch), int(scratch_bytes)
    job.distance_valid, job.inten_low, job.inten_high = float(distance_valid), float(inten_low), float(inten_high)
    job.n_scans, job.n_images, job.canvas_stride, job.n_stamp = n_scans, n_images, int(canvas_stride), n_stamp
    return job, (off, of, ptrs, steps, xy, cam_copy)


def overlay_batch_device(d_xyzi_ptr: int, offsets, image_ptrs, image_steps, image_of_scan, cam: Projection, d_canvas_ptr: int, canvas_stride: int,
                         canvas_pitch: int, d_scratch_ptr: int, scratch_bytes: int, plan: OverlayPlan, distance_valid: float = 50.0,
                         inten_low: float = 0.0, inten_high: float = 60.0, stamp=None, stream: int = 0) -> None:
    """K12b on the given hipStream_t (0 = default stream); asynchronous: ``plan.finish(n_scans)`` waits and returns n_drawn.
    `offsets` [n_scans + 1] points (K0b's), `image_ptrs` / `image_steps` the device B,G,R images, `image_of_scan` [n_scans] an index
    into them or -1; scan s is drawn on a copy of its image at d_canvas_ptr + s * canvas_pitch, rows canvas_stride apart.  stamp: None
    for the reference's 5 pixels, else up to 64 (dx, dy) pairs."""
    job, keep = overlay_batch_job(d_xyzi_ptr, offsets, image_ptrs, image_steps, image_of_scan, cam, d_canvas_ptr, canvas_stride, canvas_pitch,
                                  d_scratch_ptr, scratch_bytes, plan, distance_valid, inten_low, inten_high, stamp, stream)
    st = lib().ilcc_overlay_batch_device(C.byref(job))
    del keep
    if st != _native.OK:
        raise OverlayError(st, _last_error())


def overlay_sequence_bytes(width: int, height: int, out_bytes_per_image: int = 0) -> int:
    """Device bytes one paired scan takes in ``bag_pcd2image_all_pairs`` (0: a refused size)."""
    return int(lib().ilcc_overlay_sequence_bytes(int(width), int(height), int(out_bytes_per_image)))


def default_overlay_sequence_params() -> OverlaySequenceParams:
    sp = OverlaySequenceParams()
    lib().ilcc_default_overlay_sequence_params(C.byref(sp))
    return sp


def bag_pcd2image_all_pairs(image_bag, image_topic, lidar_topic, camera: CameraModel, T_lidar2cam, lidar_bag=None, distance_valid=5.0, quality=95,
                            sp=None, device=0):
    """Generator over every selected scan of the LiDAR topic, in scan order: (OverlayRecord, jpeg bytes, pixels), the scan drawn on
    the image whose header stamp is nearest to its own.  `pixels` is the (rows, cols, 3) uint8 B,G,R picture with ``sp.keep_pixels``,
    else None; an unpaired scan comes with ``image_message == -1``, None and None.  The chain runs when the first item is asked
    for; a failure raises OverlayError."""
    sp = sp if sp is not None else default_overlay_sequence_params()
    T = np.ascontiguousarray(T_lidar2cam, dtype=np.float64).reshape(16)
    w, h = int(camera.width), int(camera.height)
    items = []

    def on_scan(_user, rec, jpeg, jpeg_bytes, bgr):
        r = OverlayRecord.from_buffer_copy(rec.contents)
        blob = C.string_at(jpeg, int(jpeg_bytes)) if jpeg else None
        pixels = np.frombuffer(C.string_at(bgr, 3 * w * h), np.uint8).reshape(h, w, 3).copy() if bgr else None
        items.append((r, blob, pixels))
        return 0

    n_scans, n_paired = C.c_uint32(0), C.c_uint32(0)
    st = lib().ilcc_bag_pcd2image_all_pairs(int(device), os.fsencode(image_bag), image_topic.encode(),
                                            os.fsencode(lidar_bag if lidar_bag is not None else image_bag), lidar_topic.encode(), C.byref(camera),
                                            T.ctypes.data_as(C.POINTER(C.c_double)), float(distance_valid), int(quality), C.byref(sp), OVERLAY_SINK(on_scan),
                                            None, C.byref(n_scans), C.byref(n_paired))
    if st != _native.OK:
        raise OverlayError(st, _last_error())
    assert len(items) == n_scans.value
    yield from items


def write_pcd2image_files(items, jpg_prefix, ppm_prefix=None):
    """Writes ``<jpg_prefix><cloud message, 6 digits>.jpg`` (and ``<ppm_prefix>...ppm`` for items that carry pixels) for every paired
    scan of `items` (what bag_pcd2image_all_pairs yields), as ``ilcc_pcd2image --all-pairs`` does.  -> the list of files written."""
    written = []
    for rec, blob, pixels in items:
        if rec.image_message < 0:
            continue
        path = "%s%06d.jpg" % (jpg_prefix, rec.message)
        with open(path, "wb") as f:
            f.write(blob)
        written.append(path)
        if ppm_prefix is not None and pixels is not None:
            path = "%s%06d.ppm" % (ppm_prefix, rec.message)
            save_ppm_bgr(path, pixels)
            written.append(path)
    return written
