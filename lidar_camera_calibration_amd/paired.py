"""Every scan of a recording coloured from its time-paired image: ctypes mirror of ``include/ilcc_paired.h``.

``pair_by_stamp`` gives every cloud the image with the nearest header stamp, ``colourise_batch_device`` is K8b (a batch of scans,
each with an image of its own, in three launches), ``save_pcd_xyzrgb`` writes the binary PCD file of an XYZRGB cloud, and
``bag_rgblidar_all_scans`` is the chain bags -> one coloured cloud per scan.  ``tests/paired_ref.py`` restates all four."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import CameraModel
from .project import Projection

PAIRED_EXPORTS = ["ilcc_pair_by_stamp", "ilcc_colourise_plan_create", "ilcc_colourise_plan_destroy", "ilcc_colourise_batch_device",
                  "ilcc_colourise_plan_finish", "ilcc_colourise_plan_launches", "ilcc_save_pcd_xyzrgb", "ilcc_default_paired_params",
                  "ilcc_bag_rgblidar_all_scans"]


class PairedParams(C.Structure):
    _fields_ = [
        ("first", C.c_uint32), ("stride", C.c_uint32), ("max_scans", C.c_uint32),
        ("sample_raw", C.c_int32),
        ("max_dt_ns", C.c_uint64), ("staging_bytes", C.c_uint64), ("image_bytes", C.c_uint64),
    ]


class PairRecord(C.Structure):
    _fields_ = [
        ("message", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
        ("image_message", C.c_int32),
        ("image_stamp_sec", C.c_uint32), ("image_stamp_nsec", C.c_uint32),
        ("dt_ns", C.c_int64),
        ("n_points", C.c_uint64), ("n_coloured", C.c_uint64),
    ]

    def as_tuple(self):
        return tuple(getattr(self, name) for name, _ in self._fields_)


PAIR_SINK = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(PairRecord), C.c_void_p)


class PairedError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = int(status)
        msg = _native.strerror(status)
        super().__init__("%s: %s" % (msg, detail) if detail else msg)


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        vp, u64p, i64p, u32p, i32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        L.ilcc_pair_by_stamp.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64, C.c_uint64, i64p, i64p]
        L.ilcc_pair_by_stamp.restype = C.c_int32
        L.ilcc_colourise_plan_create.argtypes = [C.c_uint32, C.c_uint64]
        L.ilcc_colourise_plan_create.restype = vp
        L.ilcc_colourise_plan_destroy.argtypes = [vp]
        L.ilcc_colourise_plan_destroy.restype = None
        L.ilcc_colourise_batch_device.argtypes = [vp, u64p, C.c_uint32, C.POINTER(vp), u32p, C.c_uint32, i32p, C.POINTER(Projection), C.c_double,
                                                  vp, C.c_uint64, vp, vp]
        L.ilcc_colourise_batch_device.restype = C.c_int32
        L.ilcc_colourise_plan_finish.argtypes = [vp, u64p]
        L.ilcc_colourise_plan_finish.restype = C.c_int32
        L.ilcc_colourise_plan_launches.argtypes = [vp]
        L.ilcc_colourise_plan_launches.restype = C.c_uint32
        L.ilcc_save_pcd_xyzrgb.argtypes = [C.c_char_p, vp, C.c_uint64]
        L.ilcc_save_pcd_xyzrgb.restype = C.c_int32
        L.ilcc_default_paired_params.argtypes = [C.POINTER(PairedParams)]
        L.ilcc_default_paired_params.restype = None
        L.ilcc_bag_rgblidar_all_scans.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(CameraModel),
                                                  C.POINTER(C.c_double), C.c_double, C.POINTER(PairedParams), PAIR_SINK, vp, u32p, u32p]
        L.ilcc_bag_rgblidar_all_scans.restype = C.c_int32
        _ready = True
    return L


def _last_error():
    return _native.lib().ilcc_last_error(None).decode()


def stamp_ns(sec, nsec):
    return int(sec) * 1000000000 + int(nsec)


def pair_by_stamp(cloud_ns, image_ns, max_dt_ns):
    """Header stamps in nanoseconds -> (image_of [n_clouds] int64, -1: none within max_dt_ns; dt_ns [n_clouds] int64, image - cloud of
    the nearest image).  The nearest stamp wins, a tie goes to the lower image index."""
    c = np.ascontiguousarray(cloud_ns, dtype=np.uint64)
    m = np.ascontiguousarray(image_ns, dtype=np.uint64)
    image_of = np.zeros(len(c), np.int64)
    dt = np.zeros(len(c), np.int64)
    st = lib().ilcc_pair_by_stamp(c.ctypes.data_as(C.POINTER(C.c_uint64)), len(c), m.ctypes.data_as(C.POINTER(C.c_uint64)), len(m), int(max_dt_ns),
                                  image_of.ctypes.data_as(C.POINTER(C.c_int64)), dt.ctypes.data_as(C.POINTER(C.c_int64)))
    if st != _native.OK:
        raise PairedError(st)
    return image_of, dt


class ColourisePlan:
    """The table memory of K8b for batches of at most `max_scans` scans and `max_points` points (on the current device)."""

    def __init__(self, max_scans: int, max_points: int):
        self._p = lib().ilcc_colourise_plan_create(int(max_scans), int(max_points))
        if not self._p:
            raise PairedError(_native.HIP_ERROR, _last_error())

    @property
    def launches(self) -> int:
        return int(lib().ilcc_colourise_plan_launches(self._p))

    def finish(self, n_scans: int) -> np.ndarray:
        """Waits for the plan's last call -> its offsets [n_scans + 1] uint64 (records)."""
        out = np.zeros(int(n_scans) + 1, np.uint64)
        st = lib().ilcc_colourise_plan_finish(self._p, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st != _native.OK:
            raise PairedError(st, _last_error())
        return out

    def close(self):
        if self._p:
            lib().ilcc_colourise_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def colourise_batch_device(d_xyzi_ptr: int, offsets, image_ptrs, image_steps, image_of_scan, cam: Projection, d_out_ptr: int, cap_points: int,
                           plan: ColourisePlan, distance_valid: float = 50.0, stream: int = 0) -> None:
    """K8b on the given hipStream_t (0 = default stream); asynchronous: ``plan.finish(n_scans)`` waits and returns the record
    offsets.  `offsets` [n_scans + 1] points (K0b's), `image_ptrs` / `image_steps` the device B,G,R images, `image_of_scan` [n_scans]
    an index into them or -1."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_scans = len(off) - 1
    of = np.ascontiguousarray(image_of_scan, dtype=np.int32)
    assert len(of) == n_scans and len(image_ptrs) == len(image_steps)
    n_images = len(image_ptrs)
    ptrs = (C.c_void_p * max(1, n_images))(*[int(p) for p in image_ptrs])
    steps = np.ascontiguousarray(image_steps, dtype=np.uint32)
    st = lib().ilcc_colourise_batch_device(C.c_void_p(d_xyzi_ptr), off.ctypes.data_as(C.POINTER(C.c_uint64)), n_scans, ptrs,
                                           steps.ctypes.data_as(C.POINTER(C.c_uint32)), n_images, of.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.byref(cam), float(distance_valid), C.c_void_p(d_out_ptr), int(cap_points), plan._p, C.c_void_p(stream))
    if st != _native.OK:
        raise PairedError(st, _last_error())


def save_pcd_xyzrgb(filename, xyzrgb) -> None:
    """Binary PCD (FIELDS x y z rgb) of (n, 4) float32 records, the 4th column PCL's packed rgb as bits."""
    a = np.ascontiguousarray(xyzrgb, dtype=np.float32).reshape(-1, 4)
    st = lib().ilcc_save_pcd_xyzrgb(os.fsencode(filename), a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a))
    if st != _native.OK:
        raise PairedError(st, "can not write %s" % filename)


def default_paired_params() -> PairedParams:
    pp = PairedParams()
    lib().ilcc_default_paired_params(C.byref(pp))
    return pp


def bag_rgblidar_all_scans(image_bag, image_topic, lidar_topic, camera: CameraModel, T_lidar2cam, lidar_bag=None, distance_valid=5.0, pp=None,
                           device=0):
    """Generator over every selected scan of the LiDAR topic, in scan order: (PairRecord, (n_coloured, 4) float32 records), the scan
    coloured from the image whose header stamp is nearest to its own; an unpaired scan comes with ``image_message == -1`` and no
    records.  The chain runs when the first item is asked for; a failure raises PairedError."""
    pp = pp if pp is not None else default_paired_params()
    T = np.ascontiguousarray(T_lidar2cam, dtype=np.float64).reshape(16)
    items = []

    def on_scan(_user, rec, xyzrgb):
        r = PairRecord.from_buffer_copy(rec.contents)
        n = int(r.n_coloured)
        cloud = np.frombuffer(C.string_at(xyzrgb, 16 * n), np.float32).reshape(n, 4).copy() if n else np.zeros((0, 4), np.float32)
        items.append((r, cloud))
        return 0

    n_scans, n_paired = C.c_uint32(0), C.c_uint32(0)
    st = lib().ilcc_bag_rgblidar_all_scans(int(device), os.fsencode(image_bag), image_topic.encode(),
                                           os.fsencode(lidar_bag if lidar_bag is not None else image_bag), lidar_topic.encode(), C.byref(camera),
                                           T.ctypes.data_as(C.POINTER(C.c_double)), float(distance_valid), C.byref(pp), PAIR_SINK(on_scan), None,
                                           C.byref(n_scans), C.byref(n_paired))
    if st != _native.OK:
        raise PairedError(st, _last_error())
    assert len(items) == n_scans.value
    yield from items


def write_rgblidar_pcds(items, out_dir, merged=None):
    """Writes ``out_dir/rgb_lidar_<k>.pcd`` for the k-th PAIRED scan of `items` (what bag_rgblidar_all_scans yields), and all their
    records as one cloud into `merged` when given.  -> the list of files written, the merged one last."""
    written, clouds = [], []
    for rec, cloud in items:
        if rec.image_message < 0:
            continue
        path = os.path.join(out_dir, "rgb_lidar_%d.pcd" % len(written))
        save_pcd_xyzrgb(path, cloud)
        written.append(path)
        clouds.append(cloud)
    if merged is not None:
        save_pcd_xyzrgb(merged, np.concatenate(clouds) if clouds else np.zeros((0, 4), np.float32))
        written.append(merged)
    return written
