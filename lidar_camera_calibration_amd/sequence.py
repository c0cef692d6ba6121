"""Corners from every scan of a recording: ctypes mirror of ``include/ilcc_sequence.h``.

``bag_messages`` iterates every message of a bag topic in time order, ``unpack_batch_device`` is K0b (a batch of PointCloud2
``data[]`` -> concatenated float4 clouds in a fixed number of launches), ``fuse_corners`` merges per-scan corner sets on the
host, and ``bag_corners_all_scans`` is the chain bag -> fused corners.  ``tests/sequence_ref.py`` restates the first three."""
import ctypes as C
import os

import numpy as np

from . import _native
from ._native import MAX_CORNERS, Result
from .ingest import IngestError, Layout

SEQUENCE_EXPORTS = ["ilcc_bag_topic_open", "ilcc_bag_topic_count", "ilcc_bag_topic_time", "ilcc_bag_topic_read", "ilcc_bag_topic_close",
                    "ilcc_unpack_plan_create", "ilcc_unpack_plan_destroy", "ilcc_unpack_plan_launches",
                    "ilcc_pointcloud2_unpack_batch_device", "ilcc_fuse_corners", "ilcc_default_sequence_params",
                    "ilcc_bag_corners_all_scans"]
SEED_CLICK, SEED_AUTO, SEED_AUTO_PLANAR = 0, 1, 2
AUTO_TRIES = 8


class FusedCorners(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_scans", C.c_int32), ("n_ok", C.c_int32), ("n_used", C.c_int32),
        ("ref_scan", C.c_int32),
        ("n_corners", C.c_int32),
        ("spread_rms", C.c_double), ("spread_max", C.c_double),
        ("corners", C.c_float * (MAX_CORNERS * 3)),
    ]

    def corners_array(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.corners)[:3 * self.n_corners].reshape(-1, 3).copy()


class SequenceParams(C.Structure):
    _fields_ = [
        ("first", C.c_uint32), ("stride", C.c_uint32), ("max_scans", C.c_uint32),
        ("accept_ambiguous", C.c_int32), ("accept_low_coverage", C.c_int32),
        ("reserved0", C.c_int32),
        ("gate", C.c_double),
        ("staging_bytes", C.c_uint64),
    ]


class SequenceResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_scans", C.c_int32), ("n_ok", C.c_int32), ("n_used", C.c_int32),
        ("ref_scan", C.c_int32),
        ("n_corners", C.c_int32),
        ("spread_rms", C.c_double), ("spread_max", C.c_double),
        ("click", C.c_float * 3),
        ("n_batches", C.c_int32),
        ("corners", C.c_float * (MAX_CORNERS * 3)),
    ]

    def corners_array(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.corners)[:3 * self.n_corners].reshape(-1, 3).copy()


class ScanRecord(C.Structure):
    _fields_ = [
        ("result", Result),
        ("message", C.c_uint32),
        ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
        ("time_sec", C.c_uint32), ("time_nsec", C.c_uint32),
        ("accepted", C.c_int32), ("used", C.c_int32),
        ("reserved0", C.c_int32),
        ("distance", C.c_double),
    ]


class SequenceError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = int(status)
        msg = _native.strerror(status)
        super().__init__("%s: %s" % (msg, detail) if detail else msg)


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        vp, u8p, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        L.ilcc_bag_topic_open.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp)]
        L.ilcc_bag_topic_open.restype = C.c_int32
        L.ilcc_bag_topic_count.argtypes = [vp]
        L.ilcc_bag_topic_count.restype = C.c_uint64
        L.ilcc_bag_topic_time.argtypes = [vp, C.c_uint64, u32p, u32p]
        L.ilcc_bag_topic_time.restype = C.c_int32
        L.ilcc_bag_topic_read.argtypes = [vp, C.c_uint64, u8p, C.c_uint64, u64p]
        L.ilcc_bag_topic_read.restype = C.c_int32
        L.ilcc_bag_topic_close.argtypes = [vp]
        L.ilcc_bag_topic_close.restype = None
        L.ilcc_unpack_plan_create.argtypes = [C.c_uint32]
        L.ilcc_unpack_plan_create.restype = vp
        L.ilcc_unpack_plan_destroy.argtypes = [vp]
        L.ilcc_unpack_plan_destroy.restype = None
        L.ilcc_unpack_plan_launches.argtypes = [vp]
        L.ilcc_unpack_plan_launches.restype = C.c_uint32
        L.ilcc_pointcloud2_unpack_batch_device.argtypes = [vp, C.c_uint64, C.POINTER(Layout), u64p, C.c_uint32, vp, C.c_uint64, u64p, vp, vp]
        L.ilcc_pointcloud2_unpack_batch_device.restype = C.c_int32
        L.ilcc_fuse_corners.argtypes = [C.POINTER(C.c_float), u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(FusedCorners),
                                        u8p, C.POINTER(C.c_double)]
        L.ilcc_fuse_corners.restype = C.c_int32
        L.ilcc_default_sequence_params.argtypes = [C.POINTER(SequenceParams)]
        L.ilcc_default_sequence_params.restype = None
        L.ilcc_bag_corners_all_scans.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(SequenceParams),
                                                 C.POINTER(SequenceResult), C.POINTER(ScanRecord), C.c_uint32]
        L.ilcc_bag_corners_all_scans.restype = C.c_int32
        _ready = True
    return L


def _last_error():
    return _native.lib().ilcc_last_error(None).decode()


class BagTopic:
    """Every message on `topic` whose connection carries `md5sum` (None: PointCloud2's), in record-time order; ties by the
    chunk's position in the file, then by the offset inside the chunk.  ``len()``, ``time(i)`` -> (sec, nsec), ``read(i)`` ->
    bytes; a context manager."""

    def __init__(self, bag_path, topic, md5sum=None):
        self._it = C.c_void_p()
        st = lib().ilcc_bag_topic_open(os.fsencode(bag_path), topic.encode(), md5sum.encode() if md5sum else None, C.byref(self._it))
        if st != _native.OK:
            self._it = C.c_void_p()
            raise IngestError(st)

    def __len__(self):
        return int(lib().ilcc_bag_topic_count(self._it))

    def time(self, i):
        sec, nsec = C.c_uint32(0), C.c_uint32(0)
        st = lib().ilcc_bag_topic_time(self._it, int(i), C.byref(sec), C.byref(nsec))
        if st != _native.OK:
            raise IngestError(st)
        return sec.value, nsec.value

    def size(self, i) -> int:
        n = C.c_uint64(0)
        st = lib().ilcc_bag_topic_read(self._it, int(i), None, 0, C.byref(n))
        if st not in (_native.OK, _native.CAPACITY):
            raise IngestError(st)
        return n.value

    def read(self, i) -> bytes:
        n = self.size(i)
        buf = (C.c_uint8 * max(1, n))()
        got = C.c_uint64(0)
        st = lib().ilcc_bag_topic_read(self._it, int(i), buf, n, C.byref(got))
        if st != _native.OK:
            raise IngestError(st)
        return bytes(buf[:got.value])

    def close(self):
        if self._it:
            lib().ilcc_bag_topic_close(self._it)
            self._it = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bag_messages(bag_path, topic, md5sum=None):
    """Yields ((sec, nsec), message bytes) for every message of the topic, in the iterator's order."""
    with BagTopic(bag_path, topic, md5sum) as it:
        for i in range(len(it)):
            yield it.time(i), it.read(i)


class UnpackPlan:
    """The table memory of K0b for batches of at most `max_msgs` messages (on the current device)."""

    def __init__(self, max_msgs: int):
        self._p = lib().ilcc_unpack_plan_create(int(max_msgs))
        if not self._p:
            raise SequenceError(_native.HIP_ERROR, _last_error())

    @property
    def launches(self) -> int:
        return int(lib().ilcc_unpack_plan_launches(self._p))

    def close(self):
        if self._p:
            lib().ilcc_unpack_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unpack_batch_device(d_blob_ptr: int, blob_bytes: int, layouts, src_offsets, d_xyzi_ptr: int, cap_points: int, plan: UnpackPlan,
                        stream: int = 0) -> np.ndarray:
    """K0b on the given hipStream_t (0 = default stream); asynchronous.  `layouts`: sequence of ingest.Layout, `src_offsets`: the
    byte offset of each message's data[] inside the blob.  -> offsets [n + 1] uint64 (points)."""
    n = len(layouts)
    arr = (Layout * max(1, n))(*layouts)
    src = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    assert len(src) == n
    offsets = np.zeros(n + 1, np.uint64)
    st = lib().ilcc_pointcloud2_unpack_batch_device(C.c_void_p(d_blob_ptr), int(blob_bytes), arr, src.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                                    C.c_void_p(d_xyzi_ptr), int(cap_points), offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    plan._p, C.c_void_p(stream))
    if st != _native.OK:
        raise SequenceError(st, _last_error())
    return offsets


def fuse_corners(corners, accepted, a: int, b: int, gate: float):
    """corners [n, a*b, 3] float32, accepted [n] -> (FusedCorners, used [n] bool, dist [n] float64); the status is in the record,
    nothing is raised for ILCC_AMBIGUOUS / ILCC_BOARD_NOT_FOUND / ILCC_BAD_ARGUMENT."""
    corners = np.ascontiguousarray(corners, dtype=np.float32)
    acc = np.ascontiguousarray(np.asarray(accepted) != 0, dtype=np.uint8)
    n = len(acc)
    assert corners.size == n * a * b * 3
    out = FusedCorners()
    used = np.zeros(max(n, 1), np.uint8)
    dist = np.zeros(max(n, 1), np.float64)
    lib().ilcc_fuse_corners(_native.fptr(corners), acc.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(a), int(b), float(gate), C.byref(out),
                            used.ctypes.data_as(C.POINTER(C.c_uint8)), dist.ctypes.data_as(C.POINTER(C.c_double)))
    return out, used[:n].astype(bool), dist[:n]


def default_sequence_params() -> SequenceParams:
    sp = SequenceParams()
    lib().ilcc_default_sequence_params(C.byref(sp))
    return sp


def bag_corners_all_scans(est, bag_path, topic="/velodyne_points", click=None, seed_mode=SEED_CLICK, sp=None, per_scan=True):
    """Every selected scan of the topic through `est` (a LidarCornersBatch: anything with the library handle in ``_h``), fused.
    -> (SequenceResult, list of ScanRecord or None).  ILCC_AMBIGUOUS / ILCC_BOARD_NOT_FOUND come back in ``result.status``; any other
    failure raises SequenceError."""
    sp = sp if sp is not None else default_sequence_params()
    out = SequenceResult()
    cl = None
    if click is not None:
        cl = np.ascontiguousarray(click, dtype=np.float32)
        assert cl.size == 3
    records, cap = None, 0
    if per_scan:
        with BagTopic(bag_path, topic) as it:
            cap = len(it)
        records = (ScanRecord * max(1, cap))()
    st = lib().ilcc_bag_corners_all_scans(est._h, os.fsencode(bag_path), topic.encode(), _native.fptr(cl) if cl is not None else None,
                                          int(seed_mode), C.byref(sp), C.byref(out), records, cap)
    if st not in (_native.OK, _native.AMBIGUOUS, _native.BOARD_NOT_FOUND):
        raise SequenceError(st, _last_error())
    return out, ([records[i] for i in range(out.n_scans)] if per_scan else None)
