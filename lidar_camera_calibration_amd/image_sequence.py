"""Camera corners from every image of a recording: ctypes mirror of ``include/ilcc_image_sequence.h``.

``find_corners_batch`` is K10b (findCorners on a batch of equal-sized images in at most eight launches, byte for byte what
``image_corners.find_corners`` gives image by image), ``fuse_image_corners`` merges per-image boards on the host, and
``bag_corners_all_images`` is the chain bag -> fused ``<camera><i>.txt`` board.  ``tests/image_sequence_ref.py`` restates the
fusion, the batch cut and the candidate order.

``chessboards_from_corners_batch`` is K18 (``include/ilcc_image_structure.h``): the boards of a batch of corner lists in two
launches, each what ``image_corners.chessboard_from_corners`` gives for that list alone; ``seed_board`` is its stage output, from
the device or from the host code.  ``structure="gpu"`` sends a chain's structure recovery through it."""
import ctypes as C
import os

import numpy as np

from . import _native
from ._native import MAX_CORNERS
from .camera_image import CameraModel
from .image_corners import CORNER_DTYPE, BoardNotFound, ImageCorner

IMAGE_SEQUENCE_EXPORTS = ["ilcc_image_corner_plan_create", "ilcc_image_corner_plan_destroy", "ilcc_image_corners_batch_device",
                          "ilcc_image_corner_plan_launches", "ilcc_image_corner_plan_allocations", "ilcc_image_corner_plan_candidates",
                          "ilcc_image_corner_scratch_bytes", "ilcc_fuse_image_corners", "ilcc_default_image_sequence_params",
                          "ilcc_image_sequence_cut", "ilcc_bag_corners_all_images"]
IMAGE_STRUCTURE_EXPORTS = ["ilcc_structure_plan_create", "ilcc_structure_plan_destroy", "ilcc_chessboards_from_corners_batch",
                           "ilcc_structure_plan_launches", "ilcc_structure_plan_fallbacks", "ilcc_structure_plan_allocations",
                           "ilcc_structure_plan_seed_board", "ilcc_chessboard_seed_board"]
STRUCTURE_MAX_CORNERS = 4096     # ILCC_STRUCTURE_MAX_CORNERS: corners of one image on the device path
STRUCTURE_ROUTES = {"host": 0, "gpu": 1}


def structure_route(structure) -> int:
    """reserved0 of ImageSequenceParams for `structure`: "host" / "gpu", or the number itself (the C entry refuses one above 1)"""
    if isinstance(structure, str):
        if structure not in STRUCTURE_ROUTES:
            raise ValueError('structure must be "host" or "gpu", got %r' % (structure,))
        return STRUCTURE_ROUTES[structure]
    return int(structure)


class FusedImageCorners(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_images", C.c_int32), ("n_ok", C.c_int32), ("n_used", C.c_int32),
        ("ref_image", C.c_int32),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("reserved0", C.c_int32),
        ("gate", C.c_double),
        ("spread_rms", C.c_double), ("spread_max", C.c_double),
        ("xy", C.c_double * (MAX_CORNERS * 2)),
    ]

    def board(self) -> np.ndarray:
        """(rows, cols, 2) float64, 0-based (u, v); empty without a fused board"""
        n = self.rows * self.cols if self.status == _native.OK else 0
        return np.ctypeslib.as_array(self.xy)[:2 * n].reshape(-1, max(self.cols, 1), 2).copy() if n else np.zeros((0, 0, 2))


class ImageSequenceParams(C.Structure):
    _fields_ = [
        ("first", C.c_uint32), ("stride", C.c_uint32), ("max_images", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("gate_px", C.c_double),
        ("staging_bytes", C.c_uint64),
        ("device_bytes", C.c_uint64),
    ]


class ImageRecord(C.Structure):
    _fields_ = [
        ("message", C.c_uint32),
        ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
        ("time_sec", C.c_uint32), ("time_nsec", C.c_uint32),
        ("status", C.c_int32),
        ("n_corners", C.c_int32),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("accepted", C.c_int32), ("used", C.c_int32),
        ("reserved0", C.c_int32),
        ("distance", C.c_double),
        ("xy", C.c_double * (MAX_CORNERS * 2)),
    ]

    def board(self) -> np.ndarray:
        n = self.rows * self.cols
        return np.ctypeslib.as_array(self.xy)[:2 * n].reshape(-1, max(self.cols, 1), 2).copy() if n else np.zeros((0, 0, 2))


class ImageSequenceResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_images", C.c_int32), ("n_ok", C.c_int32), ("n_used", C.c_int32),
        ("ref_image", C.c_int32),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("n_batches", C.c_int32),
        ("gate", C.c_double),
        ("spread_rms", C.c_double), ("spread_max", C.c_double),
        ("host_recovery_ms", C.c_double),
        ("xy", C.c_double * (MAX_CORNERS * 2)),
    ]

    def board(self) -> np.ndarray:
        n = self.rows * self.cols if self.status == _native.OK else 0
        return np.ctypeslib.as_array(self.xy)[:2 * n].reshape(-1, max(self.cols, 1), 2).copy() if n else np.zeros((0, 0, 2))


class ImageSequenceError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = int(status)
        msg = _native.strerror(status)
        super().__init__("%s: %s" % (msg, detail) if detail else msg)


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        vp, u8p, u32p, i32p, f64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        L.ilcc_image_corner_plan_create.argtypes = [C.c_uint32, C.c_int32, C.c_int32]
        L.ilcc_image_corner_plan_create.restype = vp
        L.ilcc_image_corner_plan_destroy.argtypes = [vp]
        L.ilcc_image_corner_plan_destroy.restype = None
        L.ilcc_image_corners_batch_device.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, i32p, vp, vp]
        L.ilcc_image_corners_batch_device.restype = C.c_int32
        L.ilcc_image_corner_plan_launches.argtypes = [vp]
        L.ilcc_image_corner_plan_launches.restype = C.c_uint32
        L.ilcc_image_corner_plan_allocations.argtypes = [vp]
        L.ilcc_image_corner_plan_allocations.restype = C.c_uint32
        L.ilcc_image_corner_plan_candidates.argtypes = [vp, i32p, C.c_uint32, u32p]
        L.ilcc_image_corner_plan_candidates.restype = C.c_int32
        L.ilcc_image_corner_scratch_bytes.argtypes = [C.c_int32, C.c_int32]
        L.ilcc_image_corner_scratch_bytes.restype = C.c_uint64
        L.ilcc_fuse_image_corners.argtypes = [f64p, i32p, i32p, u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                              C.POINTER(FusedImageCorners), u8p, f64p]
        L.ilcc_fuse_image_corners.restype = C.c_int32
        L.ilcc_default_image_sequence_params.argtypes = [C.POINTER(ImageSequenceParams)]
        L.ilcc_default_image_sequence_params.restype = None
        L.ilcc_image_sequence_cut.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, u32p, u32p]
        L.ilcc_image_sequence_cut.restype = C.c_int32
        L.ilcc_bag_corners_all_images.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.POINTER(CameraModel), C.c_int32, C.c_int32,
                                                  C.POINTER(ImageSequenceParams), C.POINTER(ImageSequenceResult), C.POINTER(ImageRecord),
                                                  C.c_uint32]
        L.ilcc_bag_corners_all_images.restype = C.c_int32
        L.ilcc_structure_plan_create.argtypes = [C.c_uint32, C.c_uint32]
        L.ilcc_structure_plan_create.restype = vp
        L.ilcc_structure_plan_destroy.argtypes = [vp]
        L.ilcc_structure_plan_destroy.restype = None
        L.ilcc_chessboards_from_corners_batch.argtypes = [vp, C.c_int32, i32p, C.c_uint32, C.c_int32, C.c_int32, i32p, i32p, i32p, i32p, vp, vp]
        L.ilcc_chessboards_from_corners_batch.restype = C.c_int32
        for name in ("launches", "fallbacks", "allocations"):
            fn = getattr(L, "ilcc_structure_plan_" + name)
            fn.argtypes = [vp]
            fn.restype = C.c_uint32
        L.ilcc_structure_plan_seed_board.argtypes = [vp, C.c_uint32, C.c_uint32, i32p, i32p, i32p, C.c_int32, f64p]
        L.ilcc_structure_plan_seed_board.restype = C.c_int32
        L.ilcc_chessboard_seed_board.argtypes = [vp, C.c_int32, C.c_int32, i32p, i32p, i32p, C.c_int32, f64p]
        L.ilcc_chessboard_seed_board.restype = C.c_int32
        _ready = True
    return L


def _last_error():
    return _native.lib().ilcc_last_error(None).decode()


def _check(st):
    if st in (_native.BOARD_NOT_FOUND, _native.AMBIGUOUS):
        raise BoardNotFound(st, "%s: %s" % (_native.strerror(st), _last_error()))
    if st != _native.OK:
        raise ImageSequenceError(st, _last_error())


class CornerPlan:
    """A K10b plan on the current device: all scratch for up to `max_images` images of `max_width` x `max_height`.  One call at a
    time; ``close()`` (or the context manager) frees it."""

    def __init__(self, max_images, max_width, max_height):
        self._p = lib().ilcc_image_corner_plan_create(int(max_images), int(max_width), int(max_height))
        if not self._p:
            raise ImageSequenceError(_native.HIP_ERROR, _last_error())
        self.max_images, self.max_width, self.max_height = int(max_images), int(max_width), int(max_height)

    def fits(self, n, w, h):
        return self._p and n <= self.max_images and w <= self.max_width and h <= self.max_height

    @property
    def launches(self):
        return lib().ilcc_image_corner_plan_launches(self._p)

    @property
    def allocations(self):
        return lib().ilcc_image_corner_plan_allocations(self._p)

    def candidates(self, n_images, capacity=1 << 16):
        """The last call's compacted NMS maxima: ([total, 3] int32 of (image, u, v), 1-based u, v; offsets [n_images + 1])."""
        cand = np.zeros((capacity, 3), np.int32)
        off = np.zeros(n_images + 1, np.uint32)
        st = lib().ilcc_image_corner_plan_candidates(self._p, cand.ctypes.data_as(C.POINTER(C.c_int32)), capacity,
                                                     off.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st == _native.CAPACITY:
            return self.candidates(n_images, int(off[-1]))
        _check(st)
        return cand[:off[-1]].copy(), off

    def close(self):
        if self._p:
            lib().ilcc_image_corner_plan_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _device_batch(images):
    """(device tensor, n, width, height, stride, pitch): a uint8 tensor [n, h, w] on the current HIP device.  A tensor already
    there whose rows are contiguous (stride(2) == 1, stride(1) >= width, stride(0) >= stride(1) * height) is passed as it is."""
    import torch
    if isinstance(images, (list, tuple)):
        arrays = [im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im)) for im in images]
        if not arrays:
            return None, 0, 0, 0, 0, 0
        if any(a.shape != arrays[0].shape for a in arrays):
            raise ValueError("the images of a batch must have one shape")
        t = torch.stack([a.to("cuda") for a in arrays])
    else:
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError("expected uint8 grayscale images [n, h, w], got %s %s" % (tuple(t.shape), t.dtype))
    if t.shape[0] == 0:
        return None, 0, int(t.shape[2]), int(t.shape[1]), int(t.shape[2]), 0
    on_device = t.is_cuda and t.device.index == torch.cuda.current_device()
    if not (on_device and t.stride(2) == 1 and t.stride(1) >= t.shape[2] and (t.shape[0] == 1 or t.stride(0) >= t.stride(1) * t.shape[1])):
        t = t.to("cuda").contiguous()
    return t, int(t.shape[0]), int(t.shape[2]), int(t.shape[1]), int(t.stride(1)), int(t.stride(0)) if t.shape[0] > 1 else int(t.stride(1) * t.shape[1])


_plan = None


def find_corners_batch(images, plan=None, capacity=8192):
    """findCorners(img, 0.01, 1) on every image of a batch: a list of structured arrays of CORNER_DTYPE (0-based u, v), each what
    ``image_corners.find_corners`` gives for that image alone.  `images`: a torch uint8 tensor [n, h, w] or a list of
    equal-shaped 2-D arrays.  Without `plan`, a module-level plan is kept and reused while the batches fit it."""
    global _plan
    import torch
    t, n, w, h, stride, pitch = _device_batch(images)
    if n == 0:
        return []
    if plan is None:
        if _plan is None or not _plan.fits(n, w, h):
            if _plan is not None:
                _plan.close()
            _plan = CornerPlan(n, w, h)
        plan = _plan
    while True:
        out = np.zeros((n, capacity), CORNER_DTYPE)
        cnt = np.zeros(n, np.int32)
        st = lib().ilcc_image_corners_batch_device(C.c_void_p(t.data_ptr()), pitch, n, w, h, stride, out.ctypes.data_as(C.c_void_p), capacity,
                                                   cnt.ctypes.data_as(C.POINTER(C.c_int32)), plan._p,
                                                   C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
        if st != _native.CAPACITY:
            break
        capacity = int(cnt.max())
    _check(st)
    return [out[m, :cnt[m]].copy() for m in range(n)]


class StructurePlan:
    """A K18 plan on the current device: all scratch for up to `max_images` corner lists of up to `max_corners` corners.  One call
    at a time; ``close()`` (or the context manager) frees it."""

    def __init__(self, max_images, max_corners):
        self._p = lib().ilcc_structure_plan_create(int(max_images), int(max_corners))
        if not self._p:
            raise ImageSequenceError(_native.HIP_ERROR, _last_error())
        self.max_images, self.max_corners = int(max_images), int(max_corners)

    def fits(self, n, corners):
        return self._p and n <= self.max_images and corners <= self.max_corners

    @property
    def launches(self):
        return lib().ilcc_structure_plan_launches(self._p)

    @property
    def fallbacks(self):
        return lib().ilcc_structure_plan_fallbacks(self._p)

    @property
    def allocations(self):
        return lib().ilcc_structure_plan_allocations(self._p)

    def close(self):
        if self._p:
            lib().ilcc_structure_plan_destroy(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


_structure_plan = None


def chessboards_from_corners_batch(corners_per_image, board=(7, 5), plan=None, capacity=None, stream=None):
    """K18: the board of every corner list of a batch -> (statuses [n] int32, [index matrix or None]): image m's status and
    (rows, cols) int32 matrix of corner indices are what ``image_corners.chessboard_from_corners`` gives for its list alone
    (None without ILCC_OK).  `corners_per_image`: a list of structured arrays of CORNER_DTYPE.  `capacity`: the row length of the
    [n, capacity] array the lists are laid in (the longest list when not given).  `stream`: a torch stream (the current one when
    not given).  Without `plan`, a module-level plan is kept and reused while the batches fit it."""
    global _structure_plan
    import torch
    n = len(corners_per_image)
    a, b = int(board[0]), int(board[1])
    counts = np.array([len(c) for c in corners_per_image], np.int32)
    longest = int(counts.max()) if n else 0
    cap = longest if capacity is None else int(capacity)
    if plan is None:
        if _structure_plan is None or not _structure_plan.fits(n, max(longest, 1)):
            if _structure_plan is not None:
                _structure_plan.close()
            _structure_plan = StructurePlan(max(n, 1), max(longest, 1))
        plan = _structure_plan
    table = np.zeros((max(n, 1), max(cap, 1)), CORNER_DTYPE)
    for m, c in enumerate(corners_per_image):
        table[m, :min(len(c), cap)] = np.asarray(c, CORNER_DTYPE)[:cap]
    cells = max(a * b, 1)
    status, rows, cols = np.full(max(n, 1), -1, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    index = np.full((max(n, 1), cells), -1, np.int32)
    i32p = C.POINTER(C.c_int32)
    s = stream if stream is not None else torch.cuda.current_stream()
    st = lib().ilcc_chessboards_from_corners_batch(table.ctypes.data_as(C.c_void_p), cap, counts.ctypes.data_as(i32p) if n else None, n, a, b,
                                                   status.ctypes.data_as(i32p), rows.ctypes.data_as(i32p), cols.ctypes.data_as(i32p),
                                                   index.ctypes.data_as(i32p), plan._p, C.c_void_p(s.cuda_stream))
    if st != _native.OK:
        raise ImageSequenceError(st, _last_error())
    boards = [index[m, :rows[m] * cols[m]].reshape(rows[m], cols[m]).copy() if status[m] == _native.OK else None for m in range(n)]
    return status[:n].copy(), boards


def seed_board(corners=None, seed=0, plan=None, image=0):
    """The board a seed corner grows to BEFORE the overlap rule -> ((rows, cols) int32 index matrix or None, energy).  With
    `corners` (a structured array of CORNER_DTYPE) from the host code, ilcc_chessboard_seed_board; with `plan` and `image` from
    K18's stage output of the plan's last call, ilcc_structure_plan_seed_board."""
    rows, cols, energy = C.c_int32(0), C.c_int32(0), C.c_double(0)
    index = np.zeros(MAX_CORNERS, np.int32)
    i32p = C.POINTER(C.c_int32)
    if plan is not None:
        st = lib().ilcc_structure_plan_seed_board(plan._p, int(image), int(seed), C.byref(rows), C.byref(cols), index.ctypes.data_as(i32p),
                                                  index.size, C.byref(energy))
    else:
        c = np.ascontiguousarray(corners, CORNER_DTYPE)
        st = lib().ilcc_chessboard_seed_board(c.ctypes.data_as(C.c_void_p), len(c), int(seed), C.byref(rows), C.byref(cols),
                                              index.ctypes.data_as(i32p), index.size, C.byref(energy))
    if st != _native.OK:
        raise ImageSequenceError(st, _last_error())
    if rows.value == 0:
        return None, float(energy.value)
    return index[:rows.value * cols.value].reshape(rows.value, cols.value).copy(), float(energy.value)


def fuse_image_corners(boards, accepted, board=(7, 5), gate_px=0.0):
    """ilcc_fuse_image_corners: `boards` is a list of (rows, cols, 2) arrays (None or anything for a non-accepted image).
    -> (FusedImageCorners, used flags, distances)."""
    a, b = int(board[0]), int(board[1])
    n = len(accepted)
    size = 2 * a * b if a > 0 and b > 0 else 0
    xy = np.full((n, max(size, 1)), np.nan)
    rows, cols = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, bd in enumerate(boards):
        if bd is None:
            continue
        arr = np.asarray(bd, np.float64)
        if arr.ndim == 3 and arr.shape[2] == 2:
            rows[i], cols[i] = arr.shape[0], arr.shape[1]
            flat = arr.reshape(-1)[:size]
            xy[i, :len(flat)] = flat
    acc = np.ascontiguousarray(np.asarray(accepted) != 0, dtype=np.uint8)
    used = np.zeros(max(n, 1), np.uint8)
    dist = np.zeros(max(n, 1))
    out = FusedImageCorners()
    u8p, f64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib().ilcc_fuse_image_corners(xy.ctypes.data_as(f64p), rows.ctypes.data_as(i32p), cols.ctypes.data_as(i32p), acc.ctypes.data_as(u8p), n, max(a, 0),
                                  max(b, 0), float(gate_px), C.byref(out), used.ctypes.data_as(u8p), dist.ctypes.data_as(f64p))
    return out, used[:n].astype(bool), dist[:n].copy()


def default_params() -> ImageSequenceParams:
    sp = ImageSequenceParams()
    lib().ilcc_default_image_sequence_params(C.byref(sp))
    return sp


def scratch_bytes(width, height) -> int:
    return int(lib().ilcc_image_corner_scratch_bytes(int(width), int(height)))


def sequence_cut(raw_bytes, device_bytes_per_image, staging_bytes=0, device_bytes=0):
    """ilcc_image_sequence_cut -> the list of each batch's first image, the image count at the end.  Raises on ILCC_CAPACITY."""
    raw = np.ascontiguousarray(raw_bytes, dtype=np.uint64)
    first = np.zeros(len(raw) + 1, np.uint32)
    nb = C.c_uint32(0)
    st = lib().ilcc_image_sequence_cut(raw.ctypes.data_as(C.POINTER(C.c_uint64)), len(raw), int(device_bytes_per_image), int(staging_bytes),
                                       int(device_bytes), first.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nb))
    if st != _native.OK:
        raise ImageSequenceError(st, "one image is above a budget" if st == _native.CAPACITY else "")
    return [int(v) for v in first[:nb.value + 1]]


def bag_corners_all_images(bag_path, topic, camera=None, board=(7, 5), first=0, stride=1, max_images=0, gate_px=0.0, staging_bytes=0,
                           device_bytes=0, device=0, raise_on_failure=True, structure="host"):
    """Every selected image of the bag's topic -> (ImageSequenceResult, [ImageRecord]).  Raises BoardNotFound when the fusion finds
    no board (none accepted, or no majority within the gate) and ImageSequenceError on a refusal, unless raise_on_failure is
    False (then the result's status says so; the records are complete for the two fusion statuses).  structure: "host", a host
    thread, or "gpu", K18 (chessboards_from_corners_batch), recovers the boards; the records are the same."""
    L = lib()
    sp = default_params()
    sp.reserved0 = structure_route(structure)
    sp.first, sp.stride, sp.max_images, sp.gate_px = int(first), int(stride), int(max_images), float(gate_px)
    if staging_bytes:
        sp.staging_bytes = int(staging_bytes)
    if device_bytes:
        sp.device_bytes = int(device_bytes)
    out = ImageSequenceResult()
    cam = C.byref(camera) if camera is not None else None
    args = (int(device), os.fsencode(bag_path), topic.encode(), cam, int(board[0]), int(board[1]), C.byref(sp), C.byref(out))
    buf = (ImageRecord * 1)()
    st = L.ilcc_bag_corners_all_images(*args, buf, 1)       # one record is too few for most bags: the refusal says how many, nothing runs
    if st == _native.CAPACITY and out.n_images > 1:
        buf = (ImageRecord * out.n_images)()
        st = L.ilcc_bag_corners_all_images(*args, buf, out.n_images)
    detail = _last_error()
    records = list(buf)[:out.n_images] if st in (_native.OK, _native.BOARD_NOT_FOUND, _native.AMBIGUOUS) else []
    if raise_on_failure:
        if st in (_native.BOARD_NOT_FOUND, _native.AMBIGUOUS):
            raise BoardNotFound(st, "%s: %s" % (_native.strerror(st), detail))
        if st != _native.OK:
            raise ImageSequenceError(st, detail)
    return out, records
