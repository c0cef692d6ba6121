"""Finding the chessboard in a LiDAR scan without a click: ctypes mirror of ``include/ilcc_seed.h`` (K15).

``propose_seeds`` names the board-sized planar patches of whole clouds; ``extract_auto`` runs the ordinary pipeline on
every proposal and keeps, per cloud, the first it accepts.  The ``*_planar`` functions form the components from flat
cells only (K15p), which finds a board that stands on the floor or on a stand.  The functions take a ``LidarCornersBatch`` (anything with
the library handle in ``_h``), whose ``max_frames`` / points bound the candidates of one call."""
import ctypes as C

import numpy as np

from . import _native
from ._native import Params, Result

SEED_EXPORTS = ["ilcc_default_seed_params", "ilcc_seed_scratch_bytes", "ilcc_propose_seeds_device", "ilcc_propose_seeds",
                "ilcc_debug_seed_components", "ilcc_debug_seed_launch_ms", "ilcc_extract_auto_batch", "ilcc_extract_auto",
                "ilcc_default_seed_planar_params", "ilcc_seed_planar_scratch_bytes", "ilcc_propose_seeds_planar_device",
                "ilcc_propose_seeds_planar", "ilcc_debug_seed_planar_components", "ilcc_debug_seed_planar_launch_ms",
                "ilcc_extract_auto_planar_batch", "ilcc_extract_auto_planar"]
RECORD_WORDS = 11
GRID_MAX = 1024
TABLE_MIN = 64


class SeedParams(C.Structure):
    _fields_ = [
        ("cell", C.c_double),
        ("range", C.c_double),
        ("cluster_min", C.c_int32),
        ("max_components", C.c_int32),
        ("max_seeds", C.c_int32),
        ("board_w", C.c_int32), ("board_h", C.c_int32),
        ("reserved0", C.c_int32),
        ("grid_length", C.c_double),
        ("max_rms", C.c_double),
        ("size_lo", C.c_double), ("size_hi", C.c_double),
        ("max_oob_share", C.c_double),
    ]


class SeedPlanarParams(C.Structure):
    _fields_ = [("planar_rms", C.c_double), ("min_spread", C.c_double), ("own_rms", C.c_double)]


class Seed(C.Structure):
    _fields_ = [
        ("centroid", C.c_float * 3),
        ("n", C.c_int32),
        ("l1", C.c_double), ("l2", C.c_double),
        ("rms", C.c_double),
        ("score", C.c_double),
        ("key", C.c_uint32),
        ("reserved0", C.c_uint32),
    ]

    def centroid_array(self) -> np.ndarray:
        return np.array(self.centroid[:], np.float32)


class SeedError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = int(status)
        msg = _native.strerror(status)
        super().__init__("%s: %s" % (msg, detail) if detail else msg)


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        vp, fp, u64p, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        spp, sdp, ppp = C.POINTER(SeedParams), C.POINTER(Seed), C.POINTER(SeedPlanarParams)
        L.ilcc_default_seed_params.argtypes = [C.POINTER(Params), spp]
        L.ilcc_default_seed_params.restype = None
        L.ilcc_seed_scratch_bytes.argtypes = [C.c_uint32, C.c_uint64, spp]
        L.ilcc_seed_scratch_bytes.restype = C.c_uint64
        L.ilcc_propose_seeds_device.argtypes = [vp, vp, u64p, C.c_uint32, spp, vp, sdp, i32p, vp]
        L.ilcc_propose_seeds_device.restype = C.c_int32
        L.ilcc_propose_seeds.argtypes = [vp, fp, u64p, C.c_uint32, spp, sdp, i32p]
        L.ilcc_propose_seeds.restype = C.c_int32
        L.ilcc_debug_seed_components.argtypes = [vp, fp, u64p, C.c_uint32, spp, vp, C.c_uint32, C.POINTER(C.c_int64), C.c_uint32, i32p]
        L.ilcc_debug_seed_components.restype = C.c_int32
        L.ilcc_debug_seed_launch_ms.argtypes = [C.POINTER(C.c_float)]
        L.ilcc_debug_seed_launch_ms.restype = None
        L.ilcc_extract_auto_batch.argtypes = [vp, fp, u64p, C.c_uint32, spp, C.POINTER(Result), fp, i32p]
        L.ilcc_extract_auto_batch.restype = C.c_int32
        L.ilcc_extract_auto.argtypes = [vp, fp, C.c_uint32, spp, C.POINTER(Result), fp, i32p]
        L.ilcc_extract_auto.restype = C.c_int32
        L.ilcc_default_seed_planar_params.argtypes = [C.POINTER(Params), spp, ppp]
        L.ilcc_default_seed_planar_params.restype = None
        L.ilcc_seed_planar_scratch_bytes.argtypes = [C.c_uint32, C.c_uint64, spp]
        L.ilcc_seed_planar_scratch_bytes.restype = C.c_uint64
        L.ilcc_propose_seeds_planar_device.argtypes = [vp, vp, u64p, C.c_uint32, spp, ppp, vp, sdp, i32p, vp]
        L.ilcc_propose_seeds_planar_device.restype = C.c_int32
        L.ilcc_propose_seeds_planar.argtypes = [vp, fp, u64p, C.c_uint32, spp, ppp, sdp, i32p]
        L.ilcc_propose_seeds_planar.restype = C.c_int32
        L.ilcc_debug_seed_planar_components.argtypes = [vp, fp, u64p, C.c_uint32, spp, ppp, vp, C.c_uint32, C.POINTER(C.c_int64), C.c_uint32, i32p]
        L.ilcc_debug_seed_planar_components.restype = C.c_int32
        L.ilcc_debug_seed_planar_launch_ms.argtypes = [C.POINTER(C.c_float)]
        L.ilcc_debug_seed_planar_launch_ms.restype = None
        L.ilcc_extract_auto_planar_batch.argtypes = [vp, fp, u64p, C.c_uint32, spp, ppp, C.POINTER(Result), fp, i32p]
        L.ilcc_extract_auto_planar_batch.restype = C.c_int32
        L.ilcc_extract_auto_planar.argtypes = [vp, fp, C.c_uint32, spp, ppp, C.POINTER(Result), fp, i32p]
        L.ilcc_extract_auto_planar.restype = C.c_int32
        _ready = True
    return L


def default_seed_params(params: Params) -> SeedParams:
    sp = SeedParams()
    lib().ilcc_default_seed_params(C.byref(params), C.byref(sp))
    return sp


def scratch_bytes(n_frames: int, total_points: int, sp: SeedParams) -> int:
    return int(lib().ilcc_seed_scratch_bytes(int(n_frames), int(total_points), C.byref(sp)))


def _batch(clouds, offsets):
    """-> (contiguous float32 points, uint64 offsets, frames)"""
    clouds = np.ascontiguousarray(clouds, dtype=np.float32)
    if offsets is None:
        if clouds.ndim == 2:
            clouds = clouds[None]
        f, n = clouds.shape[0], clouds.shape[1]
        offsets = np.arange(f + 1, dtype=np.uint64) * np.uint64(n)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    return clouds, offsets, len(offsets) - 1


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _fail(est, st):
    raise SeedError(st, lib().ilcc_last_error(est._h).decode())


def _seed_lists(seeds, counts, max_seeds):
    """per frame: the list of its Seed, or None for a frame with more components than max_components"""
    return [None if counts[f] < 0 else [seeds[f * max_seeds + k] for k in range(counts[f])] for f in range(len(counts))]


def propose_seeds(est, clouds, offsets=None, sp=None):
    """clouds: [F, N, 4] (or [total, 4] with offsets [F + 1]) host arrays.  Per frame the ranked list of Seed (best first), or
    None where the frame holds more than sp.max_components components."""
    sp = sp if sp is not None else default_seed_params(est.params)
    clouds, offsets, f = _batch(clouds, offsets)
    seeds = (Seed * (f * sp.max_seeds))()
    counts = np.zeros(f, np.int32)
    st = lib().ilcc_propose_seeds(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), seeds,
                                  counts.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != _native.OK:
        _fail(est, st)
    return _seed_lists(seeds, counts, sp.max_seeds)


def propose_seeds_device(est, d_xyzi_ptr, offsets, sp, d_scratch_ptr, stream=None):
    """The same on clouds resident in HBM: raw device pointers (e.g. ``tensor.data_ptr()``); the scratch holds at least
    ``scratch_bytes`` bytes, 256-byte aligned, in any state."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    f = len(offsets) - 1
    seeds = (Seed * (f * sp.max_seeds))()
    counts = np.zeros(f, np.int32)
    st = lib().ilcc_propose_seeds_device(est._h, d_xyzi_ptr, _u64(offsets), f, C.byref(sp), d_scratch_ptr, seeds,
                                         counts.ctypes.data_as(C.POINTER(C.c_int32)), stream)
    if st != _native.OK:
        _fail(est, st)
    return _seed_lists(seeds, counts, sp.max_seeds)


def debug_components(est, clouds, offsets=None, frame=0, sp=None, d_scratch_ptr=None, cap_records=None):
    """Test entry: (status, [n, 11] int64 records of `frame`, sorted by key).  status is ILCC_CAPACITY where the frame holds more
    than sp.max_components records (none are returned)."""
    sp = sp if sp is not None else default_seed_params(est.params)
    clouds, offsets, f = _batch(clouds, offsets)
    cap = int(cap_records if cap_records is not None else sp.max_components)
    rec = np.zeros((max(cap, 1), RECORD_WORDS), np.int64)
    n = C.c_int32(0)
    st = lib().ilcc_debug_seed_components(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), d_scratch_ptr, int(frame),
                                          rec.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n))
    return st, rec[:n.value].copy()


LAUNCHES = ("clear", "insert", "moments", "union", "reduce", "pack")


def launch_ms() -> dict:
    """Diagnostic: the HIP-event span of each of K15's launches in this thread's last seed call, ms."""
    out = (C.c_float * len(LAUNCHES))()
    lib().ilcc_debug_seed_launch_ms(out)
    return dict(zip(LAUNCHES, (float(v) for v in out)))


def extract_auto(est, clouds, offsets=None, sp=None):
    """-> (Result array [F], seeds [F, 3] float32, ranks [F] int32).  Result f is what ``extract`` returns for cloud f with
    click = seeds[f]; ranks[f] = -1 (status ILCC_BOARD_NOT_FOUND) where no proposal was accepted."""
    sp = sp if sp is not None else default_seed_params(est.params)
    clouds, offsets, f = _batch(clouds, offsets)
    res = (Result * f)()
    seeds = np.zeros((f, 3), np.float32)
    ranks = np.zeros(f, np.int32)
    st = lib().ilcc_extract_auto_batch(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), res, _native.fptr(seeds),
                                       ranks.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != _native.OK:
        _fail(est, st)
    return res, seeds, ranks


# ---- planar seeds (K15p): each function is its sibling above with the thresholds `pp`

def default_seed_planar_params(params: Params):
    """-> (SeedParams with the planar path's max_rms, SeedPlanarParams)"""
    sp, pp = SeedParams(), SeedPlanarParams()
    lib().ilcc_default_seed_planar_params(C.byref(params), C.byref(sp), C.byref(pp))
    return sp, pp


def planar_scratch_bytes(n_frames: int, total_points: int, sp: SeedParams) -> int:
    return int(lib().ilcc_seed_planar_scratch_bytes(int(n_frames), int(total_points), C.byref(sp)))


def _planar_defaults(est, sp, pp):
    dsp, dpp = default_seed_planar_params(est.params)
    return (sp if sp is not None else dsp), (pp if pp is not None else dpp)


def propose_seeds_planar(est, clouds, offsets=None, sp=None, pp=None):
    sp, pp = _planar_defaults(est, sp, pp)
    clouds, offsets, f = _batch(clouds, offsets)
    seeds = (Seed * (f * sp.max_seeds))()
    counts = np.zeros(f, np.int32)
    st = lib().ilcc_propose_seeds_planar(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), C.byref(pp), seeds,
                                         counts.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != _native.OK:
        _fail(est, st)
    return _seed_lists(seeds, counts, sp.max_seeds)


def propose_seeds_planar_device(est, d_xyzi_ptr, offsets, sp, pp, d_scratch_ptr, stream=None):
    """the scratch holds at least ``planar_scratch_bytes`` bytes"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    f = len(offsets) - 1
    seeds = (Seed * (f * sp.max_seeds))()
    counts = np.zeros(f, np.int32)
    st = lib().ilcc_propose_seeds_planar_device(est._h, d_xyzi_ptr, _u64(offsets), f, C.byref(sp), C.byref(pp), d_scratch_ptr, seeds,
                                                counts.ctypes.data_as(C.POINTER(C.c_int32)), stream)
    if st != _native.OK:
        _fail(est, st)
    return _seed_lists(seeds, counts, sp.max_seeds)


def debug_planar_components(est, clouds, offsets=None, frame=0, sp=None, pp=None, d_scratch_ptr=None, cap_records=None):
    """Test entry: (status, [n, 11] int64 records of the core components of `frame`, sorted by key)."""
    sp, pp = _planar_defaults(est, sp, pp)
    clouds, offsets, f = _batch(clouds, offsets)
    cap = int(cap_records if cap_records is not None else sp.max_components)
    rec = np.zeros((max(cap, 1), RECORD_WORDS), np.int64)
    n = C.c_int32(0)
    st = lib().ilcc_debug_seed_planar_components(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), C.byref(pp), d_scratch_ptr,
                                                 int(frame), rec.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n))
    return st, rec[:n.value].copy()


PLANAR_LAUNCHES = ("clear", "insert", "moments", "classify", "union", "reduce", "pack")


def planar_launch_ms() -> dict:
    """Diagnostic: the HIP-event span of each launch in this thread's last planar seed call, ms."""
    out = (C.c_float * len(PLANAR_LAUNCHES))()
    lib().ilcc_debug_seed_planar_launch_ms(out)
    return dict(zip(PLANAR_LAUNCHES, (float(v) for v in out)))


def extract_auto_planar(est, clouds, offsets=None, sp=None, pp=None):
    """``extract_auto`` on planar seeds."""
    sp, pp = _planar_defaults(est, sp, pp)
    clouds, offsets, f = _batch(clouds, offsets)
    res = (Result * f)()
    seeds = np.zeros((f, 3), np.float32)
    ranks = np.zeros(f, np.int32)
    st = lib().ilcc_extract_auto_planar_batch(est._h, _native.fptr(clouds), _u64(offsets), f, C.byref(sp), C.byref(pp), res,
                                              _native.fptr(seeds), ranks.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != _native.OK:
        _fail(est, st)
    return res, seeds, ranks
