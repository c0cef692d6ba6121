"""Camera chessboard corners (libcbdetect's findCorners + chessboardsFromCorners): ctypes mirror of
``include/ilcc_image_corners.h`` (K10 on the GPU, structure recovery and the writer on the host).

Images are 8-bit grayscale pixels (numpy or torch uint8, rows x cols); the library decodes no file
format.  Positions are 0-based pixels, as the reference's ``corners.p``; ``save_cam_corners`` adds 1
back, as its dump does, so the file is what ``calib.read_cam_corners`` expects.
"""
import ctypes as C
import os

import numpy as np

from . import _native

IMAGE_CORNERS_EXPORTS = ["ilcc_image_corners_device", "ilcc_chessboard_from_corners", "ilcc_find_chessboard_device",
                         "ilcc_save_cam_corners"]

MIN_SIDE = 34   # 2 x 12 (largest template radius) + 2 x 5 (NMS margin)


class ImageCorner(C.Structure):
    _fields_ = [("u", C.c_double), ("v", C.c_double), ("v1", C.c_double * 2), ("v2", C.c_double * 2), ("score", C.c_double)]


class ImageCornerStages(C.Structure):
    _fields_ = [("d_likelihood", C.c_void_p), ("candidates", C.POINTER(C.c_int32)), ("refined", C.POINTER(ImageCorner)),
                ("capacity", C.c_int32), ("n_candidates", C.c_int32), ("ms", C.c_float * 4)]


CORNER_DTYPE = np.dtype([("u", "<f8"), ("v", "<f8"), ("v1", "<f8", 2), ("v2", "<f8", 2), ("score", "<f8")])
assert CORNER_DTYPE.itemsize == C.sizeof(ImageCorner)


class BoardNotFound(RuntimeError):
    """No board of the requested size (status ILCC_BOARD_NOT_FOUND) or more than one (ILCC_AMBIGUOUS)."""

    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        i32p = C.POINTER(C.c_int32)
        L.ilcc_image_corners_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, i32p,
                                                C.POINTER(ImageCornerStages), C.c_void_p]
        L.ilcc_image_corners_device.restype = C.c_int32
        L.ilcc_chessboard_from_corners.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p]
        L.ilcc_chessboard_from_corners.restype = C.c_int32
        L.ilcc_find_chessboard_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i32p,
                                                  i32p, C.POINTER(C.c_double), C.c_void_p]
        L.ilcc_find_chessboard_device.restype = C.c_int32
        L.ilcc_save_cam_corners.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.ilcc_save_cam_corners.restype = C.c_int32
        _ready = True
    return L


def _error(st):
    return "%s: %s" % (_native.strerror(st), _native.lib().ilcc_last_error(None).decode())


def _check(st):
    if st in (_native.BOARD_NOT_FOUND, _native.AMBIGUOUS):
        raise BoardNotFound(st, _error(st))
    if st != _native.OK:
        raise RuntimeError(_error(st))


def _device_image(image):
    """(device tensor, width, height, stride): a 2-D uint8 tensor on the current HIP device.  A tensor
    already there whose rows are contiguous (stride(1) == 1, stride(0) >= width), such as a crop view of a
    larger frame, is passed as it is, with stride(0) as the row pitch; anything else is copied."""
    import torch
    t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dtype != torch.uint8 or t.dim() != 2:
        raise ValueError("expected a 2-D uint8 grayscale image, got %s %s" % (tuple(t.shape), t.dtype))
    on_device = t.is_cuda and t.device.index == torch.cuda.current_device()
    if not (on_device and t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        t = t.to("cuda").contiguous()
    return t, int(t.shape[1]), int(t.shape[0]), int(t.stride(0))


def _stream_of(t):
    import torch
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def find_corners(image, stages=False, capacity=8192):
    """findCorners(img, 0.01, 1): structured array of CORNER_DTYPE (0-based u, v) in the reference's
    order.  With stages=True also returns a dict: likelihood map (float32 tensor), NMS candidates
    (1-based (u, v), int32), every candidate after refinement (CORNER_DTYPE, 1-based) and the
    per-stage HIP-event milliseconds."""
    import torch
    t, w, h, s = _device_image(image)
    out = np.zeros(capacity, CORNER_DTYPE)
    n = C.c_int32(0)
    st = None
    if stages:
        L = torch.empty((h, w), dtype=torch.float32, device=t.device)
        cand = np.zeros((capacity, 2), np.int32)
        ref = np.zeros(capacity, CORNER_DTYPE)
        st = ImageCornerStages()
        st.d_likelihood = L.data_ptr()
        st.candidates = cand.ctypes.data_as(C.POINTER(C.c_int32))
        st.refined = ref.ctypes.data_as(C.POINTER(ImageCorner))
        st.capacity = capacity
    rc = lib().ilcc_image_corners_device(C.c_void_p(t.data_ptr()), w, h, s, out.ctypes.data_as(C.c_void_p), capacity,
                                         C.byref(n), C.byref(st) if st is not None else None, _stream_of(t))
    _check(rc)
    corners = out[:n.value].copy()
    if not stages:
        return corners
    m = min(st.n_candidates, capacity)
    return corners, dict(likelihood=L, candidates=cand[:m].copy(), refined=ref[:m].copy(), n_candidates=st.n_candidates,
                         ms=dict(gradients=st.ms[0], likelihood=st.ms[1], nms=st.ms[2], refine_score=st.ms[3]))


def chessboard_from_corners(corners, board=(7, 5)):
    """Structure recovery on host corners (CORNER_DTYPE): the rows x cols matrix of corner indices of
    the one board of that size, either orientation.  Raises BoardNotFound otherwise.  No GPU."""
    c = np.ascontiguousarray(corners, dtype=CORNER_DTYPE)
    idx = np.zeros(board[0] * board[1], np.int32)
    r, k = C.c_int32(0), C.c_int32(0)
    _check(lib().ilcc_chessboard_from_corners(c.ctypes.data_as(C.c_void_p), len(c), board[0], board[1], C.byref(r),
                                              C.byref(k), idx.ctypes.data_as(C.POINTER(C.c_int32))))
    return idx.reshape(r.value, k.value)


def find_chessboard(image, board=(7, 5)):
    """The image's one board_w x board_h chessboard (board = (corner_in_x, corner_in_y)) as a
    (rows, cols, 2) float64 array of 0-based (u, v).  Raises BoardNotFound when there is none or
    more than one."""
    t, w, h, s = _device_image(image)
    xy = np.zeros(board[0] * board[1] * 2)
    r, k = C.c_int32(0), C.c_int32(0)
    _check(lib().ilcc_find_chessboard_device(C.c_void_p(t.data_ptr()), w, h, s, board[0], board[1], C.byref(r), C.byref(k),
                                             xy.ctypes.data_as(C.POINTER(C.c_double)), _stream_of(t)))
    return xy.reshape(r.value, k.value, 2)


def save_cam_corners(filename, board):
    """Write a (rows, cols, 2) board of 0-based (u, v) as the reference's `<camera><i>.txt`."""
    b = np.ascontiguousarray(board, dtype=np.float64)
    if b.ndim != 3 or b.shape[2] != 2:
        raise ValueError("board must be (rows, cols, 2)")
    _check(lib().ilcc_save_cam_corners(os.fsencode(filename), b.shape[0], b.shape[1], b.ctypes.data_as(C.POINTER(C.c_double))))
