"""Reading JPEG images: ctypes mirror of ``include/ilcc_jpeg.h`` -- headers and Huffman decoding on the host, inverse
DCT, chroma upsampling and colour conversion on the GPU (K13).  ``decode`` gives the pixels of a .jpg file as a device
tensor in the file's own encoding (mono8 or bgr8), which ``camera_image.to_mono8`` / ``to_bgr8`` and
``image_corners.find_chessboard`` take; ``find_chessboard`` is the MATLAB step (demo_all_pic.m) on one file."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import ENCODINGS, CameraModel, _camera_ref, _check

COMPRESSED_IMAGE_MD5 = "8f7a12909da2c9d3332d540a0977563f"
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}

JPEG_EXPORTS = ["ilcc_jpeg_parse", "ilcc_jpeg_layout", "ilcc_jpeg_entropy_decode", "ilcc_jpeg_scratch_bytes", "ilcc_jpeg_idct_device",
                "ilcc_jpeg_decode_device", "ilcc_jpeg_find_chessboard", "ilcc_compressed_image_parse"]


class Component(C.Structure):
    _fields_ = [("h", C.c_int32), ("v", C.c_int32), ("quant_index", C.c_int32), ("dc_table", C.c_int32), ("ac_table", C.c_int32),
                ("blocks_w", C.c_int32), ("blocks_h", C.c_int32), ("reserved", C.c_int32), ("coef_offset", C.c_uint64)]


class Info(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_components", C.c_int32), ("restart_interval", C.c_int32),
                ("comp", Component * 3), ("quant", (C.c_uint16 * 64) * 4), ("coef_count", C.c_uint64), ("scan_offset", C.c_uint64)]

    @property
    def encoding(self):
        return "mono8" if self.n_components == 1 else "bgr8"

    def quant_array(self):
        return np.ctypeslib.as_array(self.quant).copy()


class CompressedImageLayout(C.Structure):
    _fields_ = [("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("seq", C.c_uint32), ("reserved", C.c_uint32),
                ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64), ("frame_id", C.c_char * 64), ("format", C.c_char * 64)]


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        u8p, i32p, info, cam = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(Info), C.POINTER(CameraModel)
        L.ilcc_jpeg_parse.argtypes = [u8p, C.c_uint64, info]
        L.ilcc_jpeg_parse.restype = C.c_int32
        L.ilcc_jpeg_layout.argtypes = [info]
        L.ilcc_jpeg_layout.restype = C.c_int32
        L.ilcc_jpeg_entropy_decode.argtypes = [u8p, C.c_uint64, info, C.c_void_p, C.c_uint64]
        L.ilcc_jpeg_entropy_decode.restype = C.c_int32
        L.ilcc_jpeg_scratch_bytes.argtypes = [info]
        L.ilcc_jpeg_scratch_bytes.restype = C.c_uint64
        L.ilcc_jpeg_idct_device.argtypes = [info, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p]
        L.ilcc_jpeg_idct_device.restype = C.c_int32
        L.ilcc_jpeg_decode_device.argtypes = [u8p, C.c_uint64, C.c_void_p, C.c_int32, C.c_uint64, i32p, i32p, i32p, C.c_void_p]
        L.ilcc_jpeg_decode_device.restype = C.c_int32
        L.ilcc_jpeg_find_chessboard.argtypes = [C.c_int32, C.c_char_p, cam, C.c_int32, C.c_int32, i32p, i32p, C.POINTER(C.c_double)]
        L.ilcc_jpeg_find_chessboard.restype = C.c_int32
        L.ilcc_compressed_image_parse.argtypes = [u8p, C.c_uint64, C.POINTER(CompressedImageLayout)]
        L.ilcc_compressed_image_parse.restype = C.c_int32
        _ready = True
    return L


def _bytes_arg(data):
    data = bytes(data)
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(data if data else b"\0"), len(data)


def parse(jpg) -> Info:
    """The headers of a JPEG file: size, components, quantisation tables, coefficient layout."""
    info = Info()
    arr, n = _bytes_arg(jpg)
    _check(lib().ilcc_jpeg_parse(arr, n, C.byref(info)))
    return info


def make_info(width, height, sampling=None, quant=None) -> Info:
    """An Info for coefficients that come from elsewhere than a file: sampling None = 1 component, else "444", "422",
    "420" or luma's (h, v); quant: up to 4 tables of 64 in row-major order, component c uses table min(c, 1)."""
    info = Info()
    info.width, info.height = width, height
    info.n_components = 1 if sampling is None else 3
    h, v = (1, 1) if sampling is None else SAMPLINGS.get(sampling, sampling)
    for c in range(info.n_components):
        info.comp[c].h, info.comp[c].v = (h, v) if c == 0 else (1, 1)
        info.comp[c].quant_index = min(c, 1)
    if quant is not None:
        q = np.asarray(quant, np.uint16).reshape(-1, 64)
        for t in range(len(q)):
            info.quant[t][:] = q[t].tolist()
    _check(lib().ilcc_jpeg_layout(C.byref(info)))
    return info


def entropy_decode(jpg, info=None) -> np.ndarray:
    """The scan's quantised coefficients, de-zigzagged: int16[coef_count], coef[offset_c + (by * blocks_w_c + bx) * 64 + k]."""
    info = info if info is not None else parse(jpg)
    coef = np.zeros(info.coef_count, np.int16)
    arr, n = _bytes_arg(jpg)
    _check(lib().ilcc_jpeg_entropy_decode(arr, n, C.byref(info), coef.ctypes.data_as(C.c_void_p), coef.size))
    return coef


def scratch_bytes(info) -> int:
    return int(lib().ilcc_jpeg_scratch_bytes(C.byref(info)))


def idct(info, coef, out=None):
    """K13: int16 coefficients (numpy or device tensor, laid out as entropy_decode leaves them) -> (rows, cols) mono8 or
    (rows, cols, 3) bgr8 uint8 tensor on the current HIP device.  `out`: a uint8 device tensor (or view) whose rows hold
    bpp * width contiguous bytes; its stride(0) is the row pitch.  Asynchronous on the current stream."""
    import torch
    t = coef if isinstance(coef, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coef, np.int16))
    if t.dtype != torch.int16 or t.dim() != 1 or t.numel() != info.coef_count:
        raise ValueError("expected %d int16 coefficients, got %s %s" % (info.coef_count, tuple(t.shape), t.dtype))
    t = t.to("cuda").contiguous()
    w, h, bpp = info.width, info.height, 1 if info.n_components == 1 else 3
    if out is None:
        out = torch.empty((h, w) if bpp == 1 else (h, w, 3), dtype=torch.uint8, device=t.device)
    stride = int(out.stride(0)) if h > 1 else bpp * w
    scratch = torch.empty(max(scratch_bytes(info), 16), dtype=torch.uint8, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    _check(lib().ilcc_jpeg_idct_device(C.byref(info), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), stride,
                                       C.c_void_p(scratch.data_ptr()), scratch.numel(), stream))
    return out


def decode(jpg):
    """The pixels of a JPEG file: (rows, cols) uint8 for one component, (rows, cols, 3) B, G, R for three, on the current HIP
    device (ilcc_jpeg_decode_device).  The encoding is info.encoding: "mono8" or "bgr8"."""
    import torch
    info = parse(jpg)
    bpp = 1 if info.n_components == 1 else 3
    out = torch.empty((info.height, info.width) if bpp == 1 else (info.height, info.width, 3), dtype=torch.uint8, device="cuda")
    arr, n = _bytes_arg(jpg)
    w, h, enc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    stream = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
    _check(lib().ilcc_jpeg_decode_device(arr, n, C.c_void_p(out.data_ptr()), bpp * info.width, out.numel(), C.byref(w), C.byref(h),
                                         C.byref(enc), stream))
    assert (w.value, h.value, ENCODINGS[enc.value]) == (info.width, info.height, info.encoding)
    return out


def find_chessboard(jpg_path, camera=None, board=(7, 5), device=0) -> np.ndarray:
    """The chessboard of a .jpg file as image_corners.find_chessboard returns it: (rows, cols, 2) 0-based (u, v);
    undistorted first when a camera is given.  Raises BoardNotFound when there is none or more than one."""
    xy = np.zeros(board[0] * board[1] * 2)
    r, k = C.c_int32(0), C.c_int32(0)
    _check(lib().ilcc_jpeg_find_chessboard(device, os.fsencode(jpg_path), _camera_ref(camera), board[0], board[1], C.byref(r),
                                           C.byref(k), xy.ctypes.data_as(C.POINTER(C.c_double))))
    return xy.reshape(r.value, k.value, 2)


def parse_compressed_image(msg: bytes) -> CompressedImageLayout:
    """Layout of a serialized sensor_msgs/CompressedImage; msg[data_offset : data_offset + data_bytes] is the JPEG file."""
    lay = CompressedImageLayout()
    arr, n = _bytes_arg(msg)
    _check(lib().ilcc_compressed_image_parse(arr, n, C.byref(lay)))
    return lay
