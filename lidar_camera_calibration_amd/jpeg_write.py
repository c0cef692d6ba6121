"""Writing JPEG images: ctypes mirror of ``include/ilcc_jpeg_write.h`` -- colour conversion, chroma downsampling, forward
DCT and quantisation on the GPU (K14), Huffman coding on the host; the bytes are the ones libjpeg (cv::imwrite, Pillow)
writes for the same pixels and quality.  ``encode`` gives the file of a device tensor, ``save`` writes it, and
``bag_save_jpeg`` is the per-bag body of get_image_corners_bag: first image -> undistorted mono8 -> <camera><i>.jpg."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import ENCODINGS, CameraModel, _camera_ref, _check, _device_pixels
from .jpeg import SAMPLINGS, Info
from .jpeg import lib as _jpeg_lib

JPEG_WRITE_EXPORTS = ["ilcc_jpeg_write_info", "ilcc_jpeg_fdct_scratch_bytes", "ilcc_jpeg_fdct_device", "ilcc_jpeg_file_bound",
                      "ilcc_jpeg_entropy_encode", "ilcc_jpeg_encode_device", "ilcc_jpeg_write_file", "ilcc_bag_save_jpeg"]

_ready = False


def lib():
    global _ready
    L = _jpeg_lib()
    if not _ready:
        i32, u64, vp, info = C.c_int32, C.c_uint64, C.c_void_p, C.POINTER(Info)
        L.ilcc_jpeg_write_info.argtypes = [i32] * 7 + [info]
        L.ilcc_jpeg_write_info.restype = i32
        L.ilcc_jpeg_fdct_scratch_bytes.argtypes = [info]
        L.ilcc_jpeg_fdct_scratch_bytes.restype = u64
        L.ilcc_jpeg_fdct_device.argtypes = [info, vp, i32, i32, vp, vp, u64, vp]
        L.ilcc_jpeg_fdct_device.restype = i32
        L.ilcc_jpeg_file_bound.argtypes = [info]
        L.ilcc_jpeg_file_bound.restype = u64
        L.ilcc_jpeg_entropy_encode.argtypes = [info, vp, vp, u64, C.POINTER(u64)]
        L.ilcc_jpeg_entropy_encode.restype = i32
        L.ilcc_jpeg_encode_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, u64, C.POINTER(u64), vp]
        L.ilcc_jpeg_encode_device.restype = i32
        L.ilcc_jpeg_write_file.argtypes = [i32, C.c_char_p, vp, i32, i32, i32, i32, i32]
        L.ilcc_jpeg_write_file.restype = i32
        L.ilcc_bag_save_jpeg.argtypes = [i32, C.c_char_p, C.c_char_p, C.POINTER(CameraModel), C.c_char_p, i32]
        L.ilcc_bag_save_jpeg.restype = i32
        _ready = True
    return L


def _sampling(sampling):
    return (1, 1) if sampling is None else SAMPLINGS.get(sampling, sampling)


def write_info(width, height, sampling=None, quality=95, restart_interval=0) -> Info:
    """The Info of a file to write: sampling None = 1 component, else "444", "422", "420" or luma's (h, v); the Annex-K
    quantisation tables scaled for `quality` as libjpeg scales them."""
    info = Info()
    h, v = _sampling(sampling)
    _check(lib().ilcc_jpeg_write_info(width, height, 1 if sampling is None else 3, h, v, quality, restart_interval, C.byref(info)))
    return info


def fdct_scratch_bytes(info) -> int:
    return int(lib().ilcc_jpeg_fdct_scratch_bytes(C.byref(info)))


def file_bound(info) -> int:
    return int(lib().ilcc_jpeg_file_bound(C.byref(info)))


def fdct(info, pixels, out=None):
    """K14: (rows, cols) mono8 or (rows, cols, 3) B, G, R uint8 pixels, numpy or torch -> the info.coef_count quantised
    coefficients as an int16 tensor on the current HIP device, laid out as jpeg.entropy_decode leaves them.  A device
    tensor whose pixels are contiguous is read in place with stride(0) as the row pitch.  `out`: a 16-byte aligned int16
    device tensor of coef_count.  Asynchronous on the current stream."""
    import torch
    encoding = "mono8" if info.n_components == 1 else "bgr8"
    t, step = _device_pixels(pixels, encoding)
    if (int(t.shape[1]), int(t.shape[0])) != (info.width, info.height):
        raise ValueError("the info is for %d x %d pixels, got %d x %d" % (info.width, info.height, t.shape[1], t.shape[0]))
    if out is None:
        out = torch.empty(info.coef_count, dtype=torch.int16, device=t.device)
    scratch = torch.empty(max(fdct_scratch_bytes(info), 16), dtype=torch.uint8, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    _check(lib().ilcc_jpeg_fdct_device(C.byref(info), C.c_void_p(t.data_ptr()), step, ENCODINGS.index(encoding),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel(), stream))
    return out


def entropy_encode(info, coef) -> bytes:
    """The whole file for int16 coefficients (numpy, or a tensor that is brought to the host)."""
    if not isinstance(coef, np.ndarray):
        coef = coef.cpu().numpy()
    coef = np.ascontiguousarray(coef, np.int16)
    if coef.ndim != 1 or coef.size != info.coef_count:
        raise ValueError("expected %d int16 coefficients, got %s" % (info.coef_count, coef.shape))
    out = np.empty(file_bound(info), np.uint8)
    n = C.c_uint64(0)
    _check(lib().ilcc_jpeg_entropy_encode(C.byref(info), coef.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), out.size,
                                          C.byref(n)))
    return out[:n.value].tobytes()


def encode(pixels, quality=95, sampling="420", restart_interval=0) -> bytes:
    """The JPEG file of (rows, cols) mono8 or (rows, cols, 3) B, G, R uint8 pixels (ilcc_jpeg_encode_device); `sampling`
    applies to colour only.  A row-pitched device view is read in place."""
    import torch
    t = pixels if isinstance(pixels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pixels))
    encoding = "mono8" if t.dim() == 2 else "bgr8"
    t, step = _device_pixels(t, encoding)
    rows, cols = int(t.shape[0]), int(t.shape[1])
    h, v = _sampling(sampling)
    bound = file_bound(write_info(cols, rows, None if encoding == "mono8" else (h, v), quality, restart_interval))
    out = np.empty(bound, np.uint8)
    n = C.c_uint64(0)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    _check(lib().ilcc_jpeg_encode_device(C.c_void_p(t.data_ptr()), step, cols, rows, ENCODINGS.index(encoding), quality, h, v,
                                         restart_interval, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n), stream))
    return out[:n.value].tobytes()


def save(path, pixels, quality=95, device=0):
    """cv::imwrite(path, pixels) for host pixels, (rows, cols) mono8 or (rows, cols, 3) B, G, R (ilcc_jpeg_write_file);
    colour is written 4:2:0.  Device tensors are brought to the host: `open(path, "wb").write(encode(t))` keeps them there."""
    a = pixels if isinstance(pixels, np.ndarray) else pixels.cpu().numpy()
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("expected (rows, cols) or (rows, cols, 3) uint8 pixels, got %s" % (a.shape,))
    encoding = "mono8" if a.ndim == 2 else "bgr8"
    _check(lib().ilcc_jpeg_write_file(device, os.fsencode(path), a.ctypes.data_as(C.c_void_p), int(a.strides[0]), a.shape[1], a.shape[0],
                                      ENCODINGS.index(encoding), quality))


def bag_save_jpeg(bag_path, topic, camera, jpg_path, quality=95, device=0):
    """The per-bag body of get_image_corners_bag: the topic's first image -> mono8, undistorted with `camera` -> jpg_path."""
    _check(lib().ilcc_bag_save_jpeg(device, os.fsencode(bag_path), topic.encode(), _camera_ref(camera), os.fsencode(jpg_path), quality))
