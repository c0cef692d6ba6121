"""Writing every undistorted frame of a recording as a JPEG file: ctypes mirror of ``include/ilcc_jpeg_write_sequence.h``.

``write_headers`` gives the bytes in front of a scan (host), ``fdct_batch`` is K14b and ``huffman_encode_batch`` K17 on device
tensors, ``encode_batch`` goes from a batch of coefficients to the images' scans and statuses as numpy arrays (what
``jpeg_write.entropy_encode`` gives image by image, between its SOS header and its EOI), ``file_of`` puts a file together, and
``bag_save_jpeg_all`` is the chain: <prefix><message index, 6 digits>.jpg for every selected image of a topic."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import ENCODINGS, CameraModel, _camera_ref, _check
from .jpeg import Info
from .jpeg_write import lib as _write_lib

JPEG_WRITE_SEQUENCE_EXPORTS = ["ilcc_jpeg_write_headers", "ilcc_jpeg_fdct_batch_scratch_bytes", "ilcc_jpeg_fdct_batch_device",
                               "ilcc_jpeg_huffman_encode_scratch_bytes", "ilcc_jpeg_huffman_encode_batch_device",
                               "ilcc_default_jpeg_write_sequence_params", "ilcc_jpeg_write_sequence_bytes", "ilcc_bag_save_jpeg_all"]

DC_RANGE, AC_RANGE, CAPACITY = 0x01, 0x02, 0x04
EOI = b"\xff\xd9"
ROUTES = {"gpu": 0, "host": 1}


class FdctBatchJob(C.Structure):
    _fields_ = [("layout", C.POINTER(Info)), ("d_src", C.c_void_p), ("image_pitch", C.c_uint64), ("src_stride", C.c_int32), ("encoding", C.c_int32),
                ("d_coef", C.c_void_p), ("coef_pitch", C.c_uint64), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64), ("n_images", C.c_uint32),
                ("reserved", C.c_uint32), ("hip_stream", C.c_void_p)]


class EncodeRow(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint32), ("status", C.c_uint32)]


class EncodeJob(C.Structure):
    _fields_ = [("layout", C.POINTER(Info)), ("d_coef", C.c_void_p), ("coef_pitch", C.c_uint64), ("d_out", C.c_void_p), ("out_cap", C.c_uint64),
                ("d_rows", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64), ("n_images", C.c_uint32), ("reserved", C.c_uint32),
                ("hip_stream", C.c_void_p)]


class WriteSequenceParams(C.Structure):
    _fields_ = [("first", C.c_uint32), ("stride", C.c_uint32), ("max_images", C.c_uint32), ("route", C.c_uint32), ("staging_bytes", C.c_uint64),
                ("device_bytes", C.c_uint64), ("out_bytes_per_image", C.c_uint64)]


class WriteRecord(C.Structure):
    _fields_ = [("message", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("time_sec", C.c_uint32), ("time_nsec", C.c_uint32),
                ("route", C.c_uint32), ("file_bytes", C.c_uint64)]


class WriteSequenceResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_images", C.c_int32), ("n_batches", C.c_int32), ("n_host_encoded", C.c_int32), ("d2h_bytes", C.c_uint64),
                ("file_bytes", C.c_uint64)]


STRUCT_SIZES = {"ilcc_jpeg_fdct_batch_job": (FdctBatchJob, 80), "ilcc_jpeg_encode_row": (EncodeRow, 16), "ilcc_jpeg_huffman_encode_job": (EncodeJob, 80),
                "ilcc_jpeg_write_sequence_params": (WriteSequenceParams, 40), "ilcc_jpeg_write_record": (WriteRecord, 32),
                "ilcc_jpeg_write_sequence_result": (WriteSequenceResult, 32)}

ROW_DTYPE = np.dtype([("offset", np.uint64), ("bytes", np.uint32), ("status", np.uint32)])

_ready = False


class JpegWriteSequenceError(RuntimeError):
    def __init__(self, status, result=None, records=None):
        self.status, self.result, self.records = status, result, records
        super().__init__("%s: %s" % (_native.strerror(status), _native.lib().ilcc_last_error(None).decode()))


def lib():
    global _ready
    L = _write_lib()
    if not _ready:
        i32, u32, u64, vp, info = C.c_int32, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(Info)
        L.ilcc_jpeg_write_headers.argtypes = [info, vp, u64, C.POINTER(u64)]
        L.ilcc_jpeg_write_headers.restype = i32
        L.ilcc_jpeg_fdct_batch_scratch_bytes.argtypes = [info, u32]
        L.ilcc_jpeg_fdct_batch_scratch_bytes.restype = u64
        L.ilcc_jpeg_fdct_batch_device.argtypes = [C.POINTER(FdctBatchJob)]
        L.ilcc_jpeg_fdct_batch_device.restype = i32
        L.ilcc_jpeg_huffman_encode_scratch_bytes.argtypes = [info, u32, u64]
        L.ilcc_jpeg_huffman_encode_scratch_bytes.restype = u64
        L.ilcc_jpeg_huffman_encode_batch_device.argtypes = [C.POINTER(EncodeJob)]
        L.ilcc_jpeg_huffman_encode_batch_device.restype = i32
        L.ilcc_default_jpeg_write_sequence_params.argtypes = [C.POINTER(WriteSequenceParams)]
        L.ilcc_default_jpeg_write_sequence_params.restype = None
        L.ilcc_jpeg_write_sequence_bytes.argtypes = [i32, i32, u64]
        L.ilcc_jpeg_write_sequence_bytes.restype = u64
        L.ilcc_bag_save_jpeg_all.argtypes = [i32, C.c_char_p, C.c_char_p, C.POINTER(CameraModel), C.c_char_p, i32, C.POINTER(WriteSequenceParams),
                                             C.POINTER(WriteSequenceResult), C.POINTER(WriteRecord), u32]
        L.ilcc_bag_save_jpeg_all.restype = i32
        _ready = True
    return L


def write_headers(info) -> bytes:
    """SOI .. the SOS header of the file ilcc_jpeg_entropy_encode writes for `info`"""
    out = np.empty(1024, np.uint8)
    n = C.c_uint64(0)
    _check(lib().ilcc_jpeg_write_headers(C.byref(info), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
    return out[:n.value].tobytes()


def file_of(info, scan) -> bytes:
    """headers + scan + EOI"""
    return write_headers(info) + bytes(scan) + EOI


def fdct_batch_scratch_bytes(layout, n_images) -> int:
    return int(lib().ilcc_jpeg_fdct_batch_scratch_bytes(C.byref(layout), int(n_images)))


def huffman_encode_scratch_bytes(layout, n_images, out_cap) -> int:
    return int(lib().ilcc_jpeg_huffman_encode_scratch_bytes(C.byref(layout), int(n_images), int(out_cap)))


def sequence_bytes(width, height, out_bytes_per_image=0) -> int:
    """device bytes one image takes in the chain"""
    return int(lib().ilcc_jpeg_write_sequence_bytes(int(width), int(height), int(out_bytes_per_image)))


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return stream


def fdct_batch(layout, images, coef_pitch=None, out=None, image_pitch=None, stream=None):
    """K14b on a device tensor of n images of one geometry: uint8 (n, rows, cols) mono8 or (n, rows, cols, 3) B, G, R, contiguous (or
    a flat uint8 tensor with image_pitch bytes between packed images) -> int16 (n, coef_pitch) on the device.  Asynchronous."""
    import torch
    bpp = 1 if layout.n_components == 1 else 3
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    t = t.cuda().contiguous()
    if image_pitch is None:
        n = int(t.shape[0])
        image_pitch = int(layout.width) * int(layout.height) * bpp
        if t.numel() != n * image_pitch:
            raise ValueError("expected %d images of %d x %d x %d bytes, got %s" % (n, layout.height, layout.width, bpp, tuple(t.shape)))
    else:
        n = (t.numel() + int(image_pitch) - int(layout.width) * int(layout.height) * bpp) // int(image_pitch)
    pitch = int(coef_pitch) if coef_pitch is not None else -(-int(layout.coef_count) // 8) * 8
    if out is None:
        out = torch.empty((n, pitch), dtype=torch.int16, device=t.device)
    scratch = torch.empty(max(fdct_batch_scratch_bytes(layout, n), 16), dtype=torch.uint8, device=t.device)
    job = FdctBatchJob(C.pointer(layout), t.data_ptr(), int(image_pitch), int(layout.width) * bpp, ENCODINGS.index("mono8" if bpp == 1 else "bgr8"),
                       out.data_ptr(), pitch, scratch.data_ptr(), scratch.numel(), n, 0, _stream(stream))
    _check(lib().ilcc_jpeg_fdct_batch_device(C.byref(job)))
    return out


def huffman_encode_batch(layout, d_coef, coef_pitch, n_images, d_out, out_cap, d_rows, d_scratch, scratch_nbytes, stream=None):
    """ilcc_jpeg_huffman_encode_batch_device on device addresses (ints); `stream`: a hipStream_t as int, default the current torch stream.
    Raises CameraImageError on a refusal; asynchronous."""
    job = EncodeJob(C.pointer(layout), d_coef, int(coef_pitch), d_out, int(out_cap), d_rows, d_scratch, int(scratch_nbytes), int(n_images), 0,
                    _stream(stream))
    _check(lib().ilcc_jpeg_huffman_encode_batch_device(C.byref(job)))


def encode_batch(layout, coefs, out_cap=None, guard=0, fill=0):
    """K17 on int16 coefficients (n, coef_pitch), numpy or a device tensor -> (scans: a list of bytes, b"" where status != 0; rows: a
    numpy record array with offset, bytes, status; out: the whole output buffer, out_cap + guard bytes, as uint8).  The buffer is
    filled with `fill` before the call, so what K17 leaves alone can be seen.  out_cap defaults to what any accepted batch takes."""
    import torch
    t = coefs if isinstance(coefs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coefs, np.int16))
    t = t.cuda().contiguous()
    if t.dim() != 2 or t.dtype != torch.int16:
        raise ValueError("expected int16 coefficients of shape (n, coef_pitch), got %s %s" % (tuple(t.shape), t.dtype))
    n, pitch = int(t.shape[0]), int(t.shape[1])
    if out_cap is None:
        from .jpeg_write import file_bound
        out_cap = n * (-(-file_bound(layout) // 16) * 16)
    out = torch.full((max(int(out_cap) + int(guard), 16),), int(fill), dtype=torch.uint8, device=t.device)
    rows = torch.full((max(n, 1) * 16,), 0xEE, dtype=torch.uint8, device=t.device)
    scratch = torch.empty(max(huffman_encode_scratch_bytes(layout, n, out_cap), 256), dtype=torch.uint8, device=t.device)
    huffman_encode_batch(layout, t.data_ptr(), pitch, n, out.data_ptr(), out_cap, rows.data_ptr(), scratch.data_ptr(), scratch.numel())
    torch.cuda.synchronize()
    out_h = out.cpu().numpy()
    rows_h = rows.cpu().numpy()[:16 * n].view(ROW_DTYPE)
    scans = [out_h[int(r["offset"]):int(r["offset"]) + int(r["bytes"])].tobytes() if r["status"] == 0 else b"" for r in rows_h]
    return scans, rows_h, out_h


def default_params() -> WriteSequenceParams:
    p = WriteSequenceParams()
    lib().ilcc_default_jpeg_write_sequence_params(C.byref(p))
    return p


def bag_save_jpeg_all(bag_path, topic, camera, path_prefix, quality=95, first=0, stride=1, max_images=0, staging_bytes=0, device_bytes=0,
                      out_bytes_per_image=0, huffman="gpu", device=0, raise_on_failure=True):
    """ilcc_bag_save_jpeg_all: every selected image of the topic -> mono8, undistorted with `camera` -> <path_prefix><message index,
    6 digits>.jpg.  huffman: "gpu" (K17) or "host" (or the route's number).  -> (WriteSequenceResult, [WriteRecord])"""
    p = default_params()
    p.first, p.stride, p.max_images = int(first), int(stride), int(max_images)
    p.staging_bytes, p.device_bytes, p.out_bytes_per_image = int(staging_bytes), int(device_bytes), int(out_bytes_per_image)
    p.route = ROUTES.get(huffman, huffman)
    L = lib()
    out = WriteSequenceResult()
    args = (device, os.fsencode(bag_path), topic.encode(), _camera_ref(camera), os.fsencode(path_prefix), int(quality), C.byref(p), C.byref(out))
    records = (WriteRecord * 1)()
    st = L.ilcc_bag_save_jpeg_all(*args, records, 1)           # a selection of several images: how many records, nothing run
    if st == _native.CAPACITY and out.n_images > 1:
        records = (WriteRecord * out.n_images)()
        st = L.ilcc_bag_save_jpeg_all(*args, records, out.n_images)
    got = list(records)[:min(max(out.n_images, 0), len(records))]
    if st != _native.OK and raise_on_failure:
        raise JpegWriteSequenceError(st, out, got)
    return out, got
