"""Camera corners from every CompressedImage of a recording: ctypes mirror of ``include/ilcc_jpeg_sequence.h``.

``idct_batch`` is K13b (IDCT, upsampling and colour on a batch of JPEG images of one geometry in two launches, byte for byte
what ``jpeg.idct`` gives image by image), ``entropy_decode_many`` decodes the scans of a batch on several host threads, and
``bag_corners_all_compressed_images`` is the chain bag -> fused ``<camera><i>.txt`` board for topics that carry
``sensor_msgs/CompressedImage``, the sibling of ``image_sequence.bag_corners_all_images``."""
import ctypes as C
import os

import numpy as np

from . import _native
from .camera_image import CameraImageError, CameraModel
from .image_corners import BoardNotFound
from .image_sequence import ImageRecord, ImageSequenceError, ImageSequenceParams, ImageSequenceResult, structure_route
from .jpeg import Info, parse

JPEG_SEQUENCE_EXPORTS = ["ilcc_jpeg_batch_scratch_bytes", "ilcc_jpeg_idct_batch_device", "ilcc_jpeg_entropy_decode_many",
                         "ilcc_default_jpeg_sequence_params", "ilcc_jpeg_sequence_bytes", "ilcc_bag_corners_all_compressed_images"]


class JpegSequenceParams(C.Structure):
    _fields_ = [("seq", ImageSequenceParams), ("decode_threads", C.c_uint32), ("reserved0", C.c_uint32)]


_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        vp, info, u64p = C.c_void_p, C.POINTER(Info), C.POINTER(C.c_uint64)
        L.ilcc_jpeg_batch_scratch_bytes.argtypes = [info, C.c_uint32]
        L.ilcc_jpeg_batch_scratch_bytes.restype = C.c_uint64
        L.ilcc_jpeg_idct_batch_device.argtypes = [info, vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.c_int32, vp, C.c_uint64, vp]
        L.ilcc_jpeg_idct_batch_device.restype = C.c_int32
        L.ilcc_jpeg_entropy_decode_many.argtypes = [C.POINTER(vp), u64p, info, C.POINTER(vp), u64p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
        L.ilcc_jpeg_entropy_decode_many.restype = C.c_int32
        L.ilcc_default_jpeg_sequence_params.argtypes = [C.POINTER(JpegSequenceParams)]
        L.ilcc_default_jpeg_sequence_params.restype = None
        L.ilcc_jpeg_sequence_bytes.argtypes = [info, u64p, u64p]
        L.ilcc_jpeg_sequence_bytes.restype = C.c_int32
        L.ilcc_bag_corners_all_compressed_images.argtypes = [C.c_int32, C.c_char_p, C.c_char_p, C.POINTER(CameraModel), C.c_int32, C.c_int32,
                                                             C.POINTER(JpegSequenceParams), C.POINTER(ImageSequenceResult), C.POINTER(ImageRecord),
                                                             C.c_uint32]
        L.ilcc_bag_corners_all_compressed_images.restype = C.c_int32
        _ready = True
    return L


def _last_error():
    return _native.lib().ilcc_last_error(None).decode()


def batch_scratch_bytes(layout, n_images) -> int:
    return int(lib().ilcc_jpeg_batch_scratch_bytes(C.byref(layout), int(n_images)))


def idct_batch(layout, quants, coefs, out=None):
    """K13b: `quants` [n, 3, 64] uint16 (row c of image m is component c's table, natural order) and `coefs` [n, pitch] int16
    (numpy or device tensors; pitch >= layout.coef_count, a multiple of 8) -> [n, rows, cols] mono8 or [n, rows, cols, 3] bgr8
    uint8 tensor on the current HIP device.  `out`: a uint8 device tensor (or view) of that shape whose rows hold bpp * width
    contiguous bytes; its stride(1) is the row pitch, its stride(0) the image pitch.  Asynchronous on the current stream."""
    import torch
    q = quants if isinstance(quants, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(quants, np.uint16).view(np.int16))
    t = coefs if isinstance(coefs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(coefs, np.int16))
    if t.dtype != torch.int16 or t.dim() != 2 or t.shape[1] < layout.coef_count:
        raise ValueError("expected [n, >= %d] int16 coefficients, got %s %s" % (layout.coef_count, tuple(t.shape), t.dtype))
    n = int(t.shape[0])
    if q.dim() != 3 or tuple(q.shape) != (n, 3, 64) or q.element_size() != 2:
        raise ValueError("expected [%d, 3, 64] 16-bit quantisation tables, got %s %s" % (n, tuple(q.shape), q.dtype))
    t = t.to("cuda")
    if n and t.stride(1) != 1:
        t = t.contiguous()
    q = q.to("cuda").contiguous()
    w, h, bpp = layout.width, layout.height, 1 if layout.n_components == 1 else 3
    if out is None:
        out = torch.empty((n, h, w) if bpp == 1 else (n, h, w, 3), dtype=torch.uint8, device=t.device)
    stride = int(out.stride(1)) if h > 1 else bpp * w
    pitch = int(out.stride(0)) if n > 1 else stride * h
    scratch = torch.empty(max(batch_scratch_bytes(layout, n), 16), dtype=torch.uint8, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    st = lib().ilcc_jpeg_idct_batch_device(C.byref(layout), C.c_void_p(q.data_ptr()), C.c_void_p(t.data_ptr()), int(t.stride(0)) if n > 1 else int(t.shape[1]),
                                           n, C.c_void_p(out.data_ptr()), pitch, stride, C.c_void_p(scratch.data_ptr()), scratch.numel(), stream)
    if st != _native.OK:
        raise ImageSequenceError(st, _last_error())
    return out


def quant_rows(info) -> np.ndarray:
    """[3, 64] uint16: row c is component c's table of a parsed file (a 1-component file: row 0 three times)"""
    q = info.quant_array()
    return np.stack([q[info.comp[c if c < info.n_components else 0].quant_index] for c in range(3)])


def entropy_decode_many(jpgs, threads=0, raise_on_failure=True):
    """ilcc_jpeg_entropy_decode_many on a list of JPEG files: -> (list of int16 coefficient arrays, list of statuses); a file whose
    headers do not parse gets its parse status and None.  Raises ImageSequenceError with the lowest failing file's text unless
    raise_on_failure is False (then `entropy_decode_many.last` holds (status, text) of the call)."""
    L = lib()
    n = len(jpgs)
    statuses, infos, first_bad = [_native.OK] * n, [None] * n, None
    for i, jpg in enumerate(jpgs):
        try:
            infos[i] = parse(jpg)
        except CameraImageError as e:
            statuses[i] = int(e.status)
            if first_bad is None:
                first_bad = (i, statuses[i], _last_error())
    jobs = [i for i in range(n) if infos[i] is not None]
    k = len(jobs)
    bufs = [np.frombuffer(bytes(jpgs[i]), np.uint8) for i in jobs]
    coefs = [np.zeros(infos[i].coef_count, np.int16) for i in jobs]
    jp = (C.c_void_p * max(k, 1))(*[b.ctypes.data for b in bufs])
    cp = (C.c_void_p * max(k, 1))(*[c.ctypes.data for c in coefs])
    nb = (C.c_uint64 * max(k, 1))(*[b.size for b in bufs])
    cap = (C.c_uint64 * max(k, 1))(*[c.size for c in coefs])
    info = (Info * max(k, 1))(*[infos[i] for i in jobs])
    status = (C.c_int32 * max(k, 1))()
    st = L.ilcc_jpeg_entropy_decode_many(jp, nb, info, cp, cap, k, int(threads), status)
    text = _last_error() if st != _native.OK else ""
    out = [None] * n
    for j, i in enumerate(jobs):
        statuses[i] = int(status[j])
        out[i] = coefs[j]
    lowest = next((i for i in range(n) if statuses[i] != _native.OK), None)
    if lowest is not None and first_bad is not None and first_bad[0] == lowest:
        st, text = first_bad[1], first_bad[2]
    elif lowest is not None:
        st = statuses[lowest]
    entropy_decode_many.last = (int(st), text)
    if raise_on_failure and lowest is not None:
        raise ImageSequenceError(st, text)
    return out, statuses


entropy_decode_many.last = (_native.OK, "")


def sequence_bytes(layout):
    """(staged bytes, device bytes) one image of `layout` takes in the chain: what it cuts its batches with"""
    staged, device = C.c_uint64(0), C.c_uint64(0)
    st = lib().ilcc_jpeg_sequence_bytes(C.byref(layout), C.byref(staged), C.byref(device))
    if st != _native.OK:
        raise ImageSequenceError(st, _last_error())
    return int(staged.value), int(device.value)


def default_params() -> JpegSequenceParams:
    sp = JpegSequenceParams()
    lib().ilcc_default_jpeg_sequence_params(C.byref(sp))
    return sp


def bag_corners_all_compressed_images(bag_path, topic, camera=None, board=(7, 5), first=0, stride=1, max_images=0, gate_px=0.0, staging_bytes=0,
                                      device_bytes=0, decode_threads=0, device=0, raise_on_failure=True, huffman="host", structure="host"):
    """Every selected CompressedImage of the bag's topic -> (ImageSequenceResult, [ImageRecord]).  Raises BoardNotFound when the
    fusion finds no board and ImageSequenceError on a refusal, unless raise_on_failure is False (then the result's status says
    so; the records are complete for the two fusion statuses).  huffman: "host", the decode pool, or "gpu", K16 (jpeg_huffman); the
    records are the same.  structure: "host" or "gpu" (K18), as in ``image_sequence.bag_corners_all_images``."""
    L = lib()
    sp = default_params()
    sp.seq.reserved0 = structure_route(structure)
    sp.seq.first, sp.seq.stride, sp.seq.max_images, sp.seq.gate_px = int(first), int(stride), int(max_images), float(gate_px)
    if staging_bytes:
        sp.seq.staging_bytes = int(staging_bytes)
    if device_bytes:
        sp.seq.device_bytes = int(device_bytes)
    sp.decode_threads = int(decode_threads)
    sp.reserved0 = {"host": 0, "gpu": 1}[huffman] if isinstance(huffman, str) else int(huffman)
    out = ImageSequenceResult()
    cam = C.byref(camera) if camera is not None else None
    args = (int(device), os.fsencode(bag_path), topic.encode(), cam, int(board[0]), int(board[1]), C.byref(sp), C.byref(out))
    buf = (ImageRecord * 1)()
    st = L.ilcc_bag_corners_all_compressed_images(*args, buf, 1)    # one record is too few for most bags: the refusal says how many, nothing runs
    if st == _native.CAPACITY and out.n_images > 1:
        buf = (ImageRecord * out.n_images)()
        st = L.ilcc_bag_corners_all_compressed_images(*args, buf, out.n_images)
    detail = _last_error()
    records = list(buf)[:out.n_images] if st in (_native.OK, _native.BOARD_NOT_FOUND, _native.AMBIGUOUS) else []
    if raise_on_failure:
        if st in (_native.BOARD_NOT_FOUND, _native.AMBIGUOUS):
            raise BoardNotFound(st, "%s: %s" % (_native.strerror(st), detail))
        if st != _native.OK:
            raise ImageSequenceError(st, detail)
    return out, records
