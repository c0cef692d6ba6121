"""K16, the Huffman scans of a batch of JPEG frames decoded on the GPU: ctypes mirror of ``include/ilcc_jpeg_huffman.h``.

``scan_prepare`` is the host's part (unstuffing, restart markers, the tables as the kernel reads them), ``Batch`` lays the prepared
images of one geometry out as the entry takes them, ``huffman_batch`` is the entry on device tensors, and ``decode_batch`` goes from
a list of files to their coefficients and statuses as numpy arrays: what ``jpeg.entropy_decode`` gives file by file."""
import ctypes as C

import numpy as np

from . import _native
from .camera_image import _check
from .jpeg import Info, _bytes_arg, parse

JPEG_HUFFMAN_EXPORTS = ["ilcc_jpeg_scan_bound", "ilcc_jpeg_scan_prepare", "ilcc_jpeg_huffman_scratch_bytes", "ilcc_jpeg_huffman_batch_device",
                        "ilcc_jpeg_huffman_sequence_bytes"]

DEFAULT_BITS = 2048
SUBSEQUENCE_BITS = (256, 512, 1024, 2048)
NO_CODE, RUN_PAST_63, DC_CATEGORY, DC_RANGE, ENDS_EARLY, BAD_ROWS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20


class Segment(C.Structure):
    _fields_ = [("byte_offset", C.c_uint32), ("byte_count", C.c_uint32), ("first_mcu", C.c_uint32), ("mcu_count", C.c_uint32)]


class Table(C.Structure):
    _fields_ = [("look", C.c_uint16 * 512), ("maxcode", C.c_int32 * 17), ("first", C.c_int32 * 17), ("values", C.c_uint8 * 256)]


class Tables(C.Structure):
    _fields_ = [("dc", Table * 3), ("ac", Table * 3)]


class Image(C.Structure):
    _fields_ = [("scan_offset", C.c_uint64), ("scan_bytes", C.c_uint32), ("first_segment", C.c_uint32), ("n_segments", C.c_uint32),
                ("reserved", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("subsequences", C.c_uint32), ("chunks", C.c_uint32), ("rounds", C.c_uint32), ("max_rounds", C.c_uint32)]


class Job(C.Structure):
    _fields_ = [("layout", C.POINTER(Info)), ("d_scans", C.c_void_p), ("scans_bytes", C.c_uint64), ("d_tables", C.c_void_p),
                ("d_segments", C.c_void_p), ("d_images", C.c_void_p), ("d_coef", C.c_void_p), ("coef_pitch", C.c_uint64),
                ("d_status", C.c_void_p), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_uint64), ("n_images", C.c_uint32),
                ("n_segments", C.c_uint32), ("max_segments", C.c_uint32), ("subsequence_bits", C.c_uint32), ("hip_stream", C.c_void_p)]


STRUCT_SIZES = {"ilcc_jpeg_huffman_segment": (Segment, 16), "ilcc_jpeg_huffman_table": (Table, 1416), "ilcc_jpeg_huffman_tables": (Tables, 8496),
                "ilcc_jpeg_huffman_image": (Image, 24), "ilcc_jpeg_huffman_counters": (Counters, 16), "ilcc_jpeg_huffman_job": (Job, 112)}

_ready = False


def lib():
    global _ready
    L = _native.lib()
    if not _ready:
        u8p, info, u64p, u32p = C.POINTER(C.c_uint8), C.POINTER(Info), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        L.ilcc_jpeg_scan_bound.argtypes = [info, C.c_uint64, u64p, u32p]
        L.ilcc_jpeg_scan_bound.restype = C.c_int32
        L.ilcc_jpeg_scan_prepare.argtypes = [u8p, C.c_uint64, info, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint32, u32p, C.POINTER(Tables)]
        L.ilcc_jpeg_scan_prepare.restype = C.c_int32
        L.ilcc_jpeg_huffman_scratch_bytes.argtypes = [C.c_uint32]
        L.ilcc_jpeg_huffman_scratch_bytes.restype = C.c_uint64
        L.ilcc_jpeg_huffman_batch_device.argtypes = [C.POINTER(Job)]
        L.ilcc_jpeg_huffman_batch_device.restype = C.c_int32
        L.ilcc_jpeg_huffman_sequence_bytes.argtypes = [info, C.c_uint64, C.c_uint32, u64p, u64p]
        L.ilcc_jpeg_huffman_sequence_bytes.restype = C.c_int32
        _ready = True
    return L


def scan_bound(info, file_bytes):
    """(unstuffed bytes, segments) at most that scan_prepare writes for a file of that size with these headers"""
    nb, ns = C.c_uint64(0), C.c_uint32(0)
    _check(lib().ilcc_jpeg_scan_bound(C.byref(info), int(file_bytes), C.byref(nb), C.byref(ns)))
    return int(nb.value), int(ns.value)


def scan_prepare(jpg, info=None, scan_cap=None, segment_cap=None):
    """-> (scan uint8[scan_bytes], segments uint32[n, 4] (byte offset, byte count, first MCU, MCU count), Tables) of a file;
    raises CameraImageError with the host decoder's words where it refuses.  The capacities default to scan_bound's."""
    info = info if info is not None else parse(jpg)
    arr, n = _bytes_arg(jpg)
    if scan_cap is None or segment_cap is None:
        nb, ns = scan_bound(info, n)
        scan_cap = nb if scan_cap is None else scan_cap
        segment_cap = ns if segment_cap is None else segment_cap
    scan = np.zeros(max(int(scan_cap), 1), np.uint8)
    rows = np.zeros((max(int(segment_cap), 1), 4), np.uint32)
    tables = Tables()
    used, n_rows = C.c_uint64(0), C.c_uint32(0)
    _check(lib().ilcc_jpeg_scan_prepare(arr, n, C.byref(info), scan.ctypes.data_as(C.c_void_p), int(scan_cap), C.byref(used),
                                        rows.ctypes.data_as(C.c_void_p), int(segment_cap), C.byref(n_rows), C.byref(tables)))
    return scan[:used.value].copy(), rows[:n_rows.value].copy(), tables


def scratch_bytes(n_images) -> int:
    return int(lib().ilcc_jpeg_huffman_scratch_bytes(int(n_images)))


def sequence_bytes(layout, data_bytes, n_segments):
    """(staged bytes, device bytes) one image takes in the chain on the K16 route"""
    staged, device = C.c_uint64(0), C.c_uint64(0)
    _check(lib().ilcc_jpeg_huffman_sequence_bytes(C.byref(layout), int(data_bytes), int(n_segments), C.byref(staged), C.byref(device)))
    return int(staged.value), int(device.value)


class Batch:
    """The prepared images of one geometry as ilcc_jpeg_huffman_batch_device takes them: numpy arrays `scans` (uint8, concatenated),
    `tables` (uint8 [n, 8496]), `segments` (uint32 [rows, 4]), `images` (uint8 [n, 24]) and max_segments.  `prepared`: what
    scan_prepare returned for each image."""

    def __init__(self, prepared):
        self.n = len(prepared)
        scans, rows, images, at, row = [], [], (Image * max(self.n, 1))(), 0, 0
        for m, (scan, seg, _) in enumerate(prepared):
            images[m].scan_offset, images[m].scan_bytes, images[m].first_segment, images[m].n_segments = at, len(scan), row, len(seg)
            scans.append(scan)
            rows.append(seg)
            at += len(scan)
            row += len(seg)
        self.scans = np.concatenate(scans + [np.zeros(1, np.uint8)]) if self.n else np.zeros(1, np.uint8)   # never empty: a device pointer
        self.scans_bytes = at
        self.segments = np.concatenate(rows).astype(np.uint32).reshape(-1, 4) if row else np.zeros((1, 4), np.uint32)
        self.n_segments = row
        self.max_segments = max([len(seg) for _, seg, _ in prepared], default=0)
        self.tables = np.stack([np.frombuffer(bytes(t), np.uint8) for _, _, t in prepared]) if self.n else np.zeros((1, C.sizeof(Tables)), np.uint8)
        self.images = np.frombuffer(bytes(images), np.uint8).reshape(-1, C.sizeof(Image))[:max(self.n, 1)].copy()


def huffman_batch(layout, d_scans, scans_bytes, d_tables, d_segments, n_segments, d_images, n_images, max_segments, d_coef, coef_pitch,
                  d_status, d_scratch, scratch_nbytes, subsequence_bits=0, stream=None):
    """ilcc_jpeg_huffman_batch_device on device addresses (ints); `stream`: a hipStream_t as int, default the current torch stream.
    Raises CameraImageError on a refusal; asynchronous."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    job = Job(C.pointer(layout), d_scans, int(scans_bytes), d_tables, d_segments, d_images, d_coef, int(coef_pitch), d_status, d_scratch,
              int(scratch_nbytes), int(n_images), int(n_segments), int(max_segments), int(subsequence_bits), stream)
    _check(lib().ilcc_jpeg_huffman_batch_device(C.byref(job)))


def decode_batch(jpgs, subsequence_bits=0, coef_pitch=None, fill=0, with_counters=False):
    """K16 on a list of JPEG files of one geometry -> (coef int16 [n, coef_pitch], status uint32 [n]) as numpy arrays; with
    with_counters also uint32 [n, 4] (subsequences, chunks, rounds, max_rounds).  Row m of coef holds image m's coef_count
    coefficients as jpeg.entropy_decode gives them wherever status[m] == 0; what lies behind them keeps `fill`.  The files'
    headers must parse and the scans must pass scan_prepare (CameraImageError otherwise); what is wrong INSIDE a scan comes back
    as that image's status."""
    import torch
    infos = [parse(j) for j in jpgs]
    if not infos:
        raise ValueError("decode_batch needs at least one file")
    layout = infos[0]
    for i in infos[1:]:
        same = (i.width, i.height, i.n_components) == (layout.width, layout.height, layout.n_components) and all(
            (i.comp[c].h, i.comp[c].v) == (layout.comp[c].h, layout.comp[c].v) for c in range(layout.n_components))
        if not same:
            raise ValueError("the files of a batch must share width, height, component count and sampling")
    b = Batch([scan_prepare(j, i) for j, i in zip(jpgs, infos)])
    pitch = int(coef_pitch) if coef_pitch is not None else -(-int(layout.coef_count) // 8) * 8
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("scans", b.scans), ("tables", b.tables), ("segments", b.segments), ("images", b.images))}
    coef = torch.full((b.n, pitch), int(fill), dtype=torch.int16, device="cuda")
    status = torch.full((b.n,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(max(scratch_bytes(b.n), 16), dtype=torch.uint8, device="cuda")
    huffman_batch(layout, dev["scans"].data_ptr(), b.scans_bytes, dev["tables"].data_ptr(), dev["segments"].data_ptr(), b.n_segments,
                  dev["images"].data_ptr(), b.n, b.max_segments, coef.data_ptr(), pitch, status.data_ptr(), scratch.data_ptr(), scratch.numel(),
                  subsequence_bits)
    torch.cuda.synchronize()
    out = coef.cpu().numpy(), status.cpu().numpy().view(np.uint32)
    if with_counters:
        out += (scratch.cpu().numpy()[:16 * b.n].view(np.uint32).reshape(b.n, 4),)
    return out
