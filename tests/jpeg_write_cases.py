"""Inputs shared by tests/test_jpeg_write_cpu.py, tests/test_jpeg_write.py and the fixture generator of
tests/golden/jpeg_write: the case grid, the seeded source pixels and the restatement's result for each case."""
import functools
import hashlib
import json
import os
import zlib

import numpy as np

import jpeg_write_ref as W

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_write")

# (w, h): both sides of the 8-pixel block, the 16-pixel MCU and the 256-pixel workgroup row.  For 4:2:0 luma: no dummy
# block (9 x 9, 16 x 16, 31 x 16, 255 x 9), a dummy column alone (257 x 9, 263 x 15), a dummy row alone (15 x 17), both (the
# rest); odd sizes whose chroma planes end in padded columns and rows that are no real samples
SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (33, 17), (31, 16), (24, 24), (40, 24), (255, 9), (257, 9),
         (263, 15)]
MODES = ["gray", "444", "422", "420"]
QUALITIES = [1, 50, 95, 100]          # 1 clamps the table at 255, 100 has every divisor equal to 8
RESTARTS = [0, 2]
COMMITTED_SIZES = [(1, 1), (7, 5), (9, 9)]   # the files kept beside expected.json: noise at quality 95, every mode


def case_name(kind, w, h, mode, quality, restart):
    return "%s_%dx%d_%s_q%d_r%d" % (kind, w, h, mode, quality, restart)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (kind, w, h, mode, quality, restart).  Noise over the whole grid; the ramp and the checker, which exercise
    the arithmetic and not the layout, at quality 95 and 100 without restarts."""
    out = {}
    for w, h in SIZES:
        for mode in MODES:
            for q in QUALITIES:
                for r in RESTARTS:
                    out[case_name("noise", w, h, mode, q, r)] = ("noise", w, h, mode, q, r)
            for kind, q in (("ramp", 95), ("checker", 100)):
                out[case_name(kind, w, h, mode, q, 0)] = (kind, w, h, mode, q, 0)
    return out


def committed_files():
    return [case_name("noise", w, h, mode, 95, 0) + ".jpg" for w, h in COMMITTED_SIZES for mode in MODES]


@functools.lru_cache(maxsize=None)
def source(name):
    """The case's pixels: (h, w) mono8 or (h, w, 3) B, G, R uint8, from a seed that is the CRC-32 of the name."""
    kind, w, h, mode, _, _ = cases()[name]
    channels = 1 if mode == "gray" else 3
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        a = np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, (h, w, channels), dtype=np.uint8)
    elif kind == "ramp":
        a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)][:channels],
                     axis=-1).astype(np.uint8)
    else:   # two levels in 3-pixel squares: the DCT overshoots 0 and 255, a decoder clamps at both ends
        c = (((x // 3 + y // 3) & 1) * 255).astype(np.uint8)
        a = np.stack([c, 255 - c, c][:channels], axis=-1)
    a = np.ascontiguousarray(a[..., 0] if channels == 1 else a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(HERE, "expected.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(info, coefficients, file bytes) of a case by the restatement; computed once, never written to."""
    _, w, h, mode, q, r = cases()[name]
    info = W.make_info(w, h, W.SAMPLINGS[mode], q, r)
    coef = W.coefficients(info, source(name))
    coef.setflags(write=False)
    return info, coef, W.entropy_encode(info, coef)


def sha256(data):
    return hashlib.sha256(bytes(data)).hexdigest()
