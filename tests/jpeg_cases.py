"""Inputs shared by tests/test_jpeg_cpu.py and tests/test_jpeg.py: the fixtures of tests/golden/jpeg, the files every
refusal of include/ilcc_jpeg.h is provoked with (patched byte strings of two fixtures), and constructed coefficients."""
import functools
import hashlib
import json
import os

import numpy as np

import jpeg_ref as R

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
SAMPLING_OF = {"gray": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}


@functools.lru_cache(maxsize=None)
def expected():
    with open(os.path.join(HERE, "expected.json")) as f:
        return json.load(f)


def small_fixtures():
    return sorted(n for n in expected() if not n.startswith("pointgrey"))


def reference_images():
    return ["pointgrey%d.jpg" % i for i in range(1, 7)]


@functools.lru_cache(maxsize=None)
def data(name):
    with open(os.path.join(HERE, name), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def restated(name):
    """(info, coefficients, pixels) of a fixture by the restatement; computed once, never written to."""
    info = R.parse(data(name))
    coef = R.entropy_decode(data(name), info)
    px = R.pixels(info, coef)
    coef.setflags(write=False)
    px.setflags(write=False)
    return info, coef, px


def sha256(pixels):
    return hashlib.sha256(np.ascontiguousarray(pixels).tobytes()).hexdigest()


# ---------------------------------------------------------------- refusals

GRAY, COLOUR, MANY_BLOCKS = "noise_9x7_gray_q50_r0.jpg", "noise_17x33_420_q50_r0.jpg", "noise_50x35_gray_q50_r0.jpg"


def _segment(jpg, marker, nth=0):
    """Offset of the nth 0xFF `marker` segment's marker in the headers."""
    at = 2
    while at < len(jpg):
        assert jpg[at] == 0xFF
        m, length = jpg[at + 1], (jpg[at + 2] << 8) | jpg[at + 3]
        if m == marker:
            if nth == 0:
                return at
            nth -= 1
        if m == 0xDA:
            break
        at += 2 + length
    raise KeyError(hex(marker))


def _patched(jpg, at, *values):
    out = bytearray(jpg)
    out[at:at + len(values)] = bytes(values)
    return bytes(out)


def _inserted(jpg, at, segment):
    return jpg[:at] + segment + jpg[at:]


def _without(jpg, marker):
    at = _segment(jpg, marker)
    return jpg[:at] + jpg[at + 2 + ((jpg[at + 2] << 8) | jpg[at + 3]):]


def _without_all(jpg, marker):
    while True:
        try:
            jpg = _without(jpg, marker)
        except KeyError:
            return jpg


def _codes(info, cls, index):
    """symbol -> (code, length) of one Huffman table of the file."""
    counts, values = info.huff[(cls, index)]
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[values[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _with_scan(jpg, bits):
    """The file with its entropy-coded data replaced by `bits` (a string of 0 / 1), padded with 1 and byte-stuffed."""
    info = R.parse(jpg)
    bits += "1" * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    return jpg[:info.scan_offset] + raw + b"\xff\xd9"


def _bits(code_len):
    return format(code_len[0], "0%db" % code_len[1])


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (bytes, the restatement's cause, words the library's last-error text must hold)."""
    g, c, many = data(GRAY), data(COLOUR), data(MANY_BLOCKS)
    sof_g, sof_c, sos_c, sos_g = _segment(g, 0xC0), _segment(c, 0xC0), _segment(c, 0xDA), _segment(g, 0xDA)
    ginfo, minfo = R.parse(g), R.parse(many)
    dc, ac = _codes(ginfo, 0, 0), _codes(ginfo, 1, 0)
    mdc, mac = _codes(minfo, 0, 0), _codes(minfo, 1, 0)
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    eoi_g = g.rindex(b"\xff\xd9")
    cases = {
        "progressive": (_patched(g, sof_g + 1, 0xC2), "progressive", "progressive"),
        "lossless": (_patched(g, sof_g + 1, 0xC3), "lossless", "lossless"),
        "arithmetic": (_patched(g, sof_g + 1, 0xC9), "arithmetic", "arithmetic"),
        "12-bit samples": (_patched(g, sof_g + 4, 12), "12-bit", "12-bit"),
        "16-bit quantisation table": (_patched(g, _segment(g, 0xDB) + 4, 0x10), "16-bit quantisation", "16-bit quantisation"),
        "2 components": (_patched(c, sof_c + 9, 2), "components", "2 components"),
        "4 components": (_patched(c, sof_c + 9, 4), "components", "4 components"),
        "Adobe transform 0": (_inserted(c, 2, adobe), "Adobe transform 0", "Adobe transform 0"),
        "sampling 1x2": (_patched(c, sof_c + 11, 0x12), "sampling", "sampling"),
        "sampling 4x1": (_patched(c, sof_c + 11, 0x41), "sampling", "sampling"),
        "chroma sampled 2x1": (_patched(c, sof_c + 14, 0x21), "sampling", "sampling"),
        "a scan of one component": (_patched(c, sos_c + 4, 1), "several scans", "several scans"),
        "a second scan": (_inserted(g, eoi_g, g[sos_g:sos_g + 2 + ((g[sos_g + 2] << 8) | g[sos_g + 3])] + b"\x00"), "several scans",
                          "several scans"),
        "DNL in the headers": (_inserted(g, sos_g, b"\xff\xdc\x00\x04\x00\x07"), "DNL", "DNL"),
        "DNL behind the scan": (_inserted(g, eoi_g, b"\xff\xdc\x00\x04\x00\x07"), "DNL", "DNL"),
        "quantisation table missing": (_without(g, 0xDB), "table used before it is defined", "before it is defined"),
        "quantisation table 3 not defined": (_patched(g, sof_g + 12, 3), "table used before it is defined", "before it is defined"),
        "Huffman table 2 not defined": (_patched(g, sos_g + 6, 0x20), "table used before it is defined", "before it is defined"),
        "Huffman tables missing": (_without_all(c, 0xC4), "table used before it is defined",
                                   "before it is defined"),
        "a code in no table": (_with_scan(g, "1" * 64), "Huffman code in no table", "in no table"),
        "four ZRL": (_with_scan(g, _bits(dc[0]) + _bits(ac[0xF0]) * 4), "run past coefficient 63", "run past coefficient 63"),
        "a run of 15 at coefficient 49": (_with_scan(g, _bits(dc[0]) + _bits(ac[0xF0]) * 3 + _bits(ac[0xF1]) + "1"),
                                          "run past coefficient 63", "run past coefficient 63"),
        "DC sum above 32767": (_with_scan(many, (_bits(mdc[11]) + "1" * 11 + _bits(mac[0])) * 35), "DC predictor leaves int16",
                               "DC predictor leaves int16"),
        "DC sum below -32768": (_with_scan(many, (_bits(mdc[11]) + "0" * 11 + _bits(mac[0])) * 35), "DC predictor leaves int16",
                                "DC predictor leaves int16"),
        "cut inside the scan": (c[:R.parse(c).scan_offset + 40], "ends early", "ends early"),
        "cut inside the headers": (g[:sos_g + 3], "ends early", "ends early"),
        "only SOI and EOI": (b"\xff\xd8\xff\xd9", "ends early", "ends early"),
        "height 0": (_patched(g, sof_g + 5, 0, 0), "width or height of 0", "width or height of 0"),
        "width 0": (_patched(g, sof_g + 7, 0, 0), "width or height of 0", "width or height of 0"),
    }
    return cases


def restatement_refuses(jpg):
    """The cause the restatement refuses the bytes for, None when it decodes them."""
    try:
        info = R.parse(jpg)
        R.entropy_decode(jpg, info)
    except R.JpegRefusal as e:
        return e.cause
    return None


# ---------------------------------------------------------------- constructed coefficients (no Huffman involved)

QUANTS = {"ones": np.ones(64, np.uint16), "255": np.full(64, 255, np.uint16), "ramp": (1 + 4 * np.arange(64)).astype(np.uint16)}

# block grids (blocks_w, blocks_h) with image sizes that clip the last block to 1 and to 7 pixels on each axis
GRIDS = [(1, 1, 1, 1), (1, 1, 7, 7), (2, 1, 9, 7), (2, 1, 15, 1), (1, 2, 1, 15), (1, 2, 7, 9), (33, 2, 257, 9), (33, 2, 263, 15),
         (32, 3, 249, 17), (32, 3, 255, 23), (32, 3, 256, 24)]       # (blocks_w, blocks_h, width, height)


def grid_coefficients(count, seed, amplitude=300):
    """Sparse-ish random coefficients of `count` int16: strong DC, decaying AC, as an encoder leaves them."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-amplitude, amplitude + 1, (count // 64, 64))
    decay = 1.0 / (1 + np.arange(64) % 8 + np.arange(64) // 8)
    c = (c * decay * (rng.random((count // 64, 64)) < 0.5)).astype(np.int16)
    c[:, 0] = rng.integers(-60, 61, count // 64)
    return c.reshape(-1)


def single_coefficient_blocks():
    """(coef, what): one block per (k, sign, amplitude) with only coefficient k set -- 64 x 2 x 2 = 256 blocks side by side.
    With quant 8 the amplitude 4 gives +-32 (at most 128 +- 4 * 8 * 8 / 8: no clamp), 120 gives +-960 (clamps)."""
    blocks = []
    for amplitude in (4, 120):
        for sign in (1, -1):
            for k in range(64):
                b = np.zeros(64, np.int16)
                b[k] = sign * amplitude
                blocks.append(b)
    return np.concatenate(blocks)
