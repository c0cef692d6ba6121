"""numpy restatement of the JPEG writer of include/ilcc_jpeg_write.h: libjpeg's default forward path (jccolor, the plain
h2v1 / h2v2 downsamplers with their edge expansion, jfdctint "islow", its quantiser, the dummy blocks of an interleaved
scan) and a baseline Huffman encoder with the Annex-K tables.  Written from the JPEG standard (ITU-T T.81) and the
arithmetic the header states; independent of the C++ / HIP code it checks.  Its files are tied to libjpeg by the recorded
hashes of tests/golden/jpeg_write/expected.json (and to Pillow directly where it imports).

    info = make_info(w, h, sampling, quality, restart_interval)      a jpeg_ref.Info: sampling None (1 component) or (h, v)
    coef = coefficients(info, px)         int16 in the decoder's layout, dummy blocks included; px (h, w) or (h, w, 3) B, G, R
    data = entropy_encode(info, coef)     the whole file; raises Unencodable for a value libjpeg refuses
    data = encode(px, quality, sampling, restart_interval)
"""
import numpy as np

import jpeg_ref as R

SAMPLINGS = {"gray": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}

# ITU-T T.81 Annex K.1, natural (row-major) order
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
            100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
              99] + [99] * 32

# Annex K.3: (class, index) -> (counts of the code lengths 1 .. 16, symbols)
STD_HUFF = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
             [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
              240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
              213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
              249, 250]),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
              240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
              69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
              120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
              165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
              210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247,
              248, 249, 250]),
}


class Unencodable(ValueError):
    """A DC difference outside 11 bits or an AC value outside 10 bits: libjpeg refuses these too."""


def quant_tables(quality):
    """(2, 64) uint16: the Annex-K tables scaled as libjpeg's jpeg_set_quality(quality, force_baseline) does."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    std = np.array([STD_LUMA, STD_CHROMA], np.int64)
    return np.clip((std * scale + 50) // 100, 1, 255).astype(np.uint16)


def make_info(width, height, sampling=None, quality=95, restart_interval=0):
    info = R.make_info(width, height, sampling, quant_tables(quality))
    info.have_quant = [True, True, False, False]
    for i, c in enumerate(info.comps):
        c.td = c.ta = min(i, 1)
    info.huff = {k: v for k, v in STD_HUFF.items() if k[1] < (1 if sampling is None else 2)}
    info.restart_interval = restart_interval
    return info


# ---------------------------------------------------------------- pixels -> sample planes

def colour_planes(px):
    """(h, w, 3) B, G, R uint8 -> Y, Cb, Cr int32 at full resolution (jccolor.c)."""
    b, g, r = [px[..., k].astype(np.int32) for k in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return y, cb, cr


def _replicate(a, rows, cols):
    """`a` grown to (rows, cols) by repeating its last column, then its last row."""
    a = np.concatenate([a, np.repeat(a[:, -1:], cols - a.shape[1], axis=1)], axis=1) if cols > a.shape[1] else a
    return np.concatenate([a, np.repeat(a[-1:], rows - a.shape[0], axis=0)], axis=0) if rows > a.shape[0] else a


def sample_planes(info, px):
    """The sample plane of every component over its REAL blocks (ceil(real size / 8) each way), int32."""
    w, h = info.width, info.height
    if info.n_components == 1:
        return [_replicate(np.asarray(px).astype(np.int32), -(-h // 8) * 8, -(-w // 8) * 8)]
    hs, vs = info.sampling
    full = colour_planes(np.asarray(px))
    out = [_replicate(full[0], -(-h // 8) * 8, -(-w // 8) * 8)]
    wc, hc = -(-w // hs), -(-h // vs)
    cols, rows = -(-wc // 8) * 8, -(-hc // 8) * 8
    for p in full[1:]:
        # full-resolution columns are replicated BEFORE downsampling; an odd last row is replicated once
        p = _replicate(p, hc * vs, cols * hs)
        if hs == 2 and vs == 1:
            bias = np.arange(cols) & 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif hs == 2:
            bias = 1 + (np.arange(cols) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_replicate(p, rows, cols))            # below that, DOWNSAMPLED rows are replicated
    return out


# ---------------------------------------------------------------- samples -> quantised coefficients

def _fdct_pass(d, first):
    """One 8-point pass of jfdctint.c along the last axis of an int64 array."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    s = 11 if first else 15
    half = 1 << (s - 1)
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o2 = (z1 + t13 * 6270 + half) >> s
    o6 = (z1 - t12 * 15137 + half) >> s
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o7 = (t4 + z1 + z3 + half) >> s
    o5 = (t5 + z2 + z4 + half) >> s
    o3 = (t6 + z2 + z3 + half) >> s
    o1 = (t7 + z1 + z4 + half) >> s
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def fdct_blocks(samples):
    """(n, 8, 8) samples 0 .. 255 -> (n, 8, 8) int64 DCT coefficients scaled by 8 (as libjpeg leaves them)."""
    x = samples.astype(np.int64) - 128
    rows = _fdct_pass(x, True)                                        # pass 1 over rows
    return _fdct_pass(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)   # pass 2 over columns


def quantise(c, quant):
    """(n, 8, 8) DCT coefficients, quant (64,) -> (n, 64): sign(c) * ((|c| + (d >> 1)) / d), d = 8 * quant."""
    d = quant.reshape(8, 8).astype(np.int64) * 8
    return (np.sign(c) * ((np.abs(c) + (d >> 1)) // d)).reshape(-1, 64)


def plane_coefficients(plane, quant):
    """A sample plane of (bh * 8, bw * 8) -> (bh, bw, 64) quantised coefficients."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    return quantise(fdct_blocks(blocks), quant).reshape(bh, bw, 64)


def coefficients(info, px):
    """The coefficient buffer of the decoder (jpeg_ref.entropy_decode), the dummy blocks of an interleaved scan as
    libjpeg makes them: all AC zero; DC of the block to the left, in a row below the real blocks of the previous block
    in MCU order."""
    out = np.zeros(info.coef_count, np.int16)
    for c, plane in zip(info.comps, sample_planes(info, px)):
        real = plane_coefficients(plane, info.quant[c.tq])
        rbh, rbw = real.shape[:2]
        grid = np.zeros((c.blocks_h, c.blocks_w, 64), np.int64)
        grid[:rbh, :rbw] = real
        assert c.blocks_w - rbw in (0, c.h - 1) and c.blocks_h - rbh in (0, c.v - 1)
        if c.blocks_w > rbw:
            grid[:rbh, rbw, 0] = grid[:rbh, rbw - 1, 0]
        if c.blocks_h > rbh:                                         # v == 2: both take the DC of the MCU's top-right block
            top_right = grid[rbh - 1, c.h - 1::c.h, 0]
            grid[rbh, :, 0] = np.repeat(top_right, c.h)
        out[c.offset:c.offset + grid.size] = grid.reshape(-1).astype(np.int16)
    return out


# ---------------------------------------------------------------- coefficients -> file

def _codes(counts, values):
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[values[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):                                                 # 1-bits up to the byte boundary
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def headers(info):
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    n = info.n_components
    for t in range(1 if n == 1 else 2):
        out += _segment(0xDB, bytes([t]) + bytes(int(info.quant[t][k]) for k in R.ZIGZAG))
    sof = bytes([8, info.height >> 8, info.height & 255, info.width >> 8, info.width & 255, n])
    for i, c in enumerate(info.comps):
        sof += bytes([i + 1, (c.h << 4) | c.v, c.tq])
    out += _segment(0xC0, sof)
    for t in range(1 if n == 1 else 2):
        for cls in (0, 1):
            counts, values = STD_HUFF[(cls, t)]
            out += _segment(0xC4, bytes([(cls << 4) | t]) + bytes(counts) + bytes(values))
    if info.restart_interval:
        out += _segment(0xDD, bytes([info.restart_interval >> 8, info.restart_interval & 255]))
    sos = bytes([n])
    for i, c in enumerate(info.comps):
        sos += bytes([i + 1, (c.td << 4) | c.ta])
    return out + _segment(0xDA, sos + b"\x00\x3f\x00")


def entropy_encode(info, coef):
    coef = np.asarray(coef)
    assert coef.size == info.coef_count
    dc = {c.td: _codes(*STD_HUFF[(0, c.td)]) for c in info.comps}
    ac = {c.ta: _codes(*STD_HUFF[(1, c.ta)]) for c in info.comps}
    if info.n_components == 1:
        c = info.comps[0]
        mcus_w, mcus_h = c.blocks_w, c.blocks_h
        units = [(0, c, 0, 0)]
    else:
        hmax, vmax = info.sampling
        mcus_w, mcus_h = info.comps[0].blocks_w // hmax, info.comps[0].blocks_h // vmax
        units = [(i, c, dx, dy) for i, c in enumerate(info.comps) for dy in range(c.v) for dx in range(c.h)]
    zz = R.ZIGZAG.tolist()
    w = _BitWriter()
    pred = [0, 0, 0]
    values = coef.astype(np.int64).tolist()
    for m in range(mcus_w * mcus_h):
        if info.restart_interval and m and m % info.restart_interval == 0:
            w.flush()
            w.out += bytes([0xFF, 0xD0 + (m // info.restart_interval - 1) % 8])
            pred = [0, 0, 0]
        my, mx = divmod(m, mcus_w)
        for i, c, dx, dy in units:
            at = c.offset + ((my * c.v + dy) * c.blocks_w + mx * c.h + dx) * 64
            block = values[at:at + 64]
            diff = block[0] - pred[i]
            pred[i] = block[0]
            bits = abs(diff).bit_length()
            if bits > 11:
                raise Unencodable("DC difference %d outside 11 bits" % diff)
            w.put(*dc[c.td][bits])
            if bits:
                w.put(diff if diff > 0 else diff + (1 << bits) - 1, bits)
            run = 0
            codes = ac[c.ta]
            for k in range(1, 64):
                v = block[zz[k]]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*codes[0xF0])
                    run -= 16
                bits = abs(v).bit_length()
                if bits > 10:
                    raise Unencodable("AC value %d outside 10 bits" % v)
                w.put(*codes[(run << 4) | bits])
                w.put(v if v > 0 else v + (1 << bits) - 1, bits)
                run = 0
            if run:
                w.put(*codes[0])
    w.flush()
    return headers(info) + bytes(w.out) + b"\xff\xd9"


def encode(px, quality=95, sampling=(2, 2), restart_interval=0):
    px = np.asarray(px)
    info = make_info(px.shape[1], px.shape[0], None if px.ndim == 2 else sampling, quality, restart_interval)
    return entropy_encode(info, coefficients(info, px))
