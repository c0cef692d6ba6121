"""numpy restatement of the JPEG decoder of include/ilcc_jpeg.h: marker parse, Huffman entropy decode, libjpeg's
`islow` inverse DCT, "fancy" chroma upsampling and fixed-point YCbCr -> BGR.  Written from the JPEG standard
(ITU-T T.81) and the arithmetic the header states; independent of the C++ / HIP code it checks.  Its pixels are
tied to libjpeg by the recorded hashes of tests/golden/jpeg/expected.json (and to Pillow directly where it imports).

    info = parse(data)                    headers only; raises JpegRefusal(cause)
    coef = entropy_decode(data, info)     int16, de-zigzagged: coef[offset_c + (by * blocks_w_c + bx) * 64 + k]
    px = pixels(info, coef)               (h, w) mono8 or (h, w, 3) B, G, R; checks the int32 domain in int64
    px = decode(data)
"""
import struct

import numpy as np

COMPRESSED_IMAGE_MD5 = "8f7a12909da2c9d3332d540a0977563f"

# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# the causes a file is refused for; the library's last-error text holds the same words
REFUSALS = ("progressive", "lossless", "arithmetic", "12-bit", "16-bit quantisation", "components", "Adobe transform 0",
            "sampling", "several scans", "DNL", "table used before it is defined", "Huffman code in no table",
            "run past coefficient 63", "DC predictor leaves int16", "ends early", "width or height of 0")


class JpegRefusal(ValueError):
    def __init__(self, cause, detail=""):
        self.cause = cause
        super().__init__(cause + (": " + detail if detail else ""))


class Component:
    def __init__(self, ident, h, v, tq):
        self.ident, self.h, self.v, self.tq = ident, h, v, tq
        self.td = self.ta = 0
        self.blocks_w = self.blocks_h = self.offset = 0


class Info:
    """What ilcc_jpeg_info holds, plus the Huffman tables the scan uses."""

    def __init__(self):
        self.width = self.height = 0
        self.comps = []
        self.quant = np.zeros((4, 64), np.uint16)      # natural order
        self.have_quant = [False] * 4
        self.huff = {}                                   # (class, index) -> (counts[16], values)
        self.restart_interval = 0
        self.coef_count = 0
        self.scan_offset = 0                             # of the first entropy-coded byte
        self.adobe_transform = None

    @property
    def n_components(self):
        return len(self.comps)

    @property
    def sampling(self):
        return (self.comps[0].h, self.comps[0].v) if self.n_components == 3 else (1, 1)


def layout(info):
    """blocks_w / blocks_h (padded to whole MCUs), offsets and coef_count from the size and the sampling factors."""
    if info.n_components == 1:
        c = info.comps[0]
        c.h = c.v = 1                                    # a single-component scan is not interleaved
        c.blocks_w, c.blocks_h = -(-info.width // 8), -(-info.height // 8)
    else:
        hmax, vmax = info.sampling
        mw, mh = -(-info.width // (8 * hmax)), -(-info.height // (8 * vmax))
        for c in info.comps:
            c.blocks_w, c.blocks_h = mw * c.h, mh * c.v
    at = 0
    for c in info.comps:
        c.offset = at
        at += c.blocks_w * c.blocks_h * 64
    info.coef_count = at
    return info


def make_info(width, height, sampling=None, quant=None):
    """An Info without a file: sampling None = 1 component, else (h, v) of luma with 1 x 1 chroma; quant (n, 64)."""
    info = Info()
    info.width, info.height = width, height
    if sampling is None:
        info.comps = [Component(1, 1, 1, 0)]
    else:
        info.comps = [Component(1, sampling[0], sampling[1], 0), Component(2, 1, 1, 1), Component(3, 1, 1, 1)]
    if quant is not None:
        q = np.asarray(quant, np.uint16).reshape(-1, 64)
        info.quant[:len(q)] = q
    return layout(info)


_SOF_REFUSED = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "progressive", 0xC6: "progressive", 0xC7: "lossless",
                0xC9: "arithmetic", 0xCA: "arithmetic", 0xCB: "arithmetic", 0xCD: "arithmetic", 0xCE: "arithmetic",
                0xCF: "arithmetic", 0xCC: "arithmetic"}


def parse(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegRefusal("ends early" if n < 4 else "not a JPEG", "no SOI")
    info = Info()
    at = 2
    have_sof = False
    while True:
        if at >= n:
            raise JpegRefusal("ends early", "no scan")
        if data[at] != 0xFF:
            raise JpegRefusal("not a JPEG", "marker expected at byte %d" % at)
        while at < n and data[at] == 0xFF:
            at += 1
        if at >= n:
            raise JpegRefusal("ends early", "no scan")
        m = data[at]
        at += 1
        if m == 0x00:
            raise JpegRefusal("not a JPEG", "stuffed byte outside a scan")
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue                                      # TEM / a stray RSTn: no length
        if m == 0xD8:
            raise JpegRefusal("not a JPEG", "second SOI")
        if m == 0xD9:
            raise JpegRefusal("ends early", "EOI before any scan")
        if at + 2 > n:
            raise JpegRefusal("ends early", "segment length")
        length = (data[at] << 8) | data[at + 1]
        if length < 2 or at + length > n:
            raise JpegRefusal("ends early", "segment runs past the data")
        seg = data[at + 2:at + length]
        at += length
        if m in _SOF_REFUSED:
            raise JpegRefusal(_SOF_REFUSED[m])
        if m == 0xC8:
            raise JpegRefusal("not a JPEG", "reserved frame type")
        if m == 0xDC:
            raise JpegRefusal("DNL")
        if m in (0xC0, 0xC1):
            if have_sof:
                raise JpegRefusal("not a JPEG", "second frame header")
            if len(seg) < 6:
                raise JpegRefusal("ends early", "SOF")
            precision, info.height, info.width, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if precision == 12:
                raise JpegRefusal("12-bit")
            if precision != 8:
                raise JpegRefusal("not a JPEG", "sample precision %d" % precision)
            if info.width == 0 or info.height == 0:
                raise JpegRefusal("width or height of 0")
            if nc not in (1, 3):
                raise JpegRefusal("components", "%d" % nc)
            if len(seg) != 6 + 3 * nc:
                raise JpegRefusal("ends early", "SOF")
            for i in range(nc):
                ident, hv, tq = seg[6 + 3 * i:9 + 3 * i]
                if tq > 3:
                    raise JpegRefusal("not a JPEG", "quantisation table index")
                info.comps.append(Component(ident, hv >> 4, hv & 15, tq))
            for c in info.comps:
                if not (1 <= c.h <= 4 and 1 <= c.v <= 4):
                    raise JpegRefusal("sampling", "%dx%d" % (c.h, c.v))
            if nc == 3:
                s = [(c.h, c.v) for c in info.comps]
                if s[0] not in ((1, 1), (2, 1), (2, 2)) or s[1] != (1, 1) or s[2] != (1, 1):
                    raise JpegRefusal("sampling", str(s))
            have_sof = True
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq, tq = seg[p] >> 4, seg[p] & 15
                if pq == 1:
                    raise JpegRefusal("16-bit quantisation")
                if pq != 0 or tq > 3:
                    raise JpegRefusal("not a JPEG", "DQT")
                if p + 65 > len(seg):
                    raise JpegRefusal("ends early", "DQT")
                info.quant[tq, ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                info.have_quant[tq] = True
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                if tc > 1 or th > 3 or p + 17 > len(seg):
                    raise JpegRefusal("not a JPEG" if tc > 1 or th > 3 else "ends early", "DHT")
                counts = list(seg[p + 1:p + 17])
                total = sum(counts)
                if total > 256 or p + 17 + total > len(seg):
                    raise JpegRefusal("not a JPEG" if total > 256 else "ends early", "DHT")
                code = 0
                for ln in range(16):                      # the codes of each length must fit that length
                    code += counts[ln]
                    if code > (1 << (ln + 1)):
                        raise JpegRefusal("not a JPEG", "DHT over-subscribed")
                    code <<= 1
                info.huff[(tc, th)] = (counts, list(seg[p + 17:p + 17 + total]))
                p += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegRefusal("not a JPEG", "DRI")
            info.restart_interval = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                info.adobe_transform = seg[11]
        elif m == 0xDA:
            if not have_sof:
                raise JpegRefusal("not a JPEG", "scan before the frame header")
            if len(seg) < 1:
                raise JpegRefusal("ends early", "SOS")
            ns = seg[0]
            if ns != info.n_components:
                raise JpegRefusal("several scans", "a scan of %d of %d components" % (ns, info.n_components))
            if len(seg) != 4 + 2 * ns:
                raise JpegRefusal("ends early", "SOS")
            for i, c in enumerate(info.comps):
                if seg[1 + 2 * i] != c.ident:
                    raise JpegRefusal("not a JPEG", "scan components out of frame order")
                c.td, c.ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if c.td > 3 or c.ta > 3:
                    raise JpegRefusal("not a JPEG", "Huffman table index")
                if not info.have_quant[c.tq] or (0, c.td) not in info.huff or (1, c.ta) not in info.huff:
                    raise JpegRefusal("table used before it is defined")
            if info.n_components == 3 and info.adobe_transform == 0:
                raise JpegRefusal("Adobe transform 0")
            info.scan_offset = at
            return layout(info)
        # APPn, COM and anything else with a length: skipped


def _huff_lookup(counts, values):
    """16-bit prefix -> (length << 8) | symbol, 0 where no code matches."""
    look = [0] * 65536
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            lo = code << (16 - ln)
            look[lo:lo + (1 << (16 - ln))] = [(ln << 8) | values[k]] * (1 << (16 - ln))
            code += 1
            k += 1
        code <<= 1
    return look


def _split_scan(data, start):
    """The scan's entropy-coded segments, unstuffed: [(bytes, number of the RSTn that ends it, or None)], and the
    offset of the marker that ends the scan (len(data) when the data just stops).  As in libjpeg, any run of 0xFF
    bytes counts as one: followed by 0x00 it is the data byte 0xFF, followed by anything else it opens a marker."""
    out, pieces = [], []
    piece_start = at = start
    n = len(data)
    while True:
        f = data.find(b"\xff", at)
        g = f + 1
        while 0 <= f and g < n and data[g] == 0xFF:
            g += 1
        if f < 0 or g >= n:                              # no further marker: the data stops
            pieces.append(data[piece_start:n if f < 0 else f].replace(b"\xff\x00", b"\xff"))
            out.append((b"".join(pieces), None))
            return out, n
        if data[g] == 0x00:
            if g > f + 1:                                # 0xFF 0xFF ... 0x00: cut the extra 0xFF bytes out
                pieces.append(data[piece_start:f].replace(b"\xff\x00", b"\xff") + b"\xff")
                piece_start = g + 1
            at = g + 1
            continue
        pieces.append(data[piece_start:f].replace(b"\xff\x00", b"\xff"))
        if 0xD0 <= data[g] <= 0xD7:
            out.append((b"".join(pieces), data[g] - 0xD0))
            pieces = []
            piece_start = at = g + 1
        else:
            out.append((b"".join(pieces), None))
            return out, f


def entropy_decode(data, info):
    data = bytes(data)
    coef = np.zeros(info.coef_count, np.int16)
    dc_look = {c.td: _huff_lookup(*info.huff[(0, c.td)]) for c in info.comps}
    ac_look = {c.ta: _huff_lookup(*info.huff[(1, c.ta)]) for c in info.comps}
    segs, end = _split_scan(data, info.scan_offset)
    if info.n_components == 1:
        c = info.comps[0]
        mcus_w, mcus_h = c.blocks_w, c.blocks_h
        units = [(c, 0, 0)]
    else:
        hmax, vmax = info.sampling
        mcus_w, mcus_h = info.comps[0].blocks_w // hmax, info.comps[0].blocks_h // vmax
        units = [(c, dx, dy) for c in info.comps for dy in range(c.v) for dx in range(c.h)]
    total = mcus_w * mcus_h
    per_seg = info.restart_interval if info.restart_interval else total
    zz = ZIGZAG.tolist()
    out = coef                                            # written through a list per block for speed
    mcu = 0
    seg_i = 0
    while mcu < total:
        if seg_i >= len(segs):
            raise JpegRefusal("ends early", "restart marker missing")
        buf, rst = segs[seg_i]
        count = min(per_seg, total - mcu)
        if mcu + count < total and rst != seg_i % 8:
            raise JpegRefusal("ends early", "restart marker missing or out of order")
        pos, acc, nacc, nbuf = 0, 0, 0, len(buf)
        pred = {id(c): 0 for c in info.comps}
        for m in range(mcu, mcu + count):
            my, mx = divmod(m, mcus_w)
            for c, dx, dy in units:
                bx, by = mx * c.h + dx, my * c.v + dy
                block = [0] * 64
                # --- DC
                while nacc < 32 and pos < nbuf:
                    acc = (acc << 8) | buf[pos]
                    pos += 1
                    nacc += 8
                e = dc_look[c.td][((acc << 16) >> nacc) & 0xFFFF if nacc >= 16 else (acc << (16 - nacc)) & 0xFFFF]
                ln, t = e >> 8, e & 255
                if ln == 0:
                    raise JpegRefusal("ends early" if nacc < 16 and pos >= nbuf else "Huffman code in no table")
                if ln > nacc:
                    raise JpegRefusal("ends early")
                nacc -= ln
                acc &= (1 << nacc) - 1
                if t > 15:
                    raise JpegRefusal("DC predictor leaves int16", "category %d" % t)
                diff = 0
                if t:
                    if t > nacc:
                        raise JpegRefusal("ends early")
                    v = acc >> (nacc - t)
                    nacc -= t
                    acc &= (1 << nacc) - 1
                    diff = v if v >= (1 << (t - 1)) else v - (1 << t) + 1
                p = pred[id(c)] + diff
                if not -32768 <= p <= 32767:
                    raise JpegRefusal("DC predictor leaves int16")
                pred[id(c)] = p
                block[0] = p
                # --- AC
                look = ac_look[c.ta]
                k = 1
                while k < 64:
                    while nacc < 32 and pos < nbuf:
                        acc = (acc << 8) | buf[pos]
                        pos += 1
                        nacc += 8
                    e = look[((acc << 16) >> nacc) & 0xFFFF if nacc >= 16 else (acc << (16 - nacc)) & 0xFFFF]
                    ln, rs = e >> 8, e & 255
                    if ln == 0:
                        raise JpegRefusal("ends early" if nacc < 16 and pos >= nbuf else "Huffman code in no table")
                    if ln > nacc:
                        raise JpegRefusal("ends early")
                    nacc -= ln
                    acc &= (1 << nacc) - 1
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break                         # EOB
                        if k + 16 > 64:
                            raise JpegRefusal("run past coefficient 63")
                        k += 16
                        continue
                    k += r
                    if k > 63:
                        raise JpegRefusal("run past coefficient 63")
                    if s > nacc:
                        raise JpegRefusal("ends early")
                    v = acc >> (nacc - s)
                    nacc -= s
                    acc &= (1 << nacc) - 1
                    block[zz[k]] = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
                    k += 1
                at = c.offset + (by * c.blocks_w + bx) * 64
                out[at:at + 64] = block
        mcu += count
        seg_i += 1
    # what follows the scan: another scan or a DNL is refused, anything else (EOI, nothing) ends the image
    at = end
    n = len(data)
    while at < n and data[at] == 0xFF:
        at += 1
    if 0 < at < n and data[at - 1] == 0xFF:
        if data[at] == 0xDA:
            raise JpegRefusal("several scans")
        if data[at] == 0xDC:
            raise JpegRefusal("DNL")
    return coef


# ---------------------------------------------------------------- coefficients -> pixels

class DomainError(ArithmeticError):
    """An intermediate of the IDCT left int32: outside the domain where libjpeg's C and SIMD code agree."""


def _check32(*arrays):
    for a in arrays:
        if a.size and (int(a.max()) > 2 ** 31 - 1 or int(a.min()) < -2 ** 31):
            raise DomainError("IDCT intermediate outside int32")


def _pass(c, shift):
    """One 8-point pass along the last axis of an int64 array; DESCALE by `shift`."""
    c0, c1, c2, c3, c4, c5, c6, c7 = [c[..., i] for i in range(8)]
    z1 = (c2 + c6) * 4433
    t2 = z1 - c6 * 15137
    t3 = z1 + c2 * 6270
    t0 = (c0 + c4) << 13
    t1 = (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = c7, c5, c3, c1
    z1b, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    p0, p1, p2, p3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    m1, m2 = z1b * -7373, z2 * -20995
    m3, m4 = z3 * -16069, z4 * -3196
    _check32(z1, t2, t3, t0, t1, t10, t13, t11, t12, z5, p0, p1, p2, p3, m1, m2, m3, m4)
    m3, m4 = m3 + z5, m4 + z5
    s13, s24, s23, s14 = m1 + m3, m2 + m4, m2 + m3, m1 + m4
    _check32(m3, m4, s13, s24, s23, s14)
    o0, o1, o2, o3 = p0 + s13, p1 + s24, p2 + s23, p3 + s14
    _check32(o0, o1, o2, o3)
    outs = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    half = 1 << (shift - 1)
    outs = [o + half for o in outs]
    _check32(*outs)
    return np.stack([o >> shift for o in outs], axis=-1)


def idct_blocks(coef, quant):
    """coef (n, 64) int16, quant (64,) -> (n, 8, 8) uint8 samples."""
    x = coef.reshape(-1, 8, 8).astype(np.int64) * quant.reshape(8, 8).astype(np.int64)
    _check32(x)
    ws = _pass(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # pass 1 over columns
    out = _pass(ws, 18) + 128                                    # pass 2 over rows
    return np.clip(out, 0, 255).astype(np.uint8)


def planes(info, coef):
    """The padded sample plane of every component: (blocks_h * 8, blocks_w * 8) uint8."""
    out = []
    for c in info.comps:
        n = c.blocks_w * c.blocks_h
        s = idct_blocks(coef[c.offset:c.offset + n * 64].reshape(n, 64), info.quant[c.tq])
        out.append(s.reshape(c.blocks_h, c.blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(c.blocks_h * 8, c.blocks_w * 8))
    return out


def upsample(s, hs, vs):
    """A chroma plane cropped to its real size -> (hc * vs, wc * hs) int32, libjpeg's choice of upsampler."""
    s = s.astype(np.int32)
    hc, wc = s.shape
    if hs == 1 and vs == 1:
        return s
    if wc <= 2:                                              # libjpeg takes the "fancy" path only for wc > 2
        return np.repeat(np.repeat(s, vs, axis=0), hs, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((hc, 2 * wc), np.int32)
        out[:, 0::2] = (3 * s + left + 1) >> 2
        out[:, 1::2] = (3 * s + right + 2) >> 2
        return out
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    r = np.empty((2 * hc, wc), np.int32)
    r[0::2] = 3 * s + up
    r[1::2] = 3 * s + down
    rl = np.concatenate([r[:, :1], r[:, :-1]], axis=1)
    rr = np.concatenate([r[:, 1:], r[:, -1:]], axis=1)
    out = np.empty((2 * hc, 2 * wc), np.int32)
    out[:, 0::2] = (3 * r + rl + 8) >> 4
    out[:, 1::2] = (3 * r + rr + 7) >> 4
    return out


def pixels(info, coef):
    p = planes(info, coef)
    w, h = info.width, info.height
    if info.n_components == 1:
        return p[0][:h, :w].copy()
    hs, vs = info.sampling
    wc, hc = -(-w // hs), -(-h // vs)
    y = p[0][:h, :w].astype(np.int32)
    cb = upsample(p[1][:hc, :wc], hs, vs)[:h, :w] - 128
    cr = upsample(p[2][:hc, :wc], hs, vs)[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    info = parse(data)
    return pixels(info, entropy_decode(data, info))


# ---------------------------------------------------------------- sensor_msgs/CompressedImage

COMPRESSED_IMAGE_DEFINITION = ("Header header\nstring format\nuint8[] data\n"
                               "================================================================================\n"
                               "MSG: std_msgs/Header\nuint32 seq\ntime stamp\nstring frame_id\n")


def compressed_image_msg(jpg, fmt="jpeg", seq=0, stamp=(0, 0), frame_id="camera"):
    """A serialized sensor_msgs/CompressedImage (what BagWriter.add_connection(..., COMPRESSED_IMAGE_MD5) carries)."""
    fid, f = frame_id.encode(), fmt.encode()
    return (struct.pack("<IIII", seq, stamp[0], stamp[1], len(fid)) + fid + struct.pack("<I", len(f)) + f +
            struct.pack("<I", len(jpg)) + bytes(jpg))
