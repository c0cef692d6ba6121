"""numpy restatement of K17 (include/ilcc_jpeg_write_sequence.h), step by step as the kernels do it: every block's codes and bit
count from its own coefficients and the previous DC of its component, the prefix of the counts inside each restart segment, the
segments' byte offsets (a hole of two bytes behind each but the last), the codes ORed into a zeroed unstuffed buffer at their bit
offsets, the 0xFF bytes counted per chunk of 4096, every byte scattered to its index plus the 0xFF bytes before it, the RSTn
markers into the holes, and the images placed in the batch's output under the capacity rule.  It is the specification; it shares
the Annex-K tables and the Info with tests/jpeg_write_ref.py and nothing else: W.entropy_encode is the sequential encoder it is
checked against.

    scan, status = encode_image(info, coef)                     the bytes between the SOS header and EOI; b"" when status != 0
    scans, rows = encode_batch(info, coefs, out_cap)            rows: (offset, bytes, status) per image
"""
import numpy as np

import jpeg_ref as R
import jpeg_write_ref as W

DC_RANGE, AC_RANGE, CAPACITY = 0x01, 0x02, 0x04
CHUNK = 4096
TILE = 256


def scan_order(info):
    """[(component index, offset of the block's coefficients)] in the order the scan holds the blocks, and the blocks an MCU"""
    c0 = info.comps[0]
    if info.n_components == 1:
        return [(0, c0.offset + k * 64) for k in range(c0.blocks_w * c0.blocks_h)], 1
    mcus_w, mcus_h = c0.blocks_w // c0.h, c0.blocks_h // c0.v
    out = [(i, c.offset + ((my * c.v + dy) * c.blocks_w + mx * c.h + dx) * 64)
           for my in range(mcus_h) for mx in range(mcus_w) for i, c in enumerate(info.comps) for dy in range(c.v) for dx in range(c.h)]
    return out, sum(c.h * c.v for c in info.comps)


def segment_blocks(info, n_blocks, mcu_blocks):
    """blocks of every segment but the last, and the number of segments"""
    mcus = n_blocks // mcu_blocks
    interval = info.restart_interval if 0 < info.restart_interval < mcus else mcus
    return interval * mcu_blocks, -(-mcus // interval)


def block_codes(block, pred, dc, ac):
    """One block -> ([(bits, length)], refusal flags).  A refused value is clamped to its limit, as the kernel clamps it."""
    flags = 0
    out = []
    diff = int(block[0]) - pred
    n = abs(diff).bit_length()
    if n > 11:
        flags |= DC_RANGE
        n = 11
    code, length = dc[n]
    out.append(((code << n) | ((diff if diff >= 0 else diff - 1) & ((1 << n) - 1)), length + n))
    run = 0
    for k in range(1, 64):
        v = int(block[R.ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac[0xF0])
            run -= 16
        n = abs(v).bit_length()
        if n > 10:
            flags |= AC_RANGE
            n = 10
        code, length = ac[(run << 4) | n]
        out.append(((code << n) | ((v if v >= 0 else v - 1) & ((1 << n) - 1)), length + n))
        run = 0
    if run:
        out.append(ac[0])
    return out, flags


def count(info, coef):
    """step 1: per block in scan order its codes, its bit count and its flags"""
    order, mcu_blocks = scan_order(info)
    per_segment, _ = segment_blocks(info, len(order), mcu_blocks)
    dc = {c.td: W._codes(*W.STD_HUFF[(0, c.td)]) for c in info.comps}
    ac = {c.ta: W._codes(*W.STD_HUFF[(1, c.ta)]) for c in info.comps}
    coef = np.asarray(coef).astype(np.int64)
    codes, bits, flags = [], np.zeros(len(order), np.int64), 0
    last = {}                                                   # component -> scan index of its previous block
    for s, (i, at) in enumerate(order):
        c = info.comps[i]
        before = last.get(i)
        pred = 0 if before is None or before // per_segment != s // per_segment else int(coef[order[before][1]])
        last[i] = s
        got, f = block_codes(coef[at:at + 64], pred, dc[c.td], ac[c.ta])
        codes.append(got)
        bits[s] = sum(length for _, length in got)
        flags |= f
    return codes, bits, flags


def layout(info, bits):
    """step 2: the exclusive prefix of the bit counts by tiles of 256 blocks, each segment's bytes = ceil(bits / 8) + 2 for its marker
    (none behind the last), their exclusive prefix -> (bit offset of every block inside its segment, byte offset of every segment,
    unstuffed bytes of the image)"""
    n = len(bits)
    _, mcu_blocks = scan_order(info)
    per_segment, n_segments = segment_blocks(info, n, mcu_blocks)
    tiles = [bits[t:t + TILE] for t in range(0, n, TILE)]
    tile_base = np.concatenate([[0], np.cumsum([t.sum() for t in tiles])])
    before = np.concatenate([tile_base[k] + np.cumsum(t) - t for k, t in enumerate(tiles)] + [tile_base[-1:]])   # [n] is the sum
    seg_bytes = []
    for k in range(n_segments):
        first, end = k * per_segment, min((k + 1) * per_segment, n)
        seg_bytes.append(-(-int(before[end] - before[first]) // 8) + (2 if k + 1 < n_segments else 0))
    seg_at = np.concatenate([[0], np.cumsum(seg_bytes)]).astype(np.int64)
    in_segment = np.array([before[s] - before[(s // per_segment) * per_segment] for s in range(n)], np.int64)
    return in_segment, seg_at, int(seg_at[-1])


def pack(info, codes, bits, in_segment, seg_at, size):
    """step 3: every block ORs its codes into the zeroed buffer at 8 * (its segment's byte offset) + (its bit offset there); a
    segment's last block appends the 1-bits up to the byte boundary.  The order of the blocks does not matter: it is reversed here."""
    n = len(codes)
    _, mcu_blocks = scan_order(info)
    per_segment, _ = segment_blocks(info, n, mcu_blocks)
    u = np.zeros(size, np.uint8)
    for s in reversed(range(n)):
        k = s // per_segment
        start = 8 * int(seg_at[k]) + int(in_segment[s])
        value, length = 0, 0
        for b, ln in codes[s]:
            value, length = (value << ln) | b, length + ln
        assert length == bits[s]
        if s + 1 == min((k + 1) * per_segment, n):
            pad = -(start + length) % 8
            value, length = (value << pad) | ((1 << pad) - 1), length + pad
        first, lead = start // 8, start % 8
        nbytes = (lead + length + 7) // 8
        value <<= nbytes * 8 - lead - length
        u[first:first + nbytes] |= np.frombuffer(value.to_bytes(nbytes, "big"), np.uint8)
    return u


def stuff(u, seg_at):
    """step 4: the 0xFF bytes per chunk of 4096, their prefix, and every byte to index + (0xFF bytes before it) with a 0x00 behind
    each 0xFF; the two bytes of every hole become FF, D0 + (segment & 7)"""
    ff = (u == 255).astype(np.int64)
    chunk_sums = [int(ff[c:c + CHUNK].sum()) for c in range(0, len(u), CHUNK)]
    chunk_base = np.concatenate([[0], np.cumsum(chunk_sums)]).astype(np.int64)
    before = np.concatenate([chunk_base[k] + np.cumsum(ff[c:c + CHUNK]) - ff[c:c + CHUNK] for k, c in enumerate(range(0, len(u), CHUNK))]) if len(u) else ff
    out = np.zeros(len(u) + int(ff.sum()), np.uint8)
    at = np.arange(len(u)) + before
    out[at] = u
    for k in range(len(seg_at) - 2):                            # every segment but the last
        hole = int(seg_at[k + 1]) - 2
        assert u[hole] == 0 and u[hole + 1] == 0
        out[at[hole]] = 0xFF
        out[at[hole + 1]] = 0xD0 + (k & 7)
    return out.tobytes()


def encode_image(info, coef):
    codes, bits, flags = count(info, coef)
    if flags:
        return b"", flags
    in_segment, seg_at, size = layout(info, bits)
    return stuff(pack(info, codes, bits, in_segment, seg_at, size), seg_at), 0


def place(sizes, statuses, out_cap):
    """the batch: images in order at offsets that are multiples of 16; a refused image takes nothing; once an image's end lies
    past out_cap, it and every image behind it get CAPACITY and nothing -> [(offset, bytes, status)]"""
    rows, at, full = [], 0, False
    for size, status in zip(sizes, statuses):
        size = 0 if status else size
        full = full or at + size > out_cap
        rows.append((at, 0 if full or status else size, status | (CAPACITY if full else 0)))
        at += -(-size // 16) * 16
    return rows


def encode_batch(info, coefs, out_cap):
    got = [encode_image(info, c) for c in coefs]
    rows = place([len(s) for s, _ in got], [f for _, f in got], out_cap)
    return [s if row[2] == 0 else b"" for (s, _), row in zip(got, rows)], rows
