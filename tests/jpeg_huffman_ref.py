"""Plain-Python restatement of K16 (include/ilcc_jpeg_huffman.h): the host's preparation of a scan on jpeg_ref._split_scan, and the
staged decoder -- subsequences of S bits, chunks of `chunk` subsequences, a cold pass, rounds until no exit state changes, the
count, the write pass from exact states and the DC sums -- for any S and any chunk size.  Written from the header's text; slow, for
the small fixtures.

    scan, rows, tables = prepare(data, info)            raises jpeg_ref.JpegRefusal(cause)
    coef, status, rounds = decode(info, scan, rows, tables, S, chunk)
                                                         rounds: [(segment, subsequences in the chunk, rounds taken)]
"""
import struct

import numpy as np

import jpeg_ref as R

NO_CODE, RUN_PAST_63, DC_CATEGORY, DC_RANGE, ENDS_EARLY, BAD_ROWS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
LOOK_BITS = 9


class Table:
    """One Huffman table as the kernel reads it: look[512], maxcode[17], first[17], values[256]"""

    def __init__(self, counts, values):
        self.look, self.maxcode, self.first, self.values = [0] * 512, [0] * 17, [0] * 17, list(values) + [0] * (256 - len(values))
        code = k = 0
        for ln in range(1, 17):
            self.first[ln] = k - code
            for _ in range(counts[ln - 1]):
                if ln <= LOOK_BITS:
                    lo = code << (LOOK_BITS - ln)
                    self.look[lo:lo + (1 << (LOOK_BITS - ln))] = [(ln << 8) | values[k]] * (1 << (LOOK_BITS - ln))
                code += 1
                k += 1
            self.maxcode[ln] = code - 1 if counts[ln - 1] else -1
            code <<= 1

    def packed(self):
        return struct.pack("<512H17i17i256B", *(self.look + self.maxcode + self.first + self.values))

    def symbol(self, code16):
        """-> (length, symbol) of the code at the head of 16 bits; length 0: in no table"""
        e = self.look[code16 >> 7]
        if e:
            return e >> 8, e & 255
        for ln in range(LOOK_BITS + 1, 17):
            code = code16 >> (16 - ln)
            if code <= self.maxcode[ln]:
                return ln, self.values[self.first[ln] + code]
        return 0, 0


def geometry(info):
    """(MCUs in a row, MCUs, [(component index, dx, dy)] of the MCU's blocks in scan order)"""
    if info.n_components == 1:
        c = info.comps[0]
        return c.blocks_w, c.blocks_w * c.blocks_h, [(0, 0, 0)]
    hmax, vmax = info.sampling
    mcus_w, mcus_h = info.comps[0].blocks_w // hmax, info.comps[0].blocks_h // vmax
    return mcus_w, mcus_w * mcus_h, [(i, dx, dy) for i, c in enumerate(info.comps) for dy in range(c.v) for dx in range(c.h)]


def prepare(data, info):
    """-> (the unstuffed scan, [(byte offset, byte count, first MCU, MCU count)], [(dc Table, ac Table)] by component)"""
    data = bytes(data)
    segs, end = R._split_scan(data, info.scan_offset)
    _, total, _ = geometry(info)
    interval = info.restart_interval or total
    n_rows = -(-total // interval)
    rows, scan = [], b""
    for k in range(n_rows):
        if k >= len(segs) or (k + 1 < n_rows and segs[k][1] != k % 8):
            raise R.JpegRefusal("ends early", "restart marker missing or out of order")
        rows.append((len(scan), len(segs[k][0]), k * interval, min(interval, total - k * interval)))
        scan += segs[k][0]
    at, n = end, len(data)
    while at < n and data[at] == 0xFF:
        at += 1
    if 0 < at < n and data[at - 1] == 0xFF:
        if data[at] == 0xDA:
            raise R.JpegRefusal("several scans")
        if data[at] == 0xDC:
            raise R.JpegRefusal("DNL")
    tables = [(Table(*info.huff[(0, c.td)]), Table(*info.huff[(1, c.ta)])) for c in info.comps]
    return scan, rows, tables


def packed_tables(tables):
    """the bytes of an ilcc_jpeg_huffman_tables"""
    zero = bytes(1416)
    dc = [t[0].packed() for t in tables] + [zero] * (3 - len(tables))
    ac = [t[1].packed() for t in tables] + [zero] * (3 - len(tables))
    return b"".join(dc + ac)


class _Segment:
    def __init__(self, buf, blocks, first_mcu):
        self.n_bits = 8 * len(buf)
        self.word = int.from_bytes(buf + bytes(5), "big")
        self.blocks, self.first_mcu = blocks, first_mcu

    def peek32(self, pos):
        return (self.word >> (self.n_bits + 40 - 32 - pos)) & 0xFFFFFFFF


def _span(seg, tables, units, state, end, write=None):
    """Decodes from state (pos, unit, k) to the first symbol boundary at or behind `end` -> (state, blocks completed, fault).
    write None: a guess or a count, nothing is an error.  write (first block, store): from an exact state; store(block, k, value);
    stops at the segment's block count and at the first refusal."""
    pos, unit, k = state
    done = fault = 0
    block = write[0] if write else 0
    while pos < end:
        if write and block >= seg.blocks:
            break
        window = seg.peek32(pos)
        left = seg.n_bits - pos
        ln, sym = tables[units[unit][0]][0 if k == 0 else 1].symbol(window >> 16)
        if ln == 0:
            if write:
                fault |= ENDS_EARLY if left < 16 else NO_CODE
                break
            pos += 1                                         # the rule for a guess: skip one bit
            continue
        if ln > left:
            fault |= ENDS_EARLY
            pos = seg.n_bits
            break
        close, at, nxt = False, k, k + 1
        if k == 0:
            size = sym
            if size > 15:
                if write:
                    fault |= DC_CATEGORY
                    break
                size = 0                                     # a guess: a difference of 0 without extra bits
        else:
            run, size = sym >> 4, sym & 15
            if size == 0:
                if run != 15:
                    close = True
                elif k + 16 > 64:
                    if write:
                        fault |= RUN_PAST_63
                        break
                    close = True                             # a guess: the block is closed
                else:
                    nxt = k + 16
            elif k + run > 63:
                if write:
                    fault |= RUN_PAST_63
                    break
                size, close = 0, True
            else:
                at = k + run
                nxt = at + 1
        if ln + size > left:
            fault |= ENDS_EARLY
            pos = seg.n_bits
            break
        pos += ln + size
        if write and size:
            raw = (window << ln & 0xFFFFFFFF) >> (32 - size)
            write[1](block, at, raw if raw >= (1 << (size - 1)) else raw - (1 << size) + 1)
        k = nxt
        if k >= 64:
            close = True
        if close:
            k = 0
            unit = (unit + 1) % len(units)
            done += 1
            block += 1
    return (pos, unit, k), done, (fault if write else 0)


def decode(info, scan, rows, tables, S=1024, chunk=256):
    """-> (coefficients int16[coef_count], status bits, [(segment, subsequences of the chunk, rounds)])"""
    mcus_w, mcus, units = geometry(info)
    coef = np.zeros(info.coef_count, np.int64)
    zz = R.ZIGZAG.tolist()
    status, rounds_of = 0, []

    def place(mcu, c, dx, dy):
        comp = info.comps[c]
        my, mx = divmod(mcu, mcus_w)
        return comp.offset + ((my * comp.v + dy) * comp.blocks_w + mx * comp.h + dx) * 64

    for si, (offset, count, first_mcu, mcu_count) in enumerate(rows):
        if offset + count > len(scan) or first_mcu + mcu_count > mcus:
            status |= BAD_ROWS
            continue
        seg = _Segment(bytes(scan[offset:offset + count]), mcu_count * len(units), first_mcu)

        def store(block, k, value):
            c, dx, dy = units[block % len(units)]
            coef[place(seg.first_mcu + block // len(units), c, dx, dy) + zz[k]] = value

        n_sub = -(-seg.n_bits // S)
        entry, first_block = (0, 0, 0), 0
        for base in range(0, n_sub, chunk):
            if first_block >= seg.blocks:
                break
            n = min(chunk, n_sub - base)
            ends = [min((base + i + 1) * S, seg.n_bits) for i in range(n)]
            start = [entry if i == 0 else ((base + i) * S, 0, 0) for i in range(n)]
            res = [_span(seg, tables, units, start[i], ends[i]) for i in range(n)]
            rounds = 0
            for _ in range(1, n):                            # at most n - 1 rounds: subsequence i is exact after round i
                left = [start[0]] + [res[i - 1][0] for i in range(1, n)]
                changed = False
                for i in range(1, n):
                    if left[i] != start[i]:
                        start[i] = left[i]
                        now = _span(seg, tables, units, start[i], ends[i])
                        changed |= now[0] != res[i][0]
                        res[i] = now
                rounds += 1
                if not changed:
                    break
            rounds_of.append((si, n, rounds))
            for i in range(n):
                status |= _span(seg, tables, units, start[i], ends[i], (first_block, store))[2]
                first_block += res[i][1]
            entry = res[n - 1][0]
        if first_block < seg.blocks:
            status |= ENDS_EARLY
        for c, comp in enumerate(info.comps):                # DC differences -> values, per component in scan order
            pred = 0
            per = comp.h * comp.v
            for j in range(mcu_count * per):
                at = place(first_mcu + j // per, c, j % per % comp.h, j % per // comp.h)
                pred += int(coef[at])
                if not -32768 <= pred <= 32767:
                    status |= DC_RANGE
                    break
                coef[at] = pred
    return coef.astype(np.int16), status, rounds_of


def decode_file(data, S=1024, chunk=256):
    info = R.parse(data)
    return (info,) + decode(info, *prepare(data, info), S=S, chunk=chunk)
