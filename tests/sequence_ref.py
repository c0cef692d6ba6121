"""numpy restatement of include/ilcc_sequence.h -- the specification the library is tested against:
the order of a topic's messages, the PointCloud2 unpack (K0 / K0b), and the fusion of per-scan corners."""
import struct

import numpy as np

FLOAT32 = 7
OK, BAD_ARGUMENT, BOARD_NOT_FOUND, AMBIGUOUS = 0, 6, 10, 11


# ---- 1. message order ------------------------------------------------------------------------------------------------------
def message_order(chunks, conns_wanted):
    """chunks: as BagWriter.chunks -- per chunk, in file order, the list of (conn, (sec, nsec), payload) in the order written.
    -> [((sec, nsec), payload)] of the wanted connections: by record time, ties by chunk position, then by position in the chunk."""
    keyed = []
    for c, msgs in enumerate(chunks):
        for k, (conn, tm, payload) in enumerate(msgs):
            if conn in conns_wanted:
                keyed.append(((tm[0], tm[1], c, k), tm, payload))
    keyed.sort(key=lambda e: e[0])
    return [(tm, payload) for _, tm, payload in keyed]


# ---- 2. unpack ---------------------------------------------------------------------------------------------------------------
def parse_pointcloud2(msg: bytes) -> dict:
    at = 0

    def u32():
        nonlocal at
        v = struct.unpack_from("<I", msg, at)[0]
        at += 4
        return v

    def u8():
        nonlocal at
        v = msg[at]
        at += 1
        return v

    def string():
        nonlocal at
        n = u32()
        s = msg[at:at + n]
        at += n
        return s.decode()

    out = {"seq": u32(), "stamp": (u32(), u32()), "frame_id": string(), "height": u32(), "width": u32()}
    off = {}
    for _ in range(u32()):
        name, offset, datatype, count = string(), u32(), u8(), u32()
        if datatype == FLOAT32 and count == 1 and name in ("x", "y", "z", "intensity"):
            off[name] = offset          # a later field of the same name wins, as in the library
    out["off"] = [off.get(k) for k in ("x", "y", "z", "intensity")]
    out["is_bigendian"], out["point_step"], out["row_step"] = u8(), u32(), u32()
    n = u32()
    out["data"] = msg[at:at + n]
    return out


def unpack(msg: bytes) -> np.ndarray:
    """-> [height * width, 4] float32 {x, y, z, intensity}; unmatched members 0; bit patterns copied (NaN payloads included)."""
    m = parse_pointcloud2(msg)
    h, w, ps, rs = m["height"], m["width"], m["point_step"], m["row_step"]
    raw = np.frombuffer(m["data"], np.uint8)
    out = np.zeros((h * w, 4), np.uint32)
    if h * w:
        base = (np.arange(h, dtype=np.int64)[:, None] * rs + np.arange(w, dtype=np.int64)[None, :] * ps).reshape(-1)
        for k, o in enumerate(m["off"]):
            if o is None:
                continue
            b = [raw[base + o + i].astype(np.uint32) for i in range(4)]
            out[:, k] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)
    return out.view(np.float32)


# ---- 3. fusion ---------------------------------------------------------------------------------------------------------------
class Fused:
    def __init__(self):
        self.status = OK
        self.n_scans = self.n_ok = self.n_used = self.n_corners = 0
        self.ref_scan = -1
        self.spread_rms = self.spread_max = 0.0
        self.corners = np.zeros((0, 3), np.float32)
        self.used = None
        self.dist = None
        self.variants = None


def variant_perm(a, b, v):
    """perm[c] = index, in a scan numbered by variant v, of corner c of the reference numbering"""
    i, j = np.divmod(np.arange(a * b), b)
    if v & 1:
        i = a - 1 - i
    if v & 2:
        j = b - 1 - j
    return i * b + j


def _seq_sum(values):
    s = np.float64(0.0)
    for v in values:
        s = s + v
    return s


def _median(rows):
    """per column over the rows of a 2-D fp64 array; even count: (lo + hi) / 2"""
    s = np.sort(rows, axis=0)
    n = len(s)
    return s[n // 2].copy() if n & 1 else (s[n // 2 - 1] + s[n // 2]) / 2


def _max_d2(x, m):
    """x, m: [C, 3] fp64 -> (largest ((dx dx + dy dy) + dz dz), all of them)"""
    d = x - m
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d2.max(), d2


def fuse(corners, accepted, a, b, gate) -> Fused:
    corners = np.asarray(corners, np.float32).reshape(-1, a * b, 3)
    accepted = np.asarray(accepted) != 0
    n, C = len(accepted), a * b
    out = Fused()
    out.n_scans = n
    out.used = np.zeros(n, bool)
    out.dist = np.full(n, -1.0)
    out.variants = np.full(n, -1)
    if not (gate > 0) or not np.isfinite(gate) or a < 1 or b < 1 or C > 256:
        out.status = BAD_ARGUMENT
        return out
    S = [i for i in range(n) if accepted[i]]
    out.n_ok = len(S)
    if not S:
        out.status = BOARD_NOT_FOUND
        return out
    if not np.isfinite(corners[S]).all():
        out.status = BAD_ARGUMENT
        return out
    out.ref_scan = S[0]
    ref = corners[S[0]].astype(np.float64)
    aligned = np.zeros((len(S), C, 3))
    for r, s in enumerate(S):
        scan = corners[s].astype(np.float64)
        best, best_cost = 0, None
        for v in range(4):
            d = (scan[variant_perm(a, b, v)] - ref).reshape(-1)      # corners in index order, then x, y, z
            cost = _seq_sum(d * d)
            if best_cost is None or cost < best_cost:
                best, best_cost = v, cost
        out.variants[s] = best
        aligned[r] = scan[variant_perm(a, b, best)]
    m0 = _median(aligned.reshape(len(S), -1)).reshape(C, 3)
    gate2 = np.float64(gate) * np.float64(gate)
    d2 = np.array([_max_d2(aligned[r], m0)[0] for r in range(len(S))])
    used_rows = [r for r in range(len(S)) if d2[r] <= gate2]
    out.n_used = len(used_rows)
    for r in used_rows:
        out.used[S[r]] = True
    if not used_rows or 2 * len(used_rows) <= len(S):
        out.status = AMBIGUOUS
        out.dist[S] = np.sqrt(d2)
        return out
    m1 = _median(aligned[used_rows].reshape(len(used_rows), -1)).reshape(C, 3).astype(np.float32)
    out.corners = m1
    out.n_corners = C
    m1d = m1.astype(np.float64)
    worst, total = 0.0, np.float64(0.0)
    for r in used_rows:
        w, all_d2 = _max_d2(aligned[r], m1d)
        worst = max(worst, w)
        total = total + _seq_sum(all_d2)
    out.spread_max = float(np.sqrt(worst))
    out.spread_rms = float(np.sqrt(total / (np.float64(len(used_rows)) * np.float64(C))))
    for r, s in enumerate(S):
        out.dist[s] = np.sqrt(_max_d2(aligned[r], m1d)[0])
    return out
