"""numpy restatement of include/ilcc_image_sequence.h -- the specification the library is tested against: the fusion of
per-image boards, the selection of a topic's images and their cut into batches, and the order of K10b's candidate list."""
import numpy as np

OK, BAD_ARGUMENT, CAPACITY, BOARD_NOT_FOUND, AMBIGUOUS = 0, 6, 7, 10, 11
MAX_CORNERS = 256
DEFAULT_STAGING_BYTES, DEFAULT_DEVICE_BYTES = 256 << 20, 512 << 20
NMS_N, NMS_MARGIN = 3, 5


# ---- 1. fusion -----------------------------------------------------------------------------------------------------------------
class Fused:
    def __init__(self):
        self.status = OK
        self.n_images = self.n_ok = self.n_used = 0
        self.ref_image = -1
        self.rows = self.cols = 0
        self.gate = 0.0
        self.spread_rms = self.spread_max = 0.0
        self.xy = np.zeros((0, 0, 2))
        self.used = None
        self.dist = None
        self.variants = None


def variant_perm(R, C, v):
    """perm[c] = flat index, in an image numbered by variant v, of entry c = i C + j of the R x C reference numbering.
    Variants 0-3: the image is R x C, read at (i2, j2); 4-7: it is C x R, read at (j2, i2)."""
    i, j = np.divmod(np.arange(R * C), C)
    if v & 1:
        i = R - 1 - i
    if v & 2:
        j = C - 1 - j
    return j * R + i if v & 4 else i * C + j


def _seq_sum(values):
    s = np.float64(0.0)
    for v in values:
        s = s + v
    return s


def _median(rows):
    s = np.sort(rows, axis=0)
    n = len(s)
    return s[n // 2].copy() if n & 1 else (s[n // 2 - 1] + s[n // 2]) / 2


def _d2(x, m):
    """x, m: [N, 2] fp64 -> every corner's du du + dv dv"""
    d = x - m
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def default_gate(m0, R, C):
    """half the least distance between lattice neighbours of the R x C board m0 ([R C, 2])"""
    b = m0.reshape(R, C, 2)
    least = None
    for i in range(R):
        for j in range(C):
            for i2, j2 in ((i + 1, j), (i, j + 1)):
                if i2 >= R or j2 >= C:
                    continue
                du, dv = b[i2, j2, 0] - b[i, j, 0], b[i2, j2, 1] - b[i, j, 1]
                d = np.sqrt(du * du + dv * dv)
                if least is None or d < least:
                    least = d
    return least / 2


def fuse(boards, accepted, a, b, gate_px=0.0) -> Fused:
    """boards: per image a (rows, cols, 2) array (anything for a non-accepted image: it is never read)."""
    accepted = np.asarray(accepted) != 0
    n = len(accepted)
    out = Fused()
    out.n_images = n
    out.used = np.zeros(n, bool)
    out.dist = np.full(n, -1.0)
    out.variants = np.full(n, -1)
    if a < 3 or b < 3 or a * b > MAX_CORNERS or not np.isfinite(gate_px):
        out.status = BAD_ARGUMENT
        return out
    S = [i for i in range(n) if accepted[i]]
    out.n_ok = len(S)
    if not S:
        out.status = BOARD_NOT_FOUND
        return out
    N = a * b
    for s in S:
        bd = np.asarray(boards[s], np.float64)
        if bd.ndim != 3 or bd.shape[2] != 2 or bd.shape[:2] not in ((a, b), (b, a)) or not np.isfinite(bd).all():
            out.status = BAD_ARGUMENT
            return out
    out.ref_image = S[0]
    ref_board = np.asarray(boards[S[0]], np.float64)
    R, C = ref_board.shape[:2]
    out.rows, out.cols = R, C
    ref = ref_board.reshape(N, 2)
    aligned = np.zeros((len(S), N, 2))
    for r, s in enumerate(S):
        bd = np.asarray(boards[s], np.float64)
        flat = bd.reshape(N, 2)
        best, best_cost = None, None
        for v in range(8):
            if bd.shape[:2] != ((R, C) if v < 4 else (C, R)):
                continue
            d = (flat[variant_perm(R, C, v)] - ref).reshape(-1)      # entries in the reference's index order, then u, v
            cost = _seq_sum(d * d)
            if best is None or cost < best_cost:
                best, best_cost = v, cost
        out.variants[s] = best
        aligned[r] = flat[variant_perm(R, C, best)]
    m0 = _median(aligned.reshape(len(S), -1)).reshape(N, 2)
    gate = np.float64(gate_px) if gate_px > 0 else default_gate(m0, R, C)
    out.gate = float(gate)
    gate2 = gate * gate
    d2 = np.array([_d2(aligned[r], m0).max() for r in range(len(S))])
    used_rows = [r for r in range(len(S)) if d2[r] <= gate2]
    out.n_used = len(used_rows)
    for r in used_rows:
        out.used[S[r]] = True
    if not used_rows or 2 * len(used_rows) <= len(S):
        out.status = AMBIGUOUS
        out.dist[S] = np.sqrt(d2)
        return out
    m1 = _median(aligned[used_rows].reshape(len(used_rows), -1)).reshape(N, 2)
    out.xy = m1.reshape(R, C, 2)
    worst, total = 0.0, np.float64(0.0)
    for r in used_rows:
        all_d2 = _d2(aligned[r], m1)
        worst = max(worst, all_d2.max())
        for v in all_d2:                                              # corner by corner, image by image: the library's order
            total = total + v
    out.spread_max = float(np.sqrt(worst))
    out.spread_rms = float(np.sqrt(total / (np.float64(len(used_rows)) * np.float64(N))))
    for r, s in enumerate(S):
        out.dist[s] = np.sqrt(_d2(aligned[r], m1).max())
    return out


# ---- 2. selection and batches --------------------------------------------------------------------------------------------------
def select(count, first=0, stride=1, max_images=0):
    stride = stride or 1
    sel = list(range(first, count, stride))
    return sel[:max_images] if max_images else sel


def nms_blocks(side):
    n, m = NMS_N, NMS_MARGIN
    return (side - n - m - (n + 1 + m)) // (n + 1) + 1 if side - n - m >= n + 1 + m else 0


def _up(v, k=256):
    return (v + k - 1) // k * k


def scratch_bytes(w, h):
    """K10b's device bytes per image: gradients (short2), map (float), slots (int2), candidates (4 x int32), each rounded up to 256"""
    if w < 34 or h < 34:
        return 0
    nblk = nms_blocks(w) * nms_blocks(h)
    return _up(4 * w * h) + _up(4 * w * h) + _up(8 * nblk) + _up(16 * nblk)


def device_bytes_per_image(w, h):
    return _up(w * h) + scratch_bytes(w, h)


def cut(raw_bytes, per_image, staging_bytes=0, device_bytes=0):
    """-> [first image of each batch ..., n], or CAPACITY when one image is above a budget"""
    staging, device = staging_bytes or DEFAULT_STAGING_BYTES, device_bytes or DEFAULT_DEVICE_BYTES
    firsts, raw, dev, held = [0], 0, 0, 0
    for i, r in enumerate(raw_bytes):
        r = _up(int(r))
        if r > staging or per_image > device:
            return CAPACITY
        if held and (raw + r > staging or dev + per_image > device):
            firsts.append(i)
            raw = dev = held = 0
        raw, dev, held = raw + r, dev + per_image, held + 1
    if held:
        firsts.append(len(raw_bytes))
    return firsts


# ---- 3. K10b's candidate order -------------------------------------------------------------------------------------------------
def block_id(u, v, h):
    """scan block of the 1-based NMS maximum (u, v) in an image h pixels high: bx nby + by (u outer, v inner)"""
    first = NMS_N + 1 + NMS_MARGIN
    return (u - first) // (NMS_N + 1) * nms_blocks(h) + (v - first) // (NMS_N + 1)


def compact(per_image_candidates, h):
    """per image the 1-based (u, v) maxima in ANY order -> ([total, 3] of (image, u, v) ordered by (image, block id), offsets)"""
    rows, offsets = [], [0]
    for m, cand in enumerate(per_image_candidates):
        cand = np.asarray(cand, np.int64).reshape(-1, 2)
        order = np.argsort([block_id(u, v, h) for u, v in cand], kind="stable")
        rows += [(m, int(cand[k, 0]), int(cand[k, 1])) for k in order]
        offsets.append(len(rows))
    return np.array(rows, np.int32).reshape(-1, 3), np.array(offsets, np.uint32)
