"""Constructed inputs for K2 (seeded clustering) and K1 (ROI crop), with numpy restatements of what the kernels decide.
Not a test module: tests/test_cluster_constructed.py builds every set once and runs it through each clustering path.

K2 decides one thing per pair of occupied cells within +-2 per axis: does the pair hold two points with float
d2 = (dx*dx + dy*dy) + dz*dz < (float)(tol*tol)?  A LINK PROBE is a frame whose answer hangs on exactly one such pair:

    anchor ......  A4 - A3 - A2 - A1 - [d d p]  ~~~  [q d d d d] - B1 - B2 - B3 - B4        (click = A4)

two arms of points 0.6 tol apart (a small perpendicular zigzag keeps them from being collinear) joined by (p, q) alone, with
|q - p| = tol (1 -+ 1e-4): p in a chosen cell (of side 0.57 tol, counted from the cloud's minimum corner, which the anchor
fixes), q in the cell at a chosen offset, p's cell at a chosen position inside its 4 x 4 x 4 block of the hashed paths.  Decoys
in p's and q's own cells (behind p, beyond q) give those cells 3 and 5 points, of which only (p, q) can be within tol.  The
expected cluster -- arm A, plus arm B when the probe is linked -- is known without any clustering code.

EXACT TIES: tol = 15/128 makes (float)(tol^2) = 225/16384 exactly, 150 integer vectors v/128 have that squared length, and on
the 1/128 lattice every difference, square and sum is exact in float32: d2 == tol2, which the strict test must not link; q
pulled in by 2^-21 m must link.
"""
import numpy as np

CELL_OVER_TOL = np.float32(0.57)          # k2_common.h: kFineCellOverTol
FINE_BITS = 96 * 1024                     # kFineBits: cells of the padded bounding grid the LDS bitmap holds
CELLS_CAP_FRESH = 512                     # kClusterCellsMin: occupied cells a fresh handle's LDS arrays hold
LDS_POINTS_FRESH = 2048                   # a fresh handle's LDS capacity for the cell-sorted points ...
LDS_POINTS_MAX = 4096                     # ... and the largest it ever grows to (kClusterLdsPointsMax)
HASH_POINTS_MAX = 65536                   # kHashPointsMax
HASH_MIN_FRAME_POINTS = 256               # kHashMinFramePoints: INPUT points of the frame
SMALL_BATCH = 64                          # kSmallBatchFrames: batches this small run K2 at 1024 threads
LIST_BLOCK = 1024                         # kListBlock: listed frames per pass of for_each_listed_chunk
TIE_TOL = 15.0 / 128.0

OFFSETS = np.array([(x, y, z) for z in range(-2, 3) for y in range(-2, 3) for x in range(-2, 3)
                    if (z, y, x) > (0, 0, 0)], dtype=np.int64)                 # one of each +-d: the 62 unordered offsets
POSITIONS = np.array([(i, j, (i + j) % 4) for i in range(4) for j in range(4)], dtype=np.int64)
LAB_OTHER, LAB_A, LAB_B = 0, 1, 2
N_ARM = 4
_DECOYS_A = np.array([0.008, 0.016])                   # cell sides behind p: p's cell holds 3 points
_DECOYS_B = np.array([0.006, 0.012, 0.018, 0.024])     # cell sides beyond q: q's cell holds 5 points
_MARGIN = 0.03                                         # p and q stay this far (cell sides) from their cells' faces, room permitting


# ------------------------------------------------------------------ the kernels' float32 arithmetic, restated
def cell_inv(tol):
    """g.inv = 1.0f / ((float)tol * 0.57f)"""
    return np.float32(1.0) / (np.float32(tol) * CELL_OVER_TOL)


def padded_cells(xyz, lo, tol):
    """(int)floorf((x - lo) * inv) + 2 per axis, in float32 like fine_key / hb_cell; xyz [..., 3], lo broadcastable"""
    t = (np.asarray(xyz, np.float32) - np.asarray(lo, np.float32)) * cell_inv(tol)
    assert t.dtype == np.float32
    return np.floor(t).astype(np.int64) + 2


def tol2_f32(tol):
    return np.float32(float(tol) * float(tol))


def d2_f32(a, b):
    """float32, unfused: d2 = ex*ex; d2 = d2 + ey*ey; d2 = d2 + ez*ez"""
    e = np.asarray(b, np.float32) - np.asarray(a, np.float32)
    d2 = e[..., 0] * e[..., 0]
    d2 = d2 + e[..., 1] * e[..., 1]
    d2 = d2 + e[..., 2] * e[..., 2]
    assert d2.dtype == np.float32
    return d2


def bounding_grid(xyz, tol):
    """(nx, ny, nz) of the padded bounding grid of fine_cluster_frame / hash_setup"""
    xyz = np.asarray(xyz, np.float32)
    ext = (xyz.max(0) - xyz.min(0)) * cell_inv(tol)
    return tuple(int(v) + 5 for v in np.floor(ext))


def k2_path(n_input, roi_xyz, tol, cells_cap=CELLS_CAP_FRESH):
    """Which algorithm k2_seeded_cluster takes for a frame of n_input points of which roi_xyz survive the crop:
    'fine_lds' / 'fine_hbm' (fine_cluster_frame<true / false>; frames of 2049..4096 ROI points depend on what the handle has
    seen: 'fine_either'), 'hashed' (hashed_cluster_frame; the k2h_* chain in the online caller's second tier, which never
    tries the fine grid), 'point' (point_level_cluster_frame)."""
    m = len(roi_xyz)
    assert m > 0
    nx, ny, nz = bounding_grid(roi_xyz, tol)
    assert max(nx, ny, nz) < 8192 + 5
    occupied = len(np.unique(padded_cells(roi_xyz, np.asarray(roi_xyz, np.float32).min(0), tol), axis=0))
    if nx * ny * nz <= FINE_BITS and occupied <= cells_cap:
        return "fine_lds" if m <= LDS_POINTS_FRESH else ("fine_hbm" if m > LDS_POINTS_MAX else "fine_either")
    return k2_hashed_or_point(n_input, roi_xyz, tol)


def k2_hashed_or_point(n_input, roi_xyz, tol):
    """hash_setup's verdict (the only one the k2h_* chain asks for)"""
    m = len(roi_xyz)
    nx, ny, nz = bounding_grid(roi_xyz, tol)
    blocks = ((nx + 3) >> 2) * ((ny + 3) >> 2) * ((nz + 3) >> 2)
    if 0 < m <= HASH_POINTS_MAX and n_input >= HASH_MIN_FRAME_POINTS and blocks < 0xFFFFFFFF:
        return "hashed"
    return "point"


def k2_threads(n_frames, online=False):
    """launch_cluster: 1024 threads in batches of <= 64 frames and for the online caller's first tier, else 256"""
    return 1024 if (n_frames <= SMALL_BATCH or online) else 256


def components_f32(xyz, tol):
    """Smallest member index of every point's component of the radius graph (float32 strict test); xyz [F, P, 3]"""
    xyz = np.asarray(xyz, np.float32)
    adj = d2_f32(xyz[:, :, None, :], xyz[:, None, :, :]) < tol2_f32(tol)
    n = xyz.shape[1]
    reach = adj | np.eye(n, dtype=bool)[None]
    for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
        reach = (reach.astype(np.float32) @ reach.astype(np.float32)) > 0
    return np.argmax(reach, axis=2)      # first True = smallest index reachable


# ------------------------------------------------------------------ link probes
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(v):
    """a unit vector perpendicular to each unit vector of v [F, 3]"""
    e = np.eye(3)[np.argmin(np.abs(v), axis=1)]
    return _unit(np.cross(v, e))


def _arms(p, q, v, tol, lattice=None):
    """arm A behind p, arm B beyond q: N_ARM points each, 0.6 tol apart along v with a +-0.05 tol zigzag"""
    w = _perp(v)
    k = np.arange(1, N_ARM + 1)[None, :, None]
    zig = np.where(k % 2 == 1, 0.05, -0.05) * tol * w[:, None, :]
    step = k * 0.6 * tol * v[:, None, :]
    da, db = -step + zig, step + zig
    if lattice:
        da, db = np.round(da * lattice) / lattice, np.round(db * lattice) / lattice
    return p[:, None, :] + da, q[:, None, :] + db


def link_probes(offsets, positions, linked, tol, seed, base_cell=16, far_cells=0, lo0=(1.0, -2.0, -1.5)):
    """One probe per row: offsets [F, 3] (q's cell - p's cell), positions [F, 3] (p's padded cell mod 4; -1: any),
    linked [F].  base_cell: p's cell is base_cell..base_cell+3 per axis (the arms reach +-5 cells around it); far_cells > 0 adds
    a second anchor that many cells above the first on every axis (a bounding grid no bitmap holds).
    Returns a dict: xyz [F, P, 3] float32 (anchors first, then A = p, decoys, arm; then B), lab [P], click [F, 3] (the far end
    of arm A), point [F, 3] (1.35 m beyond it, along the arm), v [F, 3], draws (the most candidate draws a probe needed)."""
    offsets, positions, linked = np.asarray(offsets, np.int64), np.asarray(positions, np.int64), np.asarray(linked, bool)
    F = len(offsets)
    rng = np.random.default_rng(seed)
    s = 1.0 / float(cell_inv(tol))
    lo = (np.asarray(lo0) + rng.uniform(-0.3, 0.3, (F, 3))).astype(np.float32)
    r = tol * np.where(linked, 1.0 - 1e-4, 1.0 + 1e-4)
    free = positions < 0
    cp = base_cell + np.where(free, rng.integers(0, 4, (F, 3)), (positions - 2 - base_cell) % 4)
    p32 = np.zeros((F, 3), np.float32)
    q32 = np.zeros((F, 3), np.float32)
    draws = np.zeros(F, np.int64)
    todo = np.arange(F)
    K = 64
    t2 = tol2_f32(tol)
    for _ in range(400):
        if not len(todo):
            break
        d = offsets[todo].astype(np.float64)
        v = _unit(d[:, None, :] + rng.uniform(-0.6, 0.6, (len(todo), K, 3)))
        g = (r[todo] / s)[:, None, None] * v                                   # q - p in cell sides
        u_lo = np.maximum(0.0, d[:, None, :] - g)
        u_hi = np.minimum(1.0, d[:, None, :] + 1.0 - g)
        ok = ((u_hi - u_lo) > 0.008).all(-1)       # (offsets of +-2 on all three axes leave p ~0.013 cell sides: |q - p| = 1.754 sides)
        m = np.minimum(_MARGIN, 0.25 * (u_hi - u_lo))
        u_lo, u_hi = u_lo + m, u_hi - m
        first = np.argmax(ok, axis=1)
        rows = np.arange(len(todo))
        draws[todo] += np.where(ok.any(1), first + 1, K)
        u = u_lo[rows, first] + rng.uniform(0, 1, (len(todo), 3)) * (u_hi - u_lo)[rows, first]
        p = lo[todo].astype(np.float64) + (cp[todo] + u) * s
        q = p + g[rows, first] * s
        pf, qf = p.astype(np.float32), q.astype(np.float32)
        # accepted on the kernels' own arithmetic: cells, block position, the distance test, and room to the cells' faces
        cpf, cqf = padded_cells(pf, lo[todo], tol), padded_cells(qf, lo[todo], tol)
        good = ok.any(1) & (cqf - cpf == offsets[todo]).all(1) & (cpf == cp[todo] + 2).all(1)
        good &= (d2_f32(pf, qf) < t2) == linked[todo]
        for x in (pf, qf):
            t = (x - lo[todo]) * cell_inv(tol)
            fr = t - np.floor(t)
            good &= ((fr > 0.002) & (fr < 0.998)).all(1)     # (>= 100 ulp of the cell coordinate)
        vf = _unit(g[rows, first])[:, None, :]
        dec_a = (p[:, None, :] - (_DECOYS_A * s)[None, :, None] * vf).astype(np.float32)
        dec_b = (q[:, None, :] + (_DECOYS_B * s)[None, :, None] * vf).astype(np.float32)
        good &= (padded_cells(dec_a, lo[todo][:, None, :], tol) == cpf[:, None, :]).all((1, 2))
        good &= (padded_cells(dec_b, lo[todo][:, None, :], tol) == cqf[:, None, :]).all((1, 2))
        p32[todo[good]], q32[todo[good]] = pf[good], qf[good]
        todo = todo[~good]
    assert not len(todo), "no probe found for offsets %s" % offsets[todo]
    v = _unit(q32.astype(np.float64) - p32.astype(np.float64))
    P, Q = p32.astype(np.float64), q32.astype(np.float64)
    arm_a, arm_b = _arms(P, Q, v, tol)
    dec_a = P[:, None, :] - (_DECOYS_A * s)[None, :, None] * v[:, None, :]
    dec_b = Q[:, None, :] + (_DECOYS_B * s)[None, :, None] * v[:, None, :]
    parts = [lo[:, None, :].astype(np.float64)]
    if far_cells:
        parts.append((lo.astype(np.float64) + far_cells * s)[:, None, :])
    n_anchor = len(parts)
    parts += [P[:, None, :], dec_a, arm_a, Q[:, None, :], dec_b, arm_b]
    xyz = np.concatenate(parts, axis=1).astype(np.float32)
    n_a, n_b = 1 + len(_DECOYS_A) + N_ARM, 1 + len(_DECOYS_B) + N_ARM
    lab = np.array([LAB_OTHER] * n_anchor + [LAB_A] * n_a + [LAB_B] * n_b)
    click = xyz[:, n_anchor + n_a - 1].copy()
    point = (click.astype(np.float64) - 1.35 * v).astype(np.float32)
    return dict(xyz=xyz, lab=lab, click=click, point=point, v=v, lo=lo, tol=tol, linked=linked, offsets=offsets,
                positions=np.where(free, (cp + 2) % 4, positions), i_p=n_anchor, i_q=n_anchor + n_a, draws=int(draws.max()),
                n_anchor=n_anchor)


def probe_plan(n_positions, seeds=1):
    """(offsets, positions, linked) rows: every unordered offset (both orientations over the seeds and positions) x the first
    n_positions block positions (0: any position) x {linked, unlinked} x seeds"""
    rows = []
    for sd in range(seeds):
        for io, d in enumerate(OFFSETS):
            for ip in range(max(n_positions, 1)):
                for ln in (True, False):
                    sign = -1 if (io + ip + sd) % 2 else 1
                    rows.append((tuple(sign * d), tuple(POSITIONS[ip]) if n_positions else (-1, -1, -1), ln))
    off = np.array([r[0] for r in rows])
    pos = np.array([r[1] for r in rows])
    return off, pos, np.array([r[2] for r in rows])


def assert_complete(core, n_positions):
    """every unordered offset (x every listed block position) x {linked, unlinked} is there, measured on the points themselves"""
    xyz, lo, tol = core["xyz"], core["lo"], core["tol"]
    cp = padded_cells(xyz[:, core["i_p"]], lo, tol)
    cq = padded_cells(xyz[:, core["i_q"]], lo, tol)
    d = cq - cp
    d = np.where((np.where(d[:, [2]] != 0, d[:, [2]], np.where(d[:, [1]] != 0, d[:, [1]], d[:, [0]])) < 0), -d, d)   # the +d of each pair
    pos = cp % 4
    seen = set()
    for k in range(len(d)):
        seen.add((tuple(d[k]), tuple(pos[k]) if n_positions else None, bool(core["linked"][k])))
    want = {(tuple(o), tuple(POSITIONS[ip]) if n_positions else None, ln)
            for o in OFFSETS for ip in range(max(n_positions, 1)) for ln in (True, False)}
    assert len(OFFSETS) == 62 and len(POSITIONS) == 16
    assert want <= seen, sorted(want - seen)[:5]
    if n_positions == 16:      # every axis sees all four positions, every pair of axes all sixteen
        for a in range(3):
            assert set(pos[:, a]) == {0, 1, 2, 3}
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert len({(x, y) for x, y in zip(pos[:, a], pos[:, b])}) == 16


# ------------------------------------------------------------------ exact ties
def tie_directions():
    from itertools import permutations, product
    out = set()
    for base in ((15, 0, 0), (9, 12, 0), (5, 10, 10), (2, 10, 11), (2, 5, 14)):
        for perm in permutations(base):
            for sg in product((1, -1), repeat=3):
                out.add(tuple(int(a * b) for a, b in zip(perm, sg)))
    out = np.array(sorted(out), dtype=np.int64)
    assert len(out) == 150 and ((out ** 2).sum(1) == 225).all()
    return out


def tie_probes(seed, wide=False):
    """300 frames on the 1/128 lattice, tol = 15/128: direction k exactly AT the tolerance (frame 2k: not linked) and with the
    largest component of q pulled in by 2^-21 m (frame 2k + 1: linked).  wide: the anchors 8 m apart and 4 m from p (the
    hashed paths; and no point nearer to `point` than the end of arm A)."""
    rng = np.random.default_rng(seed)
    dirs = np.repeat(tie_directions(), 2, axis=0)
    F = len(dirs)
    linked = np.arange(F) % 2 == 1
    tol = TIE_TOL
    P = 2.5 + rng.integers(-8, 9, (F, 3)) / 128.0
    Q = P + dirs / 128.0
    v = dirs / 15.0
    arm_a, arm_b = _arms(P, Q, v, tol, lattice=128.0)
    big = np.argmax(np.abs(dirs), axis=1)
    rows = np.arange(F)
    Qp = Q.copy()
    Qp[rows, big] -= np.where(linked, np.sign(dirs[rows, big]) * 2.0 ** -21, 0.0)
    lo = (-1.5 if wide else 1.25) + rng.integers(-16, 17, (F, 3)) / 128.0
    parts = [lo[:, None, :]]
    if wide:
        parts.append(lo[:, None, :] + 8.0)
    n_anchor = len(parts)
    parts += [P[:, None, :], arm_a, Qp[:, None, :], arm_b]
    xyz64 = np.concatenate(parts, axis=1)
    xyz = xyz64.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), xyz64)                    # every coordinate is a float32
    n_a = 1 + N_ARM
    lab = np.array([LAB_OTHER] * n_anchor + [LAB_A] * n_a + [LAB_B] * n_a)
    click = xyz[:, n_anchor + n_a - 1].copy()
    point = (click.astype(np.float64) - 1.35 * v).astype(np.float32)
    return dict(xyz=xyz, lab=lab, click=click, point=point, v=v, lo=lo.astype(np.float32), tol=tol, linked=linked, dirs=dirs,
                i_p=n_anchor, i_q=n_anchor + n_a, n_anchor=n_anchor)


# ------------------------------------------------------------------ frames
def subset(core, idx):
    out = dict(core)
    for k in ("xyz", "click", "point", "v", "lo", "linked"):
        out[k] = core[k][idx]
    return out


def sheet(core, n, cells, seed):
    """n points over the cells x cells x 1 cells of a sheet two cells above the anchor: hundreds of occupied cells, > 4 tol below
    the arms, one big admissible component that the click is not in"""
    rng = np.random.default_rng(seed)
    s = 1.0 / float(cell_inv(core["tol"]))
    F = len(core["xyz"])
    cell = np.concatenate([rng.integers(0, cells, (F, n, 2)), np.full((F, n, 1), 2)], axis=2)
    return (core["lo"].astype(np.float64)[:, None, :] + (cell + rng.uniform(0.1, 0.9, (F, n, 3))) * s).astype(np.float32)


def assemble(core, seed, extra=None, n_nan=0, n_outside=0):
    """Frames [F, N, 4] in a seeded input order: the core's points, `extra` [F, E, 3] (finite points that are in nobody's arm),
    n_nan non-finite points (NaN or inf in one coordinate) and n_outside finite points 40 m away (outside any ROI used here).
    -> clouds, lab [F, N] (LAB_*; -1 for points the crop must drop)"""
    rng = np.random.default_rng(seed)
    xyz = core["xyz"]
    F = len(xyz)
    parts, labs = [xyz], [np.broadcast_to(core["lab"], xyz.shape[:2])]
    if extra is not None:
        parts.append(extra)
        labs.append(np.full(extra.shape[:2], LAB_OTHER))
    if n_nan:
        bad = np.broadcast_to(xyz[:, -1:, :], (F, n_nan, 3)).copy()
        which = rng.integers(0, 3, (F, n_nan))
        val = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, (F, n_nan))]
        np.put_along_axis(bad, which[..., None], val[..., None], axis=2)
        parts.append(bad)
        labs.append(np.full((F, n_nan), -1))
    if n_outside:
        parts.append((xyz[:, -1:, :] + 40.0 + rng.uniform(0, 1, (F, n_outside, 3))).astype(np.float32))
        labs.append(np.full((F, n_outside), -1))
    pts = np.concatenate(parts, axis=1).astype(np.float32)
    lab = np.concatenate(labs, axis=1)
    inten = rng.uniform(5, 90, pts.shape[:2]).astype(np.float32)
    order = np.argsort(rng.random(pts.shape[:2]), axis=1)
    clouds = np.concatenate([pts, inten[..., None]], axis=2)
    clouds = np.take_along_axis(clouds, order[..., None], axis=1)
    return np.ascontiguousarray(clouds), np.take_along_axis(lab, order, axis=1)


def expected(clouds, lab, linked, f):
    """(ROI cloud, cluster cloud) of frame f, in input order"""
    keep = (lab[f] == LAB_A) | ((lab[f] == LAB_B) & bool(linked[f]))
    return clouds[f][lab[f] >= 0], clouds[f][keep]


# ------------------------------------------------------------------ K1: the crop's limits
CROP_LENGTHS = (1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8193)
CROP_PATTERNS = ("all", "none", "first", "last", "third", "lane0", "lane63", "after2048", "after4096")


def crop_box(click, half):
    """lo = (float)((double)click - half), hi likewise"""
    c = np.asarray(click, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (c - np.asarray(half, np.float64)).astype(np.float32), (c + np.asarray(half, np.float64)).astype(np.float32)


def crop_mask(cloud, click, half):
    """what the three PassThrough filters keep: finite x, y, z and not (below lo or above hi), float32 comparisons"""
    lo, hi = crop_box(click, half)
    xyz = np.asarray(cloud, np.float32)[:, :3]
    with np.errstate(invalid="ignore"):
        return np.isfinite(xyz).all(1) & ~((xyz < lo) | (xyz > hi)).any(1)


def _survivor_pattern(name, n):
    i = np.arange(n)
    return {"all": i >= 0, "none": i < 0, "first": i == 0, "last": i == n - 1, "third": i % 3 == 0, "lane0": i % 64 == 0,
            "lane63": i % 64 == 63, "after2048": i >= 2048, "after4096": i >= 4096}[name]


def crop_frame(n, pattern, click, half, rng):
    """n points of which exactly those of `pattern` lie inside the box of (click, half): survivors anywhere inside, a tenth of them
    ON a limit; the others just outside one limit, far outside, or non-finite"""
    lo, hi = crop_box(click, half)
    keep = _survivor_pattern(pattern, n)
    u = rng.random((n, 3))
    xyz = (lo.astype(np.float64) + u * (hi.astype(np.float64) - lo.astype(np.float64))).astype(np.float32)
    xyz = np.minimum(np.maximum(xyz, lo), hi)
    on = rng.random((n, 3)) < 0.1
    xyz = np.where(on, np.where(rng.random((n, 3)) < 0.5, lo, hi), xyz)
    ax = rng.integers(0, 3, n)
    kind = rng.integers(0, 6, n)
    out_val = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                        [np.nextafter(lo, np.float32(-np.inf))[ax], np.nextafter(hi, np.float32(np.inf))[ax], hi[ax] + np.float32(7.0),
                         np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]).astype(np.float32)
    bad = xyz.copy()
    bad[np.arange(n), ax] = out_val
    xyz = np.where(keep[:, None], xyz, bad)
    cloud = np.concatenate([xyz, rng.uniform(1, 99, (n, 1)).astype(np.float32)], axis=1).astype(np.float32)
    assert np.array_equal(crop_mask(cloud, click, half), keep)
    return cloud, keep


def crop_limit_frame(click, half):
    """every limit, its two float neighbours, +-inf and NaN, and both zeros, on each axis; the other coordinates at the click.
    -> cloud, the expected mask (written out by hand: inclusive limits, nothing non-finite)"""
    lo, hi = crop_box(click, half)
    c = np.asarray(click, np.float32)
    rows, keep = [], []
    ninf, pinf = np.float32(-np.inf), np.float32(np.inf)
    for a in range(3):
        for val, inside in ((lo[a], True), (hi[a], True), (np.nextafter(lo[a], ninf), False), (np.nextafter(lo[a], pinf), True),
                            (np.nextafter(hi[a], pinf), False), (np.nextafter(hi[a], ninf), True), (pinf, False), (ninf, False),
                            (np.float32(np.nan), False), (np.float32(-0.0), bool(lo[a] <= 0.0 <= hi[a])),
                            (np.float32(0.0), bool(lo[a] <= 0.0 <= hi[a]))):
            q = c.copy()
            q[a] = val
            rows.append(q)
            keep.append(inside)
    cloud = np.concatenate([np.array(rows, np.float32), np.full((len(rows), 1), 50.0, np.float32)], axis=1)
    return cloud, np.array(keep)
