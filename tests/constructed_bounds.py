"""Constructed labelled points for K6's PRUNING (the frame's bound, the per-tile box pre-pass, the common pre-pass of a theta group)
and fp64 restatements of the rules the pruning rests on: K5w's point classes, box_term's lower bound of a tile, and five
deliberately wrong variants of that bound (used by the CPU tests only, to show that a case can tell them from the right one).

Plain module beside constructed_points.py (no fixtures).  Inputs and restatements only: nothing here is tuned against the kernels.
`p` is any parameter struct with the board and grid fields (the library's or the oracle's).

The fenced board.  A noise-free, correctly coloured board (constructed_points.ideal_board) costs exactly 0 under every translation
that keeps each point in its cell: with in-cell offsets U(-J, J) that is a shift of up to 1/2 - J squares.  A FENCE -- a few points
just outside the outline on two sides -- makes the cost fall strictly as the board shifts towards those sides: the functor charges
an out-of-board point |u_i| + |u_j| (distance to the outline across it plus depth along it), and the fence points sit where both
shrink.  The argmin is then the LAST grid step before in-board points start to cross cell borders, the in-board points cost
nothing there, and the whole cost is the fence's.  When that step is the corner of its 4 x 4 tile in the direction of the pull, the
tile's box bound over the fence points EQUALS the argmin's cost / 2 in real arithmetic: the tile survives by the safety factors
alone.
"""
import numpy as np

import constructed_points as cp

# restated constants: k6_common.h / ilcc_internal.h / k5w_walk_order.h / ilcc_api.cpp
K_TILE = 4                                  # kTile
K_THETA_GROUP = 7                           # kThetaGroup
K_RIM = np.float32(-300.0 * 1e-3)           # -(float)kRimMilli * 1e-3f
K_INTERIOR_MARGIN = np.float32(1e-4)
K_WIDE = 0.5                                # k6_group_prepass: images further apart than this on an axis -> the point counts 0
K_TIE_EPS = float(np.float32(2e-5))         # kTieEps
K_BOX_SAFETY = 1.0 - 2.0 ** -12             # kBoxSafety
BOX_POINTS = 48                             # ILCC_BOX_POINTS
K_GROUP_SHIFT_SMALL, K_GROUP_SHIFT_LARGE = 2, 1   # kGroupShiftSmall / kGroupShiftLarge
K_GRID_LARGE_FROM = 2048                    # kGridLargeFrom: staging above it -> the 512-thread instance
K_GRID_LDS_POINTS_MAX = 8192                # kGridLdsPointsMax
K_BOX_FIRST_ROUND = 32                      # kBoxFirstRound
K_BOX_TILES_MAX = 4096                      # kBoxTilesMax

CLEAR = 2.0 ** -10                           # the distance every constructed point keeps from a cell border / a class threshold

MUTANTS = ("high_short", "low_late", "last_theta_out", "inflated", "clamp_short")


def axis_tiles(n):
    return (n + K_TILE - 1) // K_TILE


def tables(p):
    """the float32 tables upload_tables (ilcc_api.cpp) builds, as float64 arrays of float32 values: cos / g, sin / g per theta, the
    translations in squares from the board's low outline, and the indices nearest zero"""
    g = p.grid_length
    th = p.th_min + np.arange(p.n_th) * p.th_step
    cth = (np.cos(th) / g).astype(np.float32).astype(np.float64)
    sth = (np.sin(th) / g).astype(np.float32).astype(np.float64)
    ay = (((p.ty_min + np.arange(p.n_ty) * p.ty_step) + p.board_w * g / 2.0) / g).astype(np.float32).astype(np.float64)
    az = (((p.tz_min + np.arange(p.n_tz) * p.tz_step) + p.board_h * g / 2.0) / g).astype(np.float32).astype(np.float64)

    def near_zero(vmin, step, n):
        return int(min(max(int(np.floor(-vmin / step + 0.5)), 0), n - 1))

    centre = (near_zero(p.th_min, p.th_step, p.n_th), near_zero(p.ty_min, p.ty_step, p.n_ty), near_zero(p.tz_min, p.tz_step, p.n_tz))
    return cth, sth, ay, az, centre


def rotated(yz, cth, sth):
    """k5w_walk_order.h rotate() in fp64: (cth y - sth z, cth z + sth y), in squares"""
    y, z = yz[:, 0].astype(np.float64), yz[:, 1].astype(np.float64)
    return cth * y - sth * z, cth * z + sth * y


# ---------------------------------------------------------------------------------------------------------------- point classes
def walk_classes(p, yz):
    """K5w's class rule (k5w_walk_order.h walk_order_frame) in fp64 -> (cls[m]: 0 interior, 1 other border class, 2 rim;
    margin[m]: distance in squares of the point from the threshold that decided its class).
    interior: |i| <= |y| max|cos / g| + |z| max|sin / g| (likewise j) stays, with 1e-4 square to spare, inside the room the
    translation tables leave on both axes -> in the board under every entry of the tables;
    rim: not interior, and within kRimMilli / 1000 square of the outline (or outside it) at the grid's centre candidate."""
    cth, sth, ay, az, (c_th, c_ty, c_tz) = tables(p)
    Wh, Hh = 0.5 * p.board_w, 0.5 * p.board_h
    cmax, smax = np.abs(cth).max(), np.abs(sth).max()
    room_i = min(min(ay[0], ay[-1]), 2.0 * Wh - max(ay[0], ay[-1]))
    room_j = min(min(az[0], az[-1]), 2.0 * Hh - max(az[0], az[-1]))
    y, z = np.abs(yz[:, 0].astype(np.float64)), np.abs(yz[:, 1].astype(np.float64))
    bi, bj = y * cmax + z * smax, z * cmax + y * smax
    m_i, m_j = room_i - (bi + float(K_INTERIOR_MARGIN)), room_j - (bj + float(K_INTERIOR_MARGIN))
    inside = (m_i > 0) & (m_j > 0)
    pi, pj = rotated(yz, cth[c_th], sth[c_th])
    uc, wc = np.abs((pi + ay[c_ty]) - Wh) - Wh, np.abs((pj + az[c_tz]) - Hh) - Hh
    rim_d = np.maximum(uc, wc) - float(K_RIM)
    cls = np.where(inside, 0, np.where(rim_d > 0, 2, 1))
    # an interior point is decided by the smaller of its two rooms; a point that is not by the room it lacks (the more negative) AND the rim test
    margin = np.where(inside, np.minimum(m_i, m_j), np.minimum(np.abs(np.minimum(m_i, m_j)), np.abs(rim_d)))
    return cls, margin


# ---------------------------------------------------------------------------------------------------------------- box bound
def tile_box(p, tile, mutant=None):
    """(alo, ahi, zlo, zhi): the extreme translations of tile (qa, qb) as box_prepass_rounds takes them -- entries qa * 4 + d, d = 0 .. 3,
    clamped to the table's last entry (a partial tile).  Mutants: the high extreme one table step short, the low one a step late,
    the clamp at the entry before the last."""
    _, _, ay, az, _ = tables(p)
    qa, qb = tile
    d = list(range(K_TILE))
    if mutant == "high_short":
        d = d[:-1]
    if mutant == "low_late":
        d = d[1:]
    last = 2 if mutant == "clamp_short" else 1
    va = [ay[min(qa * K_TILE + e, p.n_ty - last)] for e in d]
    vz = [az[min(qb * K_TILE + e, p.n_tz - last)] for e in d]
    return min(va), max(va), min(vz), max(vz)


def point_intervals(p, sample_yz, thetas, mutant=None):
    """(i_lo, i_hi, j_lo, j_hi, wide) of every sample point over the thetas (k6_group_prepass's staging loop): the extremes of its
    rotated images; wide: the images lie more than 0.5 square apart on an axis -> the point is left out (counts 0).  spread: the
    larger of the two spreads.  Mutant: the last theta left out."""
    cth, sth, _, _, _ = tables(p)
    ks = list(thetas)
    if mutant == "last_theta_out" and len(ks) > 1:
        ks = ks[:-1]
    im = np.stack([np.stack(rotated(sample_yz, cth[k], sth[k])) for k in ks])   # [theta, axis, point]
    lo, hi = im.min(axis=0), im.max(axis=0)
    spread = (hi - lo).max(axis=0)
    return lo[0], hi[0], lo[1], hi[1], ~((hi[0] - lo[0] <= K_WIDE) & (hi[1] - lo[1] <= K_WIDE)), spread


def box_bound(p, sample_yz, thetas, tile, mutant=None):
    """box_term (k6_common.h) summed over the sample in fp64: a lower bound of cost / 2 for every candidate (either phase) of the
    4 x 4 tile at every theta of `thetas` (one theta: a workgroup's own pre-pass; a group's: the common pre-pass).  A point counts
    only when it is out of the board at every translation of the box; then with the |u| nearest zero over the box on each axis."""
    if len(sample_yz) == 0:
        return 0.0
    Wh, Hh, delta = 0.5 * p.board_w, 0.5 * p.board_h, float(p.huber_delta)
    alo, ahi, zlo, zhi = tile_box(p, tile, mutant)
    pi_lo, pi_hi, pj_lo, pj_hi, wide, _ = point_intervals(p, sample_yz, thetas, mutant)
    pi_lo, pi_hi, pj_lo, pj_hi = (np.where(wide, 0.0, v) for v in (pi_lo, pi_hi, pj_lo, pj_hi))   # (as a point at the board's centre)
    ui_lo, ui_hi = np.abs(pi_lo + alo - Wh) - Wh, np.abs(pi_hi + ahi - Wh) - Wh
    uj_lo, uj_hi = np.abs(pj_lo + zlo - Hh) - Hh, np.abs(pj_hi + zhi - Hh) - Hh
    out_all = np.maximum(np.minimum(ui_lo, ui_hi), np.minimum(uj_lo, uj_hi)) >= 0.0
    med0 = lambda a, b: np.median(np.stack([a, b, np.zeros_like(a)]), axis=0)
    R = np.abs(med0(ui_lo, ui_hi)) + np.abs(med0(uj_lo, uj_hi))
    Q = np.minimum(R, delta)
    T = Q * (R - 0.5 * Q)
    lb = float(np.sum(np.where(out_all, 0.5 * T, 0.0)))
    return lb * (1.0 + 2.0 ** -10) if mutant == "inflated" else lb


def group_sample_size(M, Mi, lds_points):
    """n_pre of k6_group_prepass for a frame of M labelled points, Mi of them interior, staged with lds_points capacity:
    box_sample(box_points, M, M, Mi, kGroupShift of the instance) capped by group_prepass_points"""
    shift = K_GROUP_SHIFT_LARGE if lds_points > K_GRID_LARGE_FROM else K_GROUP_SHIFT_SMALL
    cap = max(lds_points // 2 + 64, BOX_POINTS)
    return min(min(max(BOX_POINTS, M >> shift), M - Mi), cap)


def solve_lds_points(m):
    """the staging capacity ilcc_grid_solve runs a fresh handle's m points with (diagnostic_ctx)"""
    lds = 1024
    while lds < m and lds < K_GRID_LDS_POINTS_MAX:
        lds <<= 1
    return lds


def theta_groups(n_th):
    return [list(range(k0, min(k0 + K_THETA_GROUP, n_th))) for k0 in range(0, n_th, K_THETA_GROUP)]


# ---------------------------------------------------------------------------------------------------------------- fenced board
def fenced_board(p, corner, steps=(3, 3), n_fence=5, dist=0.28, K=8, seed=0, keep_out=0.35, cells=None, inner=(0, 0.0)):
    """The family of the module's docstring at pose (0, 0, 0).  corner: two letters, 'h' / 'l' per axis (ty, tz): the side the fence
    pulls the board to.  steps: grid steps from the pose to the designed argmin per axis (the in-cell offsets are U(-J, J) with
    J = 1/2 - steps * step: a shift of `steps` keeps every point in its cell, one more does not).  n_fence points per fence, `dist`
    squares outside the outline, spread along the half of the side where the depth |u| of the OTHER axis also shrinks with the
    pull (and at least one square from the corner of the board).  No in-board point lies closer than keep_out square to the
    outline (clamped), within 2^-9 square of a cell border at the designed argmin, or of the threshold of its class.  cells: the (ci, cj) cells to fill (default: all).  inner = (n, d): n more points per fence only d < steps * step
    squares outside the outline, which the board swallows on its way to the designed argmin: there each sits in the middle of an
    outer cell along its side, in that cell's colour, and costs nothing.  -> (yz float32 [m, 2], label uint8 [m], n_in_board)"""
    rng = np.random.default_rng(seed)
    W, H, g = p.board_w, p.board_h, p.grid_length
    Ji, Jj = 0.5 - steps[0] * p.ty_step / g, 0.5 - steps[1] * p.tz_step / g
    assert Ji > 0 and Jj > 0
    if cells is None:
        ci, cj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
        ci, cj = ci.ravel(), cj.ravel()
    else:
        ci, cj = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    ci, cj = np.repeat(ci, K), np.repeat(cj, K)
    m = len(ci)
    i, j = np.zeros(m), np.zeros(m)
    todo = np.ones(m, bool)
    for _ in range(64):   # offsets 2 CLEAR short of +-J (at the designed argmin no point is nearer a cell border); a point nearer
        # than 2 CLEAR to the threshold of K5w's class rule is drawn again
        n = int(todo.sum())
        i[todo] = np.clip(ci[todo] + 0.5 + rng.uniform(-Ji + 2 * CLEAR, Ji - 2 * CLEAR, n), keep_out, W - keep_out)
        j[todo] = np.clip(cj[todo] + 0.5 + rng.uniform(-Jj + 2 * CLEAR, Jj - 2 * CLEAR, n), keep_out, H - keep_out)
        todo = walk_classes(p, cp.from_board(p, i, j))[1] < 2 * CLEAR
        if not todo.any():
            break
    assert not todo.any()
    lab = (ci + cj) & 1
    hi_a, hi_b = corner[0] == "h", corner[1] == "h"

    def along(lo, hi, n, step):   # a fence point's coordinate along its side: 2 CLEAR from a cell border under every translation of the grid
        v = rng.uniform(lo, hi, n)
        for _ in range(64):
            bad = np.abs(v / step - np.rint(v / step)) * step < 2 * CLEAR
            if not bad.any():
                break
            v[bad] = rng.uniform(lo, hi, int(bad.sum()))
        return v
    # fence across i (pulls along ty): outside the low outline for a pull to high ty; along j on the half whose depth shrinks with the tz pull
    fi = np.full(n_fence, -dist if hi_a else W + dist)
    fj = along(H / 2 + 0.5, H - 1, n_fence, p.tz_step / g) if hi_b else along(1, H / 2 - 0.5, n_fence, p.tz_step / g)
    # fence across j (pulls along tz)
    gj = np.full(n_fence, -dist if hi_b else H + dist)
    gi = along(W / 2 + 0.5, W - 1, n_fence, p.ty_step / g) if hi_a else along(1, W / 2 - 0.5, n_fence, p.ty_step / g)
    i, j = np.concatenate([i, fi, gi]), np.concatenate([j, fj, gj])
    lab = np.concatenate([lab, np.arange(2 * n_fence) & 1])
    n_inner, d_inner = inner
    if n_inner:
        sa, sb = (1 if hi_a else -1) * steps[0] * p.ty_step / g, (1 if hi_b else -1) * steps[1] * p.tz_step / g   # the designed shift
        cjs = rng.integers(H // 2 + 1, H - 1, n_inner) if hi_b else rng.integers(1, H // 2 - 1, n_inner)
        cis = rng.integers(W // 2 + 1, W - 1, n_inner) if hi_a else rng.integers(1, W // 2 - 1, n_inner)
        i = np.concatenate([i, np.full(n_inner, -d_inner if hi_a else W + d_inner), cis + 0.5 - sa])
        j = np.concatenate([j, cjs + 0.5 - sb, np.full(n_inner, -d_inner if hi_b else H + d_inner)])
        lab = np.concatenate([lab, ((0 if hi_a else W - 1) + cjs) & 1, (cis + (0 if hi_b else H - 1)) & 1])
    return cp.from_board(p, i, j), lab.astype(np.uint8), len(ci)


def half_turn_union(yz, lab):
    """the set united with its image under (y, z) -> (-y, -z), labels kept (constructed_points.dyadic_points_symmetric): on a
    board with an even number of squares on both axes the half turn maps the pattern onto itself with its colours, and negation
    is exact, so cost(th, ty, tz) == cost(th, -ty, -tz) EXACTLY"""
    return np.concatenate([yz, -yz]), np.concatenate([lab, lab])


def dead_tiles(states, mask, n_ty, n_tz):
    """fetch_group_prepass's output -> bool [groups, tiles along ty, tiles along tz]: True where the common pre-pass rejected the tile
    (a state-0 group: all of them; state 2: none)"""
    nta, ntb = axis_tiles(n_ty), axis_tiles(n_tz)
    out = np.zeros((len(states), nta, ntb), bool)
    for gidx, st in enumerate(states):
        if st == 0:
            out[gidx] = True
        elif st == 1:
            for q in range(nta * ntb):
                out[gidx, q // ntb, q % ntb] = bool((int(mask[gidx, q >> 5]) >> (q & 31)) & 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- walk layout
def walk_stride(M):
    """ilcc_internal.h walk_stride: ~0.618 M, odd, coprime to M"""
    if M <= 2:
        return 1
    S = int(np.float32(M) * np.float32(0.6180339)) | 1
    while np.gcd(S, M) != 1:
        S += 2
    return 1 if S >= M else S


def walk_layout(p, yz):
    """-> (order[m]: index of the input point at each position of K5w's layout [interior | rim | other border class], each part in
    golden-ratio walk order (slot s <- point (s S) mod M, a stable partition), Mi, n_rim)"""
    M = len(yz)
    cls, _ = walk_classes(p, yz)
    S = walk_stride(M)
    slots = (np.arange(M, dtype=np.int64) * S) % M
    c = cls[slots]
    order = np.concatenate([slots[c == 0], slots[c == 2], slots[c == 1]])
    return order, int((c == 0).sum()), int((c == 2).sum())
