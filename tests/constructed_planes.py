"""Constructed clusters for K3 (RANSAC plane), K4 (plane frame) and K5 (gray-zone histogram), with numpy restatements of what the
kernels decide.  Not a test module: tests/test_plane_hist_constructed.py builds every frame once and runs it through each path.

A FRAME is one cluster: every point of it lies within 1 m of every other, the click is its first point, and with
cluster_tol = 1, cluster_min = 3 and a wide ROI the whole cloud, in input order, is what K3 gets.

The EXACT setting (families A, C, E, F): points on a lattice of spacing 2^-5 .. 2^-7 in the plane x = 2.  Every difference, product
and sum that a hypothesis from three lattice points needs is exact in float32: its plane is +-(1, 0, 0, -+2) and a point's
distance is |x - 2|, exactly (Sterbenz).  The PCA refit of inliers that all have x = 2 -- or come in pairs 2 +- d -- has a
covariance whose x row is exactly 0 off the diagonal: the normal stays (1, 0, 0).  Coordinates are multiples of 2^-10 below 4
(outliers and the 2^-21 offsets aside) and a frame has at most 4097 points, so every double sum of them is exact in any order.
"""
import math

import numpy as np

LDS_POINTS = 2048          # k3_ransac_plane.h: kRansacLdsPoints
SMALL_BATCH = 64           # kSmallBatchFrames: batches this small run K3 at 1024 threads, larger ones at 256
X_PLANE = 2.0
THR_EXACT = 1.0 / 32.0
CENTRE = np.array([X_PLANE, 0.5, 0.25])
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------ the kernels' arithmetic, restated
def hash_u32(x):
    """the two-round 32-bit hash of k3_ransac_plane.h, on uint64 arrays masked to 32 bits"""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def sample_index(seed, h, k, m):
    """(uint32)(((uint64)hash(seed ^ hash(h * 3 + k + 0x9E3779B9)) * m) >> 32); seed, h broadcast"""
    key = (np.asarray(h, np.uint64) * np.uint64(3) + np.uint64(k) + np.uint64(0x9E3779B9)) & _M32
    r = hash_u32((np.asarray(seed, np.uint64) & _M32) ^ hash_u32(key))
    return ((r * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def sample_triple(seed, h, m):
    return tuple(int(sample_index(seed, h, k, m)) for k in range(3))


def plane_from_3(p0, p1, p2):
    """float32, one operation per line as in the kernel -> (valid, pl[4]); the caller tests the indices for duplicates"""
    p0, p1, p2 = (np.asarray(p, np.float32) for p in (p0, p1, p2))
    ax = p1[0] - p0[0]
    ay = p1[1] - p0[1]
    az = p1[2] - p0[2]
    bx = p2[0] - p0[0]
    by = p2[1] - p0[1]
    bz = p2[2] - p0[2]
    t0 = ay * bz
    t1 = az * by
    nx = t0 - t1
    t0 = az * bx
    t1 = ax * bz
    ny = t0 - t1
    t0 = ax * by
    t1 = ay * bx
    nz = t0 - t1
    n2 = nx * nx
    n2 = n2 + ny * ny
    n2 = n2 + nz * nz
    assert n2.dtype == np.float32
    if not n2 > np.float32(1e-12):
        return False, np.zeros(4, np.float32)
    nrm = np.sqrt(n2)
    nx = nx / nrm
    ny = ny / nrm
    nz = nz / nrm
    d = nx * p0[0]
    d = d + ny * p0[1]
    d = d + nz * p0[2]
    pl = np.array([nx, ny, nz, -d])
    assert pl.dtype == np.float32
    return True, pl


def plane_dist(pl, pts):
    """fabsf(((pl0 x + pl1 y) + pl2 z) + pl3) in float32; pts [M, >= 3]"""
    pl = np.asarray(pl, np.float32)
    q = np.asarray(pts, np.float32)
    s = pl[0] * q[:, 0]
    s = s + pl[1] * q[:, 1]
    s = s + pl[2] * q[:, 2]
    s = s + pl[3]
    assert s.dtype == np.float32
    return np.abs(s)


def hypothesis(pts, seed, h, thr):
    """-> (count or None for a degenerate sample, plane, the sample's indices)"""
    m = len(pts)
    i0, i1, i2 = sample_triple(seed, h, m)
    if i0 == i1 or i0 == i2 or i1 == i2:
        return None, None, (i0, i1, i2)
    ok, pl = plane_from_3(pts[i0, :3], pts[i1, :3], pts[i2, :3])
    if not ok:
        return None, None, (i0, i1, i2)
    return int((plane_dist(pl, pts) < np.float32(thr)).sum()), pl, (i0, i1, i2)


def pcl_loop(pts, thr, seed, probability, max_it):
    """pcl::RandomSampleConsensus::computeModel's loop as orc_ransac_plane and the kernel run it
    -> (best_count, best_h, h_stop, iterations, skipped, counts): h_stop is the first hypothesis NOT drawn, counts[h] the inlier
    count of every drawn one (None: degenerate)."""
    m = len(pts)
    log_probability = math.log(1.0 - probability)
    one_over_indices = 1.0 / float(m)
    best, best_h, k, it, skip, h = 0, -1, 1.0, 0, 0, 0
    max_skip = 10 * max_it
    counts = []
    while it < k and skip < max_skip:
        cnt = hypothesis(pts, seed, h, thr)[0]
        counts.append(cnt)
        h += 1
        if cnt is None:
            skip += 1
            continue
        if cnt > best:
            best, best_h = cnt, h - 1
            w = best * one_over_indices
            p_no_outliers = 1.0 - w * w * w
            p_no_outliers = max(2.220446049250313e-16, p_no_outliers)
            p_no_outliers = min(1.0 - 2.220446049250313e-16, p_no_outliers)
            k = log_probability / math.log(p_no_outliers)
        it += 1
        if it > max_it:
            break
    return best, best_h, h, it, skip, counts


def fixed_best(pts, thr, seed, n_hyp):
    """ransac_probability <= 0: the most inliers of hypotheses [0, n_hyp), ties -> the lowest index -> (best_count, best_h)"""
    best, best_h = 0, -1
    for h in range(n_hyp):
        cnt = hypothesis(pts, seed, h, thr)[0]
        if cnt is not None and cnt > best:
            best, best_h = cnt, h
    return best, best_h


def behind_the_stop(pts, thr, seed, best, h_stop, width):
    """the hypotheses a round of `width` wavefronts scores BEHIND PCL's stop that have more inliers than the winner: [(h, count)]"""
    end = -(-h_stop // width) * width
    out = []
    for h in range(h_stop, end):
        cnt = hypothesis(pts, seed, h, thr)[0]
        if cnt is not None and cnt > best:
            out.append((h, cnt))
    return out


def classes(intensity, gz):
    """fetch_classes: 0 black (< gz0, tested first), 2 white (> gz1), 1 gray; the comparisons in double"""
    w = np.asarray(intensity, np.float32).astype(np.float64)
    black = w < gz[0]
    white = ~black & (w > gz[1])
    return np.where(black, 0, np.where(white, 2, 1)).astype(np.uint8)


# ------------------------------------------------------------------ lattices in the plane x = 2
def _cloud(xyz, inten):
    xyz64 = np.asarray(xyz, np.float64)
    out = np.concatenate([xyz64, np.asarray(inten, np.float64)[:, None]], axis=1).astype(np.float32)
    assert np.array_equal(out.astype(np.float64)[:, :3], xyz64)                 # every coordinate is a float32
    return np.ascontiguousarray(out)


def symmetric_lattice(n, step=1.0 / 32.0):
    """n >= 4 points of the plane x = 2 around CENTRE whose centroid is CENTRE and whose covariance is diagonal, exactly:
    quadruples (+-a, +-b) step, a in 1..8 and b in 1..4 (y extent twice the z extent), then a pair (+-9, 0) and the centre as
    n mod 4 asks"""
    assert 4 <= n <= 4 * 32 + 3
    quads = [(a, b) for a in range(8, 0, -1) for b in range(4, 0, -1)]
    yz = []
    for a, b in quads[:n // 4]:
        yz += [(a, b), (-a, -b), (a, -b), (-a, b)]
    if n % 4 >= 2:
        yz += [(9, 0), (-9, 0)]
    if n % 2:
        yz.append((0, 0))
    yz = np.array(yz, np.float64) * step
    return np.concatenate([np.zeros((n, 1)), yz], axis=1) + CENTRE


# A: the full 17 x 9 lattice and quadruples at distance thr, thr - 2^-21, thr + 2^-21 of the plane
A_OFFSETS = (THR_EXACT, THR_EXACT - 2.0 ** -21, THR_EXACT + 2.0 ** -21)
# input orders (permutation seeds; 0: as built) per mode: "adaptive", or the ransac_hyp of the fixed mode.  Under every one listed
# the winner is a hypothesis from three lattice points (in the fixed mode a tilted one through a quadruple point may collect more:
# those orders are left out of that mode); orders 0, 7, 20, 25, 29 have such a hypothesis, with fewer inliers, in FRONT of the winner
A_CASES = {"adaptive": (0, 1, 3, 7, 9, 16, 20, 25, 29), 1: (1, 3, 7, 9), 4: (0, 1, 3, 7, 20, 25, 29), 7: (0, 1, 3, 20, 25, 29),
           16: (0, 1, 3, 20, 25, 29), 17: (0, 1, 3, 20, 25, 29)}


def exact_plane_frame(order):
    """-> cloud, inlier mask.  153 lattice points (inliers), 3 quadruples (2 +- d, +-(y, z)) on the lattice's axes (their y z products vanish too): d = thr out, thr - 2^-21 in,
    thr + 2^-21 out.  Intensities 1 (y below the centre) / 7, one 0 and one 8: a gray zone of (3.4, 4.6) that holds nobody."""
    iy, iz = np.meshgrid(np.arange(-8, 9), np.arange(-4, 5), indexing="ij")
    yz = np.stack([iy.ravel(), iz.ravel()], axis=1) / 32.0
    pts = [np.concatenate([np.zeros((len(yz), 1)), yz], axis=1)]
    inl = [np.ones(len(yz), bool)]
    for d, (a, b) in zip(A_OFFSETS, ((5, 0), (7, 0), (0, 4))):
        pts.append(np.array([(sx * d, sy * a / 32.0, sy * b / 32.0) for sx in (1, -1) for sy in (1, -1)]))
        inl.append(np.full(4, d < THR_EXACT))
    xyz = np.concatenate(pts) + CENTRE
    inl = np.concatenate(inl)
    inten = np.where(xyz[:, 1] < CENTRE[1], 1.0, 7.0)
    inten[0], inten[1] = 0.0, 8.0
    perm = np.arange(len(xyz)) if order == 0 else np.random.default_rng(order).permutation(len(xyz))
    return _cloud(xyz[perm], inten[perm]), inl[perm]


# ------------------------------------------------------------------ B: noisy planes
B_THR = 0.03
B_P20 = 1.0 - 2.0 ** -20          # a ransac_probability under which the loop runs for about a round of 16
# data seeds of noisy_plane, picked with pcl_loop / behind_the_stop alone (tests: test_noisy_planes_stop_where_intended)
B_SEEDS = (71, 6, 4, 25, 42, 22, 16, 1300, 1748, 4278)
B_SEEDS_P20 = (43, 66, 75, 198, 180, 92)
B_HYP_CAPS = (1, 2, 3, 5)


def noisy_plane(seed, n=300, extent=(0.6, 0.4), sigma=0.5 * B_THR):
    """n points of a tilted plane about 2.5 m away, Gaussian noise of sigma along the normal; intensities 20 / 80 by half, with
    one 0 and one 100"""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.9, 0.3, -0.2])
    nrm /= np.linalg.norm(nrm)
    u = np.cross(nrm, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    a = rng.uniform(-0.5, 0.5, n) * extent[0]
    b = rng.uniform(-0.5, 0.5, n) * extent[1]
    xyz = np.array([2.5, 0.2, -0.1]) + a[:, None] * u + b[:, None] * v + rng.normal(0.0, sigma, n)[:, None] * nrm
    inten = np.where(a < 0.02, 20.0, 80.0)
    inten[0], inten[1] = 0.0, 100.0
    return np.ascontiguousarray(np.concatenate([xyz, inten[:, None]], axis=1).astype(np.float32))


# ------------------------------------------------------------------ C: a line and a few points off it
def line_frame(m, off):
    """m points of the plane x = 2: all on the line z = CENTRE.z (2^-7 apart along y) but those at the indices `off`, which sit
    1/8 or 1/4 m above it.  A sample is degenerate unless it holds a point of `off` (three points of the line: a cross product
    of exactly 0).  Intensities as in exact_plane_frame."""
    xyz = np.zeros((m, 3))
    xyz[:, 1] = (np.arange(m) - m // 2) / 128.0
    for k, i in enumerate(off):
        xyz[i, 2] = 0.125 * (1 + k % 2)
    xyz += CENTRE
    inten = np.where(np.arange(m) % 3 == 0, 7.0, 1.0)
    inten[0], inten[1] = 0.0, 8.0
    return _cloud(xyz, inten)


def line_frame_first_valid_at(h_first, seed, sizes=range(20, 96)):
    """-> (cloud, off) of the smallest m of `sizes` for which three indices `off` exist such that no sample before hypothesis
    h_first holds one of them, that hypothesis' sample holds exactly one and has no duplicate, and a sample before it has one"""
    for m in sizes:
        tr = [sample_triple(seed, h, m) for h in range(h_first + 1)]
        early = {i for t in tr[:h_first] for i in t}
        t = tr[h_first]
        if len(set(t)) < 3 or not any(len(set(s)) < 3 for s in tr[:h_first]):
            continue
        mine = [i for i in t if i not in early]
        free = [i for i in range(m) if i not in early and i not in t]
        if len(mine) >= 1 and len(free) >= 2:
            off = (mine[0], free[0], free[len(free) // 2])
            if sum(i in off for i in t) == 1:
                return line_frame(m, off), off
    raise AssertionError("no line frame for h_first %d" % h_first)


# ------------------------------------------------------------------ D: few inliers
D_THR = 2.0 ** -13


def twisted_curve(m=12):
    """m points of a moment curve, stretched: no plane through three of them passes within 8 thr of a fourth"""
    t = np.linspace(-1.0, 1.0, m) + 0.013 * np.sin(7.0 * np.arange(m))
    return np.stack([2.0 + 0.3 * t ** 3 - 0.09 * t, 0.36 * t, 0.27 * t ** 2 + 0.045 * t], axis=1).astype(np.float32).astype(np.float64)


def few_inliers_frame(seed, extra):
    """The twisted curve; with `extra` one more point, last, at the centroid of the first sample that does not hold it (a fourth
    inlier of that plane).  -> cloud, that sample's hypothesis, the plane's points.  They get intensities 0, 0, (0,) 8 in input
    order (hist_bins = 2 puts the one empty bin's edge above their mean), everybody else 3."""
    xyz = twisted_curve()
    m = len(xyz) + (1 if extra else 0)
    h = 0
    while len(set(sample_triple(seed, h, m))) < 3 or m - 1 in sample_triple(seed, h, m):
        h += 1
    tri = sample_triple(seed, h, m)
    if extra:
        c = xyz[list(tri)].mean(0).astype(np.float32).astype(np.float64)
        xyz = np.concatenate([xyz, c[None]])
    else:
        h, tri = 0, sample_triple(seed, 0, m)
        assert len(set(tri)) == 3
    members = sorted(set(tri) | ({m - 1} if extra else set()))
    inten = np.full(m, 3.0)
    inten[members] = 0.0
    inten[members[-1]] = 8.0
    return _cloud(xyz, inten), h, members


# ------------------------------------------------------------------ E: keep masks and sizes
E_SIZES = (3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
E_MASKS = ("all", "drop_first", "drop_last", "drop_lane0", "drop_lane63", "only_lane0", "only_lane63", "chunk_edges",
           "after256", "after1024", "after2048")
E_THR = 2.0 ** -14
E_BINS = 4096
E_ZONE = (1700.0, 2300.0)          # low = 500, high = 3500 at gray_rate 2.5
E_MIN_KEPT = 16
E_MINORITY = ("only_lane0", "only_lane63", "chunk_edges")   # as K3 masks they lose to any other plane unless hypothesis 0 is theirs:
E_MINORITY_SIZES = (1025, 2049, 4097)                      # a ransac_seed of its own per frame, so only at these sizes


def keep_mask(name, m):
    i = np.arange(m)
    return {"all": i >= 0, "drop_first": i != 0, "drop_last": i != m - 1, "drop_lane0": i % 64 != 0, "drop_lane63": i % 64 != 63,
            "only_lane0": i % 64 == 0, "only_lane63": i % 64 == 63,
            "chunk_edges": (i % 256 == 0) | (i % 256 == 255) | (i % 1024 == 1023),
            "after256": i >= 256, "after1024": i >= 1024, "after2048": i >= 2048}[name]


def e_cases():
    """(m, K3 mask, K5 mask): every size with everything kept; from 257 points up every mask once for K3's inliers and once for
    K5's labelled points, where it keeps at least E_MIN_KEPT points (a plane and both colours need some)"""
    out = [(m, "all", "all") for m in E_SIZES if m > 3]        # (three points: three_point_frame, with D's histogram)
    for m in E_SIZES:
        if m < 257:
            continue
        for name in E_MASKS[1:]:
            if int(keep_mask(name, m).sum()) >= E_MIN_KEPT:
                if name not in E_MINORITY or m in E_MINORITY_SIZES:
                    out.append((m, name, "all"))
                out.append((m, "all", name))
    return out


def three_point_frame():
    """the smallest cluster: three lattice points of the plane x = 2, intensities 0, 0, 8 (hist_bins = 2 as in few_inliers_frame)"""
    return _cloud(_sheet(3, 3), [0.0, 0.0, 8.0])


def _sheet(m, seed):
    """m distinct points of a 96 x 48 lattice of spacing 2^-7 in the plane x = 2, in a seeded order"""
    rng = np.random.default_rng(seed)
    cell = rng.permutation(96 * 48)[:m]
    yz = np.stack([cell // 48 - 48, cell % 48 - 24], axis=1) / 128.0
    return np.concatenate([np.zeros((m, 1)), yz], axis=1) + CENTRE


def _zone_intensities(keep):
    """Integer intensities for hist_bins = 4096 over [0, 4096] (bin width 1): the kept points 0, 4096, then 500 (black) and, every
    third, 3500 (white); the others gray, spread over 1700 .. 2300 -- BOTH ends included, which the strict tests must leave
    gray -- so that no gray bin outnumbers a peak.  low = 500, high = 3500: the zone is E_ZONE."""
    out = np.zeros(len(keep))
    j = np.arange(int(keep.sum()))
    out[keep] = np.where(j == 0, 0.0, np.where(j == 1, 4096.0, np.where(j % 3 == 0, 3500.0, 500.0)))
    g = np.arange(int((~keep).sum()))
    out[~keep] = 1700.0 + (g * 7) % 601
    return out


def mask_frame(m, k3_mask, k5_mask, seed):
    """-> cloud, K3's inlier mask over the cloud, K5's labelled mask over the inliers.  Inliers: lattice points of the sheet;
    the others lie 16 thr .. 0.2 m off it at random, spread so that no slab of 2 thr holds more than a few."""
    rng = np.random.default_rng(seed)
    inl = keep_mask(k3_mask, m)
    xyz = _sheet(m, seed)
    n_out = int((~inl).sum())
    dx = rng.uniform(16 * E_THR, 0.2, n_out) * rng.choice([-1.0, 1.0], n_out)
    xyz[~inl, 0] += dx
    xyz = xyz.astype(np.float32).astype(np.float64)
    lab = keep_mask(k5_mask, int(inl.sum()))
    inten = np.full(m, 2000.0)
    inten[inl] = _zone_intensities(lab)
    return _cloud(xyz, inten), inl, lab


def seed_whose_first_sample_is_kept(inl, xyz, start=0, block=1 << 18):
    """the first ransac_seed >= start whose hypothesis 0 samples three distinct kept points that are not collinear (the sheet
    then is hypothesis 0's plane, whatever the others do).  Only sample_index is evaluated, vectorised."""
    m = len(inl)
    for s0 in range(start, start + 64 * block, block):
        seeds = np.arange(s0, s0 + block, dtype=np.uint64)
        i = [sample_index(seeds, 0, k, m) for k in range(3)]
        ok = inl[i[0]] & inl[i[1]] & inl[i[2]] & (i[0] != i[1]) & (i[0] != i[2]) & (i[1] != i[2])
        for k in np.flatnonzero(ok):
            if plane_from_3(xyz[i[0][k]], xyz[i[1][k]], xyz[i[2][k]])[0]:
                return int(seeds[k])
    raise AssertionError("no seed found")


# ------------------------------------------------------------------ F: count patterns
F_BINS = 8


def pattern_intensities(counts):
    """per-bin counts c[0..8] (c[8]: the maximum's spare slot) -> intensities 0..8, bin by bin"""
    assert len(counts) == F_BINS + 1 and counts[0] >= 1 and counts[F_BINS] >= 1
    return np.repeat(np.arange(F_BINS + 1, dtype=np.float64), counts)


# by hand: (name, intensities)
_P = pattern_intensities
F_BY_HAND = (
    # bins 1 and 6 tie at 3: bin 1 alone stands for the count; the upper side comes from the count 2 (bin 5), not from bin 6
    ("tie_across_mean_other_count", _P([1, 3, 0, 0, 0, 2, 3, 0, 1])),
    # ... and with no other count above the mean there is no upper side at all
    ("tie_across_mean_degenerate", _P([1, 3, 0, 0, 0, 0, 3, 0, 1])),
    # the count 0 (first empty bin: 5) is the only representative above the mean 3.5
    ("empty_bin_is_the_upper_side", _P([1, 2, 3, 3, 3, 0, 2, 1, 1])),
    # the mean is 4, the edge of bin 4, whose count 3 is the largest: on neither side
    ("mean_on_the_top_bin_edge", _P([1, 2, 0, 0, 3, 0, 0, 2, 1])),
    # ... and with the other counts on both sides: low = 0 (count 2), high = 6 (count 1)
    ("mean_on_the_top_bin_edge_ok", _P([2, 0, 2, 0, 3, 0, 1, 2, 1])),
    # exact half bins: 2.5 rounds to bin 3 and 4.5 to bin 5 (away from zero), where they make the largest counts
    ("half_bins", np.array([0, 0, 2.5, 2.5, 2.5, 3, 1, 4.5, 4.5, 5, 5, 7, 8.0])),
    ("half_bins_both_sides", np.array([0, 1, 1, 2.5, 2.5, 2.5, 2.5, 4.5, 4.5, 4.5, 6, 6, 8.0])),
    # low = 1, high = 6: gz0 = 7.5 / 2.5 = 3 and gz1 = 10 / 2.5 = 4 exactly; the points at 3 and 4 are gray
    ("points_on_both_zone_ends", _P([1, 3, 0, 1, 1, 0, 2, 0, 1])),
)
F_RANDOM = 300


def random_patterns(n=F_RANDOM, seed=5):
    """n patterns of per-bin counts drawn from {0, 1, 2, 3} (the minimum's bin and the maximum's slot from {1, 2, 3}), at least 4 points"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = rng.integers(0, 4, F_BINS + 1)
        c[0], c[F_BINS] = max(c[0], 1), max(c[F_BINS], 1)
        if c.sum() >= 4:
            out.append(pattern_intensities(c))
    return out


def pattern_frame(inten, seed):
    """the intensities, in a seeded order, on the symmetric lattice of as many points"""
    inten = np.asarray(inten, np.float64)
    perm = np.random.default_rng(seed).permutation(len(inten))
    return _cloud(symmetric_lattice(len(inten)), inten[perm])


def histogram(inten, bins):
    """(hist[bins + 1], mean, bin width, minimum) as calHist computes them, in double"""
    d = np.sort(np.asarray(inten, np.float32).astype(np.float64))
    mn, mx = d[0], d[-1]
    factor = bins / (mx - mn)
    hist = np.zeros(bins + 1, np.int64)
    for v in d:
        hist[min(int(math.floor((v - mn) * factor + 0.5)), bins)] += 1
    return hist, sum(d.tolist()) / len(d), (mx - mn) / bins, mn


# the zone's ends themselves, at the default 100 bins: low = 10, high = 90, rate 2.5 -> 42 and 58 exactly
ZONE_ENDS_100 = np.array([0, 10, 10, 10, 10, 10, 41, 42, 42, 50, 58, 58, 59, 90, 90, 90, 90, 100.0])
