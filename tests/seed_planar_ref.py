"""The specification of the planar seeds (K15p, include/ilcc_seed.h) in numpy.  Quantisation, grid, `measure` and `finish` are
tests/seed_ref.py's; the rest is restated here: per-cell and block sums and their translation in Python integers (object
arrays), one `float()` per covariance entry, eig3_sym operation for operation, the three tests in the header's order, and the
26-connected components of the core cells.  The GPU's integer records must equal `components` exactly.

eig3_sym is restated twice: `eig3_sym` on Python floats, which reads like csrc/eig3.h, and `eig3_sym_many`, the same
operations on float64 arrays with one lane per matrix and every branch of the scalar code as a mask (IEEE binary64
+ - x / sqrt either way, so the two agree bit for bit: tests/test_seed_planar_cpu.py holds them together).  `classify` uses the
second, so that a whole scan takes a fraction of a second."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import seed_ref as R


@dataclasses.dataclass
class PlanarParams:
    """ilcc_default_seed_planar_params for the default ilcc_params"""
    planar_rms: float = 0.03
    min_spread: float = 0.06
    own_rms: float = 0.02


def default_params(**kw) -> R.SeedParams:
    """the SeedParams half of ilcc_default_seed_planar_params: max_rms 0.05"""
    base = dict(max_rms=0.05)
    base.update(kw)
    return R.SeedParams(**base)


def frame_fits(n_points: int, g: R.Grid) -> bool:
    return n_points * 2 * g.cq < (1 << 31)


def eig3_sym(a_in):
    """csrc/eig3.h on Python floats: a_in 9 floats row-major -> (w ascending [3], v [3][3], v[c] = unit eigenvector c)"""
    a = [[a_in[3 * i + j] for j in range(3)] for i in range(3)]
    q = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(64):
        off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
        diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2]
        if off <= 1e-32 * diag or off == 0.0:
            break
        for pp in range(2):
            for qq in range(pp + 1, 3):
                if a[pp][qq] == 0.0:
                    continue
                theta = (a[qq][qq] - a[pp][pp]) / (2.0 * a[pp][qq])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = a[k][pp], a[k][qq]
                    a[k][pp] = c * akp - s * akq
                    a[k][qq] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = a[pp][k], a[qq][k]
                    a[pp][k] = c * apk - s * aqk
                    a[qq][k] = s * apk + c * aqk
                for k in range(3):
                    qkp, qkq = q[k][pp], q[k][qq]
                    q[k][pp] = c * qkp - s * qkq
                    q[k][qq] = s * qkp + c * qkq
    order = [0, 1, 2]
    d = [a[0][0], a[1][1], a[2][2]]
    for i in range(2):
        for j in range(2 - i):
            if d[order[j]] > d[order[j + 1]]:
                order[j], order[j + 1] = order[j + 1], order[j]
    w, v = [], []
    for c in range(3):
        w.append(d[order[c]])
        nrm = 0.0
        for k in range(3):
            nrm += q[k][order[c]] * q[k][order[c]]
        nrm = math.sqrt(nrm)
        v.append([q[k][order[c]] / nrm for k in range(3)])
    return w, v


def eig3_sym_many(a_in: np.ndarray):
    """eig3_sym on [M, 9] float64: -> (w [M, 3], v [M, 3, 3]).  `live` are the matrices that have not left the sweep loop."""
    m = len(a_in)
    a = [[a_in[:, 3 * i + j].astype(np.float64).copy() for j in range(3)] for i in range(3)]
    q = [[np.full(m, 1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    live = np.ones(m, bool)
    with np.errstate(all="ignore"):
        for _ in range(64):
            off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2]
            diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2]
            live = live & ~((off <= 1e-32 * diag) | (off == 0.0))
            if not live.any():
                break
            for pp in range(2):
                for qq in range(pp + 1, 3):
                    do = live & (a[pp][qq] != 0.0)
                    theta = (a[qq][qq] - a[pp][pp]) / (2.0 * a[pp][qq])
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c

                    def put(dst, val):
                        dst[do] = val[do]

                    for k in range(3):
                        akp, akq = a[k][pp].copy(), a[k][qq].copy()
                        put(a[k][pp], c * akp - s * akq)
                        put(a[k][qq], s * akp + c * akq)
                    for k in range(3):
                        apk, aqk = a[pp][k].copy(), a[qq][k].copy()
                        put(a[pp][k], c * apk - s * aqk)
                        put(a[qq][k], s * apk + c * aqk)
                    for k in range(3):
                        qkp, qkq = q[k][pp].copy(), q[k][qq].copy()
                        put(q[k][pp], c * qkp - s * qkq)
                        put(q[k][qq], s * qkp + c * qkq)
        d = np.stack([a[0][0], a[1][1], a[2][2]], 1)
        order = np.tile(np.arange(3), (m, 1))
        rows = np.arange(m)
        for i in range(2):
            for j in range(2 - i):
                swap = d[rows, order[:, j]] > d[rows, order[:, j + 1]]
                oj = order[:, j].copy()
                order[swap, j] = order[swap, j + 1]
                order[swap, j + 1] = oj[swap]
        qm = np.stack([np.stack(row, 1) for row in q], 1)            # [M, k, column]
        w = np.zeros((m, 3))
        v = np.zeros((m, 3, 3))
        for c in range(3):
            col = order[:, c]
            w[:, c] = d[rows, col]
            e = [qm[rows, k, col] for k in range(3)]
            nrm = np.zeros(m)
            for k in range(3):
                nrm = nrm + e[k] * e[k]
            nrm = np.sqrt(nrm)
            for k in range(3):
                v[:, c, k] = e[k] / nrm
    return w, v


def _translate(mom, o):
    """the ten moments (columns: n, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz; Python integers) about the origins o [cells, 3]"""
    n, s = mom[:, 0], [mom[:, 1], mom[:, 2], mom[:, 3]]
    out = [n] + [s[a] - n * o[:, a] for a in range(3)]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for k, (a, b) in enumerate(pairs):
        out.append(mom[:, 4 + k] - o[:, a] * s[b] - o[:, b] * s[a] + n * o[:, a] * o[:, b])
    return out


@dataclasses.dataclass
class Cells:
    key: np.ndarray      # int64 [cells], ascending
    index: np.ndarray    # int64 [cells, 3]: the cell index per axis, 0 .. N-1 (offset included)
    mom: np.ndarray      # object [cells, 10]: Python integers
    core: np.ndarray     # bool [cells]
    keep: np.ndarray     # over the cloud's points
    cell_of_point: np.ndarray   # per kept point: row of its cell


def cell_moments(cloud, g: R.Grid):
    keep, q = R.quantise(cloud, g)
    idx = q // g.cq + g.off
    key = idx[:, 0] + g.N * (idx[:, 1] + g.N * idx[:, 2])
    ukey, inv = np.unique(key, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    starts = np.nonzero(np.diff(inv[order], prepend=-1))[0]
    qo = q[order].astype(object)
    cols = [np.ones(len(qo), np.int64).astype(object), qo[:, 0], qo[:, 1], qo[:, 2], qo[:, 0] * qo[:, 0], qo[:, 0] * qo[:, 1],
            qo[:, 0] * qo[:, 2], qo[:, 1] * qo[:, 1], qo[:, 1] * qo[:, 2], qo[:, 2] * qo[:, 2]]
    mom = np.stack([np.add.reduceat(c, starts) for c in cols], 1) if len(qo) else np.zeros((0, 10), object)
    index = np.stack([ukey % g.N, (ukey // g.N) % g.N, ukey // (g.N * g.N)], 1) if len(ukey) else np.zeros((0, 3), np.int64)
    return ukey, index, mom, keep, inv


def classify(cloud, pp: PlanarParams, g: R.Grid) -> Cells:
    key, index, mom, keep, inv = cell_moments(cloud, g)
    m = len(key)
    if m == 0:
        return Cells(key, index, mom, np.zeros(0, bool), keep, inv)
    block = np.zeros((m, 10), object)
    for d in range(27):
        j = index + [d % 3 - 1, (d // 3) % 3 - 1, d // 9 - 1]
        inside = ((j >= 0) & (j < g.N)).all(1)                    # outside the grid: skipped, never wrapped
        jkey = j[:, 0] + g.N * (j[:, 1] + g.N * j[:, 2])
        at = np.minimum(np.searchsorted(key, jkey), m - 1)
        found = inside & (key[at] == jkey)
        block[found] += mom[at[found]]
    o = ((index - g.off) * g.cq).astype(object)
    tb, to = _translate(block, o), _translate(mom, o)
    nb_i = tb[0]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    c6 = [nb_i * tb[4 + k] - tb[1 + a] * tb[1 + b] for k, (a, b) in enumerate(pairs)]
    assert all(abs(int(v)) < (1 << 63) for col in c6 for v in col)
    f = [np.array([float(v) for v in col]) for col in c6]         # one conversion each, round to nearest
    cov = np.stack([f[0], f[1], f[2], f[1], f[3], f[4], f[2], f[4], f[5]], 1)
    w, v = eig3_sym_many(cov)
    flat_q2 = (1024.0 * pp.planar_rms) * (1024.0 * pp.planar_rms)
    spread_q2 = (1024.0 * pp.min_spread) * (1024.0 * pp.min_spread)
    own_q2 = (1024.0 * pp.own_rms) * (1024.0 * pp.own_rms)
    as_f = lambda col: np.array([float(x) for x in col])
    nb = as_f(nb_i)
    nb2 = nb * nb
    flat = w[:, 0] <= nb2 * flat_q2
    surface = 12.0 * w[:, 1] >= nb2 * spread_q2
    no = as_f(to[0])
    mc = [as_f(tb[1 + a]) / nb for a in range(3)]
    sd = [as_f(to[1 + a]) for a in range(3)]
    ss6 = [as_f(to[4 + k]) for k in range(6)]
    ssd = [[ss6[0], ss6[1], ss6[2]], [ss6[1], ss6[3], ss6[4]], [ss6[2], ss6[4], ss6[5]]]
    v0 = [v[:, 0, k] for k in range(3)]
    r = []
    for a in range(3):
        A = [((ssd[a][e] - mc[a] * sd[e]) - mc[e] * sd[a]) + (no * mc[a]) * mc[e] for e in range(3)]
        r.append((A[0] * v0[0] + A[1] * v0[1]) + A[2] * v0[2])
    quad = (v0[0] * r[0] + v0[1] * r[1]) + v0[2] * r[2]
    own = quad <= no * own_q2
    return Cells(key, index, mom, flat & surface & own, keep, inv)


def components(cloud, sp: R.SeedParams, pp: PlanarParams, g: R.Grid | None = None, want_cells: bool = False):
    """Records of the core components of at least sp.cluster_min points, sorted by key: lists of 11 Python ints."""
    g = g or R.grid(sp)
    cells = classify(cloud, pp, g)
    recs = []
    if cells.core.any():
        idx = cells.index[cells.core]
        lo = idx.min(0)
        occ = np.zeros(tuple(int(x) for x in idx.max(0) - lo + 1), bool)
        occ[tuple((idx - lo).T)] = True
        lab, n_lab = R._label(occ)
        clab = lab[tuple((idx - lo).T)]
        ckey, cmom = cells.key[cells.core], cells.mom[cells.core]
        for label in range(1, n_lab + 1):
            sel = clab == label
            sums = cmom[sel].sum(0)
            if int(sums[0]) >= sp.cluster_min:
                recs.append([int(ckey[sel].min())] + [int(x) for x in sums])
        recs.sort(key=lambda r: r[0])
    return (recs, cells) if want_cells else recs


def propose(cloud, sp: R.SeedParams, pp: PlanarParams, g: R.Grid | None = None):
    recs = components(cloud, sp, pp, g)
    if len(recs) > sp.max_components:
        return None                                    # ILCC_CAPACITY for the frame
    return R.finish(recs, sp)
