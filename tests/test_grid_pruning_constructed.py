"""K6's PRUNING -- the frame's bound from the locate launches, the per-tile box pre-pass (box_term / box_prepass_rounds), the common
pre-pass of a group of 7 thetas (k6_group_prepass) with the candidate cut behind them -- on CONSTRUCTED points where the bounds are
TIGHT (tests/constructed_bounds.py): fenced boards whose argmin sits on the corner of its 4 x 4 tile towards which the fence pulls,
so that the tile's box bound over the sampled rim points EQUALS the argmin's cost / 2 in real arithmetic and the tile survives by
kBoxSafety against 1 + kTieEps alone.  The rest of the suite meets the pruning only where a rejected tile's bound is many times
the minimum, or where every limit is exactly 0.

The CPU tests (no marker) establish that the inputs are what the GPU tests take them for, with the oracle's cost volume and the fp64
restatements alone.  The GPU tests run the pipeline's GRID solver on each case, compare it with the oracle, with its own cut-free
run, and read what the common pre-pass left behind (LidarCornersBatch.fetch_group_prepass): no rejected tile may hold a candidate
within the near-tie window of the minimum, and every rejected tile's restated bound must exceed the limit.

Families: A the four tile corners; B partial tiles (n_ty = 30, n_tz = 29: last tiles 2 and 1 candidates wide; argmin in the last
tiles, argmin at table index 0); C theta groups (th_step = 2^-12; n_th = 21 with the argmin at the first / middle / last theta of a
group, 15 = 7 + 7 + 1, 8 = 7 + 1, 6 = no common pre-pass; A is the loose contrast at the dyadic th_step); D sample edges
(border-class point counts 0, 1, 47, 48, 49, 64, 65); E
rim points far from the rotation centre on either side of the `wide` threshold; F exact ties across tiles (the set united with its
half turn); G the 512-thread instance and a frame too large for the walk layout.

Where a case could not meet a condition as first intended, the condition is asserted in the form given here, and the figures
are printed by the tests:
  * C and D (th_step = 2^-12): a theta step moves no point of a 6 x 8 board by 2^-10 square (at most 3.65 squares x 2^-12 rad), so
    consecutive thetas cost the same to a few 1e-5 (relative) until a point crosses a cell border: the cost has PLATEAUS in theta,
    8 to 17 thetas long here, and the argmin is the end of one (the fence's cost is monotone along it).  There the runner-up is
    the neighbouring theta, +0.0035 %: "at least 1 % above" is asserted for the candidates at other translations and for the
    thetas off the plateau; the point about to cross lies 3.4e-4 (C) / 7.8e-4 (D) square from its border, not 2^-10: asserted
    as >= 1e-4, the margin of test_grid_backend_constructed (25 x ILCC_FLAG_BORDER_RISK's window); and a plateau's costs run
    across the edge of the near-tie window, so the window condition below is not asserted for them.  The COMMON bound of the
    argmin's tile reaches 0.998 of cost / 2 (7 thetas spread a fence point by 0.2 % of its distance), not 1 - 2^-13: these
    cases are tight for a workgroup's own pre-pass (1.0), which is what `tight` asserts everywhere, and nearly so for the common
    one.  C15_single, C8_single: the argmin is the last, single theta of its group.
  * "the last theta of the group left out": no tight case can reject its tile through this mutant (a bound over 6 of 7 thetas
    exceeds the right one only by the spread that tightness forbids), so it is looked for where it shows, in the GPU's own
    output: check (d) recomputes every rejected tile's bound over ALL thetas of its group.  A fifth mutant, the clamp of a
    partial tile one entry short, stands in for the box extremes where the last tile is 2 or 1 candidates wide (B_last).
  * ILCC_FLAG_BORDER_RISK looks at the 26 grid neighbours of the argmin too: the distance kept there is 1e-5 square (2.5 x its
    window; 8 274 points under 18 poses keep no more), and 2^-10 at the argmin itself.
  * F: the half turn (y, z) -> (-y, -z) maps (th, ty, tz) to (th, -ty, -tz): the exact tie lies in another TILE of the same
    theta group (no symmetry of the term maps th to -th exactly in floating point).  Each fence gets three points the board
    swallows on its way out (without them the two fences' costs, both linear, cancel over the whole plateau).
  * "no candidate within relative 2^-13 of (1 + kTieEps) min" cannot hold as written (the minimum itself lies 2e-5 below that
    value): asserted as "every candidate is either within HALF the window above the minimum, or more than 2^-13 beyond its edge".
  * G: ilcc_grid_solve sizes the staging to its frame, so the full pass's OVERFLOW form (more points than the staging holds, still a
    walk layout) is out of its reach; G_global is a frame too large for the walk layout itself (every group in state 2).
  * D_0, D_1 have no fence at all (the minimum is 0 on a plateau, as in test_zero_cost_plateaus): all points interior, and all but one.
  * Non-vacuity (half of the tiles rejected against 4 x the minimum) is asserted for the tight cases, over all border-class
    points; D, E and F print their figure.
  * (b): grid_solve's `ties`, and ILCC_FLAG_TIE_OVERFLOW which is that count against kTieCap, follow the history of the frame's
    bound (every candidate that lowers it is listed) and differ from run to run: D_64 listed 241 and 277 in two pruned runs, 451
    cut-free, with one real near tie.  Every other field is compared.  D_49 and D_64 show a loose bound behind the locate
    launches (hundreds of candidates lower it in turn): a finding about the locate bound, not about soundness.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import constructed_bounds as cb
import constructed_points as cp
from test_grid_backend_constructed import _assert_downstream, _cell, _flags, _i8, _nparams, _oparams, _solve_case   # noqa: F401

FINE = 2.0 ** -12             # C's theta step
S_ALLOW = 2.0 ** -11          # (d)'s allowance, derived in test_pruned_solve_matches_the_oracle_and_rejects_only_losers's docstring
MAX_POINTS = 8448


def _grid(a0=16, b0=16, **kw):
    """the dyadic grid with table index (a0, b0) at translation 0 (the points are at pose (0, 0, 0)), other fields replaced"""
    f = cp.dyadic_params()
    f.update(ty_min=-a0 * 2.0 ** -6, tz_min=-b0 * 2.0 ** -6)
    f.update(kw)
    return f


def _fine(n_th, k0, **kw):
    return _grid(th_step=FINE, n_th=n_th, th_min=-k0 * FINE, **kw)


def _fenced(corner, **kw):
    return lambda op: cb.fenced_board(op, corner, **kw)[:2]


def _subset(border, seed=5):
    """D: the hh fenced board with 10 points per cell, cut down to all its interior-class points and `border` border-class ones:
    the 10 fence points (none when border < 10: the minimum is then 0 on a plateau) and in-board points of the other border class"""
    def build(op):
        yz, lab, n_in = cb.fenced_board(op, "hh", K=10, seed=seed)
        cls, _ = cb.walk_classes(op, yz)
        fence = np.arange(n_in, len(lab))
        assert (cls[fence] == 2).all() and not (cls[:n_in] == 2).any()
        other = np.random.default_rng(seed).permutation(np.where(cls[:n_in] == 1)[0])
        if border < len(fence):   # no fence at all: a noise-free board, the minimum is 0
            fence = fence[:0]
        keep = np.concatenate([np.where(cls == 0)[0], fence, other[:border - len(fence)]])
        keep.sort()
        return yz[keep], lab[keep]
    return build


def _far(seed=1):
    """E: the hh fenced board and 8 rim points 0.98 ... 1.7 squares outside the low j outline (4.98 ... 5.7 squares from the rotation
    centre), on the side of the pull: the images of the first four under the 7 thetas of a dyadic group lie less than half a
    square apart, those of the last four more"""
    def build(op):
        yz, lab, _ = cb.fenced_board(op, "hh", seed=seed)
        r = np.array([4.98, 5.05, 5.12, 5.19, 5.52, 5.58, 5.64, 5.7])
        i = 4.2 + 0.01 * np.arange(len(r))
        far = cp.from_board(op, i, op.board_h / 2 - r)
        return np.concatenate([yz, far]), np.concatenate([lab, (np.arange(len(r)) & 1).astype(np.uint8)])
    return build


def _tied(seed=1):
    def build(op):
        yz, lab, _ = cb.fenced_board(op, "hh", seed=seed, inner=(3, 2.5 / 16))
        return cb.half_turn_union(yz, lab)
    return build


_SMALL = dict(n_th=9, th_min=-4 * 2.0 ** -6, n_ty=16, n_tz=16)   # G: 9 x 16 x 16 candidates, groups of 7 and 2

# name: fields, build(op) -> (yz, lab), designed argmin (k, a, b, phase), and what the case is for:
#   tight: "own" -- the argmin's tile has box bound == cost / 2 for its own theta; mutants: the wrong bounds that must reject that tile
#   gap: "1pct" runner-up >= 1 % above; "plateau" (C) see the module docstring; "tie" (F); "zero" the minimum is 0 on a plateau
#   fence: rim points the case is designed to have (None: not a fenced case)
CASES = {
    "A_hh": dict(fields=_grid(16, 16), build=_fenced("hh", seed=1), argmin=(10, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10),
    "A_ll": dict(fields=_grid(15, 15), build=_fenced("ll", seed=1), argmin=(10, 12, 12, 0), tight="own", mutants=("low_late", "inflated"), fence=10),
    "A_hl": dict(fields=_grid(16, 15), build=_fenced("hl", seed=1), argmin=(10, 19, 12, 0), tight="own", mutants=("high_short", "low_late", "inflated"), fence=10),
    "A_lh": dict(fields=_grid(15, 16), build=_fenced("lh", seed=1), argmin=(10, 12, 19, 0), tight="own", mutants=("high_short", "low_late", "inflated"), fence=10),
    "B_last": dict(fields=_grid(26, 25, n_ty=30, n_tz=29), build=_fenced("hh", seed=2), argmin=(10, 29, 28, 0), tight="own",
                   mutants=("clamp_short", "inflated"), fence=10),
    "B_first": dict(fields=_grid(3, 3, n_ty=30, n_tz=29), build=_fenced("ll", seed=2), argmin=(10, 0, 0, 0), tight="own",
                    mutants=("low_late", "inflated"), fence=10),
    "B_inner": dict(fields=_grid(16, 16, n_ty=30, n_tz=29), build=_fenced("hh", seed=2), argmin=(10, 19, 19, 0), tight="own",
                    mutants=("high_short", "inflated"), fence=10),
    "C21_first": dict(fields=_fine(21, 2), build=_fenced("hh", seed=8), argmin=(7, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "C21_middle": dict(fields=_fine(21, 5), build=_fenced("hh", seed=8), argmin=(10, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "C21_last": dict(fields=_fine(21, 8), build=_fenced("hh", seed=8), argmin=(13, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "C15_single": dict(fields=_fine(15, 9), build=_fenced("hh", seed=8), argmin=(14, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "C8_single": dict(fields=_fine(8, 2), build=_fenced("hh", seed=8), argmin=(7, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "C6_none": dict(fields=_fine(6, 0), build=_fenced("hh", seed=8), argmin=(5, 19, 19, 0), tight="own", mutants=("high_short", "inflated"), fence=10, gap="plateau"),
    "D_0": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(0), argmin=None, gap="zero", border=0),
    "D_1": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(1), argmin=None, gap="zero", border=1),
    "D_47": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(47), argmin=(20, 19, 19, 0), border=47, fence=10, gap="plateau"),
    "D_48": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(48), argmin=(20, 19, 19, 0), border=48, fence=10, gap="plateau"),
    "D_49": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(49), argmin=(20, 19, 19, 0), border=49, fence=10, gap="plateau"),
    "D_64": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(64), argmin=(20, 19, 19, 0), border=64, fence=10, gap="plateau"),
    "D_65": dict(fields=_fine(21, 10, n_ty=24, n_tz=24), build=_subset(65), argmin=(20, 19, 19, 0), border=65, fence=10, gap="plateau"),
    "E_far": dict(fields=_grid(16, 16), build=_far(1), argmin=(10, 19, 19, 0), fence=18),
    "F_tied": dict(fields=_grid(16, 16), build=_tied(1), argmin=(10, 13, 19, 0), gap="tie", fence=32),
    "G_large": dict(fields=_grid(16, 16, n_th=9, th_min=-4 * 2.0 ** -6), build=_fenced("hh", seed=13, K=48, n_fence=30), argmin=(4, 19, 19, 0), tight="own",
                    mutants=("high_short", "inflated"), fence=60),
    "G_global": dict(fields=_grid(8, 8, **_SMALL), build=_fenced("hh", seed=17, K=168, n_fence=105), argmin=(4, 11, 11, 0), fence=210),
}
TIGHT = [n for n, c in CASES.items() if c.get("tight")]


@functools.lru_cache(maxsize=None)
def _ref(ob, name):
    """the case's points, the oracle's whole cost volume and argmin, the restated classes and sample: computed once, shared by the
    CPU and the GPU tests, never modified"""
    case = CASES[name]
    op = _oparams(ob, case["fields"])
    yz, lab = case["build"](op)
    flat, cost, vol = ob.grid_search(yz[:, 0], yz[:, 1], _i8(lab), op, 1, want_volume=True)
    vol = vol.reshape(op.n_th, op.n_ty, op.n_tz, 2)
    M = len(lab)
    layout = M <= cb.K_GRID_LDS_POINTS_MAX
    order, Mi, n_rim = cb.walk_layout(op, yz) if layout else (np.zeros(0, np.int64), 0, 0)
    cls, margin = cb.walk_classes(op, yz)
    n_pre = cb.group_sample_size(M, Mi, cb.solve_lds_points(M)) if layout else 0
    for a in (yz, lab, vol, order, cls, margin):
        a.setflags(write=False)
    k, a, b = _cell(op, flat)
    return SimpleNamespace(case=case, op=op, yz=yz, lab=lab, flat=flat, cost=cost, vol=vol, M=M, layout=layout, order=order, Mi=Mi, n_rim=n_rim,
                           cls=cls, margin=margin, n_pre=n_pre, sample=yz[order[Mi:Mi + n_pre]], argmin=(k, a, b, flat & 1),
                           tile=(a // cb.K_TILE, b // cb.K_TILE), groups=cb.theta_groups(op.n_th))


def _limit(r):
    """what a tile's bound is compared with: half the near-tie window's edge above the oracle's minimum"""
    return 0.5 * (1.0 + cb.K_TIE_EPS) * r.cost


def _group_of(r, k):
    return [g for g in r.groups if k in g][0]


def _tile_min(r, ks, tile):
    """the cheapest candidate (either phase) of a tile over the thetas ks, the tile clipped to the table"""
    qa, qb = tile
    return float(r.vol[ks[0]:ks[-1] + 1, qa * cb.K_TILE:(qa + 1) * cb.K_TILE, qb * cb.K_TILE:(qb + 1) * cb.K_TILE, :].min())


# ================================================================================================================== CPU tests
@pytest.mark.parametrize("name", list(CASES))
def test_case_argmin_gap_and_window(ob, name):
    """The oracle's exhaustive argmin is where the case is designed to put it; the runner-up is at least 1 % above it (C, D: among
    the candidates at other translations, and a theta at the argmin's translation is either on the plateau or 1 % above; F: but
    for the exact tie; D_0, D_1: a zero-cost plateau); and, but for the plateau cases, every candidate is either within half the
    near-tie window above the minimum or more than 2^-13 (relative) beyond the window's edge -- no fp32 sum can move a candidate
    across the edge."""
    r = _ref(ob, name)
    gap = r.case.get("gap", "1pct")
    srt = np.sort(r.vol.ravel())
    print("case %s: M %d, oracle argmin %s cost %.6f, runner-up +%.4f %%, third +%.4f %%" %
          (name, r.M, r.argmin, r.cost, 100 * (srt[1] / srt[0] - 1) if srt[0] > 0 else 0.0, 100 * (srt[2] / srt[0] - 1) if srt[0] > 0 else 0.0))
    if r.case["argmin"] is not None:
        assert r.argmin == r.case["argmin"]
    if gap == "zero":
        assert r.cost == 0.0
        return
    assert r.cost > 0.0
    k, a, b, _ = r.argmin
    if gap == "1pct":
        assert srt[1] >= 1.01 * srt[0]
    elif gap == "tie":
        mirror = (k, 2 * cb.tables(r.op)[4][1] - a, 2 * cb.tables(r.op)[4][2] - b)
        assert r.vol[mirror].min() == r.cost and srt[1] == srt[0] and srt[2] >= 1.01 * srt[0]
        assert (mirror[1] // 4, mirror[2] // 4) != r.tile
    else:   # "plateau": other translations 1 % above; a theta at the argmin's translation is on the plateau (within 1e-3) or 1 % above
        other = r.vol.copy()
        other[:, a, b, :] = np.inf
        prof = r.vol[:, a, b, r.argmin[3]] / r.cost - 1.0
        print("   theta plateau at the argmin's translation: thetas %s, up to +%.1e" % (np.where(prof < 1e-3)[0], prof[prof < 1e-3].max()))
        assert other.min() >= 1.01 * r.cost and ((prof < 1e-3) | (prof >= 0.01)).all()
        return
    edge = (1.0 + cb.K_TIE_EPS) * r.cost
    v = r.vol.ravel()
    assert not ((v > (1.0 + 0.5 * cb.K_TIE_EPS) * r.cost) & (v <= edge * (1.0 + 2.0 ** -13))).any()


@pytest.mark.parametrize("name", list(CASES))
def test_case_points_keep_their_distance_from_every_threshold(ob, name):
    """No point within 2^-10 square of a cell border at the argmin (ILCC_FLAG_BORDER_RISK must stay clear: its window is 4e-6), of
    the threshold that decides its class, or -- the sampled points, over every theta group -- of the `wide` threshold; the fence is
    exactly the rim class and fits the common pre-pass's sample; the border-class count is the one D asks for; and the fp32
    rounding of the sample's terms stays below 2^-13 of the limit (the allowance s of check (d))."""
    r = _ref(ob, name)
    k, a, b, _ = r.argmin
    x = (r.op.th_min + k * r.op.th_step, r.op.ty_min + a * r.op.ty_step, r.op.tz_min + b * r.op.tz_step)
    i, j = cp.board_coords(r.op, r.yz, x)
    border = min(np.abs(i - np.rint(i)).min(), np.abs(j - np.rint(j)).min())
    # what the flag really looks at (k7r first_round_is_settled): the 3 thetas x (3 + 3) axis translations around the argmin, a window of
    # 4e-6 square where fp32 and fp64 coordinates agree to ~1e-6: 1e-5 clears it (no set of 8 000 points keeps more under 18 poses)
    around = 1.0
    for dk in (-1, 0, 1):
        for d in (-1, 0, 1):
            if 0 <= k + dk < r.op.n_th:
                ni, nj = cp.board_coords(r.op, r.yz, (r.op.th_min + (k + dk) * r.op.th_step, r.op.ty_min + (a + d) * r.op.ty_step, r.op.tz_min + (b + d) * r.op.tz_step))
                around = min(around, np.abs(ni - np.rint(ni)).min() if 0 <= a + d < r.op.n_ty else 1.0, np.abs(nj - np.rint(nj)).min() if 0 <= b + d < r.op.n_tz else 1.0)
    if r.cost > 0.0:
        assert around >= 1e-5, around
    wide_margin = 1.0
    for g in r.groups:
        if len(g) > 1 and r.n_pre:
            lo_i, hi_i, lo_j, hi_j, _, _ = cb.point_intervals(r.op, r.sample, g)
            wide_margin = min(wide_margin, np.abs(np.concatenate([hi_i - lo_i, hi_j - lo_j]) - cb.K_WIDE).min())
    print("case %s: nearest cell border %.2e (under the 26 neighbours %.2e), class threshold %.2e, wide threshold %.2e square; Mi %d rim %d sample %d" %
          (name, border, around, r.margin.min(), wide_margin, r.Mi, r.n_rim, r.n_pre))
    # (a plateau case's argmin is the last theta before a point crosses a cell border, and a step of 2^-12 rad moves no point of this
    # board by 2^-10 square: there the margin is that of test_grid_backend_constructed, 1e-4 = 25 x the flag's window)
    assert border >= (1e-4 if r.case.get("gap") == "plateau" else 2.0 ** -10) and r.margin.min() >= 2.0 ** -10 and wide_margin >= 2.0 ** -10
    if r.case.get("fence") is not None and r.layout:
        i0, j0 = cp.board_coords(r.op, r.yz, (0.0, 0.0, 0.0))
        outside = (i0 < 0) | (i0 > r.op.board_w) | (j0 < 0) | (j0 > r.op.board_h)
        assert r.n_rim == r.case["fence"] and np.array_equal(outside, r.cls == 2)
        assert r.n_rim <= r.n_pre
    if "border" in r.case:
        assert r.M - r.Mi == r.case["border"]
    if r.cost > 0.0 and r.layout:
        # |dT / dR| <= delta, a term is T / 2, and fp32 moves R by less than 2^-18 square (five roundings of values below 8 per axis)
        assert r.n_pre * 0.5 * r.op.huber_delta * 2.0 ** -18 <= 2.0 ** -13 * 0.5 * r.cost


def test_far_points_lie_on_either_side_of_the_wide_threshold(ob):
    """E: of the 8 far rim points, the restatement leaves at least two out of every theta group's bound and keeps at least two in,
    each 0.5 +- 0.05 square wide; all 8 are in the sample."""
    r = _ref(ob, "E_far")
    far = np.arange(r.M - 8, r.M)
    pos = {int(v): n for n, v in enumerate(r.order[r.Mi:r.Mi + r.n_pre])}
    assert all(int(f) in pos for f in far)
    for g in r.groups:
        _, _, _, _, wide, spread = cb.point_intervals(r.op, r.yz[far], g)
        print("E_far group %s: spreads %s" % (g[0] // 7, np.array2string(spread, precision=3)))
        assert wide.sum() >= 2 and (~wide).sum() >= 2 and (np.abs(spread - cb.K_WIDE) <= 0.05).all()


@pytest.mark.parametrize("name", TIGHT)
def test_tight_cases_are_tight_and_tell_the_mutants_apart(ob, name):
    """The box bound of the argmin's tile at the argmin's theta, over the sample the common pre-pass takes, is at least
    (1 - 2^-13) cost / 2 -- and does not reject the tile by the kernel's own rule (bound x kBoxSafety > limit) -- while each of the
    case's mutants does: a box extreme one table step short or late, a clamp one entry short, a bound inflated by 2^-10.  The
    common bound over the argmin's whole theta group is printed; in C (th_step = 2^-12) it must stay within the loss the spread of
    7 thetas allows: delta x 2 axes x 6 steps x 2^-12 x 5 squares per rim point."""
    r = _ref(ob, name)
    k = r.argmin[0]
    own = cb.box_bound(r.op, r.sample, [k], r.tile)
    grp = cb.box_bound(r.op, r.sample, _group_of(r, k), r.tile)
    mut = {m: cb.box_bound(r.op, r.sample, [k], r.tile, m) for m in r.case["mutants"]}
    print("case %s: tightness own %.6f, group of %d thetas %.6f; mutants %s" %
          (name, own / (0.5 * r.cost), len(_group_of(r, k)), grp / (0.5 * r.cost), {m: "%.5f" % (v / (0.5 * r.cost)) for m, v in mut.items()}))
    assert own >= (1.0 - 2.0 ** -13) * 0.5 * r.cost
    assert not own * cb.K_BOX_SAFETY > _limit(r) and not grp * cb.K_BOX_SAFETY > _limit(r)
    for m, v in mut.items():
        assert v * cb.K_BOX_SAFETY > _limit(r), m
    if name.startswith("C"):
        assert grp >= 0.5 * r.cost - r.n_rim * 0.5 * r.op.huber_delta * 2 * 6 * FINE * 5.0


def test_every_extreme_mutant_is_caught_by_two_tight_cases():
    for m in ("high_short", "low_late", "inflated"):
        assert sum(m in CASES[n]["mutants"] for n in TIGHT) >= 2, m
    assert any("clamp_short" in CASES[n]["mutants"] for n in TIGHT)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.get("fence") and n != "G_global"])
def test_box_bound_rejects_half_of_the_tiles(ob, name):
    """Non-vacuity, for every tight case: at the argmin's theta the restated bound over all the border-class points (the most a
    pre-pass's sample can hold) exceeds even 4 x the limit for at least half of the tiles.  Printed for the other fenced cases: D cuts
    the border class down to a few dozen points on purpose, E's far points and F's second fence double the minimum itself."""
    r = _ref(ob, name)
    nta, ntb = cb.axis_tiles(r.op.n_ty), cb.axis_tiles(r.op.n_tz)
    border = r.yz[r.order[r.Mi:]]
    rejected = sum(cb.box_bound(r.op, border, [r.argmin[0]], (qa, qb)) * cb.K_BOX_SAFETY > 4.0 * _limit(r) for qa in range(nta) for qb in range(ntb))
    print("case %s: %d of %d tiles rejected against 4 x the minimum" % (name, rejected, nta * ntb))
    if r.case.get("tight"):
        assert 2 * rejected >= nta * ntb


# ================================================================================================================== GPU tests
@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, MAX_POINTS, _nparams())
    yield e
    e.close()


def _record(got):
    """grid_solve's record but for what the suite knows to depend on timing (test_front_end_launches.TIMING_DEPENDENT_FIELDS,
    tests/sequence_cases.py): how many candidates the full pass LISTED as near ties -- every candidate that lowers the frame's bound
    when it completes is listed, so the count follows the bound's history -- and the overflow flag, which is that count against
    kTieCap.  D_64: 241 listed by the pruned run, 451 (ILCC_FLAG_TIE_OVERFLOW) by the cut-free one, 1 real near tie."""
    tie_overflow, _ = _flags()
    return {k: (tuple(int(x) for x in v) if k == "lat" else v & ~tie_overflow if k == "flags" else v) for k, v in got.items() if k != "ties"}


def _near_ties(r):
    """candidates, the argmin included, within HALF the near-tie window of the oracle's minimum: whatever fp32 does to their sums
    (1e-6), the full pass must have listed them"""
    return int((r.vol <= (1.0 + 0.5 * cb.K_TIE_EPS) * r.cost).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pruned_solve_matches_the_oracle_and_rejects_only_losers(ob, est, name):
    """(a) test_grid_backend_constructed's _solve_case: everything downstream of the grid argmin == the oracle, and the argmin IS
    the oracle's, ILCC_FLAG_BORDER_RISK clear.  (b) The record with grid_prune = 0 == the record with grid_prune = 1, field for
    field.  (c) The walk layout's class sizes (and the layout itself) == the restatement.  (d) Of every tile the common pre-pass
    rejected (a state-0 group: all): no candidate of it, either phase, any theta of the group, costs <= (1 + kTieEps) x the
    oracle's minimum; and with the kernel's own sample walk_yz[Mi : Mi + n_pre], box_bound x (1 + s) > 0.5 (1 + kTieEps) minimum.
    (e) A group that must have no common pre-pass -- one theta, no border-class point, a frame without walk layout -- reports
    state 2; a grid of fewer than 7 thetas reports no groups.  (f) Tight cases: the argmin's group has at least one rejected tile
    (the locate bound was good enough for the pre-pass to engage).

    s = 2^-11.  The kernel rejects on fl(sum) x (1 - 2^-12) > fl(0.5 (1 + kTieEps) bound).  fl(sum) of <= 4096 non-negative fp32
    terms, in any order, is at most (1 + 2^-12) x their real sum: kBoxSafety cancels that.  The bound word is the fp32 cost of a
    complete candidate, a sum of <= 4096 non-negative terms: at least (1 - 2^-12) x its real cost >= (1 - 2^-12) x the minimum:
    2^-12.  The fp32 terms of the sample differ from the fp64 restatement's by less than 2^-13 of the limit (asserted per case
    by the CPU test above), and the roundings of the constants and of the two products are a few 2^-24: together below another
    2^-12.  kBoxSafety itself is 2^-12: the kernel's allowance for its own sum only."""
    from lidar_camera_calibration_amd import _native as N
    r = _ref(ob, name)
    _, border_risk = _flags()
    est.set_params(_nparams(dict(r.case["fields"], grid_prune=1)))
    got, same = _solve_case(ob, est, r.op, r.yz, r.lab)                                                    # (a)
    assert same and got["grid_index"] == r.flat and not (got["flags"] & border_risk), (got, r.flat)
    wyz, wlab, Mi, n_rim = est.fetch_solve_walk()
    gp = est.fetch_group_prepass()
    est.set_params(_nparams(dict(r.case["fields"], grid_prune=0)))
    assert est.fetch_group_prepass()["groups"] == 0
    free = est.grid_solve(r.yz, r.lab)                                                                     # (b)
    print("case %s: ties %d (flags %d) pruned, %d (flags %d) cut-free; candidates within half the window of the oracle's minimum: %d" %
          (name, got["ties"], got["flags"], free["ties"], free["flags"], _near_ties(r)))
    assert _record(free) == _record(got)
    assert min(got["ties"], free["ties"]) >= _near_ties(r) - 1
    assert (Mi, n_rim) == (r.Mi, r.n_rim)                                                                  # (c)
    if r.layout:
        assert np.array_equal(wyz, r.yz[r.order]) and np.array_equal(wlab, r.lab[r.order])
    else:
        assert len(wyz) == 0
    if r.case.get("gap") == "tie":
        assert got["ties"] >= 1
    # (e)
    if r.op.n_th < cb.K_THETA_GROUP:
        assert gp["groups"] == 0
        return
    assert gp["groups"] == len(r.groups) and gp["words"] == (cb.axis_tiles(r.op.n_ty) * cb.axis_tiles(r.op.n_tz) + 31) // 32
    no_prepass = not r.layout or r.M == r.Mi
    for g, st in zip(r.groups, gp["states"]):
        assert (st == 2) == (no_prepass or len(g) == 1), (g, st)
    # (d)
    dead = cb.dead_tiles(gp["states"], gp["mask"], r.op.n_ty, r.op.n_tz)
    sample = wyz[Mi:Mi + r.n_pre]
    edge = (1.0 + cb.K_TIE_EPS) * r.cost
    for g, d in zip(r.groups, dead):
        print("case %s group %d (thetas %d-%d): state %d, %d of %d tiles rejected" % (name, g[0] // 7, g[0], g[-1], gp["states"][g[0] // 7], d.sum(), d.size))
        for qa, qb in zip(*np.nonzero(d)):
            assert _tile_min(r, g, (qa, qb)) > edge, (g, qa, qb)
            assert cb.box_bound(r.op, sample, g, (qa, qb)) * (1.0 + S_ALLOW) > 0.5 * edge, (g, qa, qb)
    k, a, b, _ = r.argmin
    assert not dead[k // cb.K_THETA_GROUP, a // cb.K_TILE, b // cb.K_TILE]
    if r.case.get("gap") == "tie":
        c_ty, c_tz = cb.tables(r.op)[4][1:]
        assert not dead[k // cb.K_THETA_GROUP, (2 * c_ty - a) // cb.K_TILE, (2 * c_tz - b) // cb.K_TILE]
    # (f)
    if r.case.get("tight") and gp["states"][k // cb.K_THETA_GROUP] != 2:
        assert dead[k // cb.K_THETA_GROUP].any()
