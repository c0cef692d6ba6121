"""The VALUES K6 computes -- rotate(), accumulate<OOB>, accumulate_interior, the tables of upload_tables -- held against an
operation-for-operation float32 restatement of the term (tests/grid_term_ref.py) on constructed frames (tests/constructed_costs.py).
The other constructed K6 suites assert decisions (argmin, rejected tiles, the form that ran); the two places that compare values
(test_gpu_parity's volume tests, test_locate_anchor) do so on random points with a tolerance and an exemption that one wrong point
per candidate fits into.

EXACT frames: points on multiples of 1/16 square, theta = 0, translation steps of 1/16 square -- every term and every partial sum
of a candidate is a float32, so the summation order cannot matter and the volume is asserted with `==` on the float32 BITS, in every
form the library computes it: ilcc_grid_cost with and without the volume, ilcc_grid_solve (staged, LDS-free), ilcc_debug_grid_solve_batch
(fresh handle: the OVERFLOW forms; reserved handle: the 512-thread instance; 65 and 512 frames: the separate locate launches and
k6_locate), ilcc_debug_locate.  The branches of the term sit in these frames: i or j an exact integer, both outlines of both axes,
exact half cells, R == delta, negative floors, frames without / with only interior-class points, a frame outside the board, one-colour
labels; boards 6 x 8 and 7 x 5 (as the library takes it: 5 wide, 7 high), tables 32 x 32, 30 x 29, 3 x 3, 1 x 1.
GENERAL frames (test_gpu_parity's random points, theta != 0): |volume - exact sum of the restated terms| <= (M + 2) 2^-24 S for
EVERY candidate, S the sum of the terms' magnitudes.  Derived, not measured: a lane adds its points by fmaf(T, w, A) with T w exact,
the four lanes of a quad meet in two more additions, the doubling is exact -- at most M + 2 roundings, each at most 2^-24 of a partial
sum of non-negative terms, which is at most S (in fact the lanes' sums are quarters: the real figure is near (M / 4 + 2) 2^-24 S).
A point on the wrong side of a branch costs a whole term, thousands of times the bound.

The CPU tests (no marker) establish the restatement: its fmaf against integer arithmetic; on every exact frame a three-way `==`
between the restatement, an integer evaluation of the functor's definition written here, and the fp64 oracle; the exactness
condition (every term a whole number of 2^-12, every candidate's sum below 2^24 of them) with integers; the general frames within
test_gpu_parity's oracle tolerance; and that six wrong variants of the restatement each change a candidate of the exact frames.

What they found: no kernel bug.  On an MI355X every exact candidate came out bit for bit, in every form; on the general frames the
largest |volume - exact| was 0.049 of the bound (M = 63; 0.004 at M = 2 500: the error grows like the lanes' quarter sums, as
derived), and the non-exact slices of the 21-theta frames stayed below 0.017 of it.  k6_locate's records all lay in the exact slice.
"""
import ctypes as C
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import constructed_costs as K
import constructed_points as cp
import grid_term_ref as T
from test_grid_backend_constructed import _cell, _i8, _nparams, _oparams

U = 2.0 ** -24


def _p(fields):
    return SimpleNamespace(**fields)


@functools.lru_cache(maxsize=None)
def _volume(kind, name, use_oob):
    """the restated volume of a frame: computed once, shared by the CPU and the GPU tests, never modified"""
    fr = {"exact": K.exact_frame, "produced": K.produced_frame, "general": K.general_frame}[kind](name)
    p = _p(dict(_default_term_fields(), **fr.fields))
    exact = (fr.exact_k, K.EXACT_UNIT_LOG2) if fr.exact_k is not None else None
    return fr, p, T.volume_ref(p, fr.yz, fr.lab, use_oob, exact=exact)


def _default_term_fields():
    """board and term fields of the default parameters (the general frames run on the default board)"""
    from oracle import binding
    d = binding.default_params()
    return dict(board_w=d.board_w, board_h=d.board_h, grid_length=d.grid_length, huber_delta=d.huber_delta)


# ================================================================================================================== CPU tests
def _round_f32(q):
    """a rational in float32's normal range, rounded to nearest even, as a Fraction"""
    if q == 0:
        return Fraction(0)
    e = 0
    a = abs(q)
    while a >= 2:
        a /= 2
        e += 1
    while a < 1:
        a *= 2
        e -= 1
    n = cp._rint_half_even(a * 2 ** 23)
    return (1 if q > 0 else -1) * Fraction(n) * Fraction(2) ** (e - 23)


def test_restated_fma_is_one_rounding():
    """fma32 == round(a b + c) in integer arithmetic: random triples, triples whose product nearly cancels c (the sum then holds
    bits far below float32's of either), and triples that put a b + c exactly between two float32 (the float64 detour of
    float32(float64(a) * b + c) rounds those twice)."""
    rng = np.random.default_rng(7)
    n = 4000
    a = rng.uniform(-8, 8, n).astype(np.float32)
    b = rng.uniform(-8, 8, n).astype(np.float32)
    c = rng.uniform(-64, 64, n).astype(np.float32)
    # cancelling: c = -float32(a b), so that a b + c is the product's own rounding error
    c[1000:2000] = -(a[1000:2000] * b[1000:2000])
    # ties: a b = 2^16 - 2^-30 (from (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46) and c = 2^40 + 2^17, whose last float32 bit is set: a b + c
    # lies 2^-30 BELOW the middle between c and the next float32, float64 rounds it onto that middle, and ties-to-even then goes up
    scale = 2.0 ** rng.integers(-20, 21, 1000)
    a[2000:3000] = (256.0 * (1 + 2.0 ** -23) * scale).astype(np.float32)
    b[2000:3000] = np.float32(256.0 * (1 - 2.0 ** -23))
    c[2000:3000] = ((2.0 ** 40 + 2.0 ** 17) * scale).astype(np.float32)
    got = T.fma32(a, b, c)
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    differ = 0
    for k in range(n):
        want = _round_f32(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert Fraction(float(got[k])) == want, (k, a[k], b[k], c[k], got[k])
        differ += Fraction(float(twice[k])) != want
    print("fma32: %d triples; the double-rounding detour is wrong on %d of them" % (n, differ))
    assert differ >= 1000   # (the ties are what the restatement's single rounding is for)


def _integer_volume(fr, use_oob):
    """The functor's definition at theta = 0 in int64 arithmetic, independent of the restatement and of the oracle (in the style of
    constructed_points.exact_cost_q): coordinates in sixteenths of a square; strictly inside the board a wrong-colour point pays
    its distance to the nearer border of its cell on both axes, a point not strictly inside pays its distance to the nearer outline
    on both axes (nothing without the out-of-board term); 1/2 rho(r^2) = r^2 / 2 up to delta, delta (r - delta / 2) beyond.
    -> int64 [n_ty, n_tz, 2] in units of 2^-9 (r in sixteenths: r^2 / 512; delta = 2 sixteenths: 2 (r - 1) / 256)"""
    p = _p(fr.fields)
    S = K.SUB
    W16, H16 = p.board_w * S, p.board_h * S
    y16 = np.rint(fr.yz[:, 0].astype(np.float64) / p.grid_length * S * 2).astype(np.int64)   # thirty-seconds: W / 2 may be a half square
    z16 = np.rint(fr.yz[:, 1].astype(np.float64) / p.grid_length * S * 2).astype(np.int64)
    assert np.array_equal(y16 / (2.0 * S) * p.grid_length, fr.yz[:, 0].astype(np.float64))
    ta = np.rint((p.ty_min + np.arange(p.n_ty) * p.ty_step) / p.grid_length * S).astype(np.int64)
    tb = np.rint((p.tz_min + np.arange(p.n_tz) * p.tz_step) / p.grid_length * S).astype(np.int64)
    i = (y16[:, None] + W16) // 2 + ta[None, :]          # [m, na]
    j = (z16[:, None] + H16) // 2 + tb[None, :]
    assert ((y16 + W16) % 2 == 0).all() and ((z16 + H16) % 2 == 0).all()
    d16 = int(round(p.huber_delta * S))
    assert d16 == 2
    out = np.zeros((p.n_ty, p.n_tz, 2), np.int64)
    lab = fr.lab.astype(np.int64)
    for lo in range(0, len(lab), 1024):
        s = slice(lo, lo + 1024)
        ii, jj = i[s][:, :, None], j[s][:, None, :]
        inside = (ii > 0) & (ii < W16) & (jj > 0) & (jj < H16)
        fi, fj = ii // S, jj // S
        ri, rj = ii - fi * S, jj - fj * S
        cell = np.minimum(ri, S - ri) + np.minimum(rj, S - rj)
        edge = np.minimum(np.abs(ii), np.abs(ii - W16)) + np.minimum(np.abs(jj), np.abs(jj - H16))
        odd = (fi + fj) & 1
        for phase in (0, 1):
            white = np.where(odd == 1, 1 - phase, phase)          # topleftWhite = phase: an even cell is white iff phase
            r = np.where(inside, np.where(lab[s][:, None, None] != white, cell, 0), edge if use_oob else 0)
            half_rho = np.where(r <= d16, r * r, 4 * (r - 1))     # units of 2^-9
            out[:, :, phase] += half_rho.sum(axis=0)
    return out


EXACT_CASES = [(n, o) for n in K.EXACT for o in (1, 0)]


def test_exact_frames_hold_what_they_claim():
    """the point counts asked for, both boards, the four tables; on the mixed frames a point ON each branch at translation 0"""
    assert tuple(sorted({K.EXACT[n][0] for n in K.EXACT} - {600})) == K.EXACT_M
    assert {K.EXACT[n][1] for n in K.EXACT} == {(6, 8), (5, 7)}
    assert {K.EXACT[n][2] for n in K.EXACT} == {(32, 32), (30, 29), (3, 3), (1, 1)}
    for name in ("m63", "m8192", "m8193", "m2049"):
        fr = K.exact_frame(name)
        p = _p(fr.fields)
        i, j = cp.board_coords(p, fr.yz, (0.0, 0.0, 0.0))
        W, H = p.board_w, p.board_h
        assert (i == 0).any() and (i == W).any() and (j == 0).any() and (j == H).any()
        assert ((i == np.rint(i)) & (i > 0) & (i < W)).any() and ((j == np.rint(j)) & (j > 0) & (j < H)).any()
        assert ((i % 1 == 0.5) & (j % 1 == 0.5)).any()
        inside = (i > 0) & (i < W) & (j > 0) & (j < H)
        dist = lambda v: np.abs(v - np.rint(v))
        assert (inside & (dist(i) + dist(j) == p.huber_delta)).any()
        assert (~inside & (np.minimum(np.abs(i), np.abs(i - W)) + np.minimum(np.abs(j), np.abs(j - H)) == p.huber_delta)).any()
        neg = (i < 0) & (j < 0)
        assert (neg & ((np.floor(i) + np.floor(j)) % 2 == 1)).any()
    for name, want in (("m64_no_interior", 0), ("m2833_no_interior", 0), ("m255_only_interior", 255)):
        fr = K.exact_frame(name)
        assert int(T.interior_class(_p(fr.fields), fr.yz).sum()) == want
    fr = K.exact_frame("m256_outside")
    p = _p(fr.fields)
    for ty in (p.ty_min, p.ty_min + (p.n_ty - 1) * p.ty_step):
        for tz in (p.tz_min, p.tz_min + (p.n_tz - 1) * p.tz_step):
            i, j = cp.board_coords(p, fr.yz, (0.0, ty, tz))
            assert ((i < 0) | (i > p.board_w) | (j < 0) | (j > p.board_h)).all()
    assert K.exact_frame("m1023_white").lab.all() and not K.exact_frame("m1024_black").lab.any()


@pytest.mark.parametrize("name,use_oob", EXACT_CASES)
def test_exact_frames_three_ways(ob, name, use_oob):
    """On the exact slice of every exact frame: the restated volume == the integer evaluation of the functor == the fp64 oracle's
    volume; every restated term is a whole number of 2^-12 (asserted inside volume_ref) and every candidate's sum -- half its
    cost -- is below 2^24 of them, with integers: the condition under which any fp32 summation order gives the exact sum."""
    fr, p, vol = _volume("exact", name, use_oob)
    k = fr.exact_k
    units = T.term_units(vol.num[k], K.EXACT_UNIT_LOG2 + 1)   # cost in 2^-13 = the candidate's sum (cost / 2) in 2^-12
    top = max(int(v) for v in units.ravel())
    print("frame %s use_oob %d: M %d, %d interior class, largest candidate sum %d units of 2^-12 (2^24 = %d)" %
          (name, use_oob, len(fr.lab), int(vol.interior.sum()), top, 1 << 24))
    assert top < (1 << 24)
    integer = _integer_volume(fr, use_oob)
    assert (T.term_units(vol.num[k], 9) == integer.astype(object)).all()
    op = _oparams(ob, fr.fields)
    assert op.th_min + k * op.th_step == 0.0
    _, _, ovol = ob.grid_search(fr.yz[:, 0], fr.yz[:, 1], _i8(fr.lab), op, use_oob, want_volume=True)
    ovol = ovol.reshape(p.n_th, p.n_ty, p.n_tz, 2)
    assert np.array_equal(ovol[k], integer.astype(np.float64) * 2.0 ** -9)
    assert np.array_equal(ovol[k], vol.val[k])
    T.float32_bits(vol.num[k])   # (every candidate's value is a float32)


@pytest.mark.parametrize("name", list(K.PRODUCED))
def test_produced_frames_have_one_minimum_in_the_exact_slice(ob, name):
    """The frames sent through the production entries: exact on the slice theta = 0 (three ways, as above); the minimum of that
    slice is unique and the runner-up, in any slice, lies more than 1e-3 (relative) above it -- fifty near-tie windows: neither
    the fp32 order of another slice's sums ((M + 2) 2^-24 S, subtracted here) nor K7r's recount of near ties can move the argmin."""
    fr, p, vol = _volume("produced", name, 1)
    k = fr.exact_k
    assert (T.term_units(vol.num[k], 9) == _integer_volume(fr, 1).astype(object)).all()
    assert max(int(v) for v in T.term_units(vol.num[k], K.EXACT_UNIT_LOG2 + 1).ravel()) < (1 << 24)
    _, _, ovol = ob.grid_search(fr.yz[:, 0], fr.yz[:, 1], _i8(fr.lab), _oparams(ob, fr.fields), 1, want_volume=True)
    assert np.array_equal(ovol.reshape(vol.val.shape)[k], vol.val[k])
    flat = T.argmin_ref(p, vol.val)
    low = vol.val * (1.0 - (len(fr.lab) + 2) * U)
    low[k] = vol.val[k]
    low.reshape(-1)[flat] = np.inf
    best = vol.val.reshape(-1)[flat]
    print("frame %s: argmin %s phase %d cost %.6f, runner-up +%.3f %%" % (name, _cell(p, flat), flat & 1, best, 100 * (low.min() / best - 1)))
    assert _cell(p, flat)[0] == k and best > 0 and low.min() > (1.0 + 1e-3) * best


@pytest.mark.parametrize("m", K.GENERAL_M)
@pytest.mark.parametrize("use_oob", [1, 0])
def test_restatement_within_the_oracle_tolerance_on_general_frames(ob, m, use_oob):
    """test_grid_cost_volume_matches_oracle's comparison, with the restatement in the kernel's place"""
    fr, p, vol = _volume("general", m, use_oob)
    op = cp.apply_fields(ob.default_params(), fr.fields)
    _, _, ovol = ob.grid_search(fr.yz[:, 0], fr.yz[:, 1], _i8(fr.lab), op, use_oob, want_volume=True)
    err = np.abs(vol.val.reshape(-1) - ovol)
    bad = err > 2e-5 * np.abs(ovol) + 2e-6
    print("general M %d use_oob %d: %d of %d candidates beyond the tolerance, largest error %.3g" % (m, use_oob, bad.sum(), bad.size, err.max()))
    assert bad.mean() <= (0.002 if use_oob else 0.0), (bad.sum(), err.max())
    assert err[bad].max(initial=0.0) < 0.5


MUTANT_FRAMES = ("m63", "m65_one_candidate", "m255_only_interior", "m600_3x3", "m1_outline")


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_wrong_restatements_change_a_candidate(mutant):
    """Non-vacuity: `>= 0` read as `> 0` on the outline, the parity taken without hw, min(R, delta) dropped, accumulate_interior
    used for a border-class point, the last point left out, the last table entry clamped one short -- each changes at least one
    candidate of the exact frames (looked for on the small ones)."""
    changed = []
    for name in MUTANT_FRAMES:
        for use_oob in (1, 0):
            fr, p, vol = _volume("exact", name, use_oob)
            wrong = T.volume_ref(p, fr.yz, fr.lab, use_oob, mutant=mutant)
            n = int((wrong.num != vol.num).sum())
            if n:
                changed.append((name, use_oob, n))
    print("mutant %s changes: %s" % (mutant, changed))
    assert changed


# ================================================================================================================== GPU tests
MAX_POINTS = 8448


@pytest.fixture(scope="module")
def est():
    from lidar_camera_calibration_amd import LidarCornersBatch
    e = LidarCornersBatch(1, MAX_POINTS, _nparams())
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits1(x):
    """the bits of one float32"""
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _assert_within_order(got, vol, ks, what):
    """|got - exact| <= (M + 2) 2^-24 S on the slices ks; -> the largest ratio to the bound"""
    worst = 0.0
    for k in ks:
        S = vol.val[k]
        err = np.abs(got[k].astype(np.float64) - S)
        bound = (vol.n_points + 2) * U * S
        assert (err <= bound).all(), (what, k, float((err - bound).max()), np.argwhere(err > bound)[:4])
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,use_oob", EXACT_CASES)
def test_exact_volumes(est, name, use_oob):
    """A.  ilcc_grid_cost's volume on the exact slice == the exact values, as float32 bits, every candidate, no tolerance; the other
    slices of a 21-theta table within what the order allows; best_index == argmin_ref of the volume, best_cost == its bits there;
    the call without a volume (the pruned launch) returns the same index and the same bits."""
    fr, p, vol = _volume("exact", name, use_oob)
    est.set_params(_nparams(fr.fields))
    bi, bc, got = est.grid_cost(fr.yz, fr.lab, bool(use_oob), want_volume=True)
    got = got.reshape(p.n_th, p.n_ty, p.n_tz, 2)
    k = fr.exact_k
    want = T.float32_bits(vol.num[k])
    diff = _bits(got[k]) != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4], got[k][diff][:4], want[diff][:4].view(np.float32))
    others = [q for q in range(p.n_th) if q != k]
    if others:
        print("frame %s use_oob %d: other slices at most %.3f of the bound" % (name, use_oob, _assert_within_order(got, vol, others, name)))
    flat = T.argmin_ref(p, got)
    assert bi == flat and _bits1(bc) == _bits1(got.reshape(-1)[flat]), (bi, flat, bc)
    bi2, bc2, _ = est.grid_cost(fr.yz, fr.lab, bool(use_oob), want_volume=False)
    assert (bi2, _bits1(bc2)) == (bi, _bits1(bc)), (bi2, bc2, bi, bc)


@pytest.mark.gpu
@pytest.mark.parametrize("m", K.GENERAL_M)
@pytest.mark.parametrize("use_oob", [1, 0])
def test_general_volumes_within_what_the_order_allows(est, m, use_oob):
    """B.  Every candidate: |volume - exact sum of the restated float32 terms| <= (M + 2) 2^-24 S.  None exempt."""
    fr, p, vol = _volume("general", m, use_oob)
    est.set_params(_nparams(fr.fields))
    _, _, got = est.grid_cost(fr.yz, fr.lab, bool(use_oob), want_volume=True)
    worst = _assert_within_order(got.reshape(p.n_th, p.n_ty, p.n_tz, 2), vol, range(p.n_th), "general %d" % m)
    print("general M %d use_oob %d: largest |volume - exact| / ((M + 2) 2^-24 S) = %.4f" % (m, use_oob, worst))


@functools.lru_cache(maxsize=None)
def _want(name):
    """-> (argmin_ref, the exact cost's float32 bits there) of a produced frame"""
    fr, p, vol = _volume("produced", name, 1)
    flat = T.argmin_ref(p, vol.val)
    return flat, int(T.float32_bits(vol.num[fr.exact_k]).reshape(-1)[flat - fr.exact_k * p.n_ty * p.n_tz * 2])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(K.PRODUCED))
def test_grid_solve_publishes_the_exact_cost(est, name):
    """C.  ilcc_grid_solve (staging sized to the frame; 8 193 points: the LDS-free form): grid_index == argmin_ref, grid_cost == the
    exact value there, bit for bit."""
    fr = K.produced_frame(name)
    est.set_params(_nparams(fr.fields))
    got = est.grid_solve(fr.yz, fr.lab)
    flat, bits = _want(name)
    assert got["grid_index"] == flat and _bits1(got["grid_cost"]) == bits, (got, flat, np.array([bits], np.uint32).view(np.float32))


def _batch(n_frames, names, reserve=None, mode=None):
    from lidar_camera_calibration_amd import LidarCornersBatch
    frames, picks = K.batch_of(n_frames, names)
    total = sum(len(lab) for _, lab in frames)
    e = LidarCornersBatch(n_frames, total // n_frames + 1, _nparams(K.PRODUCTION))
    try:
        if mode is not None:
            e.debug_full_pass_launch(*mode)
        fresh = e.grid_solve_batch(frames)
        out = [fresh]
        if reserve:
            e.reserve(reserve, 0)
            out.append(e.grid_solve_batch(frames))
    finally:
        e.close()
    return picks, out


def _assert_batch(picks, got, lds_points):
    assert got["lds_points"] == lds_points
    assert (got["valid"] == 1).all()
    for f, name in enumerate(picks):
        flat, bits = _want(name)
        assert int(got["grid_index"][f]) == flat and _bits1(got["grid_cost"][f]) == bits, (f, name, got["grid_index"][f], got["grid_cost"][f], flat)


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [65, 512])
def test_batches_publish_the_exact_cost(n_frames):
    """C.  ilcc_debug_grid_solve_batch on a fresh handle at its 1 024 staged points (1 025 and 2 833 points: the full pass's OVERFLOW
    forms) and again reserved at 3 072 (the 512-thread instance); 65 frames: the three locate launches, 512: k6_locate.  The
    8 193-point frame (no walk layout) rides in the batch of 65."""
    from lidar_camera_calibration_amd import _native as N
    names = [n for n in K.PRODUCED if n != "p8193" or n_frames == 65]
    picks, (fresh, reserved) = _batch(n_frames, names, reserve=3072)
    _assert_batch(picks, fresh, 1024)
    _assert_batch(picks, reserved, 3072)
    want = N.LOCATE_FUSED if n_frames >= 512 else N.LOCATE_LAUNCHES
    assert fresh["locate"] == want and reserved["locate"] == want, (fresh["locate"], reserved["locate"])


@pytest.mark.gpu
def test_forced_full_pass_forms_publish_the_exact_cost():
    """C.  The full pass forced into its (n_th, F) form and into its listed form with 1 and 7 workgroups (the rest of the list then
    falls to k6_grid_cost_listed_rest), on the batch of 65: the same exact costs."""
    from lidar_camera_calibration_amd import _native as N
    for mode in ((N.FULL_PASS_GRID, 0), (N.FULL_PASS_LISTED, 1), (N.FULL_PASS_LISTED, 7)):
        picks, (fresh,) = _batch(65, list(K.PRODUCED), mode=mode)
        assert fresh["full_pass"] == mode[0], (mode, fresh["full_pass"])
        _assert_batch(picks, fresh, 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [0, 3072])
def test_locate_record_holds_the_exact_cost(reserve):
    """C.  ilcc_debug_locate (k6_locate's anchor: every labelled point of the frame, from LDS or from global memory): the record's
    cost == the exact value at its flat index where that lies in the exact slice -- `==`, where test_locate_anchor allows kTieEps --
    and within what the order allows elsewhere; the bound word holds those bits."""
    from lidar_camera_calibration_amd import LidarCornersBatch
    from lidar_camera_calibration_amd import _native as N
    names = [n for n in K.PRODUCED if n != "p8193"]
    frames, picks = K.batch_of(8, names)
    counts = [len(lab) for _, lab in frames]
    offsets = np.zeros(len(frames) + 1, np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    yz = np.ascontiguousarray(np.concatenate([a for a, _ in frames]), np.float32)
    lab = np.ascontiguousarray(np.concatenate([b for _, b in frames]), np.uint8)
    rec, bound = np.zeros((len(frames), 4), np.uint32), np.zeros(len(frames), np.uint32)
    u8, u32, u64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    e = LidarCornersBatch(len(frames), 4096, _nparams(K.PRODUCTION))
    try:
        if reserve:
            e.reserve(reserve, 0)
        st = e._lib.ilcc_debug_locate(e._h, N.fptr(yz), lab.ctypes.data_as(u8), offsets.ctypes.data_as(u64), len(frames),
                                      rec.ctypes.data_as(u32), bound.ctypes.data_as(u32))
        assert st == N.OK, e._err()
    finally:
        e.close()
    in_slice = 0
    for f, name in enumerate(picks):
        fr, p, vol = _volume("produced", name, 1)
        flat = int(rec[f, 2])
        assert flat != 0xFFFFFFFF and bound[f] == rec[f, 0], (f, name, rec[f], bound[f])
        k = _cell(p, flat)[0]
        cost = rec[f, 0:1].view(np.float32)[0]
        if k == fr.exact_k:
            in_slice += 1
            assert int(rec[f, 0]) == int(T.float32_bits(vol.num[k]).reshape(-1)[flat - k * p.n_ty * p.n_tz * 2]), (f, name, rec[f], cost)
        else:
            S = vol.val.reshape(-1)[flat]
            assert abs(float(cost) - S) <= (len(fr.lab) + 2) * U * S, (f, name, cost, S)
    print("locate records (reserve %d): %d of %d in the exact slice" % (reserve, in_slice, len(picks)))
    assert in_slice >= 1
