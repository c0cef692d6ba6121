"""tests/structure_ref.py, the independent fp64 restatement of structure recovery, bound to the host code
(csrc/image_corners_host.cpp) seed by seed and bit for bit, and what it proves about the constructed cases of structure_cases.py
before any GPU test relies on them: each tie case exercises the tie rule it is named for, is DECISIVE (the plausible wrong rule gives
another seed board or final answer) and LIBM-PROOF (nothing changes when atan2 / cos / sin are off by their OpenCL full-profile
bounds: one offset per function in all sign combinations, then a sign per call hashed from its arguments); each overlap case shows its event; each count case straddles a 64-bit word of K18's used set.

"row_first" is offered as a wrong rule of assignClosestCorners and is none: both orders take a tied set's lexicographic minimum, the
two minima are equal or share neither row nor column, and by induction over the set either order ends with the same assignment.
test_row_major_order_is_the_same_rule holds that against the restatement.  The wrong rule that shows is the LAST minimum."""
import struct

import numpy as np
import pytest

import structure_cases as S
import structure_ref as R
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import image_sequence as IS

BOUND = ["A", "B", "C", "H", "I", "K", "L", "E", "F", "Z", "N", "M", "W"] + S.EDGE_CASES      # J and the 4 096-corner lists are left to the host

_ref = {}


def ref(name):
    """the restatement's Result under the contract's rules, once per case"""
    if name not in _ref:
        c = S.case(name)
        _ref[name] = R.chessboards_from_corners(c.corners, c.board)
    return _ref[name]


def host(c):
    try:
        return N.OK, IC.chessboard_from_corners(c.corners, c.board)
    except IC.BoardNotFound as e:
        return e.status, None


def host_with(name, board):
    return IC.chessboard_from_corners(S.case(name).corners, board)


def same_board(a, b):
    return (a is None) == (b is None) and (a is None or (a.shape == b.shape and np.array_equal(a, b)))


def assert_seed(name, seed, got, want):
    assert same_board(got[0], want[0]), (name, seed, got[0], want[0])
    assert struct.pack("<d", got[1]) == struct.pack("<d", want[1]), (name, seed, got[1], want[1])


@pytest.mark.parametrize("name", BOUND)
def test_the_restatement_equals_the_host_on_every_seed_and_in_the_final_answer(name):
    c, r = S.case(name), ref(name)
    for seed in range(len(c.corners)):
        got = r.seeds[seed]
        if got[0] is not None and got[0].size > IS.MAX_CORNERS:        # more cells than the host's stage output holds: it says so
            with pytest.raises(IS.ImageSequenceError) as e:
                IS.seed_board(c.corners, seed)
            assert e.value.status == N.CAPACITY and name in ("W", "S65x4")
            continue
        assert_seed(name, seed, got, IS.seed_board(c.corners, seed))
    st, idx = host(c)
    assert st == c.status == r.status and same_board(r.index, idx)
    assert c.shape is None or idx.shape == c.shape
    print(name, r.trace.summary())


def test_the_capacity_cases_reach_the_capacities():
    tr = {name: ref(name).trace for name in S.CAPACITY_CASES + ["W"]}
    # the capacities exactly: an accepted row border of 64 predictions that makes 256 cells
    assert tr["S64x4"].max_side == 64 and tr["S64x4"].max_predicted == 64 and tr["S64x4"].max_proposed == 256 == IS.MAX_CORNERS
    assert tr["S65x4"].max_predicted == 65 and tr["S65x4"].max_proposed == 260        # above both
    assert tr["S80x3"].max_side == 3 and tr["S80x3"].max_predicted <= 64 and ref("S80x3").index.shape == (3, 80)        # by borders of three alone
    assert tr["M_strays"].max_proposed == 272 == tr["W"].max_proposed and ref("M_strays").index.shape == (16, 16)


@pytest.mark.parametrize("name,rule,least", [
    ("T_dup", "neighbor", 5), ("T_dup", "assign", 5), ("T_dup", "overlap", 5),
    ("T_grid", "neighbor", 3), ("T_grid", "assign", 10), ("T_mid", "assign", 3), ("T_border", "border", 5), ("T_equal", "overlap", 5), ("T_equal", "border", 5)])
def test_a_tie_case_meets_the_tie_it_is_named_for(name, rule, least):
    tr = ref(name).trace
    assert tr.ties[rule] >= least and len(tr.tie_seeds[rule]) >= min(least, 3), tr.summary()


def test_the_mirrored_pairs_of_the_exact_lattice_are_equidistant_and_the_lower_index_is_taken():
    c, r = S.case("T_grid"), ref("T_grid")
    u, v = c.corners["u"], c.corners["v"]
    right = [k for k in range(len(u)) if u[k] == 704 and v[k] in (350, 354)]
    below = [k for k in range(len(u)) if v[k] == 416 and u[k] in (606, 610)]
    assert len(right) == 2 and len(below) == 2
    assert r.status == N.OK and r.index.shape == (5, 6)
    cells = set(r.index.reshape(-1).tolist())
    assert min(right) in cells and max(right) not in cells and min(below) in cells and max(below) not in cells
    assert r.seeds[r.stored[0]][1] == -30 + 30 * (4.0 / 64.0)        # exactly: every other collinearity error is 0


def test_the_midway_corner_goes_to_the_lower_of_its_two_predictions():
    c, r = S.case("T_mid"), ref("T_mid")
    u, v = c.corners["u"], c.corners["v"]
    mid = [k for k in range(len(u)) if (u[k], v[k]) == (688.0, 384.0)]        # 16 px from the predictions (672, 384) and (704, 384)
    off = [k for k in range(len(u)) if (u[k], v[k]) == (720.0, 385.0)]
    assert len(mid) == 1 and len(off) == 1
    assert r.status == N.OK and r.index.shape == (4, 6)
    assert r.index[3, 4] == mid[0] and r.index[3, 5] == off[0] and [u[k] for k in r.index[3, :4]] == [544.0, 576.0, 608.0, 640.0]
    e = r.seeds[r.stored[0]][1]
    assert e == -24 + 24 * (16.0 / np.sqrt(64.0 ** 2 + 16.0 ** 2)) and e < -18        # the accepted step: a 3 x 6 board stands at -18
    last = R.chessboards_from_corners(c.corners, c.board, rules={"assign": "last"})        # the higher prediction takes it: no 6 x 4 board
    assert last.status == N.BOARD_NOT_FOUND


@pytest.mark.parametrize("name,rule,alt,seed", [
    ("T_dup", "neighbor", "highest", 11), ("T_dup", "assign", "last", 9),
    ("T_grid", "neighbor", "highest", 14), ("T_grid", "assign", "last", 12), ("T_mid", "assign", "last", 15),
    ("T_border", "border", "highest", 18), ("T_equal", "border", "highest", 20),
    ("T_equal", "overlap", "lt", None), ("T_grid", "overlap", "lt", None)])
def test_a_tie_case_is_decisive(name, rule, alt, seed):
    """under the wrong rule the named seed grows another board; seed None: the final answer is another"""
    c, r = S.case(name), ref(name)
    assert r.status == N.OK
    if seed is None:
        wrong = R.chessboards_from_corners(c.corners, c.board, rules={rule: alt})
        assert wrong.status != r.status or not same_board(wrong.index, r.index)
    else:
        assert r.seeds[seed][0] is not None and seed in r.trace.tie_seeds[rule]
        assert not same_board(R.seed_board(c.corners, seed, rules={rule: alt})[0], r.seeds[seed][0])


@pytest.mark.parametrize("name", S.TIE_CASES)
def test_row_major_order_is_the_same_rule(name):
    c, r = S.case(name), ref(name)
    other = R.chessboards_from_corners(c.corners, c.board, rules={"assign": "row_first"})
    for seed in range(len(c.corners)):
        assert_seed(name, seed, other.seeds[seed], r.seeds[seed])
    assert other.trace.ties == r.trace.ties and r.trace.ties["assign"] > 0


@pytest.mark.parametrize("name", S.TIE_CASES)
def test_a_tie_case_is_libm_proof(name):
    c, r = S.case(name), ref(name)
    combos = R.libm_extremes()        # eight constant sign combinations, sixteen patterns with a sign per function and argument
    assert len(combos) == 24 and (6, 4, 4) in combos and (-6, -4, -4) in combos and (6, 4, 4, 15) in combos
    for libm in combos:
        off = R.chessboards_from_corners(c.corners, c.board, libm=libm)
        for seed in range(len(c.corners)):
            assert_seed((name, libm), seed, off.seeds[seed], r.seeds[seed])
        assert off.status == r.status and same_board(off.index, r.index) and off.trace.ties == r.trace.ties, libm


@pytest.mark.parametrize("name", S.TIE_CASES + S.OVERLAP_CASES + ["A", "I", "N65"])
def test_the_heap_of_the_assignment_equals_the_plain_matrix_search(name):
    c, r = S.case(name), ref(name)
    for rule in ("col_first", "last"):
        fast = r if rule == "col_first" else R.chessboards_from_corners(c.corners, c.board, rules={"assign": rule})
        plain = R.chessboards_from_corners(c.corners, c.board, rules={"assign": rule}, plain=True)
        for seed in range(len(c.corners)):
            assert_seed((name, rule), seed, plain.seeds[seed], fast.seeds[seed])
        assert plain.trace.ties == fast.trace.ties and plain.status == fast.status and same_board(plain.index, fast.index)


def test_the_signs_of_the_salted_offsets_differ_between_directions_and_not_between_calls():
    c = S.case("T_grid")
    signs = set()
    for salt in range(16):
        run = R._Run(c.corners, None, (6, 4, 4, salt))
        got = tuple(run.off(0, a, 1.0, 6) > 1.0 for a in ((0.0, 32.0), (32.0, 0.0), (0.0, -32.0), (-32.0, 0.0)))
        assert got == tuple(run.off(0, a, 1.0, 6) > 1.0 for a in ((0.0, 32.0), (32.0, 0.0), (0.0, -32.0), (-32.0, 0.0)))
        signs.add(got)
    assert len(signs) >= 8        # of the 16 patterns of four directions


def test_the_offsets_reach_predict_corners():
    """on a jittered case the same offsets do move a prediction: the libm argument is not a no-op"""
    c = S.case("A")
    run0, run1 = R._Run(c.corners, None, (0, 0, 0)), R._Run(c.corners, None, (6, 4, 4))
    p = [run0.P[k] for k in (0, 1, 2)]
    assert run0.predict(*p) != run1.predict(*p)
    assert R._ulps(1.0, 4) == 1.0 + 4 * 2.0 ** -52 and R._ulps(1.0, -2) == 1.0 - 2 * 2.0 ** -53 and R._ulps(0.0, 1) == 5e-324


def test_the_overlap_cases_show_their_events():
    one, two, mixed = ref("O_one"), ref("O_two"), ref("O_mixed")
    for name, board in S.SECOND_BOARDS.items():        # what the GPU tests ask for a second time: the board that the event leaves alone
        other = R.chessboards_from_corners(S.case(name).corners, board)
        assert other.status == N.OK and other.index.shape == board and same_board(other.index, host_with(name, board))
    assert one.trace.events["replaced"] == {1: 1}
    assert two.trace.events["replaced"].get(2, 0) >= 1
    newcomer = two.trace.event_seeds["replaced"][2][0]
    survivors = [s for s in two.stored if s < newcomer]        # stored before it and never removed: disjoint from it
    assert survivors and newcomer in two.stored
    cells = set(two.seeds[newcomer][0].reshape(-1).tolist())
    assert all(not cells & set(two.seeds[s][0].reshape(-1).tolist()) for s in survivors)
    assert mixed.trace.events["dropped_mixed"] >= 1 and mixed.trace.events["replaced"] == {} and len(mixed.stored) == 3
    for r in (one, two, mixed):
        assert r.status == N.OK
        print(r.trace.summary())
    # the events of the older cases, for the record: all their newcomers are stored or dropped against an equal board
    assert ref("A").trace.events["dropped_equal"] == 14 and ref("A").trace.events["replaced"] == {}


def test_replay_overlap_rule_agrees_with_the_restatement():
    for name in S.OVERLAP_CASES + ["T_equal", "C", "K", "I"]:
        c, r = S.case(name), ref(name)
        st, idx = S.replay_overlap_rule(r.seeds, c.board)
        assert st == r.status and same_board(idx, r.index), name


@pytest.mark.parametrize("name", ["N64", "N65", "N128", "N129"])
def test_the_board_of_a_count_case_lies_on_both_sides_of_a_used_word(name):
    """64 corners have no index above the first word, so N64 cannot lie across an edge: its board holds the word's last bit, 63"""
    c, r = S.case(name), ref(name)
    n = int(name[1:])
    assert len(c.corners) == n and r.status == N.OK
    if n == 64:        # no index lies above the one word: the board holds its last bit
        assert r.index.max() == 63
    else:
        edge = 128 if n == 129 else 64        # 65 and 129: the last corner alone is in the new word, and the board holds it
        assert r.index.min() < edge <= r.index.max() and (n % 64 != 1 or r.index.max() == n - 1), (r.index.min(), r.index.max())


def test_the_magnitude_cases_sit_on_the_limit_and_one_float_above():
    for name in S.MAGNITUDE_CASES:
        c = S.case(name)
        big = max(np.abs(c.corners["u"]).max(), np.abs(c.corners["v1"]).max())
        assert (big > S.MAX_ABS) == (name in S.MARKED) and (big == S.MAX_ABS) == (name not in S.MARKED)
        assert len(c.corners) == 36 and c.status == N.OK


def test_unknown_rules_are_refused():
    with pytest.raises(ValueError):
        R.seed_board(S.case("A").corners, 0, rules={"assign": "first"})
    with pytest.raises(ValueError):
        R.seed_board(S.case("A").corners, 0, rules={"order": "lowest"})
