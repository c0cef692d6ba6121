"""K18 (csrc/k18_chessboard_structure.hip) on the edge cases of structure_cases.py, against the host code with == everywhere: exact
ties in directionalNeighbor, assignClosestCorners, the proposal energies and the overlap rule (T_), the overlap events (O_), corner
counts at the edges of the 64-bit used words (N63 ..), the board capacities (S64x4, S65x4, S80x3, M_strays) and the magnitude limit
(X_).  tests/test_structure_ref_cpu.py proves on the CPU, with the independent restatement, what each case exercises, that the tie
cases give another answer under the wrong rule and that none of it depends on the last bits of the device's atan2 / cos / sin."""
import struct

import numpy as np
import pytest

import structure_cases as S
from lidar_camera_calibration_amd import _native as N
from lidar_camera_calibration_amd import image_corners as IC
from lidar_camera_calibration_amd import image_sequence as IS

pytestmark = pytest.mark.gpu

_host = {}


def host_case(name, board=None):
    """(status, index matrix or None) of ilcc_chessboard_from_corners, once per (case, board); for the case's own board the status
    is the case table's"""
    c = S.case(name)
    key = (name, board or c.board)
    if key not in _host:
        try:
            _host[key] = (N.OK, IC.chessboard_from_corners(c.corners, key[1]))
        except IC.BoardNotFound as e:
            _host[key] = (e.status, None)
        if board is None:
            assert _host[key][0] == c.status, (name, _host[key][0], c.status)
            if c.shape is not None:
                assert _host[key][1].shape == c.shape
    return _host[key]


def assert_equals_host(status, boards, m, name, board=None):
    st, idx = host_case(name, board)
    assert status[m] == st, (name, status[m], st)
    if st == N.OK:
        assert boards[m].shape == idx.shape and np.array_equal(boards[m], idx), name
    else:
        assert boards[m] is None, name


def test_every_edge_case_in_one_batch_per_board_equals_the_host():
    groups = {}
    for n in S.EDGE_CASES:
        groups.setdefault(S.case(n).board, []).append(n)
    assert len(groups) == 9 and set(groups[(7, 5)]) >= set(S.COUNT_CASES + S.MAGNITUDE_CASES + ["T_dup", "S65x4"])
    with IS.StructurePlan(max(len(g) for g in groups.values()), 512) as plan:
        for board, names in groups.items():
            status, boards = IS.chessboards_from_corners_batch([S.case(n).corners for n in names], board, plan=plan)
            for m, n in enumerate(names):
                assert_equals_host(status, boards, m, n)
            assert plan.fallbacks == len([n for n in names if n in S.MARKED]), (board, names, plan.fallbacks)
            assert plan.launches == 2
    assert S.MARKED == {"S65x4", "M_strays", "X_u_above", "X_dir_above"}
    assert host_case("S64x4")[1].shape == (4, 64) and host_case("S80x3")[1].shape == (3, 80)


def test_the_boards_that_an_overlap_event_leaves_alone_are_still_stored():
    """K18 returns the one stored board of the shape asked for, so the same lists are asked for the other board of the event: the
    4 x 4 side board that O_two's double replacement must not touch, and the worse 3 x 5 board that O_mixed's dropped newcomer
    overlaps and must not remove.  The overlap cases go in one batch, each asked for both boards in turn."""
    assert set(S.SECOND_BOARDS) == {"O_two", "O_mixed"}
    lists = [S.case(n).corners for n in S.OVERLAP_CASES]
    with IS.StructurePlan(len(lists), 128) as plan:
        for name, board in S.SECOND_BOARDS.items():
            status, boards = IS.chessboards_from_corners_batch(lists, board, plan=plan)
            assert plan.fallbacks == 0 and plan.launches == 2
            for m, n in enumerate(S.OVERLAP_CASES):
                assert_equals_host(status, boards, m, n, board)
            at = S.OVERLAP_CASES.index(name)
            assert status[at] == N.OK and boards[at].shape == board
            own = host_case(name)[1]
            if name == "O_two":        # disjoint from the newcomer's board
                assert not set(boards[at].reshape(-1).tolist()) & set(own.reshape(-1).tolist())


@pytest.mark.parametrize("name", S.TIE_CASES + S.OVERLAP_CASES + S.COUNT_CASES + ["S64x4", "X_u", "X_dir"])
def test_every_seed_of_an_edge_case_grows_the_host_board_with_the_host_energy(name):
    c = S.case(name)
    with IS.StructurePlan(1, len(c.corners)) as plan:
        status, boards = IS.chessboards_from_corners_batch([c.corners], c.board, plan=plan)
        assert plan.fallbacks == 0 and plan.launches == 2
        assert_equals_host(status, boards, 0, name)
        grown = 0
        for seed in range(len(c.corners)):
            want, want_e = IS.seed_board(c.corners, seed)
            got, got_e = IS.seed_board(plan=plan, image=0, seed=seed)
            assert (got is None) == (want is None), seed
            if want is not None:
                grown += 1
                assert got.shape == want.shape and np.array_equal(got, want), seed
            assert struct.pack("<d", got_e) == struct.pack("<d", want_e), (seed, got_e, want_e)
        # the comparison must not pass on seeds without boards; T_mid has six that grow, all of them met by a tie
        assert grown >= (100 if name == "S64x4" else 6 if name == "T_mid" else 9)


@pytest.mark.parametrize("name", S.TIE_CASES)
def test_a_tie_case_at_the_first_a_middle_and_the_last_place_of_a_batch(name):
    c = S.case(name)
    fillers = ["A", "C", "I", "K", "L", "E", "F", "Z", "T_dup", "N64", "N129"]
    rng = np.random.default_rng(41)
    with IS.StructurePlan(24, 256) as plan:
        for at in (0, 11, 23):
            names = [fillers[k] for k in rng.integers(0, len(fillers), 24)]
            names[at] = name
            status, boards = IS.chessboards_from_corners_batch([S.case(n).corners for n in names], c.board, plan=plan)
            assert plan.fallbacks == 0 and plan.launches == 2
            assert_equals_host(status, boards, at, name)
            if c.board == (7, 5):        # the fillers are asked for their own board here: they are their hosts' too
                for m in {0, 10, 11, 12, 23} - {at}:
                    assert_equals_host(status, boards, m, names[m])
            tie_seeds = [s for s in range(len(c.corners)) if IS.seed_board(c.corners, s)[0] is not None][:6]
            for seed in tie_seeds:
                want, want_e = IS.seed_board(c.corners, seed)
                got, got_e = IS.seed_board(plan=plan, image=at, seed=seed)
                assert got is not None and np.array_equal(got, want) and struct.pack("<d", got_e) == struct.pack("<d", want_e), (at, seed)
            assert len(tie_seeds) == 6
