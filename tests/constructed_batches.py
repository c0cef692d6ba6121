"""Batches of CONSTRUCTED labelled frames for the GRID back end's batch kernels (tests/test_grid_backend_batch.py): every constructed
frame the single-frame suites send through ilcc_grid_solve or ilcc_pattern_refine, grouped by parameter set (parameters are per
handle) and laid out as one batch per group -- built by those suites' own constructors and references, not by copies of them.

Plain module (no fixtures).  `ob` is the oracle binding; everything that needs it is computed once per process and never modified.

A batch of F frames over a group's k distinct frames:
  * slot 0 and slot F // 2 carry a FAILED status (ILCC_NO_PLANE, ILCC_DEGENERATE_HIST) -- with points, those of the group's first
    and second distinct frame, so that a kernel that ignored the status would have something to compute;
  * slot F // 3 is an OK frame with no labelled point (every point gray: K5 leaves such a frame behind with ILCC_OK);
  * the other slots take the distinct frames in passes: pass r visits every frame once, in the order (r + j * step_r) mod k, where
    step_r runs through the steps coprime to k -- replicas of one frame sit at different offsets and, for k >= 4, beside different
    neighbours from pass to pass.
"""
import functools
from collections import namedtuple
from math import gcd

import numpy as np

import constructed_points as cp
import test_grid_backend_constructed as tb
import test_grid_pruning_constructed as tp
import test_k7r_sweep_forms as tk

SMALL_BATCH = 64              # kSmallBatchFrames: K7r runs 768 threads up to it, 192 above
LOCATE_MIN_FRAMES = 512       # kLocateMinFrames: k6_locate from this many frames on
F_SMALL = SMALL_BATCH + 1     # the first size with the 192-thread K7r (and the three locate launches)
F_LARGE = LOCATE_MIN_FRAMES   # the first size with k6_locate
LDS_FRESH = 1024              # a fresh handle's staging capacity (labelled points per frame)
LDS_MAX = 8192                # kGridLdsPointsMax
LOCATE_LDS_MAX = 3 * (160 * 1024 // 8)   # kLocateLdsMax
LOCATE_THETAS_MAX = 16        # kLocateThetasMax
SEED_POINTS = 128             # ILCC_SEED_POINTS
B_EDGE_FROM = 1023            # test_k7r_sweep_forms.M_SOLVER from here on: 1 023, 1 024, 1 025
STATUS_OK, STATUS_NO_PLANE, STATUS_DEGENERATE_HIST = 0, 3, 4

# rule: how the frame's grid argmin is held against the oracle's, as the frame's single-frame test does it --
#   None                the single-frame test asserts nothing about the argmin (it reaches K7r's entry only, or checks downstream only)
#   ("plateau", name)   test_zero_cost_plateaus: == _plateau_ref's argmin, cost 0, ILCC_FLAG_BORDER_RISK clear, the overflow flag by class
#   ("solve", capped)   _solve_case: == the oracle's argmin or ILCC_FLAG_BORDER_RISK; capped: one of test_point_counts_grid_solve's five
#                       cases, of which at most one may rely on the flag
#   ("pruning", name)   test_pruned_solve_matches_the_oracle_and_rejects_only_losers (a): == _ref's argmin, the flag clear
Frame = namedtuple("Frame", "name yz lab rule")
Group = namedtuple("Group", "name fields frames sides_note")
Batch = namedtuple("Batch", "frames status source offsets")   # source[f]: index of the distinct frame, -1 for the empty frame


def _frame(name, yz, lab, rule=None):
    yz = np.ascontiguousarray(yz, np.float32)
    lab = np.ascontiguousarray(lab, np.uint8)
    yz.setflags(write=False)
    lab.setflags(write=False)
    return Frame(name, yz, lab, rule)


def _far_frame(name, case):
    return _frame(name, *cp.far_points(case["m"], case["lo"], case["hi"], case["seed"]))


@functools.lru_cache(maxsize=None)
def groups(ob):
    """-> {name: Group}, every group with its own parameter set"""
    out = {}

    def add(name, fields, frames, sides_note=None):
        out[name] = Group(name, dict(fields), tuple(frames), sides_note)

    # ---- the default grid: plateaus, point counts of the solver test, trip edges of both K7r widths
    op = tb._oparams(ob)
    frames = [_frame("plateau_" + n, *tb._plateau_ref(ob, n)[:2], rule=("plateau", n)) for n in tb.PLATEAUS]
    frames += [_frame("solve_%d" % m, *cp.noisy_board(op, m, 200 + m, tb.POSE_B), rule=("solve", True)) for m in tb.M_SOLVE_DEFAULT]
    frames += [_frame("entry_%d" % m, *cp.noisy_board(op, m, 300 + m, tk.POSE_B)) for m in tk.M_ENTRY]
    # (of the 768-thread solver's trip edges, which the cut grid below holds in full, the three around a fresh handle's capacity:
    # this group's frames on either side of 1 024 -- and no more, so that every distinct frame has two replicas among 65)
    frames += [_frame("solver_%d" % m, *cp.noisy_board(op, m, 400 + m, tk.POSE_C)) for m in tk.M_SOLVER if m >= B_EDGE_FROM]
    add("default", {}, frames)

    # ---- test_point_counts_grid_solve's small grid: the last staged size and the first global-memory size
    fields = tb._small_grid(op)
    ops = tb._oparams(ob, fields)
    add("small_grid", fields, [_frame("solve_%d" % m, *cp.noisy_board(ops, m, 200 + m, tb.POSE_B), rule=("solve", True)) for m in tb.M_SOLVE_SMALL],
        "both frames are the staging edge itself (kGridLdsPointsMax and one more): above 1 024 by construction")

    # ---- the cut grid: ring fills laid out for ONE wavefront per theta, the queue fills, the 768-thread solver's trip edges
    fields = tb._cut_grid(op)
    opc = tb._oparams(ob, fields)
    frames = [_frame("ring_" + n, *cp.chunk_pattern(opc, tk._ring_counts(n, 1), 5, tk.POSE_C)[:2]) for n in tk.RING_CASES]
    frames += [_frame("queue_fills", *cp.chunk_pattern(opc, cp.chunk_counts(5), 5, tb.POSE_C)[:2], rule=("solve", False))]
    frames += [_frame("solver_%d" % m, *cp.noisy_board(opc, m, 400 + m, tk.POSE_C)) for m in tk.M_SOLVER]
    add("cut", fields, frames)

    # ---- the dyadic board at refine_div = 16: the term's branches, decision ties -- and the pruning cases on the same parameter set
    dyadic = dict(cp.dyadic_params(), refine_div=16)
    frames = [_frame("edge_points", *tk._edge_points()), _frame("crossing_points", *tk._crossing_points()),
              _frame("dyadic_symmetric", *cp.dyadic_points_symmetric(11)), _frame("dyadic_points", *cp.dyadic_points(11))]
    by_params = {}   # (the parameter struct's bytes: two spellings of one set are one group)
    for n, case in tp.CASES.items():
        fields = dict(case["fields"], grid_prune=1)
        by_params.setdefault(bytes(tb._oparams(ob, fields)), (fields, []))[1].append(n)
    small_note = "every frame is the case's own size (a few hundred points: 8 or 10 per board cell and a fence), below 1 024"
    for key, (fields, names) in by_params.items():
        case_frames = [_frame("prune_" + n, tp._ref(ob, n).yz, tp._ref(ob, n).lab, rule=("pruning", n)) for n in names]
        if key == bytes(tb._oparams(ob, dyadic)):
            add("dyadic", fields, frames + case_frames, small_note + "; the dyadic sets hold 6 to 632 points")
        else:
            one = "one distinct frame, the case's own: %d points" % len(case_frames[0].lab)
            add("prune_" + (names[0] if len(names) == 1 else names[0][0]), fields, case_frames, one if len(names) == 1 else small_note)

    # ---- the summation's domain: one group per (huber_delta, refine_div)
    far = dict(refine_max_rounds=tb.FAR_ROUNDS)
    far_note = "the far frames are 8 000 and 28 800 points by construction (the sizes that put a lane's sum on either side of 2^53)"
    add("far_delta5", dict(far, huber_delta=5.0, refine_div=16), [_far_frame("far_in", tb.FAR_IN), _far_frame("far_out", tb.FAR_OUT)], far_note)
    add("far_delta50", dict(far, huber_delta=50.0, refine_div=16), [_far_frame("far_out_192", tb.FAR_OUT_192)], far_note)
    add("far_delta50_div0", dict(far, huber_delta=50.0, refine_div=0), [_far_frame("far_out_192", tb.FAR_OUT_192)], far_note)
    return out


# the names without building anything (for parametrize): a CPU test keeps them equal to groups(ob)
GROUP_NAMES = ("default", "small_grid", "cut", "dyadic", "prune_A_ll", "prune_A_hl", "prune_A_lh", "prune_B_last", "prune_B_first",
               "prune_B_inner", "prune_C21_first", "prune_C21_middle", "prune_C21_last", "prune_C15_single", "prune_C8_single",
               "prune_C6_none", "prune_D", "prune_G_large", "prune_G_global", "far_delta5", "far_delta50", "far_delta50_div0")
FAR_GROUPS = ("far_delta5", "far_delta50", "far_delta50_div0")   # 28 800-point frames: batches of F_SMALL only


def batch_sizes(name):
    return (F_SMALL,) if name in FAR_GROUPS else (F_SMALL, F_LARGE)


# ------------------------------------------------------------------------------------------------------------------ composition
def _steps(k):
    return [s for s in range(1, k + 1) if gcd(s, k) == 1]


def special_slots(F):
    """-> (the two failed slots, the empty slot)"""
    return (0, F // 2), F // 3


def compose(group, F):
    """-> Batch of F frames over the group's distinct frames (the module docstring's layout)"""
    k = len(group.frames)
    failed, empty = special_slots(F)
    steps = _steps(k)
    frames, status, source = [], np.zeros(F, np.int32), np.zeros(F, np.int64)
    n = 0
    none = (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8))
    for f in range(F):
        if f == empty:
            frames.append(none)
            source[f] = -1
            continue
        if f in failed:
            src = failed.index(f) % k
            status[f] = (STATUS_NO_PLANE, STATUS_DEGENERATE_HIST)[failed.index(f)]
        else:
            r, j = divmod(n, k)
            src = (r + j * steps[r % len(steps)]) % k
            n += 1
        frames.append((group.frames[src].yz, group.frames[src].lab))
        source[f] = src
    offsets = np.concatenate([[0], np.cumsum([len(lab) for _, lab in frames])]).astype(np.uint64)
    return Batch(frames, status, source, offsets)


def replicas(batch, src):
    """slots of the OK replicas of distinct frame `src`"""
    return [f for f in range(len(batch.frames)) if batch.source[f] == src and batch.status[f] == STATUS_OK]


# ------------------------------------------------------------------------------------------------------------------ capacities
def reserved_capacity(group):
    """what ilcc_reserve gives a handle asked to stage every frame of the group that can be staged at all: the largest frame of
    at most kGridLdsPointsMax points, rounded up to 256, at least a fresh handle's 1 024"""
    m = max([len(fr.lab) for fr in group.frames if len(fr.lab) <= LDS_MAX] or [0])
    return min(LDS_MAX, max(LDS_FRESH, (m + 255) & ~255))


def staged(group, capacity):
    """-> (distinct frames staged in LDS at this capacity, distinct frames read from global memory)"""
    n = sum(len(fr.lab) <= capacity for fr in group.frames)
    return n, len(group.frames) - n


def locate_form(p, lds_points, n_frames):
    """the host's rule (enqueue_grid_search) restated: 0 the grid is too small to locate on, 1 seed + refinement + anchor launches,
    2 k6_locate -- from kLocateMinFrames frames on, where the seed grid has at most kLocateThetasMax thetas and the launch's dynamic
    LDS (locate_lds: sample, labels, the larger of 16 rotations of the sample and the staged frame, the four translation tables)
    stays within kLocateLdsMax"""
    stride_th, stride_t = max(2, p.n_th // 5), max(1, min(p.n_ty, p.n_tz) // 8)
    seed_th = len(range(stride_th // 2, p.n_th, stride_th))
    seed_ty, seed_tz = len(range(0, p.n_ty, stride_t)), len(range(0, p.n_tz, stride_t))
    if not (seed_th > 0 and min(p.n_th, p.n_ty, p.n_tz) >= 8):
        return 0
    sample_cap = max(SEED_POINTS, ((lds_points >> 3) + 63) & ~63)
    lds = 12 * sample_cap + max(8 * LOCATE_THETAS_MAX * sample_cap, 12 * lds_points) + 4 * (p.n_ty + p.n_tz + seed_ty + seed_tz)
    return 2 if n_frames >= LOCATE_MIN_FRAMES and seed_th <= LOCATE_THETAS_MAX and lds <= LOCATE_LDS_MAX else 1
