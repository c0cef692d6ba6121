"""Recall of the planar seed proposer (K15p), measured on the CPU: the numpy restatement (tests/seed_planar_ref.py) proposes,
the CPU oracle runs the exact path on the proposals in rank order and on a click at the true board centre, and the accept rule
of ilcc_extract_auto (status OK, coverage flag clear, n_oob share) is applied to both -- and to the ordinary proposer
(tests/seed_ref.py) beside them.  Scenes (tests/seed_planar_cases.py): the config-2 frames as they are, with the floor 5 cm
below the board, with the board 2 cm in the floor, and on a pole; --lidar hdl64 for the config-5 frames of each.

    python tools/dev_seed_planar_recall.py --frames 1024 --out profiles/r10_seed_planar_recall_cpu.json [--rows-out rows.json]
    python tools/dev_seed_planar_recall.py --frames 256 --sweep          # proposals only (no oracle) over a grid of thresholds
"""
import argparse
import functools
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEAR = 0.3   # m: a seed this close to the true centre is the board's


def accepted(r, max_oob_share=0.05):
    from oracle import binding as ob
    return r.status == 0 and not (r.flags & ob.FLAG_LOW_COVERAGE) and r.n_oob <= max_oob_share * (r.n_black + r.n_white)


def oracle_params(lidar):
    from oracle import binding as ob
    p = ob.default_params()
    p.solver = ob.SOLVER_GRID
    if lidar == "hdl64":
        p.board_w, p.board_h, p.grid_length = 9, 12, 0.10
        p.n_th, p.n_ty, p.n_tz = 129, 129, 129
        p.th_min, p.th_step = -16.0 * np.pi / 180.0, 0.25 * np.pi / 180.0
        p.ty_min = p.tz_min = -0.10
        p.ty_step = p.tz_step = 0.10 / 64
    return p


def one_frame(job, planar_rms, min_spread, own_rms, max_rms, lidar):
    import seed_planar_cases as C
    import seed_planar_ref as P
    import seed_ref as R
    from oracle import binding as ob
    scene, f = job
    cloud, pose, board = C.scene_frame(scene, f, lidar)
    sp, _ = C.seed_params(lidar)
    sp.max_rms = max_rms
    pp = P.PlanarParams(planar_rms, min_spread, own_rms)
    osp = R.SeedParams(board_w=sp.board_w, board_h=sp.board_h, grid_length=sp.grid_length)
    p = oracle_params(lidar)

    def first_accepted(seeds):
        """(rank of the first seed the oracle accepts or -1, whether the FIRST seed is accepted, distance of that first seed)"""
        rank = -1
        for k, sd in enumerate(seeds or []):
            if accepted(ob.extract(cloud, np.asarray(sd.centroid, np.float32), p)):
                rank = k
                break
        return rank

    planar = P.propose(cloud, sp, pp) or []
    ordinary = R.propose(cloud, osp) or []
    dist = lambda seeds: [float(np.linalg.norm(s.centroid - pose.centre)) for s in seeds]
    row = dict(scene=scene, frame=f, truth=bool(accepted(ob.extract(cloud, pose.centre.astype(np.float32), p))),
               planar_dist=dist(planar), planar_rank=first_accepted(planar), ordinary_dist=dist(ordinary), ordinary_rank=first_accepted(ordinary))
    if not any(d < NEAR for d in row["planar_dist"]):
        # why: the board's core component under gates thrown open
        wide = R.SeedParams(**{**sp.__dict__, "size_lo": 0.0, "size_hi": 1e9, "max_rms": 1e9, "max_seeds": 1 << 20})
        near = [s for s in R.finish(P.components(cloud, sp, pp), wide) if np.linalg.norm(s.centroid - pose.centre) < NEAR]
        row["board_component"] = [dict(n=s.n, l1=s.l1, l2=s.l2, rms=s.rms) for s in near]
    return row


def proposals_only(job, grid, lidar):
    """per threshold set: is the first planar seed the board's?"""
    import seed_planar_cases as C
    import seed_planar_ref as P
    scene, f = job
    cloud, pose, board = C.scene_frame(scene, f, lidar)
    out = []
    for (planar_rms, min_spread, own_rms, max_rms) in grid:
        sp, _ = C.seed_params(lidar)
        sp.max_rms = max_rms
        seeds = P.propose(cloud, sp, P.PlanarParams(planar_rms, min_spread, own_rms)) or []
        out.append(bool(seeds) and float(np.linalg.norm(seeds[0].centroid - pose.centre)) < NEAR)
    return out


def summarise(rows):
    out = {}
    for scene in sorted({r["scene"] for r in rows}):
        rs = [r for r in rows if r["scene"] == scene]
        truth = [r for r in rs if r["truth"]]
        miss = [r for r in truth if r["planar_rank"] < 0]
        causes = dict(no_seed=0, no_seed_near_the_board=0, near_seed_rejected_by_the_pipeline=0)
        for r in miss:
            if not r["planar_dist"]:
                causes["no_seed"] += 1
            elif not any(d < NEAR for d in r["planar_dist"]):
                causes["no_seed_near_the_board"] += 1
            else:
                causes["near_seed_rejected_by_the_pipeline"] += 1
        out[scene] = dict(frames=len(rs), truth_accepted=len(truth), planar_accepted=sum(r["planar_rank"] >= 0 for r in rs),
                          planar_accepted_of_truth=len(truth) - len(miss), ordinary_accepted=sum(r["ordinary_rank"] >= 0 for r in rs),
                          ordinary_accepted_not_planar=[r["frame"] for r in rs if r["ordinary_rank"] >= 0 and r["planar_rank"] < 0],
                          planar_first_seed_is_the_board=sum(bool(r["planar_dist"]) and r["planar_dist"][0] < NEAR for r in rs),
                          misses_of_truth_by_cause=causes, missed_frames=[r["frame"] for r in miss],
                          # sqrt(l0) of the board's core component on the missed frames that have one but no seed: the gate they fail
                          missed_board_component_rms=sorted(round(r["board_component"][0]["rms"], 3) for r in miss if r.get("board_component")),
                          # the first frames that tests/seed_planar_cases.py may commit: click accepted, FIRST planar seed accepted and
                          # within 0.1 m, no ordinary seed within NEAR of the board and none accepted
                          qualifying_frames=[r["frame"] for r in rs if qualifies(r)][:16], qualifying=sum(qualifies(r) for r in rs))
    return out


def qualifies(r):
    return (r["truth"] and r["planar_rank"] == 0 and r["planar_dist"][0] < 0.1 and r["ordinary_rank"] < 0
            and not any(d < NEAR for d in r["ordinary_dist"]))


def compact(result):
    """indented JSON with every list of numbers, and every sweep row, on one line"""
    import re
    text = json.dumps(result, indent=1)
    text = re.sub(r"\[[\s\d.,e+-]*\]", lambda m: re.sub(r"\s+", " ", m.group(0)).replace("[ ", "[").replace(" ]", "]"), text)
    return re.sub(r"\{\s*\"thresholds\"[^}]*\{[^}]*\}\s*\}", lambda m: re.sub(r"\s+", " ", m.group(0)), text) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--scenes", default="free,floor5,in2,pole")
    ap.add_argument("--lidar", default="vlp16", choices=("vlp16", "hdl64"))
    ap.add_argument("--planar-rms", type=float, default=0.03)
    ap.add_argument("--min-spread", type=float, default=0.06)
    ap.add_argument("--own-rms", type=float, default=0.02)
    ap.add_argument("--max-rms", type=float, default=0.05)
    ap.add_argument("--sweep", action="store_true", help="proposals only, one threshold moved at a time around the given values")
    ap.add_argument("--workers", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    ap.add_argument("--out", default="", help="the summary (the sweep's table)")
    ap.add_argument("--rows-out", default="", help="recall: the per-frame rows as well (large)")
    args = ap.parse_args()
    from oracle import binding as ob
    ob.build()
    jobs = [(s, f) for s in args.scenes.split(",") for f in range(args.first, args.first + args.frames)]
    base = (args.planar_rms, args.min_spread, args.own_rms, args.max_rms)
    with mp.get_context("fork").Pool(args.workers) as pool:
        if args.sweep:
            grid = [base]
            for k, factors in enumerate(((0.5, 0.75, 1.5, 2.0), (0.5, 0.75, 1.5, 2.0), (0.5, 0.75, 1.5, 2.0), (0.6, 0.8, 1.2, 2.0))):
                for fac in factors:
                    g = list(base)
                    g[k] = base[k] * fac
                    grid.append(tuple(g))
            hits = np.array(pool.map(functools.partial(proposals_only, grid=grid, lidar=args.lidar), jobs, chunksize=4))
            result = dict(kind="sweep", lidar=args.lidar, frames=args.frames, first=args.first, near_m=NEAR,
                          columns=["planar_rms", "min_spread", "own_rms", "max_rms"], rows=[])
            for k, g in enumerate(grid):
                per_scene = {s: int(hits[[j for j, job in enumerate(jobs) if job[0] == s], k].sum()) for s in args.scenes.split(",")}
                result["rows"].append(dict(thresholds=list(g), first_seed_is_the_board=per_scene))
        else:
            rows = pool.map(functools.partial(one_frame, planar_rms=base[0], min_spread=base[1], own_rms=base[2], max_rms=base[3], lidar=args.lidar),
                            jobs, chunksize=2)
            result = dict(kind="recall", lidar=args.lidar, frames=args.frames, first=args.first, near_m=NEAR,
                          thresholds=dict(planar_rms=base[0], min_spread=base[1], own_rms=base[2], max_rms=base[3]), summary=summarise(rows))
            if args.rows_out:
                with open(args.rows_out, "w") as fh:
                    json.dump(rows, fh)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(compact(result))
    print(json.dumps(result.get("summary", result.get("rows")), indent=1))


if __name__ == "__main__":
    main()
