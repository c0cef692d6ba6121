"""The bounded CPU search behind tests/structure_cases.py's OVERLAP_SEEDS: generator seeds of structure_cases.defects() on which the
overlap rule of chessboardsFromCorners, as tests/structure_ref.py restates it, shows a named event.

  O_one    a newcomer replaces exactly one stored board
  O_two    a newcomer replaces two stored boards at once while a third, disjoint one that was stored before it survives to the end
  O_mixed  a newcomer is dropped because it overlaps one worse and one better board, and nothing is removed

    python tools/dev_structure_overlap_search.py [first seed] [seeds]

prints the first seed per event and how many of the searched seeds show it.  Needs no GPU.  Of seeds 0 .. 2399 (the default),
1018 show O_one, 303 O_two and 45 O_mixed; OVERLAP_SEEDS holds the first of each.  Without the 4 x 4 side lattice in defects() none
of 1500 seeds showed O_two: no third board was ever stored beside the two that a newcomer replaced."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import structure_cases as S      # noqa: E402
import structure_ref as R        # noqa: E402


def events(corners, board=(5, 9)):
    """the named events that the list shows -> {name: the newcomer's seed}"""
    r = R.chessboards_from_corners(corners, board)
    ev, out = r.trace.event_seeds, {}
    if ev["replaced"].get(1):
        out["O_one"] = ev["replaced"][1][0]
    for s in ev["replaced"].get(2, []):
        # a board stored before the newcomer that is still stored at the end was disjoint from it, and from everything after it
        if any(t < s for t in r.stored):
            out["O_two"] = s
            break
    if ev["dropped_mixed"]:
        out["O_mixed"] = ev["dropped_mixed"][0]
    return out


def main():
    first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 2400
    found, hits = {}, {}
    for seed in range(first, first + count):
        for name, s in events(S.defects(seed)).items():
            hits[name] = hits.get(name, 0) + 1
            found.setdefault(name, (seed, s))
    for name in S.OVERLAP_CASES:
        print("%-8s %s  (%d of %d seeds)" % (name, "generator seed %d, newcomer %d" % found[name] if name in found else "not found", hits.get(name, 0), count))


if __name__ == "__main__":
    main()
