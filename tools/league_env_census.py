#!/usr/bin/env python3
"""CPU census of the seeds tests/test_gpu_league_env.py runs (no GPU): the statement of tests/league_env_statement.py
over the oracle's stamped-grid scan (noise off), the compiled reference Car, the oracle's FollowGap and the network's
host statement, one driver per car (tools/league_census.py's world).  Prints, per case of tests/league_env_cases.py,
what the reference alone meets of the conditions the GPU tests assert — crashes, races ended by attrition and by
truncation, clamped member answers, rays changed by other cars, the share of member answers that another entered member
would have given otherwise, and for the hand-over case a call in which one race re-spawns with new entries while another
still runs its old line-up — and the results the run ends with.  docs/history/league_env.md records the output.

usage: python tools/league_env_census.py [--pool-seeds A B ...]   (more pool seeds to try for every case)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import drive_cases as DC                      # noqa: E402
import league_census as LC                    # noqa: E402
import league_env_cases as CASES              # noqa: E402
import league_env_statement as LE             # noqa: E402
import seats_census as SC                     # noqa: E402
from oracle import oracle as O                # noqa: E402


def run(g, dt, name, c, pool_seed):
    R, P, B = c["R"], c["P"], c["B"]
    tables = [np.array(c["entries"])] + [np.array(t) for _, (_, t) in sorted(c.get("at", {}).items())]
    entered = sorted({int(m) for t in tables for m in t.reshape(-1) if 0 <= m < CASES.N_POP})
    w = LC.World(g, P, B, entered)
    w.S = c["S"]
    pool, _ = SC.TG._race_starts(g, dt, c["M"], P, pool_seed)
    pool[:, :, 3] = 3.0
    kw = {k: v for k, v in CASES.env_kw(c).items() if k != "substeps"}
    stmt = LE.LeagueEnvStatement(pool, R, B, w.step_cars, w.scan, w.is_crashed, w.answer, c["entries"], c["speed"],
                                 CASES.N_POP, **CASES.WINDOW, **kw)
    stmt.reset(c["seed"])
    census = CASES.Census()
    for k, a in enumerate(CASES.actions(c), 1):
        if k in c.get("at", {}):
            stmt.set_entries(c["at"][k][1])
        before = stmt.done.copy(), stmt.race_over.copy(), stmt.live.copy()
        stmt.step(CASES.masked(a, stmt.live.reshape(R, P)).reshape(-1, 2))
        census.step(stmt, *before)
        net = (stmt.live >= 0) & (stmt.live < CASES.N_POP) & ~np.isnan(stmt.steers)
        census.clamped += int((np.abs(stmt.steers[net]) > CASES.CLIP).sum())
    census.seen, census.net_answers, census.differ = w.seen, w.net_answers, w.differ
    ok = census.ok(need_mixed="at" in c)
    print("%s: %d races x %d cars, B %d, %d steps, max_ticks %d, min_running %d, seed %d, pool seed %d (noise off): %s -> %s"
          % (name, R, P, B, c["steps"], c["max_ticks"], c["min_running"], c["seed"], pool_seed, census,
             "ok" if ok else "MISSING"))
    res = stmt.read_results()
    print("  results (%s): %s" % (", ".join(LE.COLUMNS), "; ".join(
        "%s %s" % ("m%d" % r if r < CASES.N_POP else ("fg", "caller")[r - CASES.N_POP], res[r].tolist())
        for r in range(CASES.N_POP + 2))))
    return ok


def main(argv):
    O.build()
    g = DC.race_maze()
    dt = O.edt(g.occ)
    more = [int(s) for s in argv[argv.index("--pool-seeds") + 1:]] if "--pool-seeds" in argv else []
    cases = dict(CASES.MIXED, swap=CASES.SWAP)
    for name in sorted(cases):
        for pool_seed in [cases[name]["pool_seed"]] + more:
            run(g, dt, name, cases[name], pool_seed)


if __name__ == "__main__":
    main(sys.argv)
