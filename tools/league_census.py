#!/usr/bin/env python3
"""CPU census of the seeds tests/test_gpu_league.py runs (no GPU): the statement of tests/league_statement.py over the
oracle's stamped-grid scan (drive_cases.race_oracle_fan, noise off), the compiled reference Car, the oracle's FollowGap
and the network's host statement, one member per car.  Prints, per case, what the reference alone meets of the
censuses the GPU tests assert: crashes, clamped member answers, rays the other cars changed, the share of member
answers that some other entered member would have given otherwise, and the standings.  docs/history/league.md records
the output.

usage: python tools/league_census.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import drive_cases as DC                      # noqa: E402
import league_statement as LS                 # noqa: E402
import policy_statement as PS                 # noqa: E402
import seats_census as SC                     # noqa: E402
import test_gpu_league as TL                  # noqa: E402
import test_gpu_population as TP              # noqa: E402
from oracle import oracle as O                # noqa: E402
from support import MAX_STEER                 # noqa: E402


class World(SC.World):
    """seats_census.World with a member per car: the answer of entry m >= 0 is member m's network."""

    def __init__(self, g, group, B, entered):
        super().__init__(g, group, B)
        self.members = TP.members("small", TL.N_POP, TL.NET_SEED, TL.GAIN)
        self.entered = entered
        self.net_answers = self.differ = 0

    def net(self, m, row):
        return PS.forward(row[None], self.members[m], self.relu, in_start=5)[0]

    def answer(self, entry, row):
        if entry < 0:
            return np.float32(O.followgap_eval(np.ascontiguousarray(row), 15.0, MAX_STEER, 0.004))
        mine = self.net(entry, row)
        self.net_answers += 1
        self.differ += any(self.net(k, row).tobytes() != mine.tobytes() for k in self.entered if k != entry)
        return mine


def case(g, dt, name, c, noise_note):
    P, B, R, T = c["P"], c["B"], c["R"], c["T"]
    entries = np.array(c["entries"]).reshape(-1)
    w = World(g, P, B, sorted(set(entries[entries >= 0].tolist())))
    states, speeds = TL._race_starts(g, dt, R, P, c["seed"])
    if name == "indep":
        states[:, :, 8] = np.random.default_rng(c["odo_seed"]).uniform(0.0, 1.0, (R, P))
    flat = states.reshape(-1, 11)
    steer0 = np.zeros(R * P, np.float32)
    if name == "indep":                       # (test_gpu_league.race_inputs' steer0)
        steer0 = np.random.default_rng(c["seed"]).uniform(-0.2, 0.2, (R, P)).astype(np.float32).reshape(-1)
    first, final, steers, trace = LS.league_rollout(flat, (speeds + 2.0).reshape(-1), steer0, T, entries,
                                                    TL.CLIP, w.step_cars, w.scan, w.is_crashed, w.answer)
    net = entries >= 0
    clamped = int((np.abs(steers[net, :-1]) > TL.CLIP).sum())
    st = LS.standings(flat, final, first, entries, TL.N_POP, P, T)
    print("%s: %d races x %d cars, B %d, T %d, seed %d%s: %d of %d cars crash (ticks %s), %d member answers clamped, %d rays "
          "changed by other cars, %d of %d member answers differ from another entered member's"
          % (name, R, P, B, T, c["seed"], noise_note, (first >= 0).sum(), R * P, sorted(first[first >= 0].tolist()), clamped,
             w.seen, w.differ, w.net_answers))
    print("  standings (cars, gain, crashed, beaten): %s" % "; ".join(
        "m%d %d %.6f %d %d" % (m, st[m, 0], st[m, 1], st[m, 2], st[m, 3]) for m in range(TL.N_POP)))
    ok = (first >= 0).sum() >= 1 and clamped >= 1 and w.seen > 0 and w.differ >= 0.9 * w.net_answers > 0
    if name == "indep":
        gain = (final[:, 8] - flat[:, 8])[entries == 0]
        down = np.float64(0.0)
        for v in gain[::-1]:
            down = down + v
        print("  member 0's %d gains summed downwards: %r against %r upwards" % (len(gain), float(down), float(st[0, 1])))
        ok = ok and down != st[0, 1] and (first < 0).any()
    print("  -> %s" % ("ok" if ok else "MISSING"))


def main():
    O.build()
    g = DC.race_maze()
    dt = O.edt(g.occ)
    for name in sorted(TL.MIXED):
        case(g, dt, name, TL.MIXED[name], " (steer0 0, noise off)")
    case(g, dt, "indep", TL.INDEP, " (the test's steer0 and odometers)")


if __name__ == "__main__":
    main()
