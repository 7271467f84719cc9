"""What tests/test_gpu_league_env.py and tools/league_env_census.py share (no GPU, no library): the cases' shapes, seeds
and entry tables, and the census both take of a run of the statement (tests/league_env_statement.py).

The seeds were picked with tools/league_env_census.py (oracle scan, reference Car, host network, noise off);
docs/history/league_env.md holds its output."""
import numpy as np

import drive_cases as DC

CLIP = 0.2                                        # steer_clip of every case: below the members' larger answers
STD, NOISE_SEED, BASE = 0.02, 3, 777              # scan noise of every noisy case
#: the races' population: 5 seeded 40 -> 16 -> 8 -> 1 members (test_gpu_league.py's), member 4 enters nothing
N_POP, NET_SEED, GAIN = 5, 1, 4.0
WINDOW = dict(obs_window=(5, 40, 1), obs_clip=15.0, obs_scale=15.0)

#: cases 3, 4, 7 and 8: a line-up per race — the caller in different seats, one member twice in a race, FollowGap among
#: members, a race without the caller
MIXED = {
    "5x3": dict(R=5, P=3, B=65, M=4, S=4, steps=24, seed=5, pool_seed=60, act_seed=77, speed=(3.5, 4.5, 5.5),
                min_running=2, max_ticks=14,
                entries=[[-2, 0, 1], [-2, -1, 2], [-2, 3, 3], [1, -2, 0], [2, -1, -1]]),
    "2x8": dict(R=2, P=8, B=64, M=3, S=4, steps=24, seed=6, pool_seed=60, act_seed=78,
                speed=(3.5, 4.5, 5.5, 4.0, 5.0, 3.0, 4.5, 5.5), min_running=4, max_ticks=8,
                entries=[[-2, 0, 1, 2, 3, -1, 0, 1], [3, 3, -1, -2, 0, 2, -1, 1]]),
}
#: case 5: tables handed over while races run; `at`: {the step before which the table is set: (form, table)}.  The
#: device-form table names n_members and -3, which behave as the caller's
SWAP = dict(R=5, P=3, B=65, M=4, S=4, steps=24, seed=5, pool_seed=60, act_seed=79, speed=(3.5, 4.5, 5.5), min_running=2,
            max_ticks=14, entries=[[-2, 0, 1], [-2, -1, 2], [-2, 3, 3], [1, -2, 0], [2, -1, -1]],
            at={3: ("host", [[-2, 2, 2], [0, -2, -1], [-2, 1, 0], [-2, -1, 4], [-2, 3, 1]]),
                11: ("device", [[N_POP, 1, 3], [-2, 4, -3], [-1, -2, 0], [2, 2, -2], [-3, N_POP, 1]])})


def env_kw(c):
    return dict(min_running=c["min_running"], max_ticks=c["max_ticks"], auto_reset=True, crash_reward=-2.5,
                steer_clip=CLIP, substeps=c["S"])


def actions(c):
    """(steps, R, P, 2) float32 for every car; the scripted cars' rows are overwritten with NaN by the tests."""
    return DC.actions(c["act_seed"], c["steps"], c["R"] * c["P"]).reshape(c["steps"], c["R"], c["P"], 2)


def masked(acts, live):
    """``acts`` (R, P, 2) with NaN in the rows of the cars that ``live`` (R, P) scripts for ``N_POP`` members."""
    a = acts.copy()
    a[(live >= -1) & (live < N_POP)] = np.nan
    return a


class Census:
    """What a run must contain for the comparisons not to pass vacuously."""

    def __init__(self):
        self.crashes = self.attrition = self.truncation = self.clamped = self.seen = 0
        self.net_answers = self.differ = self.respawned = self.mixed_adoption = 0

    def step(self, stmt, before_done, before_over, before_live):
        """After a step of the statement ``stmt``; before_*: its done, race_over and live entries before the step."""
        P = stmt.P
        ran = (before_done == 0) & np.repeat(before_over == 0, P)
        self.crashes += int((ran & (stmt.done == 1)).sum())
        ended = (before_over == 0) & (stmt.race_over != 0)
        self.attrition += int((ended & (stmt.race_over == 1)).sum())
        self.truncation += int((ended & (stmt.race_over == 2)).sum())
        spawned = before_over != 0
        self.respawned += int(spawned.sum())
        changed = (before_live != stmt.live).reshape(-1, P).any(1)
        stale = (stmt.live != stmt.pending).reshape(-1, P).any(1) & (stmt.race_over == 0) & ~spawned
        self.mixed_adoption += int((spawned & changed).any() and stale.any())

    def ok(self, need_mixed=False):
        return (self.crashes >= 1 and self.attrition >= 1 and self.truncation >= 1 and self.clamped >= 1 and self.seen > 0
                and self.differ >= 0.9 * self.net_answers > 0 and (self.mixed_adoption >= 1 or not need_mixed))

    def __str__(self):
        return ("%d crashes, %d races ended by attrition and %d by truncation, %d re-spawns, %d member answers clamped, "
                "%d rays changed by other cars, %d of %d member answers differ from another entered member's, %d calls "
                "with a re-seated and a stale race" % (self.crashes, self.attrition, self.truncation, self.respawned,
                                                       self.clamped, self.seen, self.differ, self.net_answers,
                                                       self.mixed_adoption))
