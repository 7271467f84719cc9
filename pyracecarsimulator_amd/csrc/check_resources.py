#!/usr/bin/env python3
"""Build gate: the register / occupancy budget of the kernels whose speed depends on it, read from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (the Makefile keeps them per translation unit in .obj/*.remarks).

The march loops pin physical VGPRs in inline assembly and the stream kernels are held at 64 VGPRs / 80 SGPRs so that
eight waves share a SIMD (profiles/r05/sgpr_cap_ab.txt: 92 SGPRs cost the eighth wave and 25 % of the rate).  A compiler
bump that silently spends one register more would not fail a parity test — it fails the build here instead.
usage: check_resources.py <dir with *.remarks> [--print]"""
import os
import re
import subprocess
import sys

# (substring of the demangled kernel name, {limit: value}); every kernel matching a pattern must satisfy it
BOUNDS = [
    ("scan::rm_fan_stream_kernel<", {"vgpr": 64, "sgpr": 80, "occupancy": 8}),
    # the plain-range production shapes (two rays per lane, 1024 lanes, float32 or code map) keep nothing in scratch
    ("scan::rm_fan_stream_kernel<false, false, 1024, true, true, 2, false,", {"scratch": 0}),
    ("scan::rm_fan_stream_kernel<false, false, 1024, false, true, 2, false,", {"scratch": 0}),
    ("scan::lut_fan_lds_kernel<", {"vgpr": 56, "sgpr": 96, "occupancy": 8, "scratch": 0}),
    # its origin-corrected twin (option lut_refine): the beam table in LDS and the per-pose offsets fit the same eight waves
    ("scan::lut_fan_lds_refine_kernel<", {"vgpr": 64, "sgpr": 96, "occupancy": 8, "scratch": 0}),
    ("scan::cddt_theta_search2_kernel", {"vgpr": 64, "sgpr": 80, "occupancy": 8, "scratch": 0}),
    ("scan::cddt_theta_fan_kernel", {"vgpr": 32, "sgpr": 96, "occupancy": 8, "scratch": 0}),
    ("scan::cddt_fan_bins_kernel", {"vgpr": 64, "sgpr": 80, "occupancy": 8, "scratch": 0}),
    ("scan::bl_fan_stream_kernel<false, 1024>", {"vgpr": 56, "sgpr": 96, "occupancy": 8, "scratch": 0}),
    ("scan::rm_leftover_kernel<", {"vgpr": 48, "occupancy": 8, "scratch": 0}),
    # closed-loop roll-outs, every steering source (FollowGap, the network, the seat table): scan, crash compare, FollowGap or the network's answer and the f64
    # car step in one wave per car, no spills
    ("scan::drive_tick_kernel<", {"scratch": 0}),
    ("scan::drive_start_kernel", {"scratch": 0}),
    # the driving environment: the spawn / step lane and the observe wave keep nothing in scratch
    ("scan::env_step_kernel", {"scratch": 0}),
    ("scan::env_observe_kernel<", {"scratch": 0}),
    # the race environment: the same lane and wave with the race's rule around them
    ("scan::race_env_step_kernel", {"scratch": 0}),
    ("scan::race_env_observe_kernel<", {"scratch": 0}),
    # ... with drivers in its seats: the scripted pair's select chain and FollowGap's passes behind the ballot spill nothing
    ("scan::race_env_seat_step_kernel", {"scratch": 0}),
    ("scan::race_env_seat_observe_kernel<", {"scratch": 0}),
    # ... with a league: the per-car entry, the adoption at a spawn and the results' columns behind the barrier spill nothing
    ("scan::race_env_league_step_kernel", {"scratch": 0}),
    ("scan::race_env_league_observe_kernel<", {"scratch": 0}),
    # track progress: the f64 search, the wave's (value, index) minimum and lane 0's trigonometry spill nothing
    ("scan::track_kernel<", {"scratch": 0}),
    # track progress of the roll-outs: the same search per car and tick, the per-race rank and the one-lane-per-member
    # track scores spill nothing
    ("scan::drive_track_kernel<", {"scratch": 0}),
    ("scan::drive_track_rank_kernel", {"scratch": 0}),
    ("scan::drive_track_fitness_kernel", {"scratch": 0}),
    ("scan::drive_track_standings_kernel", {"scratch": 0}),
    # the policy network: the micro-tile accumulators stay in registers
    ("scan::policy_mlp_kernel", {"scratch": 0}),
    ("scan::policy_mlp_rows_kernel", {"scratch": 0}),
    # policy populations: the same body a member at a time, the re-layout of theta and the one-lane-per-member fitness sum
    ("scan::policy_mlp_pop_kernel", {"scratch": 0}),
    ("scan::policy_pop_pack_kernel", {"scratch": 0}),
    ("scan::policy_pop_fitness_kernel", {"scratch": 0}),
    # league races: the grouping's ballot walks and offsets scan, the network over the device's workgroup table, and the
    # one-lane-per-member standings (the LeagueSteer tick is one of the drive_tick_kernel< rows above)
    ("scan::league_count_kernel", {"scratch": 0}),
    ("scan::league_offsets_kernel", {"scratch": 0}),
    ("scan::league_fill_kernel", {"scratch": 0}),
    ("scan::policy_mlp_league_kernel", {"scratch": 0}),
    ("scan::league_standings_kernel", {"scratch": 0}),
    ("scan::drive_tick_kernel<20, scan::LeagueSteer>", {"scratch": 0}),
    # the MCTS planner: the descent, the act wave, the backup's pairwise sum and the walks keep nothing in scratch
    ("scan::mcts_start_kernel", {"scratch": 0}),
    ("scan::mcts_select_kernel", {"scratch": 0}),
    ("scan::mcts_act_kernel<", {"scratch": 0}),
    ("scan::mcts_backup_kernel", {"scratch": 0}),
    ("scan::mcts_best_kernel", {"scratch": 0}),
    ("scan::mcts_advance_kernel", {"scratch": 0}),
    ("scan::mcts_ucb_probe_kernel", {"scratch": 0}),
    # track-guided planning: the roots' wave and the term workgroup spill nothing, and eight waves share a SIMD
    ("scan::plan_root_kernel", {"scratch": 0, "occupancy": 8}),
    ("scan::plan_term_kernel", {"scratch": 0, "occupancy": 8}),
    # the track steering the search: the one-lane answer and the roll-out's wave (searches in 64 lanes, the f64 car steps
    # in lane 0) spill nothing.  The roll-out holds the search and the car step live at once: 199 VGPRs, two waves per
    # SIMD, which is its whole 8-wave workgroup on a compute unit (rollout_kernel alone is 128 VGPRs)
    ("scan::mcts_pursuit_answer_kernel", {"scratch": 0, "occupancy": 8}),
    ("scan::rollout_pursuit_kernel", {"scratch": 0, "occupancy": 2}),
    # batched races: the outline raster, and the race scan's march with the other cars' cells folded into each sample
    ("scan::outline_cells_kernel", {"scratch": 0}),
    ("scan::race_fan_kernel<", {"scratch": 0}),
    # ... and its CDDT form (option race_cddt): the bucket search and the fold of the other cars' cells spill nothing
    ("scan::race_cddt_kernel", {"scratch": 0}),
    # particle-filter weights: the fused march + sensor-model product spills nothing; eight waves per SIMD in the
    # canonical form, seven in the literal one (its libm-exact trig holds 106 SGPRs)
    ("scan::pf_weight_kernel<false>", {"scratch": 0, "occupancy": 8}),
    ("scan::pf_weight_kernel<true>", {"scratch": 0, "occupancy": 7}),
    # particle-filter localisation: the passes around the weight call are short f64 loops, none of them spills
    ("scan::mcl_motion_kernel", {"scratch": 0}),
    ("scan::mcl_weight_kernel", {"scratch": 0}),
    ("scan::mcl_norm_kernel", {"scratch": 0}),
    ("scan::mcl_base_kernel", {"scratch": 0}),
    ("scan::mcl_resample_kernel", {"scratch": 0}),
]
KEYS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}


def parse(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            rows.append(cur)
            continue
        for key, short in KEYS.items():
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur is not None and short not in cur:
                cur[short] = int(m.group(1))
    if rows:
        names = subprocess.run(["c++filt"] + [r["mangled"] for r in rows], capture_output=True, text=True).stdout.splitlines()
        for r, n in zip(rows, names):
            r["name"] = n.split("(")[0].replace("void ", "")
    return rows


def check(rows):
    bad, seen = [], {p: 0 for p, _ in BOUNDS}
    for r in rows:
        for pat, lim in BOUNDS:
            if pat not in r.get("name", ""):
                continue
            seen[pat] += 1
            for k, v in lim.items():
                got = r.get(k, -1)
                ok = got >= v if k == "occupancy" else 0 <= got <= v
                if not ok:
                    bad.append("%s: %s = %d, budget %s %d" % (r["name"], k, got, ">=" if k == "occupancy" else "<=", v))
    for pat, n in seen.items():
        if n == 0:
            bad.append("no kernel matches the budget pattern %r (renamed? update check_resources.py)" % pat)
    return bad


def main(argv):
    d = argv[1] if len(argv) > 1 else ".obj"
    text = ""
    for f in sorted(os.listdir(d)):
        if f.endswith(".remarks"):
            text += open(os.path.join(d, f), errors="replace").read()
    rows = parse(text)
    if not rows:
        print("check_resources: no kernel-resource-usage remarks under %s" % d, file=sys.stderr)
        return 2
    if "--print" in argv:
        for r in rows:
            print("%-92s VGPR %3d SGPR %3d scratch %3d occupancy %d" % (r["name"][-92:], r.get("vgpr", -1), r.get("sgpr", -1),
                                                                      r.get("scratch", -1), r.get("occupancy", -1)))
    bad = check(rows)
    for b in bad:
        print("check_resources: " + b, file=sys.stderr)
    if not bad:
        print("check_resources: %d kernels, every register / occupancy budget holds" % len(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
