/* scanlib_league.h — league races: members of a policy population as per-race seat drivers.  An extension of
 * scanlib_population.h and scanlib_seats.h (which it includes, and with them scanlib.h, whose conventions it keeps:
 * every function returns RL_OK or a negative rl_status, rl_last_error names the reason).
 * pyracecarsimulator_amd/_lib.py restates it in LEAGUE_SYMBOLS; tests/league_statement.py restates the rules below.
 *
 * ---- the league ------------------------------------------------------------------------------------------
 * Seats (scanlib_seats.h) put different drivers into one race, but every race of a call shares one seat table with at
 * most one network.  Populations (scanlib_population.h) run N networks in one launch, but car r must belong to member
 * first + r / E and every car drives alone.  Self-play over a population, tournaments and ratings, and the scoring of
 * checkpoints against each other need R races at once, each with its OWN line-up drawn from one population: the batched
 * form of the reference's two-player setup (scripts/two_player/) with a network in both cars.
 * An ENTRY names the driver of one scan row or car: m >= 0, member m of the population; -1, nobody (an evaluation) or
 * FollowGap (a race).  Entries come in any order; nothing that has no league changes.
 *
 * ---- row-indexed evaluation ------------------------------------------------------------------------------
 * rl_policy_pop_eval_rows (host pointers, synchronous) and rl_policy_pop_eval_rows_device (device pointers, only
 *   enqueued on hip_stream): scans [n][size], member [n] -> steers [n].
 *   Scan row i is answered by member member[i].  The answer is bit for bit rl_policy_eval of an rl_policy created from
 *   that member's theta: rl_policy_pop_eval's oracle, and with member[i] = first + i / E that call's bits.
 *   A row with member[i] == -1 is not answered: its element of steers keeps its bits (the host form uploads the
 *   caller's steers first, so that such rows come back unchanged).
 *   The host form refuses an entry outside [-1, n_members).  The device form cannot look at the entries: it treats an
 *   out-of-range entry as -1, by construction (the grouping below matches rows against members 0 ... n_members - 1 and
 *   an entry that is none of them is in no segment), and never reads outside the weight block.  d_member_n must not be
 *   written while the call's launches are in flight.  The device form sets the handle's foreign-stream flag as
 *   rl_policy_pop_eval_device does.
 *   Per call: the grouping, three launches (league_kernels.h) — league_count_kernel, one wave per member walking
 *   member[] in 64-row steps (a ballot and its popcount); league_offsets_kernel, one workgroup's exclusive scan over
 *   the members; league_fill_kernel, the same walk filling the row list, ordered by member and ascending by row inside
 *   each member (no atomic decides a slot), and a workgroup table with one entry per 8 rows of a member — then
 *   policy_mlp_league_kernel over that table, whose length only the device knows: the grid is the host's upper bound
 *   ceil(n / 8) + min(n, n_members) and a workgroup past the device's total returns at once.
 *
 * ---- the league roll-out ---------------------------------------------------------------------------------
 * rl_car_race_league: rl_car_race_seats' loop, bit for bit, in everything but the source of a car's answer (the race
 *   scan, noise offsets, the crash test, wrecks, traces, NaN rows and chunking are unchanged).  The arguments from
 *   states_in to states_trace_or_null are rl_car_race_seats'.  Car r P + k (P = group) is driven by entry[r P + k]:
 *     -1      FollowGap g: (double)FollowGap::eval of the whole scan, never clipped;
 *     m >= 0  member m of pop: the network's f32 output widened, clamped to +-steer_clip when steer_clip > 0
 *             (fmin(fmax(s, -clip), clip)).
 *   `steers` records the raw f32 answer.  The network is evaluated for the cars with an entry >= 0 only, wrecks
 *   included, as the seats do.  The entries are grouped once per call, before the first tick, never per tick.
 *   Identities: every entry -1 equals rl_car_race_followgap bit for bit; the same single member m in the same seats of
 *   every race (FollowGap in the others) equals rl_car_race_seats with an rl_policy of member m's theta; group = 1
 *   with entry[r] = first + r / E equals rl_car_drive_population.
 *   standings_N4 (optional, float64 [n_members][4], for EVERY member of the population), with gain(r) =
 *   states_out[r][8] - states_in[r][8] (index 8: travel_dist in getState layout) and alive(r) = the crash tick of car r,
 *   or n_ticks when it never crashed:
 *     [m][0] the number of cars member m entered;
 *     [m][1] the sum of gain over those cars, in ascending car index, from +0.0, every addition separately rounded;
 *     [m][2] how many of them have first_crashed >= 0;
 *     [m][3] the sum over them of the number of cars of the same race that the car beats: car a beats car b when
 *            alive(a) > alive(b), or when the two are equal and gain(a) > gain(b), in plain f64 comparisons; ties and
 *            NaN beat nobody.
 *   A member that entered no car reads four zeros.
 *   Per tick: race_fan_kernel, policy_mlp_league_kernel (when an entry >= 0 exists), drive_tick_kernel with the entry
 *   array as the steering source; after the last tick league_standings_kernel, one lane per member.
 *
 * Errors (RL_ERR_INVALID, nothing launched, the handles usable as before): a null required pointer (c, h, pop, the
 *   entries; member, scans, steers); a -1 entry with a null g; an entry outside [-1, n_members); n < 0; size below
 *   in_start + dims[0], and num_rays below it when an entry >= 0 exists; n size or n_races group num_rays >= 2^31; group
 *   outside [1, 8]; handles on different devices or multi-device handles; everything rl_car_race_seats and
 *   rl_car_drive_population refuse, with their codes.  n == 0 and n_races == 0 are RL_OK and launch nothing.
 *
 * Out of scope: leagues in rl_env_*; a placing by track progress in standings_N4 itself (with a track attached to the
 *   car handle the roll-out has it: scanlib_track_drive.h, rl_car_read_track_scores); a device-pointer form of the
 *   roll-out; members of different architectures; multi-device handles.                                              */
#ifndef SCANLIB_LEAGUE_H
#define SCANLIB_LEAGUE_H

#include "scanlib_population.h"
#include "scanlib_seats.h"

#ifdef __cplusplus
extern "C" {
#endif

int rl_policy_pop_eval_rows(rl_policy_pop *pop, int n, const int *member_n, const float *scans, int size, float *steers);
int rl_policy_pop_eval_rows_device(rl_policy_pop *pop, int n, const int *d_member_n, const float *d_scans, int size,
                                   float *d_steers, void *hip_stream);
int rl_car_race_league(rl_car *c, rl_method *h, rl_followgap *g_or_null, rl_policy_pop *pop, const int *entry_RP,
                       double steer_clip, const double *states_in, const double *speeds, const float *steer0_or_null,
                       int n_races, int group, int n_ticks, double dt, double scan_dist_to_base, float fov, int num_rays,
                       const double *edge, double crash_thresh, int *first_crashed, double *states_out_or_null,
                       double *velocities_or_null, float *steers_or_null, float *scan_poses_or_null,
                       double *states_trace_or_null, double *standings_N4_or_null);

#ifdef __cplusplus
}
#endif
#endif
