/* scanlib_track_drive.h — track progress in the closed-loop roll-outs, and the fitness and standings built on it.  An
 * extension of scanlib_league.h (which it includes, and with it scanlib.h, whose conventions it keeps: every function
 * returns RL_OK or a negative rl_status, rl_last_error names the reason).
 * pyracecarsimulator_amd/_lib.py restates it in TRACK_DRIVE_SYMBOLS; tests/track_drive_statement.py restates the rules
 * below on top of tests/track_statement.py.
 *
 * ---- why -------------------------------------------------------------------------------------------------
 * The roll-outs (rl_car_drive_followgap, rl_car_race_followgap, rl_car_drive_policy, rl_car_race_seats,
 * rl_car_drive_population, rl_car_race_league) are where things are scored, and every score they give is made of
 * travel_dist and crash ticks: a car that spins in a free area scores like one that drives down the track, and a
 * league's winner is the car that outlived and out-travelled the others, not the one that is ahead.  With a track
 * attached to the car handle the same calls also place every car on the track after every step it takes.
 * Opt-in: a car handle with no track attached runs exactly the launches it ran before, and with a track every output of
 * the roll-out itself (first_crashed, states_out, the traces, fitness_n2, standings_N4) keeps its meaning and bits.
 *
 * ---- the rule --------------------------------------------------------------------------------------------
 * scanlib.h's section "track progress" holds here: its projection, the d2 tie rule (the lowest index among equals),
 * the `window` candidates around the previous segment, the +-L wrap and the lap count.  All of it is f64 and every
 * operation is separately rounded.
 * A car's PLACEMENTS are its start state (states_in) and then the state after the step of every tick t it reaches.
 *   The start state is fresh: all segments are searched, progress = 0, laps = 0, s_prev = s0.
 *   A car reaches the ticks t = 0 ... first_crashed when it crashes and 0 ... n_ticks - 1 otherwise: the rows of
 *   states_trace that are not NaN.  The step of the crash tick counts, as it does in travel_dist and in the env.
 *   At each such tick: the candidates are the segments within `window` of the previous nearest segment;
 *   D = wrap(s - s_prev); laps += the crossing (+1 forwards over the start line, -1 backwards); progress += D;
 *   s_prev = s.  A frozen car (after its crash tick) changes nothing.
 * goal_tick is the first tick t after whose placement progress >= goal_dist, or -1 when there is none.
 * In a race call (group P): offset = wrap(s0 - s0 of car 0 of the race), with no lap counted; race_dist = offset +
 *   progress; rank = the number of cars k' of the race with a larger race_dist, or an equal one and k' < k, taken after
 *   the last tick, wrecks included.  Outside races offset = 0 (race_dist = 0 + progress) and rank = 0.
 * What the caller reads, per car: an f64 row [4] = (s0, s, progress, race_dist) and an int row [4] = (segment, laps,
 *   goal_tick, rank).
 * A car whose position is not a number: track_nearest's rule (every d2 is NaN: the first candidate), and s is NaN (u is
 *   NaN and stays so; fmin / fmax do not drop it here).  Its progress reads NaN after the first tick, its goal_tick -1,
 *   and it beats nobody.
 *
 * ---- the calls -------------------------------------------------------------------------------------------
 * rl_car_attach_track: t is borrowed (keep it alive as long as it is attached); a null t detaches and p is not read.
 *   window as rl_track_params'; goal_dist == 0 means the track length L.  Attaching or detaching forgets the rows of
 *   the last tracked call.
 *   Refused (RL_ERR_INVALID, the handle usable as before and what was attached still attached): null p with a track;
 *   window < 0 or > 65536; goal_dist negative or not finite; a track on another device than the car; a multi-device
 *   car handle.
 * rl_car_read_track: the rows of the last tracked call's cars, host pointers, each optional.  n_cars must equal that
 *   call's R (n_races group for a race), otherwise RL_ERR_INVALID; also RL_ERR_INVALID before any tracked call and
 *   with no track attached.  The roll-outs are synchronous, so the reads are plain copies under the car's mutex.
 * rl_car_read_track_scores: what the last tracked call left.
 *   After rl_car_drive_population n_rows = n, n_cols = 3:
 *     [m][0] the sum of progress over the member's E cars, in ascending car order from +0.0, each addition rounded;
 *     [m][1] the number of its cars with goal_tick >= 0;
 *     [m][2] the sum of (double)goal_tick over those cars, ascending.
 *   After rl_car_race_league n_rows = n_members, n_cols = 4:
 *     [m][0] the number of cars member m entered;
 *     [m][1] the sum of their progress, in ascending car index as standings_N4 sums gain;
 *     [m][2] the number of them with goal_tick >= 0;
 *     [m][3] the sum over them of the number of cars of the same race with a strictly smaller race_dist, in a plain
 *            f64 compare: ties and NaN beat nobody.
 *   A member that entered no car reads four zeros.
 *   Refused (RL_ERR_INVALID): after any other tracked call (or none), with the wrong shape, a null pointer.
 * A tracked roll-out that fails leaves nothing to read.
 *
 * Per call with a track: drive_track_kernel<true> on the start states, drive_track_kernel<false> ahead of every
 * tick's scan (one wave per car, 8 cars per workgroup, a frozen car's wave returns at once), and after the last tick
 * drive_track_rank_kernel (one lane per car) and, for a population or a league, drive_track_fitness_kernel or
 * drive_track_standings_kernel (one lane per member: the order of the sums is the contract); drive_track_kernels.h.
 *
 * Out of scope: rl_mcts_drive, which has its own track (scanlib_track_plan.h); device-pointer forms; off-track
 *   termination; multi-device handles; graph capture; a tally by track progress in rl_env_*.                        */
#ifndef SCANLIB_TRACK_DRIVE_H
#define SCANLIB_TRACK_DRIVE_H

#include "scanlib_league.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rl_drive_track_params { int window; double goal_dist; } rl_drive_track_params;
int rl_car_attach_track(rl_car *c, rl_track *t, const rl_drive_track_params *p);
int rl_car_read_track(rl_car *c, int n_cars, double *rows_n4, int *ints_n4);
int rl_car_read_track_scores(rl_car *c, int n_rows, int n_cols, double *scores);

#ifdef __cplusplus
}
#endif
#endif
