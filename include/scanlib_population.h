/* scanlib_population.h — policy populations: N steering networks in one launch and one roll-out.  An extension of
 * scanlib.h (which it includes and whose conventions it keeps: every function returns RL_OK or a negative rl_status,
 * rl_last_error names the reason).  pyracecarsimulator_amd/_lib.py restates it in POP_SYMBOLS;
 * tests/population_statement.py restates the rules below.
 *
 * ---- the population ------------------------------------------------------------------------------------
 * Evolution strategies, CMA-ES, population-based search and the scoring of a directory of checkpoints all run MANY
 * networks on the same starts.  A POPULATION is n_members networks of one architecture; the caps and the meaning of
 * n_layers, dims, relu, in_start, clip and scale are rl_policy_create's.
 * A MEMBER is one flat float32 parameter vector theta of P = sum_l (dims[l] + 1) dims[l+1] values: for l = 0 ...
 *   n_layers - 1, W[l] as dims[l] x dims[l+1] row-major, then b[l].  (The reference's network: P = 79 297.)
 * rl_policy_pop_create: all members zeroed (every answer is the all-zero network's).  RL_ERR_NOMEM when the device
 *   block cannot be had.  rl_policy_pop_destroy gives it back.
 * rl_policy_pop_layout: n_members and P (either out-pointer may be null).
 * rl_policy_pop_set: members [first, first + n) from host memory, theta_nP [n][P]; synchronous.
 * rl_policy_pop_set_device: the same from device memory; only enqueued on hip_stream.  The handle remembers that a
 *   caller's stream has work on it (rl_policy_pop_eval_device on a caller's stream counts too): the next call that
 *   launches on another stream waits for the device first, as rl_env's device forms do.
 *   Both setters run one re-layout kernel (policy_pop_pack_kernel) into the padded device layout of rl_policy_create;
 *   members outside [first, first + n) keep their bits, and the padding is never written after create has zeroed it.
 * rl_policy_pop_get: theta_P [P] of one member, exactly the bits that were set.
 *
 * ---- evaluation ----------------------------------------------------------------------------------------
 * rl_policy_pop_eval (host pointers, synchronous) and rl_policy_pop_eval_device (device pointers, enqueued on
 *   hip_stream): scans [n E][size] -> steers [n E] with E = cars_per_member.
 *   Scan row i, i < n E, is answered by member first + i / E.
 *   Each answer is bit for bit rl_policy_eval of an rl_policy created from that member's theta: the canonical
 *   k-ordered fmaf chain of scanlib.h ("the steering policy network").  No tiling can change it; this is the whole
 *   oracle.
 *   One launch: policy_mlp_pop_kernel, n x ceil(E / 8) workgroups; a workgroup's cars all belong to one member.
 *
 * ---- the closed loop -----------------------------------------------------------------------------------
 * rl_car_drive_population: rl_car_drive_policy's arguments and outputs with R = n E cars, behind c, h, pop, first, n,
 *   cars_per_member and steer_clip.  It is that call's loop (the same noise offsets walking the global ray id
 *   t R num_rays + r num_rays, the same chunking, the same traces, the same steer_clip clamp); the one difference:
 *   car r's steer at every tick comes from member first + r / E.
 *   With one member every output is rl_car_drive_policy's bits.
 *   fitness_n2 (optional, float64 [n][2]), for member m of the call:
 *     [m][0] the sum over its E cars, in ascending car order, every addition separately rounded (from +0.0), of
 *            states_out[r][8] - states_in[r][8] (index 8: travel_dist in getState layout);
 *     [m][1] the number of its cars with first_crashed >= 0.
 *   Per tick: the scan, policy_mlp_pop_kernel, drive_tick_kernel with the network as the steering source; after the
 *   last tick policy_pop_fitness_kernel, one lane per member (E is small and the order is the contract).
 *
 * Errors (RL_ERR_INVALID unless said otherwise; nothing launched, the handles usable as before): a null required
 *   pointer; n_members < 1; first < 0, n < 0 or first + n > n_members; cars_per_member < 1; size or num_rays below
 *   in_start + dims[0]; n E size (n E num_rays) >= 2^31; handles on different devices or multi-device handles;
 *   everything rl_policy_create and rl_car_drive_policy refuse, with their codes (RL_ERR_UNSUPPORTED beyond the
 *   caps).  n == 0 is RL_OK and launches nothing.
 *
 * Out of scope: populations as seat drivers (scanlib_seats.h), in rl_env_*, or as the MCTS source; a device-pointer
 *   form of the roll-out; members of different architectures.                                                       */
#ifndef SCANLIB_POPULATION_H
#define SCANLIB_POPULATION_H

#include "scanlib.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rl_policy_pop rl_policy_pop;

int rl_policy_pop_create(int device, int n_members, int n_layers, const int *dims, const unsigned char *relu,
                         int in_start, float clip, float scale, rl_policy_pop **out);
void rl_policy_pop_destroy(rl_policy_pop *pop);
int rl_policy_pop_layout(rl_policy_pop *pop, int *n_members, int *n_params);
int rl_policy_pop_set(rl_policy_pop *pop, int first, int n, const float *theta_nP);
int rl_policy_pop_set_device(rl_policy_pop *pop, int first, int n, const float *d_theta_nP, void *hip_stream);
int rl_policy_pop_get(rl_policy_pop *pop, int member, float *theta_P);
int rl_policy_pop_eval(rl_policy_pop *pop, int first, int n, int cars_per_member, const float *scans, int size,
                       float *steers);
int rl_policy_pop_eval_device(rl_policy_pop *pop, int first, int n, int cars_per_member, const float *d_scans, int size,
                              float *d_steers, void *hip_stream);
int rl_car_drive_population(rl_car *c, rl_method *h, rl_policy_pop *pop, int first, int n, int cars_per_member,
                            double steer_clip, const double *states_in, const double *speeds,
                            const float *steer0_or_null, int n_ticks, double dt, double scan_dist_to_base, float fov,
                            int num_rays, const double *edge, double crash_thresh, int *first_crashed,
                            double *states_out_or_null, double *velocities_or_null, float *steers_or_null,
                            float *scan_poses_or_null, double *states_trace_or_null, double *fitness_n2_or_null);

#ifdef __cplusplus
}
#endif
#endif
