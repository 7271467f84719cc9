/*
 * scanlib.h — C ABI of libscan_amd.so: the MI355X (gfx950) 2D lidar range library.
 *
 * Drop-in boundary for the ONE hot path of felrock/PyRacecarSimulator:
 *   ScanSimulator2D.scan / scanMany            scripts/scan_simulator.py:88-135
 *     -> range_libc.PyOMap / PyRayMarching / PyRayMarchingGPU / PyCDDTCast
 *        .calc_range_many(...)                  scripts/scan_simulator.py:72-76,103-106,130-133
 *                                               scripts/two_player/scan.py:45-46,69-70
 * range_libc is a Cython module; its FFI for this path is "float32 C-contiguous
 * numpy buffers + scalars" (SURVEY.md §8b).  Every entry point below is what a
 * ctypes / Cython stub for that path binds (INTEGRATION.md shows the stubs).
 *
 * Rules of the boundary
 *   - plain pointers and sizes only; no C++/torch types; nothing throws across it;
 *   - every function returns RL_OK (0) or a negative rl_status; rl_last_error()
 *     gives the thread-local message of the last failure;
 *   - host-pointer entry points are synchronous (results are in the caller's buffer
 *     on return) and never retain the pointers; *_device entry points take device
 *     pointers + a hipStream_t (as void*) and only enqueue work;
 *   - there is NO CPU fallback: without a usable HIP device rl_map_create fails.
 *   - a handle may be shared by threads (each call locks the handle), as the
 *     reference's rospy callbacks do (scripts/ros_interface.py:115,142,189);
 *     rl_map_update waits for every scan in progress on the map's methods (host calls
 *     hold a shared lock until their results have landed; launches the *_device entry
 *     points left in flight are waited for with a device synchronisation);
 *   - streams: *_device calls on ONE method handle may use different streams and then run
 *     concurrently on the GPU (that is how bench.py pipelines consecutive pose batches).
 *     Per-launch scratch is kept per stream (rl_launch_contexts() = 8 streams per handle without any
 *     synchronisation, more are served after a device synchronisation), lazily built
 *     tables are guarded by events.  The caller's own buffers (poses, ranges) are the
 *     caller's to order.  A stream must not be destroyed while a launch enqueued on it
 *     through this library is still running.
 *
 * Coordinates: occ[r*cols + c], r = row = world y, c = col = world x, row 0 at the
 * smallest world y (the layout of nav_msgs/OccupancyGrid.data that PyOMap reads).
 */
#ifndef SCANLIB_H
#define SCANLIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rl_map rl_map;        /* replaces range_libc.PyOMap                */
typedef struct rl_method rl_method;  /* replaces range_libc.Py<RangeMethod>       */

typedef enum rl_status {
    RL_OK = 0,
    RL_ERR_INVALID = -1,     /* bad argument (null pointer, size, kind, ...)      */
    RL_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range         */
    RL_ERR_HIP = -3,         /* a HIP runtime call failed (message has details)   */
    RL_ERR_UNSUPPORTED = -4, /* e.g. num_rays larger than the kernel's LDS fan    */
    RL_ERR_NOMEM = -5
} rl_status;

/* Range methods.  Names follow range_libc's classes. */
typedef enum rl_kind {
    RL_BRESENHAM = 0,   /* BresenhamsLine: LDS-tiled bit-packed occupancy march (K2)   */
    RL_RM = 1,          /* PyRayMarching    scan_simulator.py:72-73  step_coeff 0.999  */
    RL_RM_GPU = 2,      /* PyRayMarchingGPU scan_simulator.py:74-76  step_coeff 1.0    */
    RL_CDDT = 3,        /* PyCDDTCast       two_player/scan.py:46                      */
    RL_GIANT_LUT = 4    /* GiantLUTCast: u16 [row][col][theta] table, fan-contiguous   */
} rl_kind;

/* ---- library -------------------------------------------------------------- */
const char *rl_version(void);
const char *rl_last_error(void);          /* thread-local, never NULL              */
int rl_device_count(void);                /* 0 when no HIP device is usable        */

/* ---- map: range_libc.PyOMap(map_msg)  scripts/ros_interface.py:210 ----------
 * occ: rows*cols bytes, nonzero = occupied (the reference feeds {0,255} after its
 * binarisation, scripts/ros_interface.py:80-86; PyOMap tests data > 10).
 * res/ox/oy/oyaw: map_msg.info.resolution / origin position / yaw
 * (scripts/ros_interface.py:212-220).  The exact Euclidean distance transform
 * (range_libc DistanceTransform) is built on the device at creation.           */
int rl_map_create(const uint8_t *occ, int rows, int cols, float res, float ox, float oy,
                  float oyaw, int device, rl_map **out);
/* ---- several devices behind ONE handle (SURVEY.md section 8b "device_mask") -----------------------
 * The reference's caller of this path is ONE Python process (scripts/mcts.py:237 ->
 * scripts/racecar_simulator_v2.py:146-167 -> scripts/scan_simulator.py:113-135), so a drop-in that wants
 * the other GPUs of the node cannot ask it to become N processes.  rl_map_create_multi uploads the map to
 * every device of `devices` (an index may repeat: several contexts on one GPU) and builds the tables on
 * each; rl_method_create on that map returns a handle whose HOST-pointer entry points —
 * rl_calc_range_fan, rl_calc_range_many_fan, rl_calc_range_many, rl_check_collision_many,
 * rl_check_collision_groups, rl_car_rollout_check — cut the batch into contiguous pose blocks, one per
 * device (a device is brought in per `multi_min_poses` = 512 poses, option of the handle), run them
 * concurrently (one worker thread per device, nothing is forked) and let every device write its block of
 * the results straight into the caller's buffer.  Results are bit-identical to the single-device call:
 * noise is keyed by the global ray id, crash indices are global.  With a result buffer from
 * rl_host_alloc every device stores over its own PCIe link (4 B per ray) and nothing touches xGMI, so the
 * host-pointer scan is EXPECTED to scale with the number of links — modelled, not measured: the pool's boxes have one
 * GPU, the tests name device 0 several times there (and distinct devices wherever more are visible); the crash forms
 * return 4 B per roll-out.
 * The *_device entry points take device memory of ONE device: call them with rl_method_replica(h, i)
 * (a borrowed per-device handle; rl_map_replica likewise).  rl_map_update updates every replica.        */
int rl_map_create_multi(const uint8_t *occ, int rows, int cols, float res, float ox, float oy, float oyaw,
                        const int *devices, int n_devices, rl_map **out);
int rl_map_n_devices(const rl_map *m);                 /* 1 for a map of rl_map_create                    */
/* ... and with the results in DEVICE memory of one of the handle's devices (round 6): the reference's consumer of a
 * roll-out batch is one process (scripts/mcts.py:237 -> scripts/racecar_simulator_v2.py:146-167 -> Car::isCrashed); when
 * what comes next is itself a kernel on ONE GPU (a policy network, the tree update), the ranges — or the fused crash
 * indices — of every device should land in that GPU's HBM, not in host memory.  h: a method of a multi-device map;
 * poses (and edge): HOST pointers; `consumer`: index of the replica (0 .. rl_method_n_devices - 1) whose device owns
 * d_outs_on_consumer (n_poses * num_rays floats) / d_first_on_consumer (n_groups ints).  Every device marches its
 * contiguous pose block into its own HBM in `chunks` pieces (0 = 4) and sends each piece to the consumer with
 * hipMemcpyPeerAsync on a second stream — device to device over xGMI where peer access exists — while the next piece
 * marches; the consumer's own block is marched in place.  Synchronous: the data is in the consumer's memory on return.
 * Bit-identical to the single-device scan (noise keyed by the global ray id, crash indices global).  Tested with
 * repeated device indices on one GPU (the peer copy degenerates to a device-to-device copy) and with distinct devices
 * wherever more than one is visible; rates over xGMI are MODELLED, not measured.                 */
int rl_calc_range_fan_multi_device(rl_method *h, const float *poses, int n_poses, float fov, int num_rays, int consumer,
                                   float *d_outs_on_consumer, int chunks);
int rl_check_collision_groups_multi_device(rl_method *h, const float *poses, int n_groups, int group, float fov,
                                           int num_rays, const double *edge, double crash_thresh, int consumer,
                                           int *d_first_on_consumer);
rl_map *rl_map_replica(rl_map *m, int i);              /* NULL when i is out of range                     */
/* replace the occupancy (same shape) and rebuild the distance transform: the
 * per-scan rebuild of scripts/two_player/rcs_two_player.py:110-121 and the
 * updateMap stub of scripts/scan_simulator.py:81-86.  Methods created from the
 * map see the new data (CDDT / GiantLUT tables are rebuilt lazily).            */
int rl_map_update(rl_map *m, const uint8_t *occ);
/* ... the two-player tick without the grid crossing PCIe (round 6): the occupancy becomes the BASE map — as created or
 * last rl_map_update'd — with the n cells flat_idx[i] = row * cols + col set to `value` (nonzero = occupied; the
 * reference writes 255), and every table is rebuilt on the device.  Indices outside the grid are skipped, as the
 * reference's own guard skips them (rcs_two_player.py:113).  A stamp replaces the previous one (`ego_map[:] = org_map`,
 * rcs_two_player.py:110).  n = 0 restores the base map.                                                                */
int rl_map_stamp_cells(rl_map *m, const int32_t *flat_idx, int n, uint8_t value);
void rl_map_destroy(rl_map *m);
int rl_map_rows(const rl_map *m);
int rl_map_cols(const rl_map *m);
int rl_map_device(const rl_map *m);
/* test hooks: copy the device-built tables back (float32 rows*cols / u8 rows*cols) */
int rl_map_get_dt(rl_map *m, float *dt_out);
int rl_map_get_occ(rl_map *m, uint8_t *occ_out);

/* ---- method: range_libc.PyRayMarching(omap, mrx) etc. -----------------------
 * max_range_px: scripts/racecar_simulator_v2.py:196 (int(scan_max_range/res));
 * theta_disc: only for RL_CDDT / RL_GIANT_LUT (two_player/rcs_two_player.py:121). */
int rl_method_create(rl_map *m, int kind, float max_range_px, int theta_disc, rl_method **out);
void rl_method_destroy(rl_method *h);
int rl_method_kind(const rl_method *h);
int rl_method_n_devices(const rl_method *h);           /* devices behind the handle (rl_map_create_multi)  */
rl_method *rl_method_replica(rl_method *h, int i);     /* per-device handle for the *_device entry points  */

/* upstream 2-arg calc_range_many(ins, outs): one (x, y, theta) world row per ray.
 * scripts/two_player/scan.py:69-70.  ins: n*3 floats, outs: n floats (metres).  */
int rl_calc_range_many(rl_method *h, const float *ins_n3, float *outs_n, int n);

/* the fork's 4-arg calc_range_many(ins, outs, fov, num_rays) exactly as the
 * reference calls it (scripts/scan_simulator.py:103-106,130-133): ins has n_rows =
 * n_poses*num_rays rows of 3 floats, pose p lives in row p*num_rays (all other rows
 * are ignored), beam j of pose p is cast at theta_p - fov/2 + j*fov/num_rays and
 * written to outs[p*num_rays + j] (layout consumed by racecar/src/racecar.cpp:320).
 * Only the n_poses live rows cross PCIe.                                         */
int rl_calc_range_many_fan(rl_method *h, const float *ins_rows3, float *outs, int n_rows,
                           float fov, int num_rays);

/* dense form of the same call: poses[p*3..] -> outs[p*num_rays + j].
 * hit_cells (2 ints per ray: col,row or -1,-1) and steps (samples per ray) are
 * optional diagnostics for RL_RM / RL_RM_GPU / RL_BRESENHAM; pass NULL otherwise. */
int rl_calc_range_fan(rl_method *h, const float *poses_p3, int n_poses, float fov, int num_rays,
                      float *outs, int32_t *hit_cells_or_null, uint16_t *steps_or_null);

/* Optional: pinned host memory for result buffers.  A host-pointer scan whose `outs` lies inside a
 * block from rl_host_alloc is written by the kernel directly (no staging copy on the way back:
 * scanMany(200) 63 -> ~40 us) up to 2^21 rays per call and by DMA from HBM beyond that (faster from ~2000 poses up).  ScanSimulator2D keeps its cached output vectors
 * (scripts/scan_simulator.py:32-40) in such blocks.  rl_host_free waits for the device first.      */
int rl_host_alloc(size_t bytes, void **out);
int rl_host_free(void *p);

/* device-resident, asynchronous forms (pointers are device memory on the map's
 * device, stream is a hipStream_t or NULL for the default stream).               */
int rl_calc_range_fan_device(rl_method *h, const float *d_poses_p3, int n_poses, float fov,
                             int num_rays, float *d_outs, int32_t *d_hit_cells_or_null,
                             uint16_t *d_steps_or_null, void *hip_stream);
int rl_calc_range_many_device(rl_method *h, const float *d_ins_n3, float *d_outs_n, int n,
                              void *hip_stream);

/* Gaussian range noise (scripts/scan_simulator.py:33,109; scan_std params.yaml:32):
 * out += N(0, std) from a counter-based generator keyed by (seed, global ray id +
 * ray_offset) so a sharded batch reproduces the unsharded one.  std <= 0 disables. */
int rl_set_noise(rl_method *h, float std, uint64_t seed, uint64_t ray_offset);

/* Fused crash test (Car::isCrashed racecar/src/racecar.cpp:305-328 over the output
 * of scanMany, scripts/racecar_simulator_v2.py:146-167): scans n_poses poses and
 * returns in *first_crashed the index of the first pose with any beam j where
 * (double)range - edge[j] < crash_thresh, else -(n_poses+1).  ranges_or_null gets
 * the ranges too when non-NULL.  edge: num_rays doubles (setCarEdgeDistances).     */
int rl_check_collision_many(rl_method *h, const float *poses_p3, int n_poses, float fov,
                            int num_rays, const double *edge, double crash_thresh,
                            int *first_crashed, float *ranges_or_null);

/* The same test per roll-out of a batch: poses holds n_groups roll-outs of `group` consecutive
 * poses (scripts/mcts.py:228-231 stores 200 per roll-out); first_crashed[g] = index inside
 * roll-out g of its first crashed pose, else -(group+1).  Works for every range method.       */
int rl_check_collision_groups(rl_method *h, const float *poses_p3, int n_groups, int group,
                              float fov, int num_rays, const double *edge, double crash_thresh,
                              int *first_crashed, float *ranges_or_null);

/* device-resident, asynchronous form: every pointer is device memory, d_first_crashed gets
 * n_groups ints; d_ranges_or_null may be NULL for RL_RM / RL_RM_GPU (the test is fused into the
 * march kernel, ranges need not be stored at all) and is required scratch for the other methods. */
int rl_check_collision_groups_device(rl_method *h, const float *d_poses_p3, int n_groups, int group,
                                     float fov, int num_rays, const double *d_edge,
                                     double crash_thresh, int *d_first_crashed,
                                     float *d_ranges_or_null, void *hip_stream);

/* ---- origin-corrected GiantLUT query (option lut_refine) -----------------------------------------
 * The GiantLUT casts every table row from the integer corner (c, r) of its cell, and the default query reads the row of
 * ((int)gx, (int)gy): every pose is moved by (fx, fy) in [0, 1)^2, 0.71 cell on average, and about 78 % of its rays land
 * within one cell of exact ray marching.  rl_method_set_option(h, "lut_refine", v) — 0 = off, the default; any other value
 * stores 1 — makes every query path of an RL_GIANT_LUT handle (rl_calc_range_fan and everything that scans through it,
 * rl_calc_range_many, the repeat-angle scans, sensor-model weights and rl_pf_*) read the row of the NEAREST corner and
 * take the pose's offset from it, projected on the beam, off the entry.  The table, its bytes per query and its cache
 * protocol are the default's; the rule costs one dt probe per pose and a few FMAs per ray.  With the option at 0 the
 * handle launches what it always did.  Other kinds store the option and ignore it (as lut_debug).
 *
 * The contract (tests/lut_refine_statement.py states it in NumPy).  Every operation is a separately rounded float32
 * unless written as fma.  For a pose, (gx, gy, thg) = world_to_grid(...):
 *   outside the map (the default's test: !(gx >= 0 && gx < cols && gy >= 0 && gy < rows)): max_range * res for every beam.
 *   otherwise  c0 = (int)gx, r0 = (int)gy;
 *              cn = min((int)rintf(gx), cols - 1), rn = min((int)rintf(gy), rows - 1)     (rintf: ties to even)
 *              (c, r) = (cn, rn), unless dt[rn * cols + cn] == 0.0f (that corner's cell is occupied): then (c0, r0)
 *              fx = gx - (float)c, fy = gy - (float)r                                     (exact, in [-0.5, 1))
 *   per beam   b = the default's bin of the default's angle: thg + fan_alpha(f, j) for the fan, thg for a row of
 *                  rl_calc_range_many, thg + angles[j] for repeat angles
 *              q = lut[(r * cols + c) * theta_disc + b],  t = (float)q * dequant
 *              q == 0 (the corner is in a wall) and q == 65535 (a miss) pass through: px = t
 *              otherwise the direction is canonical ray marching's:
 *                  (st, ct) = det_sincosf(thg), (sa, ca) = det_sincosf(alpha), alpha = fan_alpha(f, j) or angles[j],
 *                  dx = fma(ct, ca, -(st sa)), dy = fma(st, ca, ct sa);
 *                  a row (x, y, theta) of rl_calc_range_many: (dy, dx) = det_sincosf(thg);
 *              p = fma(fx, dx, fy dy),  px = fminf(fmaxf(t - p, 0.0f), max_range)
 *              range = px * res, then the handle's noise, keyed exactly as without the option.
 * The dt probe reads the handle's live map: after rl_map_update / rl_map_stamp_cells the corner choice follows the new
 * distance transform, and the table is rebuilt before the next launch as always.
 * Consequences: a pose on integer grid coordinates in a free cell gives the default's bits (fx = fy = 0); a repeat-angle
 * scan with angles[j] = fma((float)j, inc, amin) equals the refined fan bit for bit; a direction table holding
 * det_sincosf(fan_alpha(f, j)) gives the bits of computing it per beam (the LDS fan kernel keeps one per workgroup).
 * Measured against exact ray marching (docs/history/lut_refine.md): within one cell 0.78 -> 0.97 of the rays of poses
 * with two cells of clearance, 0.76 -> 0.92 of wall-hugging poses; median error 0.63 -> 0.011 cell.               */

/* ---- scan consumer: Follow-the-Gap steering --------------------------
 * Replaces followgap.PyFollowGap(ws, md, ma, angle_inc).eval(lidar, size)
 * (followgap/followgap.pyx:23-31 -> FollowGap::eval, followgap/followgap.hpp:104-129; built at
 * scripts/mcts.py:97-99, scripts/two_player/simple_driver.py:31, called at scripts/mcts.py:267,
 * simple_driver.py:51) for a BATCH of scans: n_scans rows of `size` float32 ranges in, one
 * steering angle per scan out, one wave per scan.  Bit-identical to the reference's compiled
 * header (tests/golden/followgap_ref.npz).  size < 10 -> RL_ERR_INVALID (the reference indexes
 * out of bounds there); a gap consisting of the single last beam reads beam size-1 where the
 * reference reads one past the array.  Scans of up to 1280 beams run the one-bit-per-beam kernel
 * (consumer_kernels.h: followgap_bits_kernel), longer ones the per-beam walk (followgap_kernel);
 * RL_FOLLOWGAP_WALK=1 in the environment at create time forces the walk (A/B, diagnostics).      */
typedef struct rl_followgap rl_followgap;
int rl_followgap_create(int device, int window_size, float max_distance, float max_angle,
                        float angle_inc, rl_followgap **out);
void rl_followgap_destroy(rl_followgap *g);
int rl_followgap_eval(rl_followgap *g, const float *scans, int n_scans, int size, float *angles);
/* scans and angles resident on the device (e.g. the ranges a scan call just wrote)              */
int rl_followgap_eval_device(rl_followgap *g, const float *d_scans, int n_scans, int size,
                             float *d_angles, void *hip_stream);

/* ---- roll-out pose generator ---------------------------------------
 * The step in front of scanMany in MCTS.rollout (scripts/mcts.py:214-231): 200 x
 * {Car::control, Car::updatePosition(dt)} (racecar/src/racecar.cpp:53-98,118-237,294-303) per
 * roll-out, one GPU lane per roll-out in float64.
 * car_params: the 17 constructor arguments of Car in order (racecar/include/racecar.hpp:32-36).
 * states: 11 doubles per roll-out in Car::getState layout (racecar.cpp:355-376).
 * actions: (speed, steer) pairs, ceil(n_steps/action_every) per roll-out.                      */
typedef struct rl_car rl_car;
int rl_car_create(int device, const double *car_params17, rl_car **out);
/* the same over several devices (pair it with a method of rl_map_create_multi on the SAME device list):
 * rl_car_rollout and rl_car_rollout_check then cut the roll-outs into contiguous blocks, one per device  */
int rl_car_create_multi(const int *devices, int n_devices, const double *car_params17, rl_car **out);
void rl_car_destroy(rl_car *c);
/* poses_out: n_rollouts*n_steps*3 float32 (x, y, theta of the car after each step);
 * states_out (optional): final states; velocities_out (optional): state[3] after each step.   */
int rl_car_rollout(rl_car *c, const double *states_in, const double *actions, int n_rollouts,
                   int n_steps, int action_every, double dt, float *poses_out,
                   double *states_out_or_null, double *velocities_out_or_null);
/* roll-outs -> poses -> scan -> per-roll-out crash index without the poses or the ranges ever
 * leaving the device: what MCTS.rollout + checkCollisionMany compute (scripts/mcts.py:202-245,
 * scripts/racecar_simulator_v2.py:146-167), for n_rollouts roll-outs in one call.              */
int rl_car_rollout_check(rl_car *c, rl_method *h, const double *states_in, const double *actions,
                         int n_rollouts, int n_steps, int action_every, double dt, float fov,
                         int num_rays, const double *edge, double crash_thresh, int *first_crashed,
                         double *states_out_or_null, double *velocities_out_or_null);

/* ---- closed-loop Follow-the-Gap roll-outs ---------------------------------------------------
 * The reference's driving loop, where each tick's steering angle comes from that tick's scan: the simulator
 * tick (scripts/ros_interface.py:119-148: updatePose(), runScan(), checkCollision() >= 0 is a crash) answered
 * by the driver (scripts/two_player/simple_driver.py:31,48-53, scripts/follow_the_gap.py:
 * PyFollowGap(10, 15.0, max_steer, 0.004).eval(ranges), then drive(VELOCITY, angle)); MCTS.act runs the same
 * tick with generateActionFromFG (scripts/mcts.py:187-200,262-267).  R cars, T ticks, nothing leaves the device
 * between ticks.
 *
 * Inputs per car: a start state (11 doubles, getState layout), a constant speed (simple_driver.py's VELOCITY)
 * and an initial steer (steer0_or_null; null = 0).  dt is the step (0.01 in racecar_simulator_v2.py:126),
 * scan_dist_to_base where the lidar sits (0.275, params.yaml:36), fov / num_rays / edge / crash_thresh the
 * scan and crash test.  c, h and g are ordinary handles on ONE device (multi-device handles are refused).
 *
 * Tick t = 0 ... T-1, for every car still alive:
 *   1. Car::control + Car::updatePosition(dt) with (speed, steer) — car_kernels.h car_step;
 *   2. the lidar pose of Car::getScanPose (racecar.cpp:378-387): (x + d cos th, y + d sin th, th) in f64,
 *      cast to f32 as ScanSimulator2D.scan does;
 *   3. the scan of that pose with h: any kind, its options and its noise, the noise keyed by the global ray
 *      id with ray offset h.ray_offset + (t R + r) num_rays (so T ticks in one call equal T/2 + T/2 with the
 *      offset advanced by T/2 R num_rays, the states and the last steer chained);
 *   4. Car::isCrashed on that one scan (racecar.cpp:305-328): a beam with (double)range - edge[j] <
 *      crash_thresh sets first_crashed[r] = t and freezes the car — it is not stepped again;
 *   5. otherwise steer = FollowGap::eval(ranges, num_rays), bit-identical to rl_followgap_eval, cast to
 *      double for the next tick's control.
 * simple_driver.py clips the angle to +-0.4189 before drive(); with g's max_angle <= the car's MAX_STEER_ANG
 * (as the reference builds it) that clip never acts, and it is not applied here.  mcts.py:195 tests
 * checkCollision() > 0, which a single scan never returns (0 or -2); the loop follows ros_interface.py:144
 * (>= 0).
 *
 * Outputs: first_crashed[R] = the crash tick or -(T+1) (isCrashed's convention); states_out (optional) =
 * the state after the last step taken (the crash tick's for a crashed car).  Optional per-tick traces, row
 * r t of [R, T]: velocities (state[3] after the step, MCTS's reward), steers (f32; NaN on the crash tick),
 * scan_poses (3 f32), states_trace (11 f64).  Rows after a car's crash tick are NaN.
 *
 * Errors (RL_ERR_INVALID, all three handles stay usable): null pointers, n_ticks <= 0, num_rays outside
 * [10, 1280] (the one-bit-per-beam FollowGap kernel), R num_rays >= 2^31, handles on different devices,
 * multi-device handles.  R = 0 does nothing.  Synchronous; h's options and noise offset read the same after
 * the call.  Per tick: the fan launch sequence of h's planner, then one drive_tick_kernel with FollowGap as the
 * steering source (drive_kernels.h).                                                                          */
int rl_car_drive_followgap(rl_car *c, rl_method *h, rl_followgap *g, const double *states_in,
                           const double *speeds, const float *steer0_or_null, int n_rollouts, int n_ticks,
                           double dt, double scan_dist_to_base, float fov, int num_rays, const double *edge,
                           double crash_thresh, int *first_crashed, double *states_out_or_null,
                           double *velocities_or_null, float *steers_or_null, float *scan_poses_or_null,
                           double *states_trace_or_null);

/* ---- batched multi-car races ----------------------------------------------------------------------------
 * The reference's second simulator (scripts/two_player/): every car steps, then every car scans
 * (ros_interface_two_player.py:156-187), each scan with the other car's outline written into a copy of the grid and
 * the tables rebuilt (rcs_two_player.py:99-126); simple_driver.py steers each car with FollowGap.  Here R independent
 * races of `group` = P cars (1 <= P <= 8) share one static map: N = R P cars, race-major (car k of race r is car r P + k).
 *
 * Exactness.  The EDT is sqrtf((float)d2) of the integer squared distance to the nearest occupied cell, so for extra
 * cells S stamped on the grid  dt_{grid u S}(q) = min(dt_grid(q), sqrtf((float)min_{c in S} |q - c|^2))  bit for bit.
 * The march reads the map only through dt[row, col]; the race kernel (race_kernels.h, one workgroup per race, the
 * race's outline cells in LDS) replaces that read with the min above.  Ranges, hit cells and step counts equal "stamp
 * the other cars (rl_map_stamp_cells), rebuild, scan" bit for bit, with no per-race table.
 *
 * The canonical car outline (rl_car_outline_cells; the race kernel rasterises with the same device function; the host
 * statement is tests/race_statement.py).  The rectangle Car::getBound means to trace (racecar.cpp:389-459), centred on
 * the state's (x, y), LENGTH along the heading and WIDTH across it, at half-cell spacing:
 *   (s, c) = det_sincosf((float)theta) widened to double (oracle.sincosf on the host);
 *   corners in the car frame (L/2, W/2), (-L/2, W/2), (-L/2, -W/2), (L/2, -W/2); edge e runs from corner e to corner
 *   e+1 mod 4 with n_e points k = 0 ... n_e-1 at u = k / n_e, n_e = max(1, ceil(len_e / (0.5 res))) on the host in
 *   double (len_e = L for edges 0 and 2, W for 1 and 3); a = a0 + (a1 - a0) u, b likewise;
 *   xw = x + (c a - s b), yw = y + (s a + c b);
 *   gx0 = (xw - ox) inv_res, gy0 = (yw - oy) inv_res with inv_res = 1.0 / res in double and the map's float32
 *   res, ox, oy widened; gx = wa_cos gx0 - wa_sin gy0, gy = wa_sin gx0 + wa_cos gy0 (MapParams' wa_cos / wa_sin);
 *   col = floor(gx), row = floor(gy), kept inside the grid; non-finite points are skipped.
 * Every operation is a separately rounded IEEE double (the library is built with -ffp-contract=off).  The outline is
 * a set of cells: order and duplicates carry no meaning.  At most 512 points per car (RL_ERR_UNSUPPORTED beyond): the
 * default 0.4064 x 0.2032 m car takes 2 (17 + 9) = 52 at 0.05 m per cell.  Maps of 32768 or more cells a side are
 * refused (RL_ERR_UNSUPPORTED).
 *
 * Deliberate divergences from the reference:
 *   - each car sees the others, not itself: rcs_two_player.py:105-116 stamps the scanned player's own bound too,
 *     which would put its lidar inside an obstacle;
 *   - getBound's defects are not reproduced: bound[i] / bound[i+1] overwrite each other, the points are not
 *     translated to the car's position, and floatPosToPix adds +width / +height;
 *   - races run on ray marching (RM, RMGPU) and, with option race_cddt, on CDDT (below); not on the other tables;
 *   - a crashed car stays in the map as a wreck at its crash-tick state.
 *
 * Races on CDDT (option race_cddt; the kernel is cddt_kernels.h race_cddt_kernel, the host statement
 * tests/race_cddt_statement.py).  rl_method_set_option(h, "race_cddt", v) — 0 = off, the default; any other value
 * stores 1; readable through rl_method_get_info; a handle's own option, not part of rl_plan_opts; it goes to every
 * replica of a multi-device handle; kinds other than RL_CDDT store and ignore it.  With 0 an RL_CDDT handle is refused
 * by every race entry point, as before.  With 1 the race scan of an RL_CDDT handle is the following, and every call
 * built on the race scan (rl_car_race_followgap, _seats, _league, the race environment with seats, league line-ups
 * and a track, the track-progress roll-outs) takes it; ticks, noise offsets, crash ballot, wrecks, traces and
 * chunking stay as they are.
 *   Car i of a race scans against S_i, the set of outline cells of the OTHER cars of its race (rl_car_outline_cells'
 *   set, taken from the f64 states or cars_p3 exactly as the ray-marching race scan takes it).  For table bin t, with
 *   cs, sn, trans, width the static table's values of that bin, a cell (r, c) of S_i behaves as the table build
 *   treats an edge cell:
 *     px = (float)c + 0.5f, py = (float)r + 0.5f;
 *     slx = fma(px, cs, -(py sn)), sly = fma(px, sn, py cs) + trans;  half = (|sn| + |cs|) 0.5f;
 *     upper = (int)((sly + half) - 1e-5f), lower = (int)((sly - half) + 1e-5f), clamped to [0, width - 1];
 *     the cell covers bucket b iff lower <= b <= upper.
 *   A ray's bin is the CDDT query's, unchanged: the nearest bin of -heading, flipped by theta_disc / 2 into the
 *   table's half turn (with the guard for odd theta_disc); lx, ly its origin's projection, and max_range at once when
 *   ly lies outside [0, width).  With b = (int)ly let F be the static bucket's values plus slx of every cell of S_i
 *   that covers b.  Forward: x* = min{x in F : x >= lx}, range_px = fminf(x* - lx, max_range); flipped:
 *   x* = max{x in F : x <= lx}, range_px = fminf(lx - x*, max_range); max_range when no such x exists.  Then times
 *   res, plus the handle's noise keyed by the global ray id as in the ray-marching race scan.  A group of 1 equals
 *   rl_calc_range_fan of the same poses bit for bit.  No per-race table is built: the static bucket is searched once
 *   per (car, table bin) and the others' cells are folded into its two extrema.
 *   Relation to "stamp, rebuild, scan" — a deliberate divergence.  The statement equals stamping S_i
 *   (rl_map_stamp_cells), rebuilding the table and scanning, bit for bit, when both hold:
 *     (i)  every cell of S_i is an edge cell of grid u S_i (OMap::make_edge_map's 4-neighbour rule: occupied, and on
 *          the border or with a free 4-neighbour);
 *     (ii) every static edge cell is still an edge cell of grid u S_i.
 *   Where they fail — a car overlapping a wall, a wreck flush against a wall, two interlocking outlines — the
 *   rebuild drops entries the statement keeps.  On a 96-cell maze 352 of 400 line-ups with the others at least 7
 *   cells off the walls meet both and no ray differs; with the others thrown anywhere, walls included, 8 of 58 200
 *   rays differ, 0.014 % (docs/history/race_cddt.md; tests/test_race_cddt_host.py measures both).
 *   Refused with RL_ERR_UNSUPPORTED: RL_GIANT_LUT and RL_BRESENHAM whatever the option says; hit cells or step counts
 *   from an RL_CDDT handle, as the plain fan refuses them for the table kinds; group x theta_disc > 8192 (the kernel
 *   keeps that many per-bin ranges, 32 KiB, in LDS next to the outlines' 16 KiB).  Multi-device handles: RL_ERR_INVALID.
 *
 * rl_car_outline_cells: n cars (x, y, theta rows in double) on m with c's LENGTH / WIDTH -> per car its cells
 * row * cols + col (points whose cell repeats the point before dropped), counts[i] of them, -1 past the count in a row
 * of max_cells.  Errors (RL_ERR_INVALID): null pointers, n < 0, max_cells below the car's point count, handles on
 * different devices or multi-device.
 *
 * rl_calc_range_fan_cars (+ _device on device pointers, asynchronous on `hip_stream`): pose i of group g (poses_p3 row
 * g group + i, float32 world x, y, theta as rl_calc_range_fan takes them) is scanned as h scans it on the grid with the
 * outline cells (length x width) of the OTHER group - 1 cars of group g stamped: cars_p3 rows g group + k, k != i, each
 * (x, y, theta) in double.  outs / hits / steps as rl_calc_range_fan's, n_groups group num_rays rays.  Kinds RL_RM and
 * RL_RM_GPU; variant 3 (RL_RM's default) marches with the upstream-literal arithmetic (rm_literal_kernel), variants 0
 * and 1 with the canonical one (rm_march); h's step coefficient, max range and noise apply, the noise keyed by the
 * global ray id h.ray_offset + p num_rays + j as in the plain fan.  K1b planner options (slots, code map, tiles, ...)
 * do not apply and are ignored.  A group of 1 equals rl_calc_range_fan of the same poses bit for bit.
 * Errors (the handle stays usable): RL_ERR_INVALID for null pointers, group outside [1, 8], num_rays outside
 * [10, 1280], n_groups group num_rays >= 2^31, multi-device handles, a non-positive length or width;
 * RL_ERR_UNSUPPORTED for RL_CDDT (unless option race_cddt is set: "Races on CDDT" above), RL_GIANT_LUT and RL_BRESENHAM
 * (their tables cover the whole map: the single-race two_player.ScanSimulator2D with a stamp stays their path),
 * variant 2, and outlines of more than 512 points.
 *
 * rl_car_race_followgap: rl_car_drive_followgap's loop (same arguments with n_rollouts = n_races group, same outputs,
 * traces, NaN rows, noise offsets per tick, chunking and option restore) in which every tick's scan is the race scan
 * above: every car of every race steps, then every car scans with the other cars of its race in the map, read from
 * their f64 states on the device (c's LENGTH / WIDTH).  Then rl_car_drive_followgap's drive_tick_kernel: the crash
 * ballot, FollowGap, the next step.  A crashed car freezes and stays in the map; a car that drives into another
 * crashes through its own scan, since the other car's cells fall inside its edge distances.  Nothing leaves the
 * device between ticks.  Errors: those of rl_calc_range_fan_cars and rl_car_drive_followgap, n_races < 0.        */
int rl_car_outline_cells(rl_car *c, rl_map *m, const double *cars_p3, int n, int max_cells, int32_t *cells,
                         int *counts);
int rl_calc_range_fan_cars(rl_method *h, const float *poses_p3, const double *cars_p3, int n_groups, int group,
                           double length, double width, float fov, int num_rays, float *outs,
                           int32_t *hit_cells_or_null, uint16_t *steps_or_null);
int rl_calc_range_fan_cars_device(rl_method *h, const float *d_poses_p3, const double *d_cars_p3, int n_groups,
                                  int group, double length, double width, float fov, int num_rays, float *d_outs,
                                  int32_t *d_hit_cells_or_null, uint16_t *d_steps_or_null, void *hip_stream);
int rl_car_race_followgap(rl_car *c, rl_method *h, rl_followgap *g, const double *states_in, const double *speeds,
                          const float *steer0_or_null, int n_races, int group, int n_ticks, double dt,
                          double scan_dist_to_base, float fov, int num_rays, const double *edge, double crash_thresh,
                          int *first_crashed, double *states_out_or_null, double *velocities_or_null,
                          float *steers_or_null, float *scan_poses_or_null, double *states_trace_or_null);

/* ---- particle-filter weights --------------------------------------------------------------------
 * The calls range_libc was written for, Monte-Carlo localisation: every particle casts the SAME n_angles beams and
 * is weighted by a sensor model.  range_libc's source is not on the reference mount; what is said about upstream here
 * is recollection ([UPSTREAM-RECALL]) of RangeLibc.pyx: calc_range_repeat_angles, set_sensor_model,
 * eval_sensor_model, calc_range_repeat_angles_eval_sensor_model.  The contract below is what this library pins.
 *
 * Ray layout.  Ray j of particle p is outs[p * n_angles + j], cast from the world pose ins_p3 row p (x, y, theta) at
 * heading theta_p + angles[j]; angles: n_angles float32, shared by all particles [UPSTREAM-RECALL:
 * numpy_calc_range_angles].
 *
 * Arithmetic.  Each kind keeps the arithmetic of its fan with the fan's alpha_j replaced by angles[j]:
 *   RL_RM / RL_RM_GPU, variants 0 and 1 (canonical): (sa, ca) = det_sincosf(angles[j]), (st, ct) = det_sincosf(thg),
 *     dx = fma(ct, ca, -(st sa)), dy = fma(st, ca, ct sa), then the canonical march (rm_march);
 *   RL_RM / RL_RM_GPU, variant 3 (literal): the upstream-literal cast at theta_p + angles[j], the sum rounded to
 *     float32 once;
 *   RL_CDDT: the CDDT query at thg + angles[j];   RL_GIANT_LUT: the table bin of thg + angles[j];
 *   RL_BRESENHAM and variant 2: RL_ERR_UNSUPPORTED.
 * Fan equivalence — the pin to the oracle: a repeat-angle scan is bit-identical to rl_calc_range_fan of the same poses
 * when angles[j] = fma((float)j, inc, amin) for the canonical and table kinds, and angles[j] = amin + (float)j * inc,
 * each operation rounded to float32, for the literal kind (amin = -0.5f fov, inc = fov / (float)num_rays) — ranges,
 * and hit cells / steps where given (RL_RM / RL_RM_GPU only; RL_ERR_UNSUPPORTED for the table kinds).
 * The handle's step coefficient, max range, variant and noise apply; the noise key is the global ray id
 * h.ray_offset + p * n_angles + j.  K1b planner options (slots, code map, tiles, ...) do not apply and are ignored,
 * as for the race scan; the GiantLUT / CDDT debug bits (option lut_debug) are ignored too.
 *
 * Sensor model [UPSTREAM-RECALL: eval_sensor_model].  rl_set_sensor_model copies `table`, width x width doubles,
 * row = observed bin, column = expected bin, to h's device (synchronous).  Setting a table again replaces and frees
 * the old one (after the device has drained); the table dies with the method handle.  For a float32 value v in metres
 *   bin(v) = (int) fminf(fmaxf(v * inv_res, 0.0f), (float)(width - 1)),
 * inv_res the map's float32 (float)(1.0 / res) that the world -> grid transform uses.  NaN gives bin 0 (fmaxf returns
 * its other argument); upstream's behaviour there is undefined.  The weight of particle p:
 *   w = 1.0;  for j = 0 ... n_angles - 1 in ascending order:  w *= table[bin(obs[j]) * width + bin(range[p, j])]
 * — each product its own IEEE double rounding, no tree, no log domain.  obs: n_angles float32 (the observed scan);
 * rl_eval_sensor_model reads ranges laid out as above (n_particles * n_angles float32) and writes n_particles doubles.
 * rl_calc_range_repeat_angles_eval_sensor_model is the scan and the evaluation in one call: it uses exactly the float32
 * value the unfused scan would have stored (range_px * res, plus noise if set), so fused and unfused weights are the
 * same bits.  Which path each kind takes: RL_RM / RL_RM_GPU run ONE kernel (pf_weight_kernel: march, table lookup, the
 * factors parked in LDS, one lane per particle forming the product; the only global write is 8 B per particle);
 * RL_CDDT / RL_GIANT_LUT run the repeat-angle scan into scratch owned by the handle and then the evaluation kernel.
 * rl_method_last_plan is not touched by these calls.
 *
 * The *_device forms take device pointers and only enqueue on `hip_stream` (NULL: the default stream); the others
 * take host pointers and are synchronous.
 * Errors (the handle stays usable).  RL_ERR_INVALID: null pointers, n_particles < 0, n_angles outside [1, 2048],
 * n_particles * n_angles >= 2^31, width outside [2, 2048], evaluating before a table is set, multi-device handles
 * (use rl_method_replica).  n_particles = 0 does nothing.                                                              */
int rl_calc_range_repeat_angles(rl_method *h, const float *ins_p3, int n_particles, const float *angles, int n_angles,
                                float *outs, int32_t *hit_cells_or_null, uint16_t *steps_or_null);
int rl_calc_range_repeat_angles_device(rl_method *h, const float *d_ins_p3, int n_particles, const float *d_angles,
                                       int n_angles, float *d_outs, int32_t *d_hit_cells_or_null,
                                       uint16_t *d_steps_or_null, void *hip_stream);
int rl_set_sensor_model(rl_method *h, const double *table, int width);
int rl_eval_sensor_model(rl_method *h, const float *obs, const float *ranges, int n_angles, int n_particles,
                         double *weights);
int rl_eval_sensor_model_device(rl_method *h, const float *d_obs, const float *d_ranges, int n_angles, int n_particles,
                                double *d_weights, void *hip_stream);
int rl_calc_range_repeat_angles_eval_sensor_model(rl_method *h, const float *ins_p3, int n_particles,
                                                  const float *angles, const float *obs, int n_angles,
                                                  double *weights);
int rl_calc_range_repeat_angles_eval_sensor_model_device(rl_method *h, const float *d_ins_p3, int n_particles,
                                                         const float *d_angles, const float *d_obs, int n_angles,
                                                         double *d_weights, void *hip_stream);

/* ---- particle-filter localisation -----------------------------------------------------------------
 * The consumer of the calls above: a Monte-Carlo-localisation filter (mit-racecar's particle_filter.py, the program
 * range_libc's PF calls were written for) kept on the device.  rl_pf_run makes n_steps whole updates — motion,
 * likelihood, weights, estimate, resampling — with the odometry and the observations of all steps sent up once and no
 * host synchronisation or host-to-device copy between steps.  Every operation named below is one separately rounded
 * IEEE double unless it is marked f32 (the library is built with -ffp-contract=off); tests/mcl_statement.py is the same
 * step in NumPy and the device is bit-identical to it.
 *
 * rl_pf_create: a filter of n_particles particles casting the n_angles beams `angles` (float32, copied) on `h`.
 * h is borrowed and must outlive the filter; it needs a sensor model (rl_set_sensor_model) and a kind the fused weight
 * call serves (RL_RM, RL_RM_GPU, RL_CDDT, RL_GIANT_LUT; otherwise that call's RL_ERR_UNSUPPORTED).  The filter works on
 * h's stream; every call is synchronous; h's options and ray offset read the same after every call.
 * rl_pf_reset: X[p] = particles_p3 row p (x, y, theta; f64), w[p] = 1.0 / (double)P or the caller's weights taken as
 * given, t = 0, key = noise_key(seed) (the fold of rl_mcts_reset's seeds).  U(d, i) below is the planner's 53-bit
 * uniform: Philox-2x32-10 of counter (d, i) under key, ((out0 << 32 | out1) >> 11) 2^-53.
 *
 * One step.  t counts steps since the reset, so run(3) equals run(1) followed by run(2) bit for bit.
 *  1. Motion.  (dx, dy, dth) = odom row t, in the car frame.  (s, c) = det_sincosf((float)theta) widened to double;
 *       x' = (x + (c dx - s dy)) + std0 g0,   y' = (y + (s dx + c dy)) + std1 g1,   theta' = (theta + dth) + std2 g2
 *     with g_a = (sum of U(p, 64 t + 1 + 12 a + k) for k = 0 .. 11, ascending from 0.0) - 6.0: the twelve-uniform normal
 *     of Probabilistic Robotics, Table 5.4, whose bits a host reproduces.  An axis with std = 0 draws nothing
 *     and adds nothing.  Angles are not wrapped.
 *  2. Likelihood.  q[p] = ((float)x', (float)y', (float)theta'); L[p] is exactly
 *     rl_calc_range_repeat_angles_eval_sensor_model of q, angles and obs row t, with the ray offset h's offset at entry
 *     plus t P A (scan noise, when set, is fresh every step).
 *  3. omega[p] = w[p] L[p].
 *  4. Blocked sums, chunk size 256.  T_b = the sequential ascending sum of chunk b; bs(v) = the sequential ascending
 *     sum of the T_b; cum(v)[i] = B_b + s_i with B_b the sequential sum of T_0 .. T_(b-1) and s_i the inclusive partial
 *     sum inside the chunk.  W = bs(omega).  W NaN, +inf or not > 0: the step is degenerate, w[p] = 1 / P and bit 1 of
 *     the flags is set; otherwise w[p] = omega[p] / W.  The order is part of the contract (any other order gives other
 *     bits); at most 4096 chunk totals are summed by one lane.
 *  5. Estimate, before resampling.  neff = 1.0 / bs(w^2);  est = (bs(w x'), bs(w y'), bs(w ch), bs(w sh)) with
 *     (sh, ch) = det_sincosf((float)theta') widened.  The heading is atan2(est[3], est[2]), left to the caller: no atan2
 *     and no pow run on the device (a squash exponent is applied by the caller to the table, T ** (1 / squash)).
 *  6. Resample when neff < resample_ratio (double)P (ratio 0: never; ratio >= 2: always).  c = cum(w), S = its last
 *     element, u = U(0, 64 t), tau_i = ((u + (double)i) / (double)P) S, a_i = min(P - 1, number of k with c[k] <= tau_i)
 *     (c is non-decreasing for the non-negative weights of a sensor model: a bisection).  Then X <- X'[a], w <- 1 / P
 *     and bit 0 of the flags is set.  Otherwise a_i = i, X <- X', w stays.
 * rl_pf_run writes one row per step: est_t4 (n_steps x 4), neff_t, flags_t.  rl_pf_read returns the state after the
 * last step (particles, weights), that step's ancestors, c and L; each output pointer may be null.
 *
 * Errors (RL_ERR_INVALID; the handles stay usable): null required pointers, n_particles outside [1, 2^20], n_angles
 * outside [1, 2048], a negative or NaN std or ratio, n_steps < 0, t + n_steps > 2^26, rl_pf_run or rl_pf_read before a
 * reset, no sensor model set, multi-device handles.  n_steps = 0 does nothing.
 * Kernels: mcl_kernels.h (motion, weight multiply + chunk totals, normalise + estimate + in-chunk sums, chunk bases +
 * decision, ancestor search + gather) around launch_pf_weights; T steps are enqueued on one stream.             */
typedef struct rl_pf rl_pf;
typedef struct rl_pf_params {
    int n_particles, n_angles;
    double motion_std[3];
    double resample_ratio;
} rl_pf_params;
int rl_pf_create(rl_method *h, const rl_pf_params *p, const float *angles, rl_pf **out);
void rl_pf_destroy(rl_pf *f);
int rl_pf_reset(rl_pf *f, const double *particles_p3, const double *weights_or_null, uint64_t seed);
int rl_pf_run(rl_pf *f, int n_steps, const double *odom_t3, const float *obs_tA, double *est_t4, double *neff_t,
              int *flags_t);
int rl_pf_read(rl_pf *f, double *particles_p3, double *weights, int32_t *ancestors, double *cum, double *likelihood);

/* ---- the steering policy network ---------------------------------------------------------------
 * The reference's second steering source (scripts/policy.py:17-33, Policy.predict_action; driven at
 * scripts/policy_driver.py:30-49 and used by MCTS at scripts/mcts.py:252-256): a dense ReLU chain over the
 * window scan[in_start, in_start + dims[0]) of each scan, one steering angle out.  The reference's network is
 * 720 -> 64 -> 128 -> 128 -> 64 -> 1 with a ReLU after every layer but the last, in_start 180, clip = scale = 15.
 *
 * The canonical float32 form (every path is bit-identical to it: rl_policy_eval, rl_policy_eval_device,
 * rl_car_drive_policy, and the host statement tests/policy_statement.py):
 *   x_k   = (r <= clip) ? r / scale : 1.0f for r = scan[in_start + k]   (a correctly rounded f32 division; NaN and
 *           +inf give 1.0, as policy.py's `x if x <= 15.0 else 15.0`; equal to its f64 i/15.0 cast to f32)
 *   acc_j = +0.0f, then acc_j = fmaf(x_k, W[k][j], acc_j) for k = 0, 1, ..., K-1 in ascending order
 *   y_j   = acc_j + b_j (a separate rounding: MatMul then BiasAdd);  ReLU: y_j > 0 ? y_j : 0.0f
 *   steer = y_0 of the last layer.
 * No split-K, no tree sums.  TF sums in an unspecified order, so the reference's bits cannot be pinned; against a
 * float64 forward pass of the reference's weights this form differs by at most 3.8e-6 rad (p99 2.1e-6) over 20 000
 * synthetic scans (gated at 1e-5 in tests/test_policy_host.py).
 *
 * rl_policy_create: weights[l] is dims[l] x dims[l+1] row-major float32 (TF's MatMul operand), biases[l] has
 * dims[l+1] values, relu[l] != 0 puts a ReLU after layer l.  Caps (RL_ERR_UNSUPPORTED beyond them): 8 layers,
 * input width 1024, hidden widths 256, one output.  The weights are copied to the device.
 * rl_policy_eval: n_scans rows of `size` float32 ranges on the host in, n_scans steers out (synchronous).
 * rl_policy_eval_device: the same on device pointers, enqueued on the given stream (null = the null stream).
 * Errors (RL_ERR_INVALID; the handle stays usable): null pointers, n_scans < 0, size < in_start + dims[0].
 * Kernel: policy_mlp_kernel (policy_kernels.h), the whole chain in one launch.                           */
typedef struct rl_policy rl_policy;
int rl_policy_create(int device, int n_layers, const int *dims, const float *const *weights,
                     const float *const *biases, const unsigned char *relu, int in_start, float clip, float scale,
                     rl_policy **out);
void rl_policy_destroy(rl_policy *p);
int rl_policy_eval(rl_policy *p, const float *scans, int n_scans, int size, float *steers);
int rl_policy_eval_device(rl_policy *p, const float *d_scans, int n_scans, int size, float *d_steers,
                          void *stream_or_null);

/* closed-loop policy roll-outs: rl_car_drive_followgap's loop (same arguments, same outputs, same noise offsets
 * and chunking) with step 5 replaced by the network: steer = rl_policy_eval of the tick's scan.  steers_or_null
 * records that raw f32 output (NaN on the crash tick).  The car gets clamp((double)steer, -steer_clip,
 * steer_clip) with steer_clip > 0 (scripts/policy_driver.py:33, +-0.4189), otherwise (double)steer, which
 * Car::control clamps later (as scripts/mcts.py passes the raw output to drive()).  Errors (RL_ERR_INVALID, the
 * handles stay usable): those of rl_car_drive_followgap with p in g's place, and num_rays < in_start + dims[0].
 * Per tick: the fan launch sequence of h's planner, policy_mlp_kernel over every car's scan, then one
 * drive_tick_kernel with the network as the steering source (drive_kernels.h).                              */
int rl_car_drive_policy(rl_car *c, rl_method *h, rl_policy *p, const double *states_in, const double *speeds,
                        const float *steer0_or_null, int n_rollouts, int n_ticks, double dt, double scan_dist_to_base,
                        float fov, int num_rays, const double *edge, double crash_thresh, double steer_clip,
                        int *first_crashed, double *states_out_or_null, double *velocities_or_null,
                        float *steers_or_null, float *scan_poses_or_null, double *states_trace_or_null);

/* ---- the driving environment -------------------------------------------------------------------
 * The closed loops above with the steering source left to the caller: a vectorised, device-resident environment.
 * Every call takes one (speed, steer) pair per env and, for n_envs cars at once, steps them, scans them, tests them
 * for a crash, computes a reward and writes the observation; episode ends, truncation and re-spawning happen on the
 * device.  rl_car_drive_followgap and rl_car_drive_policy are closed special cases: fed FollowGap's or the network's
 * answers to its observations the environment reproduces their traces bit for bit (with their noise base set
 * n_envs num_rays above the environment's: the reset takes slot 0).  tests/env_statement.py restates this section.
 *
 * c and h are borrowed (keep them alive as long as the env) and sit on ONE device; h may be any kind, with its
 * options and its noise.  edge: num_rays doubles (rl_car_edge_distances).  starts_m11: the pool of start states,
 * n_starts rows in getState layout, copied at create.  The observation of an env is obs_count floats: beam
 * obs_start + i obs_stride of its scan for i < obs_count, raw metres (obs_scale = 0) or the policy network's input
 * form (r <= obs_clip) ? r / obs_scale : 1.0f (obs_scale > 0).
 *
 * Every f64 operation below is separately rounded (the library is built with -ffp-contract=off).
 * Counters: k counts the calls since the last reset (the reset itself is slot 0, the first step slot 1).  Per env:
 *   tick[e], episode[e], start_index[e] and done[e] in {0 running, 1 crashed, 2 truncated, 3 invalid action}.
 * Spawn of env e at episode q: state = starts[idx] with idx = start_index[e] when the caller gave start indices and
 *   q = 0, otherwise idx = min(M-1, (int)(U(e, q) * (double)M)), U the planner's 53-bit uniform (Philox-2x32-10
 *   under noise_key(seed) with counter (e, q), as in the MCTS section).
 * Reset: every env spawns with q = 0, tick = 0; then the f32 lidar pose of Car::getScanPose (as in the closed
 *   loops), the scan at ray offset base + e num_rays, and phase B below with every env "fresh".  A start inside the
 *   crash margin reads done = 1 at once.  base is h's ray offset at the reset.
 * Step k, phase A (env_step_kernel, one lane per env):
 *   done[e] != 0 and auto_reset: spawn with q = episode[e] + 1, tick = 0, the action is ignored, done = 0, the env
 *     is "fresh";
 *   done[e] != 0 without auto_reset: nothing changes (rl_car_drive_followgap's frozen car): it is scanned again at
 *     its last pose with this slot's noise;
 *   otherwise speed = (double)a[0], steer = (double)a[1]; if either is not finite: done = 3, the state is left as it
 *     is (no non-finite value reaches the car step or a lidar pose); else steer is clamped to +-steer_clip when
 *     steer_clip > 0 (fmin(fmax(steer, -clip), clip), as rl_car_drive_policy), `substeps` times Car::control +
 *     Car::updatePosition(dt) with (speed, steer), tick += 1, moved = travel_dist after - travel_dist before;
 *   every env then writes its f32 lidar pose.
 * Scan: all n_envs lidar poses with ray offset base + (k n_envs + e) num_rays.
 * Phase B (env_observe_kernel, one wave per env): Car::isCrashed on the scan; for an env that stepped or is fresh a
 *   hit sets done = 1; otherwise a stepped env with max_ticks > 0 and tick == max_ticks gets done = 2 (a crash on
 *   the max_ticks step reads 1).  reward (f32): (float)moved for a stepped env that did not crash; (float)crash_reward
 *   where this call's action set done to 1 (a stepped env) or 3; 0.0f for fresh envs (their action was ignored, also
 *   where the start lies inside the crash margin) and frozen ones.  obs: row e of [n_envs, obs_count].  aux
 *   (optional): row e of [n_envs, 4] = (velocity, steer_angle, angular_velocity, slip_angle) of the state, cast to f32.
 *
 * rl_env_reset / rl_env_step: host pointers, synchronous on c's stream.  start_index_or_null: n_envs indices into
 * the pool.  actions_n2: [n_envs, 2] f32.  rl_env_reset_device / rl_env_step_device: device pointers; they only
 * enqueue on the given stream (null = the null stream) and never wait for the device; the device form clamps start
 * indices to [0, M).  A host form (and rl_env_read) that follows device-form calls waits for the whole device first,
 * so the two may be mixed.  rl_env_read: the states [n_envs, 11] and the counters, each pointer optional.  h's
 * options and ray offset read the same after every call.
 *
 * Errors (RL_ERR_INVALID, nothing launched, the handles usable as before): null required pointers, n_envs < 1,
 * substeps outside [1, 512], num_rays outside [10, 1280], an observation window that leaves [0, num_rays), obs_count
 * or obs_stride < 1, negative or NaN steer_clip / obs_clip / obs_scale, NaN crash_reward, non-finite dt, max_ticks
 * < 0, n_starts < 1, a non-finite start state, n_envs num_rays >= 2^31, a start_index outside [0, M) (host form),
 * handles on different devices or multi-device handles, a step or read before a reset; the range method's own
 * refusals come back with their code.  After a failed launch the env needs a reset.
 * Races inside the environment: the next section, "the race environment".  Out of scope: multi-device handles,
 * graph capture (a step advances host-side counters).
 * Per call: env_step_kernel, the fan launch sequence of h's planner, env_observe_kernel (env_kernels.h).       */
typedef struct rl_env rl_env;
typedef struct rl_env_params {
    int n_envs, substeps, num_rays;
    int obs_start, obs_count, obs_stride;   /* observation = beams obs_start + i*obs_stride, i < obs_count */
    float obs_clip, obs_scale;              /* obs_scale > 0: policy_input(r, clip, scale); 0: raw metres  */
    int max_ticks;                          /* 0: never truncate                                           */
    int auto_reset;                         /* 0: a finished env freezes; 1: it re-spawns on the next step */
    double dt, scan_dist_to_base, crash_thresh, steer_clip, crash_reward;
    float fov;
} rl_env_params;
int  rl_env_create(rl_car *c, rl_method *h, const rl_env_params *p, const double *edge,
                   const double *starts_m11, int n_starts, rl_env **out);
void rl_env_destroy(rl_env *e);
int  rl_env_reset(rl_env *e, uint64_t seed, const int *start_index_or_null,
                  float *obs, float *aux_or_null, int *done);
int  rl_env_step(rl_env *e, const float *actions_n2, float *obs, float *reward, int *done, float *aux_or_null);
int  rl_env_reset_device(rl_env *e, uint64_t seed, const int *d_start_index_or_null,
                         float *d_obs, float *d_aux_or_null, int *d_done, void *hip_stream);
int  rl_env_step_device(rl_env *e, const float *d_actions_n2, float *d_obs, float *d_reward, int *d_done,
                        float *d_aux_or_null, void *hip_stream);
int  rl_env_read(rl_env *e, double *states_n11, int *ticks, int *episodes, int *start_index, int *done);

/* ---- the race environment ----------------------------------------------------------------------
 * The driving environment with the race as the episode: R races of `group` = P cars (1 <= P <= 8) that see each other
 * in every scan, as in rl_car_race_followgap, driven by the caller's actions.  A race spawns and re-spawns as a
 * whole; in between a finished car stays in the map as a wreck.  An rl_env made by rl_env_create_race is served by
 * rl_env_reset / _step (+ _device), rl_env_read and rl_env_destroy; fed FollowGap's answers it reproduces
 * rl_car_race_followgap bit for bit, and with P = 1 it is rl_env_create's environment.  tests/race_env_statement.py
 * restates this section.  Everything is as written for the driving environment except:
 *
 * Layout.  R = n_envs / P races; car k of race r is env e = r P + k.  Actions, obs, reward, done and aux stay one row
 *   per car.  starts_mp11: a pool of M = n_starts line-ups of P rows in getState layout; car k of a race spawned from
 *   line-up idx gets row idx P + k.  The cars' outline is c's LENGTH x WIDTH.
 * Per-race counters: race_tick[r], race_episode[r], race_start_index[r] and race_over[r] in {0 running, 1 over because
 *   fewer than min_running cars run (none running included), 2 truncated at max_ticks}.  Per car, episode[e] and
 *   start_index[e] mirror the race's; tick[e] counts the steps that car took in this episode (a wreck stops counting).
 * Spawn of race r at episode q: idx = start_index[r] when the caller gave start indices and q = 0 (the index arrays
 *   of rl_env_reset* hold n_races entries), otherwise idx = min(M-1, (int)(U(r, q) * (double)M)) with the env's
 *   uniform and key.  All P cars spawn together.
 * Step k, phase A (race_env_step_kernel, one lane per car):
 *   race_over[r] != 0 and auto_reset: the whole race spawns with q = race_episode[r] + 1 and race_tick = 0; every car
 *     is "fresh", its action is ignored;
 *   race_over[r] != 0 without auto_reset: every car of the race is frozen;
 *   otherwise race_tick[r] += 1, and a car with done[e] != 0 is a frozen wreck: its state stays, its action is
 *     ignored, it is scanned again where it stands with this slot's noise, and the others see it.  Every other car
 *     goes through the env's action check (done = 3 makes it a wreck), clamp and `substeps` steps.
 * Scan: the race scan of rl_calc_range_fan_cars over all n_envs lidar poses, the other cars of the race read from the
 *   f64 states as they stand after phase A; ray offset base + (k n_envs + e) num_rays.  Kinds RL_RM and RL_RM_GPU,
 *   variants 0, 1 and 3.
 * Phase B (race_env_observe_kernel, one workgroup per race, one wave per car), per car: the env's rule with
 *   race_tick[r] for the truncation test: a hit sets done = 1 for a stepped or fresh car, otherwise a stepped car with
 *   max_ticks > 0 and race_tick[r] == max_ticks gets done = 2; the reward is the env's, 0 for a wreck.
 *   Then per race, once every car has its code: running = the number of cars with done == 0.  If a car was truncated
 *   race_over = 2; else if running < min_running race_over = 1 and every car still running reads done = 2 and keeps
 *   its (float)moved reward (it survived; at a reset or re-spawn such a fresh car reads 2 with reward 0); else
 *   race_over = 0.  Cars that hit each other in the same step both read 1.  A finished race that stands (no
 *   auto_reset) keeps its codes and reads reward 0.
 *
 * Errors (RL_ERR_INVALID, nothing launched, the handles usable as before): group outside [1, 8], n_envs not a multiple
 * of group, min_running outside [1, group], everything rl_env_create refuses, a race start_index outside [0, M) (host
 * form), rl_env_read_races on an env that is not a race env or before a reset.  The refusals of rl_calc_range_fan_cars
 * come back with their codes at create and at every reset and step: RL_ERR_UNSUPPORTED for RL_CDDT, RL_GIANT_LUT,
 * RL_BRESENHAM, variant 2, outlines of more than 512 points and maps of 32768 or more cells a side.
 * rl_env_read_races: the races' counters [n_races] each, every pointer optional; it waits like rl_env_read.
 * Per call: race_env_step_kernel, race_fan_kernel, race_env_observe_kernel (env_kernels.h, race_kernels.h).        */
typedef struct rl_race_env_params {
    rl_env_params env;   /* n_envs = n_races * group cars, race-major; every other field as rl_env_create reads it */
    int group;           /* P cars per race, 1 .. 8 */
    int min_running;     /* the race is over once fewer than this many cars run: 1 .. group */
} rl_race_env_params;
int  rl_env_create_race(rl_car *c, rl_method *h, const rl_race_env_params *p, const double *edge,
                        const double *starts_mp11, int n_starts, rl_env **out);
int  rl_env_read_races(rl_env *e, int *race_ticks, int *race_episodes, int *race_start_index, int *race_over);

/* ---- track progress ----------------------------------------------------------------------------
 * Where every car of an environment is on a track, how far it came along it, its laps, a lookahead waypoint in the
 * car's frame and, in a race, its position: the global path of the reference's driver (paths/wp-u.csv,
 * scripts/mcts_driver.py:139-169) for every env on the device at every reset and step.  Opt-in: an env without a track
 * runs exactly the launches of the two sections above; with one, a single kernel (track_kernel, track_kernels.h) is
 * enqueued behind phase B on the same stream.  tests/track_statement.py restates this section line by line.
 * Every f64 operation below is separately rounded (the library is built with -ffp-contract=off).
 *
 * Track.  W points (x_i, y_i) f64, closed or open.  S segments: S = W when closed, segment i running from point i to
 *   point (i+1) mod W; S = W - 1 when open.  Per segment: dx_i = x_(i+1) - x_i, dy_i = y_(i+1) - y_i,
 *   q_i = dx_i*dx_i + dy_i*dy_i, len_i = sqrt(q_i); cum_0 = 0, cum_(i+1) = cum_i + len_i summed in ascending order;
 *   L = cum_S.  Refused (RL_ERR_INVALID): W < 2, W < 3 when closed, W > 65536, a non-finite coordinate, a segment
 *   with q_i == 0 (or not finite).
 * Projection of a car at (cx, cy, th) = state[0..2] onto segment i:
 *   ax = cx - x_i, ay = cy - y_i;  u = ax*dx_i + ay*dy_i;  t = fmin(fmax(u / q_i, 0), 1);
 *   ex = ax - t*dx_i, ey = ay - t*dy_i;  d2 = ex*ex + ey*ey.
 * Nearest segment: the candidate with the smallest d2, the lowest index i among equals.  Candidates: every segment
 *   for a fresh (just spawned) env or when window == 0; otherwise the segments within `window` of the previous
 *   nearest segment p: (p - window + m) mod S for m <= 2 window on a closed track, max(p - window, 0) ..
 *   min(p + window, S - 1) on an open one; all segments once 2*window + 1 >= S.
 * From the nearest segment i and its t:
 *   s = cum_i + t*len_i;
 *   lateral = (dx_i*ay - dy_i*ax) / len_i, left of the direction of travel positive;
 *   with hx = cos th, hy = sin th: heading_err = atan2(dx_i*hy - dy_i*hx, dx_i*hx + dy_i*hy).
 * Progress.  Fresh env: D = 0, progress = 0, laps = 0, s_prev = s.  Stepped env: D = s - s_prev; on a closed track
 *   with half = 0.5*L: D < -half gives D += L and laps += 1; D > half gives D -= L and laps -= 1; then
 *   progress += D and s_prev = s.  Frozen envs, wrecks and refused actions: D = 0, nothing else changes (their rank
 *   is still counted anew).  laps is the signed count of start-line (s = 0) crossings since the spawn.
 * Goal waypoint, lookahead l > 0 (findBestPoint's rule).  Over the candidate waypoints j in order:
 *   dist_j = sqrt((x_j-cx)*(x_j-cx) + (y_j-cy)*(y_j-cy)), g_j = fabs(l - dist_j); the best starts at 2l and j wins on
 *   g_j < best, strictly: the first candidate among equals.  No winner: goal = -1, goal point (0, 0).  Candidates:
 *   goal_span == 0: all W waypoints in index order (the reference's rule); goal_span > 0: the waypoints
 *   (i + 1 + m) mod W for m < goal_span, forward of the nearest segment i, in order of m (m < W: a second visit cannot
 *   win); an open track stops at W - 1.  In the car's frame, with rx = x_g - cx, ry = y_g - cy:
 *   gx = hx*rx + hy*ry, gy = hx*ry - hy*rx.
 * Race order.  An env of rl_env_create reads offset = 0 and rank = 0.  At a race's spawn offset[e] = s_e - s_(car 0 of
 *   the race), wrapped on a closed track by the same +-L rule as D (no lap is counted).  race_dist[e] = offset[e] +
 *   progress[e].  rank[e] = the number of cars k' of the race with a larger race_dist, or an equal one and k' < k.
 *   Wrecks keep their race_dist and are ranked with the rest.
 * What the caller sees, per env: an f32 row [8] = (D, s, lateral, heading_err, gx, gy, progress, race_dist), each cast
 *   from f64, and an int row [4] = (segment, goal, laps, rank).
 * Reward.  reward_mode 0 leaves the env's reward alone; reward_mode 1 writes (float)D exactly where the env's rule
 *   writes (float)moved: a stepped env that did not crash (a survivor of a race that ended included).  Crash, refused,
 *   fresh and frozen rewards stay.
 *
 * rl_track_create copies the points and builds the table on `device`; rl_track_read gives cum [S + 1] and L back.
 * rl_env_attach_track: t is borrowed (keep it alive as long as it is attached); a null t detaches (p is not read); the
 * env needs a reset afterwards.  rl_env_read_track: host pointers, each optional; it waits like rl_env_read.
 * rl_env_read_track_device: device pointers, each optional; it only enqueues the copies on the given stream (the one
 * of the step before it, or one ordered behind it).
 * Errors (RL_ERR_INVALID, nothing launched, the env usable as before): null params with a track, window or goal_span
 * < 0 or > 65536, reward_mode outside {0, 1}, lookahead not finite or <= 0, a track on another device than the env, a
 * track read on an env with no track attached or before a reset.  Out of scope: off-track termination, multi-device
 * handles, graph capture.                                                                                         */
typedef struct rl_track rl_track;
int  rl_track_create(int device, const double *xy_w2, int n_points, int closed, rl_track **out);
void rl_track_destroy(rl_track *t);
int  rl_track_read(rl_track *t, double *cum_s_plus_1_or_null, double *length_or_null);
typedef struct rl_track_params { int window, goal_span, reward_mode; double lookahead; } rl_track_params;
int  rl_env_attach_track(rl_env *e, rl_track *t, const rl_track_params *p);
int  rl_env_read_track(rl_env *e, float *rows_n8, int *ints_n4);
int  rl_env_read_track_device(rl_env *e, float *d_rows_n8, int *d_ints_n4, void *hip_stream);

/* ---- the MCTS planner ----------------------------------------------------------------------------
 * scripts/mcts.py's tree search (MCTS.mcts / mctsIteration / act / rollout, :109-245) for K independent trees in
 * lock step on one device: every iteration adds exactly one node to every tree, so each iteration is one batched
 * act and one batched roll-out with no host synchronisation in between.  The tree is the reference's, bit for bit,
 * as tests/mcts_statement.py restates it:
 *   - iteration (mctsIteration :150-185): a terminal node returns before it is visited; visits start at 1;
 *     sum_of_visits is the children's visit sum; the selected child maximises reward/visits +
 *     C sqrt(log(sum)/visits), the first strict maximum in insertion order (Python's max); the search descends
 *     while sqrt(sum) < n_children; when the level below reports "not expanded" the new child goes under the
 *     current node — a terminal child just descended into included (it gets a child and is not visited);
 *     Node.propagate runs at every recursion level: the new child receives rv once, its j-th ancestor (j = 1:
 *     the node it was added under) j + 1 times — j times when that node is terminal — as repeated adds; the root
 *     none;
 *   - the new action: source RL_MCTS_FG / RL_MCTS_NN: uniSample(children[0].action, uni_dev) when the node has
 *     children, otherwise the node's stored answer (FollowGap::eval of the node's own scan as rl_followgap_eval
 *     computes it, or rl_policy_eval's f32 output, widened to double, not clipped); RL_MCTS_RANDOM:
 *     uniSample(0, 0.41) always.  The reference's Node.scan aliases the simulator's one scan buffer, so its
 *     generateActionFromFG reads the LAST scan taken, not the node's; the node's own scan is used here (the
 *     evident intent), evaluated once when the node is created;
 *   - act (:187-200): Car::control + updatePosition(dt) with (speed, action) from the node's state, the lidar pose
 *     of Car::getScanPose in f64 cast to f32, the scan with h, terminal = isCrashed(scan) >= 0.  mcts.py:195 tests
 *     > 0, which a single scan never returns (0 or -2); the planner follows ros_interface.py:144 (>= 0), as
 *     rl_car_drive_followgap does;
 *   - rollout (:202-245), for non-terminal children (terminal ones take rv = crash_pen): L steps from the child's
 *     state, a new (speed, steer) every action_every steps, steer = uniform(-max_steer, max_steer) drawn before
 *     speed = uniform(0, max_speed); the car poses (not the lidar poses) scanned and tested as
 *     rl_car_rollout_check does; rv = sum(vel[:index] or all L) / |action| with IEEE inf / NaN.
 *   - root: the caller's state and recent action, never terminal, its scan taken at reset; the answer is the root
 *     child with the most visits (the first of equals, :126-131).
 * Exactness:
 *   - draws: Philox-2x32-10 (scan_device.h's rounds) with key = noise_key(seeds[k]) (the noise seed fold), counter
 *     (d, i) with i the iteration since reset: d = 0 the expansion draw, d = 1 + 2m / 2 + 2m roll-out action m's
 *     steer / speed; u = ((out0 << 32 | out1) >> 11) 2^-53; uniform(lo, hi) = lo + (hi - lo) u (NumPy's formula,
 *     each operation rounded); uniSample's lo = prediction - dev and hi = prediction + dev are rounded first;
 *   - the reward sum is numpy.sum of the contiguous float64 velocities, bit for bit: 0.0 + P(v, n) with P NumPy's
 *     pairwise_sum: a sequential sum from 0.0 for n < 8; for n <= 128 eight accumulators r[j] = v[j] + v[8+j] + ...
 *     over the multiple-of-8 prefix, folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail added in order;
 *     above 128, P(v, n2) + P(v + n2, n - n2) with n2 = n/2 - (n/2) % 8 (pinned by tests/test_mcts_host.py);
 *   - UCB: separately rounded f64 operations, log(sum) from a table of the host's log(n) (Python's math.log) built
 *     at create, the correctly rounded f64 sqrt (rl_mcts_probe_ucb pins it);
 *   - noise: h's settings; ray ids with base = h's ray offset at reset: root scans base + k B; iteration i's act
 *     scan of tree k base + (K + i K (1 + L) + k) B; its roll-out pose s base + (K + i K (1 + L) + K + k L + s) B
 *     (B = num_rays).  h's options and ray offset read the same after every call.
 *
 * rl_mcts_create: c, h and the source's handle (g for FG, p for NN; borrowed, they must outlive the planner) on ONE
 * device, multi-device handles refused.  edge: num_rays doubles (rl_car_edge_distances).  Errors (RL_ERR_INVALID):
 * null pointers, K < 1, max_nodes < 1, L outside [1, 512], action_every < 1, an unknown source or one without its
 * handle (RL_MCTS_RANDOM and RL_MCTS_PURSUIT take none), num_rays outside [10, 1280], num_rays < in_start + dims[0] for NN, K L num_rays >= 2^31, handles on
 * different devices.
 * rl_mcts_reset: the K roots (states K x 11, recent actions K, one 64-bit seed per tree); takes the root scans.
 * rl_mcts_run: n_iterations iterations, synchronous; n iterations equal n/2 followed by n/2.  Refused before any
 * launch (RL_ERR_INVALID) without a reset, or when 1 + the iterations since reset would exceed max_nodes; a
 * failed launch leaves the planner needing a reset.  The range method's own refusals (those of
 * rl_car_rollout_check) come back with the same code.
 * rl_mcts_best: per tree the best root action (NaN and visits -1 before the first iteration), its visits, and the
 * node count.  rl_mcts_read_tree: tree `tree`'s node arrays in creation order (node 0 = root, parent -1, sibling /
 * child links -1 = none), any output pointer may be null; crash = the roll-out's crash index (-(L+1): none), -1
 * for the root and terminal nodes; answer = the stored expansion answer (NaN for RANDOM); n_nodes_out = how many.
 * rl_mcts_probe_ucb: the device's UCB key of n (reward, visits >= 1, 1 <= sum <= 2^24) triples.
 *
 * rl_mcts_drive: the closed loop of scripts/mcts_driver.py:207-264 (createActionCallback) for the K = n_trees cars
 * of m: every action tick sets the simulator to the car's state (:214), builds a fresh MCTS with the recent action
 * at the root (:230-232), takes its answer (:234), drives and steps the car with it (:249-250) and keeps the answer
 * clipped as the next recent action (:254).  Synchronous, on c's stream; states_in (K x 11), recent_in (K) and the
 * K x D Philox keys go up once, before decision 0, and between decisions there is no host synchronisation and no
 * host-to-device copy.  D = n_decisions, I = n_iterations, S = steps_per_decision, L = rollout_steps, B = num_rays.
 * Per decision d = 0 ... D-1, for every car k:
 *   1. reset: tree k is re-rooted as rl_mcts_reset does it, with the car's current state as the root state, its
 *      recent action as the root action and the seed (seeds[k] + d) mod 2^64 (key = noise_key of it); the root scan
 *      and answer come from the ordinary act launch; the ray offset is base + d stride with base = h's ray offset at
 *      entry and stride = K B (1 + I (1 + L)), the rays one rl_mcts_reset plus rl_mcts_run(I) consume;
 *   2. the car's crash test: Car::isCrashed(root scan) >= 0 (ros_interface.py:144, as rl_car_drive_followgap).  A car
 *      crashed at decision d gets first[k] = d and freezes: its state and recent action no longer change,
 *      actions[k][d...] and the trace rows from d on are NaN, visits[k][d...] are -1.  Its tree is searched with the
 *      others from the frozen state and ignored.  The root node itself is never terminal, as in the reference;
 *   3. I iterations, exactly rl_mcts_run's;
 *   4. the answer, rl_mcts_best's rule: the most visited root child, the first of equals -> actions[k][d] (raw, not
 *      clipped) and visits[k][d];
 *   5. the step: S times Car::control(speed, a) + updatePosition(dt) in float64 with the raw action (:249), the
 *      state of rl_car_rollout holding (speed, a) for S steps, bit for bit; the next recent action is a clamped to
 *      +-steer_clip when steer_clip > 0 (:254), raw when it is 0; trace_states[k][d] is the state the decision was
 *      planned from.
 * Afterwards first[k] = -(D+1) for a car that never crashed; states_out / recent_out are the final states and recent
 * actions (the state after the last step is not scanned); m is ready and holds the last decision's trees
 * (rl_mcts_read_tree and rl_mcts_best work, I iterations done since its reset); h's options and ray offset read the
 * same as before the call.  A failed launch leaves the planner needing a reset.  n_decisions = 0: RL_OK, first = -1,
 * states_out = states_in, recent_out = recent_in, the planner untouched.  Errors (RL_ERR_INVALID, nothing launched,
 * the handles usable as before): a null required pointer, n_decisions < 0, n_iterations < 1, n_iterations + 1 >
 * max_nodes, steps_per_decision < 1, steer_clip negative or NaN, and the range method's refusals as in rl_mcts_run.
 * Kernels: mcts_kernels.h.
 *
 * The track steering the search (kernels: plan_pursuit_kernels.h, pursuit_device.h; tests/mcts_pursuit_statement.py).
 * The track, its options and the explicit points are those of scanlib_track_plan.h (rl_mcts_attach_track,
 * rl_mcts_set_points); a zeroed rollout_source / rollout_dev and a source below 3 are the planner above, launch for launch.
 *   - the pursuit steer of a car with state (x, y, th) = state[0..2] towards a world point (X, Y), all float64, every
 *     operation rounded separately, WB the car's wheelbase:
 *       rx = X - x; ry = Y - y; hx = cos th; hy = sin th; gx = hx rx + hy ry; gy = hx ry - hy rx  (the car frame of
 *       "track progress"); d2 = gx gx + gy gy; if !(d2 > 0): 0.0f (the point is the car, or something is NaN);
 *       else a = atan(((2.0 WB) gy) / d2), a = fmin(fmax(a, -max_steer), max_steer), the answer (float)a.
 *     The answer is float32, as FollowGap's and the network's; whoever consumes it widens it with (double)answer;
 *   - source RL_MCTS_PURSUIT (no handle): the stored expansion answer of every node, the root included, is the pursuit
 *     steer from the node's own state towards the tree's track point: the (px, py) of scanlib_track_plan.h's reward
 *     mode 1, chosen at rl_mcts_reset and at every decision of rl_mcts_drive whatever the reward mode (mode 0 with a
 *     track attached is valid); 0.0f for a tree without a point (goal -1 and no explicit point).  Everything else is
 *     the FG / NN rule: the first child takes (double)answer, later ones uniSample(children[0].action, uni_dev);
 *   - rollout_source 1 (pursuit roll-outs, any source): roll-out action m's steer, chosen from the state before step
 *     m action_every (m = 0: the child's state), is fmin(fmax(base + uniform(-rollout_dev, rollout_dev; u), -max_steer),
 *     max_steer) with u the draw d = 1 + 2m of the uniform steer it replaces and base = (double)(the pursuit steer towards
 *     the goal waypoint), 0.0 without a goal.  The goal: "track progress"'s nearest segment of the state among the
 *     segments within `window` of the segment action m - 1 found (m = 0: of the root's segment, found over all segments;
 *     window 0: all segments), then its goal rule from that segment with the attached lookahead and goal_span.  The
 *     speed (d = 2 + 2m), the steps, the scans, the crash test, the reward terms and the backup are unchanged.
 * Errors (RL_ERR_INVALID, nothing launched, the handles usable as before): rollout_source outside {0, 1}, or with 1 a
 * rollout_dev negative or not finite, at create; reset, run or drive of an RL_MCTS_PURSUIT planner with neither a track nor
 * explicit points, or of a pursuit roll-out planner without a track (explicit points do not help a roll-out); attach of
 * a lookahead not finite or <= 0, in any reward mode, to a pursuit roll-out planner or to an RL_MCTS_PURSUIT planner
 * without explicit points.                                                                                     */
typedef struct rl_mcts rl_mcts;
typedef enum rl_mcts_source { RL_MCTS_FG = 0, RL_MCTS_NN = 1, RL_MCTS_RANDOM = 2, RL_MCTS_PURSUIT = 3 } rl_mcts_source;
typedef struct rl_mcts_params {
    int n_trees, max_nodes, rollout_steps, action_every, source;
    double speed, dt, scan_dist_to_base, C, crash_pen, uni_dev, max_steer, max_speed;
    float fov;
    int num_rays;
    double crash_thresh;
    int rollout_source;                 /* 0: the uniform steer (rollout_dev not read); 1: pursuit roll-outs */
    double rollout_dev;
} rl_mcts_params;
int rl_mcts_create(rl_car *c, rl_method *h, rl_followgap *g_or_null, rl_policy *p_or_null,
                   const rl_mcts_params *params, const double *edge, rl_mcts **out);
void rl_mcts_destroy(rl_mcts *m);
int rl_mcts_reset(rl_mcts *m, const double *root_states, const double *root_actions, const uint64_t *seeds);
int rl_mcts_run(rl_mcts *m, int n_iterations);
int rl_mcts_best(rl_mcts *m, double *actions, int *visits, int *n_nodes);
int rl_mcts_drive(rl_mcts *m, const double *states_in, const double *recent_in, const uint64_t *seeds,
                  int n_decisions, int n_iterations, int steps_per_decision, double steer_clip,
                  int *first, double *states_out, double *recent_out,
                  double *actions, int *visits,            /* [K][n_decisions]                */
                  double *trace_states_or_null);           /* [K][n_decisions][11] or NULL    */
int rl_mcts_read_tree(rl_mcts *m, int tree, int *parent, int *first_child, int *next_sibling, int *n_children,
                      int *visits, int *child_visits, double *reward, double *action, int *terminal, double *state,
                      float *scan_pose, float *answer, int *crash, int *n_nodes_out);
int rl_mcts_probe_ucb(int device, const double *reward, const int *visits, const int *sum, size_t n, double C,
                      double *out);

/* Car::setCarEdgeDistances (racecar/src/racecar.cpp:239-292; called at
 * scripts/racecar_simulator_v2.py:47-50): distance from the lidar to the car's outline along each of
 * num_rays beams starting one increment after min_ang — the table every crash test above takes as
 * `edge`.  Host arithmetic (a one-off table), no device needed; the reference's quirks are kept
 * (shifted by one beam, pi = 3.145, about -1016 m for a beam at exactly 0 rad).                   */
int rl_car_edge_distances(int num_rays, double min_ang, double ang_inc, double scan_dist_to_base,
                          double width, double wheelbase, double *edge_out);
/* Car::isCrashed (racecar/src/racecar.cpp:305-328) over ranges already on the host: index of the
 * first of n_scans scans with a beam j where (double)range - edge[j] < crash_thresh, else
 * -(n_scans+1).  (Scanned batches use the fused device test: rl_check_collision_*.)               */
int rl_car_is_crashed(const float *ranges, int num_rays, int n_scans, const double *edge,
                      double crash_thresh, int *first_crashed);

/* device time of the last enqueued launch sequence of this handle, from HIP events
 * recorded on the launch stream (blocks until that work has finished).  Events are only
 * recorded after rl_method_set_option(h, "timing", 1): they cost microseconds per launch.
 * "timing" = 2 brackets the ray-marching kernel alone (the pose-binning launches in front of it
 * excluded), which is the duration a kernel trace reports for it.                              */
int rl_last_kernel_ms(rl_method *h, float *ms_out);

/* tuning / diagnostics: integer options by name.  None changes a result bit; defaults are the
 * measured optima on MI355X.
 *   schedule   variant (1 stream kernel | 0 chunk-per-wave | 2 occ_fan_lds: unit steps on an LDS occupancy
 *              window, approximate | 3 the UPSTREAM-LITERAL arithmetic of RL_RM / RL_RM_GPU — range_libc's CPU
 *              statement: per-ray glibc sinf / cosf, un-fused products and sums —, the ONE option that changes result
 *              bits: onto the checker's libm form.  A production mode since round 5 — same entry points, same stream
 *              kernel schedule, fused crash test and noise included, ~0.87x the canonical rate — and since round 6 the
 *              DEFAULT of RL_RM (the class that names range_libc's CPU RayMarching); RL_RM_GPU defaults to 1; a negative
 *              value restores the kind's default), grid_mult, wg_threads, low_water (-1 auto), run_log2 (-1 auto), xcd_bands,
 *              sort_poses, tiled (step-map layout), slots (rays per lane: 1 | 2 | 3 | 0 auto),
 *              code_map (2: launches of >= code_min_rays rays read the step map as 16-bit palette codes, palette in LDS —
 *              the same sample sequence on half the bytes; 0: float32 steps), code_min_rays (default 2^22),
 *              tail_pct / tail_wg_pct (a second generation of workgroups for whole-machine launches: measured, off),
 *              cddt_bins (one look-up per pose and table bin), cddt_theta_min (poses from which the look-ups
 *              run theta-major: all poses against one table bin at a time), cddt_lds_sort
 *   binning    inline_prep, inline_max, inline_map_kb, stripe_max, order_inline, bin_multi_min,
 *              bin_generic, bin_ppw (poses per workgroup of the grid-wide binning kernels), tile_stripe (order of the map
 *              tiles the poses are binned by: N > 0 = tile rows in stripes of N, a stripe walked column by column, so that
 *              a band of the pose list sweeps its part of the map once; 0 = row-major; -1, the default = the tile rows
 *              one of xcd_bands bands of evenly spread poses holds)
 *   launches   slice_log2 (pose slices below 2^n rays), pinned_max_rays (zero-copy host calls), direct_max_rays (a result
 *              buffer in a block of rl_host_alloc is written by the kernel itself up to this many rays, by DMA beyond),
 *              overlap_min_rays (plain host-pointer scans of at least this many rays — default 2^24 — run as four pose
 *              slices, the device-to-host copy of one overlapping the march of the next; 0 = never)
 *              spec_drain / spec_stretch (one ray per lane: value-speculating drain loop from <= N live lanes,
 *              plain samples between attempts); drain_cap / drain_stretch (several rays per lane: a wave whose
 *              stream is dry compacts its last <= N rays (<= 64) into one ray per lane and finishes them with
 *              that loop); nt_store (1: the stream kernels' ranges leave with non-temporal stores — write-once data
 *              that would otherwise displace the step map from the L2; set 0 when the next kernel on the stream
 *              reads the ranges back at once, e.g. rl_followgap_eval_device)
 *   diagnosis  timing (1 launch sequence | 2 main kernel only), debug_stamps, drain_prio, lut_debug (bits: 1 skip the
 *              gathers / searches, 2 skip the range stores, 8 non-temporal GiantLUT range stores, 16 PLAIN instead of
 *              non-temporal GiantLUT row loads — the A/B partner of the default)
 *   GiantLUT   lut_refine (0, the default | 1: the origin-corrected query, "origin-corrected GiantLUT query" above; a
 *              handle option, not part of rl_plan_opts: the plan — kernel name, grid, LDS — stays the default's and the
 *              launch takes the planned instance's refined twin; the LDS twin runs the planned waves in workgroups of
 *              512 lanes.  Stored and ignored by the other kinds)
 *   CDDT       race_cddt (0, the default | 1: batched races on the table, "Races on CDDT" above; a handle option, not
 *              part of rl_plan_opts.  Stored and ignored by the other kinds)
 *   multi-device handles: every option goes to every device's replica; multi_min_poses (poses per device
 *              from which another device is brought in, default 512) belongs to the handle itself.
 * rl_method_get_info additionally answers n_devices, n_cu, clock_khz, last_grid, map_epoch, code_entries (palette entries of
 * the handle's map incl. the two stop codes; 0 = no code map: option off, geometry or palette does not fit) and, for RL_CDDT
 * (builds the table if needed, synchronises): cddt_values, cddt_buckets, cddt_nonempty_buckets.          */
int rl_method_set_option(rl_method *h, const char *name, int value);
int rl_method_get_info(rl_method *h, const char *name, int64_t *value_out);
/* ---- launch planning -------------------------------------------------------------------------
 * Which kernel, grid, LDS size and pose-binning pass a fan call of (n_poses x num_rays) takes is
 * decided by ONE pure function of the map shape, the device's CU count and the options above —
 * no device, no handle state: rl_plan_fan can be called (and is tested) on a box without a GPU.
 * rl_method_plan_fan applies it with a handle's current options (a ray-marching handle with the code map on builds its
 * step map first — the one thing a plan needs from the device is the map's palette size); every launch goes through the
 * same function and rl_method_last_plan returns the plan the last launch of the handle used
 * (`name` is the kernel as a rocprofv3 kernel trace prints it, template arguments included).     */
/* Which fields still carry weight (round 4; every default is a measured optimum, profiles/r03/plan_sweep.txt):
 *   set by callers in production   grid_mult + slots (a caller that keeps several launches in flight: 3 and 2,
 *                                  INTEGRATION.md), slice_log2 (only to force slicing in tests)
 *   thresholds of the planner      inline_max, inline_map_kb, stripe_max, bin_multi_min, cddt_theta_min, xcd_bands,
 *                                  low_water (-1 = automatic) — change them only with a sweep in hand
 *   arithmetic                     variant 3: range_libc's CPU arithmetic stated literally — glibc sinf / cosf per ray,
 *                                  un-fused products and sums — bit-identical to the checker's libm form; the stream
 *                                  kernel's schedule (rm_fan_stream_kernel<.., LIT>), 0.87x the canonical rate; -1 (the
 *                                  struct's default) = the kind's default: 3 for RL_RM, 1 otherwise
 *   kernel selection for A/B       variant (0 chunk kernel, 2 occ_fan_lds), group_drain, handoff (round 5's measured and
 *                                  rejected drain forms), cddt_search (0 = round 4's search kernel), tiled (0 = row-major step map; the
 *                                  planner clears it by itself when the tiled geometry does not fit), cddt_bins
 *   diagnostics only               wg_threads, sort_poses, inline_prep, order_inline, bin_generic, run_log2,
 *                                  cddt_sort, lut_debug, debug_stamps
 * Out-of-range values are clamped by the planner (a zeroed struct is valid input).                              */
typedef struct rl_plan_opts {
    int variant, grid_mult, wg_threads, low_water, sort_poses, xcd_bands, slots, tiled;
    int inline_prep, inline_max, inline_map_kb, stripe_max, order_inline, bin_multi_min, bin_generic;
    int run_log2, cddt_bins, cddt_sort, lut_debug, debug_stamps, slice_log2, cddt_theta_min;
    int cddt_search;     /* theta-major CDDT: 1 = look-ups prepared once per pose, picked up by the 8-lane groups
                            (cddt_theta_search2_kernel + cddt_theta_fan_kernel, round 5), 0 = every group prepares its own
                            (round 4), 2 = search and fan of a 64-pose tile fused in one workgroup, per-bin results in
                            LDS only (cddt_theta_fused_kernel)                                                            */
    int code_map;        /* ray marching: 2 = the step map as 16-bit palette codes, the palette (exact float32 steps) in LDS
                            (rm_fan_stream_kernel<..., CODE = 2>: the same sample sequence, half the bytes per cell);
                            0 = float32 steps.  Takes effect where the map's palette fits (code_entries)                */
    int code_min_rays;   /* ... from this many rays per launch: below it the look-up's latency in every dependent sample costs a
                            lone launch more than the smaller footprint buys (profiles/r06/ab_code_map.txt)              */
    int tail_pct;        /* ray marching, launches that fill the machine: this share (%) of every band's work goes to a SECOND
                            generation of tail_wg_pct % as many workgroups, dispatched as resident ones finish (0 = off)    */
    int tail_wg_pct;
    int code_entries;    /* entries of the map's step palette with its two stop codes — a handle knows it once its step map
                            is built (rl_method_get_info "code_entries", filled in by rl_method_plan_fan); 0 = unknown or
                            too many: the device-less rl_plan_fan then plans the float32 map                          */
} rl_plan_opts;

typedef enum rl_kernel_id {
    RL_K_NONE = 0,
    RL_K_RM_CHUNK = 1,      /* rm_fan_kernel<AUX, CRASH>: one 64-beam chunk per wave (variant 0)          */
    RL_K_RM_STREAM = 2,     /* rm_fan_stream_kernel<AUX, CRASH, NT, INLINE, TILED, SLOTS, LIT, CODE> (default) */
    RL_K_OCC_LDS = 3,       /* occ_fan_lds_kernel<AUX> (variant 2)                                        */
    RL_K_BL_STREAM = 4,     /* bl_fan_stream_kernel<AUX, 1024>                                            */
    RL_K_BL_LDS = 5,        /* bl_fan_kernel<AUX> (variant 0)                                             */
    RL_K_LUT_LDS = 6,       /* lut_fan_lds_kernel<NL, CH>                                                 */
    RL_K_LUT_FAN = 7,       /* lut_fan_kernel<CH>                                                         */
    RL_K_CDDT_BINS = 8,     /* cddt_fan_bins_kernel                                                       */
    RL_K_CDDT_RAYS = 9,     /* cddt_fan_kernel                                                            */
    RL_K_CDDT_THETA = 10,   /* cddt_theta_search[2]_kernel + cddt_theta_fan_kernel | cddt_theta_fused_kernel (large batches) */
    RL_K_RM_LITERAL = 11,   /* rm_literal_kernel<AUX, RAYS>: upstream-literal arithmetic, one lane per ray — variant 3 with
                               diagnostics (hit cells / sample counts), the 2-argument per-ray form, fans below 64 beams */
    RL_K_RM_STREAM_LIT = 12 /* rm_fan_stream_kernel<false, CRASH, 1024, true, true, SLOTS, true, CODE>: variant 3 in production —
                               the upstream-literal arithmetic on the stream kernel's schedule (ranges, fused crash test,
                               noise; two rays per lane; batches above 8192 poses in pose slices)                 */
} rl_kernel_id;

typedef enum rl_binning {
    RL_BIN_NONE = 0,          /* the march kernel derives the pose records of its own blocks (LDS)        */
    RL_BIN_SMALL_KEYS = 1,    /* pose_bin_small_kernel<true>: tile order only, one workgroup              */
    RL_BIN_SMALL_RECORDS = 2, /* pose_bin_small_kernel<false>: records in tile order, one workgroup       */
    RL_BIN_GRID_SORT = 3,     /* pose_prep -> tile_scan_a -> pose_scatter (grid-wide)                    */
    RL_BIN_GRID_UNSORTED = 4, /* pose_prep only (caller's order kept)                                     */
    RL_BIN_GENERIC = 5        /* pose_bin_kernel: one workgroup, any size                                 */
} rl_binning;

typedef struct rl_launch_plan {
    int kernel;          /* rl_kernel_id                                                                  */
    int grid, block;     /* workgroups, threads per workgroup                                             */
    int lds_bytes;       /* dynamic LDS per workgroup                                                     */
    int binning;         /* rl_binning pass in front of the march (0 = none)                              */
    int record_source;   /* RL_K_RM_STREAM: 0 records binned in HBM | 1 derived in LDS, caller's order |
                            2 derived in LDS, row-stripe bands compacted by every workgroup |
                            3 derived in LDS, tile order from the keys-only binning pass                  */
    int slots;           /* rays per lane                                                                 */
    int bands, run_log2, k_max, tiled, aux, crash;
    int nl, ch;          /* GiantLUT: 16-B loads per lane and row, 64-beam chunks per pose; CDDT per-bin
                            kernel: lanes per pose, poses per workgroup pass                              */
    int slices;          /* > 1: the batch goes through in this many pose slices of slice_poses poses,    */
    int slice_poses;     /*      each its own launch sequence planned like this one (for its own size)    */
    int code;            /* RL_K_RM_STREAM[_LIT]: 2 = marches on the 16-bit code map, 0 = float32 step map  */
    int code_entries;    /*      ... palette entries the workgroups copy to LDS                           */
    int gen1;            /* > 0: the first gen1 workgroups are the resident generation, grid - gen1 follow (tail_pct) */
    char name[192];
} rl_launch_plan;

int rl_plan_default_opts(rl_plan_opts *out);
/* kind: rl_kind; want_aux: hit cells / step counts requested; want_crash: fused crash test.
 * opts_or_null = defaults.  Pure host arithmetic.                                                 */
int rl_plan_fan(int kind, int n_cu, int rows, int cols, float max_range_px, int theta_disc,
                const rl_plan_opts *opts_or_null, int n_poses, int num_rays, int want_aux,
                int want_crash, rl_launch_plan *out);
int rl_method_plan_fan(rl_method *h, int n_poses, int num_rays, int want_aux, int want_crash,
                       rl_launch_plan *out);
int rl_method_last_plan(rl_method *h, rl_launch_plan *out);
/* launch contexts (per-stream scratch sets) a handle keeps: streams beyond this count are served
 * after a device synchronisation (callers that pipeline batches stay at or below it).            */
int rl_launch_contexts(void);

/* test hook (RL_GIANT_LUT): builds the table if needed and copies rows [row0,row1) of
 * uint16 lut[row][col][theta_bin] (entry = rint(min(range_px,max_range)*65535/max_range)). */
int rl_method_read_lut(rl_method *h, int row0, int row1, uint16_t *out);
/* diagnostics: after a launch with option "debug_stamps"=1, copies 4 words per wave of the
 * stream kernel (start, end in 100 MHz ticks; services<<32 | longest drain chain;
 * (drain start - start)<<32 | blocks<<8 | band);
 * returns the number of words copied (>= 0) or a negative rl_status.                       */
int rl_debug_read_stamps(rl_method *h, uint64_t *out, int max_words);

/* ---- 16-bit ranges for the multi-GPU exchange (opt-in, LOSSY) ---------------------------------
 * The all-gather of ranges BASELINE.json's north_star names moves 4 B per ray over xGMI; these two
 * streaming passes let a caller exchange 2 B per ray instead: q = rint(clamp(r, 0, max) * 65535 / max),
 * r' = q * max / 65535.  Error <= max/131070 plus float32 rounding (< 0.12 mm at the reference's 15 m, params.yaml:39) —
 * inside north_star's one-cell tolerance, but NOT bit-exact: only bench.py --gather ranges_u16 and
 * distributed.ShardedScan(mode="ranges_u16") use them, and both label their results.
 * Device pointers (any element alignment; 16-byte aligned pairs take the wide path); asynchronous on
 * hip_stream.                                                                                       */
int rl_ranges_to_u16_device(int device, const float *d_ranges, size_t n, float max_range_m,
                            uint16_t *d_out_u16, void *hip_stream);
int rl_ranges_from_u16_device(int device, const uint16_t *d_in_u16, size_t n, float max_range_m,
                              float *d_ranges, void *hip_stream);

/* diagnostics: how fast a CU of this device retires a wave-wide global_load_dword whose
 * `active_lanes` live lanes read unrelated cells of a cache-resident table — the instruction the
 * ray-marching kernels are bound by (tools/probes/tcp_probe3.hip is the same
 * probe stand-alone).  Returns active lanes per clock per CU; chip peak in samples/s =
 * lanes_per_clk_per_cu * n_cu * clock_hz.  bench.py reports `roofline_gather` against it.        */
int rl_probe_gather_rate(int device, int active_lanes, double *lanes_per_clk_per_cu,
                         double *clock_hz_or_null, int *n_cu_or_null);

/* diagnostics: HBM stream rates of this device with hand-written 16-B-per-lane kernels on two buffers of
 * `bytes`: gbs_out5 = {copy, read-only, write-only, copy with non-temporal stores, fill with non-temporal
 * stores} in GB/s (copy counts read + write).  The practical ceiling next to the 8 TB/s spec of
 * bench.py's roofline (MI355X_MICROARCH.md quotes 6.29 TB/s for a float4 copy).                     */
int rl_probe_hbm(int device, size_t bytes, double *gbs_out5);
/* ... the same kernels with NON-TEMPORAL loads (what the GiantLUT row fetch uses): gbs_out3 = {read-only, copy, copy
 * with non-temporal stores}.                                                                          */
int rl_probe_hbm_nt(int device, size_t bytes, double *gbs_out3);

/* diagnostics: the audit mode's sinf / cosf (glibc's algorithm in double precision, csrc/literal_kernels.h) of n
 * host floats, evaluated on the device — tests hold it against the host's libm.                        */
int rl_probe_literal_sincosf(int device, const float *x, size_t n, float *sin_out, float *cos_out);

#ifdef __cplusplus
}
#endif
#endif /* SCANLIB_H */
