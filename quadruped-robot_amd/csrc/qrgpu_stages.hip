// ============================================================================
// libqrgpu.so host side: the per-robot stages around the solves -- estimator, gaits, ground, footholds, swing, stance, pose planner, state
// packing, MPC front-end, the plant -- and the defaults of their parameter blocks.  Every entry point is "check the arguments, normalise the block where
// the reference does, one launch on the context's stream"; the kernels take the caller's blocks (include/qrgpu.h) by value.
// ============================================================================
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

#include "qrgpu_ctx.h"
#include "qr_episode.h"

// One launch of a stage kernel on the context's stream.
template <typename... KArgs, typename... Args>
static int launch_stage(qrgpu_ctx *c, void (*kernel)(KArgs...), dim3 grid, dim3 block, Args... args)
{
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, args...);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}
// Robot i is thread i: workgroups of one wavefront.
static dim3 per_robot(int n) { return dim3((n + 63) / 64); }

extern "C" {

void qrgpu_estimator_desc_default(qrgpu_estimator_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->hip_l = 0.08505f; d->upper_l = 0.2f; d->lower_l = 0.2f;
    const float ho[12] = {0.1805f, -0.047f, 0.f, 0.1805f, 0.047f, 0.f, -0.1805f, -0.047f, 0.f, -0.1805f, 0.047f, 0.f};
    memcpy(d->hip_offset, ho, sizeof(ho));
    d->time_step = 0.002f; d->accelerometer_variance = 0.1f; d->sensor_variance = 0.1f; d->window = 120; d->body_height = 0.28f;
}

int qrgpu_estimator_state_doubles(int window) { return window > 0 ? 96 + 3 * window : 0; }

int qrgpu_estimator_update_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const float *d_est_in, const unsigned *d_tick,
                                 double *d_est_state, float *d_est_out)
{
    if (!batch_ok(c, n) || !desc || !d_est_in || !d_tick || !d_est_state || !d_est_out) return QRGPU_ERR_BAD_ARG;
    if (desc->window <= 0 || desc->window > 4096) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_estimator_kernel, per_robot(n), dim3(64), n, *desc, d_est_in, d_tick, d_est_state, d_est_out, stage_args(c, 1, 1));
}

void qrgpu_gait_desc_default(qrgpu_gait_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int l = 0; l < 4; ++l) { d->stance_duration[l] = 0.5f; d->duty_factor[l] = 0.6f; d->initial_leg_state[l] = 1; }
    d->initial_leg_phase[0] = 0.5f; d->initial_leg_phase[3] = 0.5f;
    d->contact_detection_phase_threshold = 0.5f; d->wait_time = 1.0f; d->advanced_trot = 1;
}

int qrgpu_gait_update_batch(qrgpu_ctx *c, int n, const qrgpu_gait_desc *desc, float current_time, int robot_stop, int reset, const float *d_contact,
                            float *d_gait_state, float *d_gait_out, float *d_fe_in)
{
    if (!batch_ok(c, n) || !desc || !d_contact || !d_gait_state) return QRGPU_ERR_BAD_ARG;
    if (reset != 0 && reset != QRGPU_GAIT_RESET_CONSTRUCT && reset != QRGPU_GAIT_RESET_LIVE) return QRGPU_ERR_BAD_ARG;
    for (int l = 0; l < 4; ++l) if (!(desc->duty_factor[l] > 0.001f) || !(desc->stance_duration[l] > 0.f)) return QRGPU_ERR_BAD_ARG;   // USERDEFINED_SWING legs are not built
    return launch_stage(c, qr_gait_kernel, per_robot(n), dim3(64), n, *desc, current_time, robot_stop, reset, d_contact, d_gait_state, d_gait_out, d_fe_in,
                        stage_args(c, QRGPU_GAIT_RESET_CONSTRUCT, QRGPU_GAIT_RESET_LIVE));
}

void qrgpu_walk_gait_desc_default(qrgpu_walk_gait_desc *d)
{   // config/a1_sim/openloop_gait_generator.yaml, gait "walk"
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int l = 0; l < 4; ++l) { d->stance_duration[l] = 7.5f; d->duty_factor[l] = 0.75f; d->initial_leg_state[l] = 1; }
    d->initial_leg_phase[0] = 0.5f; d->initial_leg_phase[1] = 0.f; d->initial_leg_phase[2] = 0.75f; d->initial_leg_phase[3] = 0.25f;
    d->contact_detection_phase_threshold = 0.1f;
    d->n_states = 4;
    d->state_switch[0] = 7; d->state_switch[1] = 6; d->state_switch[2] = 8; d->state_switch[3] = 5;
    d->state_ratio[0] = 0.2f; d->state_ratio[1] = 0.3f; d->state_ratio[2] = 0.3f; d->state_ratio[3] = 0.2f;
}

int qrgpu_walk_gait_update_batch(qrgpu_ctx *c, int n, const qrgpu_walk_gait_desc *desc, float current_time, int robot_stop, int reset,
                                 const float *d_contact, float *d_walk_state, float *d_walk_out, float *d_ratio, float *d_vmc_in)
{
    if (!batch_ok(c, n) || !desc || !d_contact || !d_walk_state || reset < 0 || reset > 2) return QRGPU_ERR_BAD_ARG;
    if (desc->n_states < 1 || desc->n_states > 4) return QRGPU_ERR_BAD_ARG;
    for (int l = 0; l < 4; ++l) if (!(desc->duty_factor[l] > 0.001f) || !(desc->duty_factor[l] < 1.f) || !(desc->stance_duration[l] > 0.f)) return QRGPU_ERR_BAD_ARG;
    // the constructor's bookkeeping (qr_walk_gait_generator.cpp:87-157): sub-states below a ratio of 0.01 are dropped, the stance-like ones
    // in front of true_swing add up to its start, running sums in float
    WalkDesc D;
    memset(&D, 0, sizeof(D));
    float stand = 0.f;
    for (int k = 0; k < desc->n_states; ++k) {
        if (desc->state_ratio[k] < 0.01) continue;
        const int st = desc->state_switch[k];
        if (st != 5 && st != 6 && st != 7 && st != 8) return QRGPU_ERR_BAD_ARG;
        if (st == 8) D.true_swing_start_in_swing = stand; else stand += desc->state_ratio[k];
        D.que[D.nq] = st; D.ratio[D.nq] = desc->state_ratio[k]; ++D.nq;
    }
    if (D.nq < 1) return QRGPU_ERR_BAD_ARG;
    D.accum[0] = 0.f;
    for (int k = 0; k < D.nq; ++k) D.accum[k + 1] = D.accum[k] + D.ratio[k];
    if (!(fabsf(D.accum[D.nq] - 1.0f) < 1e-4f)) return QRGPU_ERR_BAD_ARG;       // "not vaild ratio definition" (:124)
    for (int l = 0; l < 4; ++l) {
        D.duty_factor[l] = desc->duty_factor[l]; D.initial_leg_phase[l] = desc->initial_leg_phase[l]; D.initial_leg_state[l] = desc->initial_leg_state[l];
        D.full[l] = desc->stance_duration[l] / desc->duty_factor[l];
        D.state_index0[l] = 0;
        if (desc->initial_leg_state[l] == 0) {
            const float ph = (desc->initial_leg_phase[l] - desc->duty_factor[l]) / desc->duty_factor[l];
            int k = 0;
            while (k < D.nq && ph > D.accum[k]) k++;
            D.state_index0[l] = k - 1 > 0 ? k - 1 : 0;
        }
    }
    D.contact_detection_phase_threshold = desc->contact_detection_phase_threshold;
    return launch_stage(c, qr_walk_gait_kernel, per_robot(n), dim3(64), n, D, current_time, robot_stop, reset, d_contact, d_walk_state, d_walk_out, d_ratio, d_vmc_in,
                        stage_args(c, 2, 1));
}

int qrgpu_ground_update_batch(qrgpu_ctx *c, int n, int reset, const float *d_ground_in, double *d_ground_state, float *d_ground_out, float *d_est_in)
{
    if (!batch_ok(c, n) || !d_ground_in || !d_ground_state) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_ground_kernel, per_robot(n), dim3(64), n, reset, d_ground_in, d_ground_state, d_ground_out, d_est_in, stage_args(c, 1, 1));
}

void qrgpu_foothold_desc_default(qrgpu_foothold_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    const float ho[12] = {0.1805f, -0.047f, 0.f, 0.1805f, 0.047f, 0.f, -0.1805f, -0.047f, 0.f, -0.1805f, 0.047f, 0.f};
    const float hp[12] = {0.185f, -0.135f, 0.f, 0.185f, 0.135f, 0.f, -0.185f, -0.135f, 0.f, -0.185f, 0.135f, 0.f};     // config/a1_sim/a1_sim.yaml:40-43
    memcpy(d->hip_offset, ho, sizeof(ho)); memcpy(d->default_hip_position, hp, sizeof(hp));
    d->hip_l = 0.08505f; d->swing_kp[0] = d->swing_kp[1] = d->swing_kp[2] = 0.16f; d->foot_clearance = 0.01f;
}

int qrgpu_footholds_batch(qrgpu_ctx *c, int n, const qrgpu_foothold_desc *desc, const float *d_fh_in, const float *d_gait_state,
                          const float *d_gait_out, float *d_swing_in)
{
    if (!batch_ok(c, n) || !desc || !d_fh_in || !d_swing_in) return QRGPU_ERR_BAD_ARG;
    if ((d_gait_state == nullptr) != (d_gait_out == nullptr)) return QRGPU_ERR_BAD_ARG;      // both or neither
    return launch_stage(c, qr_foothold_kernel, per_robot(n), dim3(64), n, *desc, d_fh_in, d_gait_state, d_gait_out, d_swing_in);
}

// The three stages that take a qrgpu_estimator_desc for the leg geometry alone (swing velocity, swing targets, swing action) pass the caller's block
// as it is: their kernels read hip_l, upper_l, lower_l and hip_offset and nothing else of it (tests/test_gpu_swing_modes.py pins it).
int qrgpu_swing_velocity_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const qrgpu_swing_velocity_desc *vdesc, const float *d_swing_vel_in,
                               float *d_out)
{
    if (!batch_ok(c, n) || !desc || !vdesc || !d_swing_vel_in || !d_out) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_swing_velocity_kernel, per_robot(n), dim3(64), n, *desc, *vdesc, d_swing_vel_in, d_out);
}

int qrgpu_swing_targets_batch(qrgpu_ctx *c, int n, const qrgpu_estimator_desc *desc, const float *d_swing_in, float *d_wbc_cmd, float *d_foot_target_world,
                              float *d_qdes)
{
    if (!batch_ok(c, n) || !desc || !d_swing_in || (!d_wbc_cmd && !d_foot_target_world && !d_qdes)) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_swing_kernel, per_robot(n), dim3(64), n, *desc, d_swing_in, d_wbc_cmd, d_foot_target_world, d_qdes);
}

void qrgpu_swing_mode_desc_default(qrgpu_swing_mode_desc *d, int mode)
{   // config/a1_sim: terrain.yaml (terrain_type 3, gaps 0.51 1.31 1.91, gap_width 0.14) after qrGroundSurfaceEstimator::Reset (:73-100)
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->mode = mode; d->is_sim = 1; d->foothold_delta = 0.10f;
    d->terrain = mode == QRGPU_MODE_POSITION ? 1 : mode == QRGPU_MODE_ADVANCED_TROT ? 2 : 3;
    d->gap_width = 0.14f;
    if (mode == QRGPU_MODE_POSITION) { d->n_gaps = 3; d->gap_distance[0] = 0.51f; d->gap_distance[1] = 1.31f; d->gap_distance[2] = 1.91f; }
}

static bool swing_mode_desc(const qrgpu_swing_mode_desc *d, qrgpu_swing_mode_desc &M)
{
    if (!d || d->mode < 0 || d->mode > 3 || d->n_gaps < 0 || d->n_gaps > QRGPU_SWING_MAX_GAPS) return false;
    M = *d;
    M.n_gaps = d->terrain == 1 ? d->n_gaps : 0;                // the stepper copies gaps on PLUM_PILES only (qr_foot_stepper.cpp:31-38)
    return true;
}

int qrgpu_swing_update_batch(qrgpu_ctx *c, int n, const qrgpu_swing_mode_desc *desc, int reset, int robot_stop, const float *d_est_in,
                             const float *d_est_out, const float *d_gait_out, const float *d_gait_state, float *d_swing_state,
                             float *d_swing_in, float *d_swing_vel_in, float *d_fe_in, int *d_swing_flags)
{
    (void)d_gait_state;
    qrgpu_swing_mode_desc M;
    if (!batch_ok(c, n) || !swing_mode_desc(desc, M) || reset < 0 || reset > 2) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_gait_out || !d_swing_state || !d_swing_flags) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_swing_update_kernel, per_robot(n), dim3(64), n, M, reset, robot_stop ? 1 : 0, d_est_in, d_est_out, d_gait_out, d_swing_state, d_swing_in,
                        d_swing_vel_in, d_fe_in, d_swing_flags, stage_args(c, 2, 1));
}

int qrgpu_swing_action_batch(qrgpu_ctx *c, int n, const qrgpu_swing_mode_desc *desc, const qrgpu_estimator_desc *geom, int robot_stop,
                             const float *d_est_in, const float *d_est_out, const float *d_gait_out, const float *d_gait_state,
                             float *d_swing_state, float *d_out, int *d_swing_flags)
{
    qrgpu_swing_mode_desc M;
    if (!batch_ok(c, n) || !swing_mode_desc(desc, M) || !geom) return QRGPU_ERR_BAD_ARG;
    if (M.mode != QRGPU_MODE_POSITION && M.mode != QRGPU_MODE_WALK) return QRGPU_ERR_BAD_ARG;      // the other two have kernels of their own
    if (!d_est_in || !d_est_out || !d_gait_out || !d_swing_state || !d_out || !d_swing_flags) return QRGPU_ERR_BAD_ARG;
    if (M.mode == QRGPU_MODE_POSITION && !d_gait_state) return QRGPU_ERR_BAD_ARG;                   // allowSwitchLegState
    return launch_stage(c, qr_swing_action_kernel, per_robot(n), dim3(64), n, M, *geom, robot_stop ? 1 : 0, d_est_in, d_est_out, d_gait_out, d_gait_state,
                        d_swing_state, d_out, d_swing_flags);
}

int qrgpu_pack_state_batch(qrgpu_ctx *c, int n, const float com_offset[3], const float *d_est_in, const float *d_est_out, const float *d_rpy,
                           float *d_mpc_state, float *d_fb_state)
{
    if (!batch_ok(c, n) || !com_offset || !d_est_in || !d_est_out || (!d_mpc_state && !d_fb_state)) return QRGPU_ERR_BAD_ARG;
    if (d_mpc_state && !d_rpy) return QRGPU_ERR_BAD_ARG;
    return launch_stage(c, qr_pack_state_kernel, per_robot(n), dim3(64), n, com_offset[0], com_offset[1], com_offset[2], d_est_in, d_est_out, d_rpy, d_mpc_state,
                        d_fb_state);
}

void qrgpu_stance_desc_default(qrgpu_stance_desc *d, int mode)
{   // config/a1_sim/stance_leg_controller.yaml (stance_leg_params of the mode), config/user_parameters.yaml:19-21,40, config/a1_sim/a1_sim.yaml:14,62-67
    // (qr_robot_a1_sim.cpp:104-105), terrain as qrgpu_swing_mode_desc_default
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->mode = mode;
    d->terrain = mode == QRGPU_MODE_POSITION ? 1 : mode == QRGPU_MODE_ADVANCED_TROT ? 2 : 3;
    d->force_in_world = 1;
    static const float KP[4][6] = {{100.f, 100.f, 100.f, 200.f, 200.f, 0.f}, {100.f, 200.f, 200.f, 100.f, 100.f, 200.f}, {100.f, 200.f, 100.f, 100.f, 100.f, 200.f},
                                   {100.f, 100.f, 100.f, 200.f, 200.f, 100.f}};
    static const float KD[4][6] = {{20.f, 20.f, 10.f, 20.f, 20.f, 25.f}, {40.f, 30.f, 10.f, 10.f, 10.f, 30.f}, {40.f, 30.f, 10.f, 10.f, 10.f, 30.f},
                                   {30.f, 20.f, 10.f, 20.f, 20.f, 25.f}};
    const int m = mode >= 0 && mode <= 3 ? mode : 0;
    for (int k = 0; k < 6; ++k) {
        d->kp[k] = KP[m][k]; d->kd[k] = KD[m][k];
        d->max_ddq[k] = (m == 3 || k < 3) ? 10.f : 20.f;
        d->min_ddq[k] = -d->max_ddq[k];
    }
    d->desired_height = 0.27f;
    d->body_height = 0.28f;
    for (int j = 0; j < 12; ++j) { d->motor_kp[j] = 100.f; d->motor_kd[j] = (j % 3 == 0) ? 1.f : 2.f; }
}

static bool stance_desc(const qrgpu_stance_desc *d, qrgpu_stance_desc &S)
{
    if (!d || d->mode < 0 || d->mode > 3 || d->terrain < 0 || d->terrain > 4) return false;
    S = *d;
    S.force_in_world = d->force_in_world ? 1 : 0;
    return true;
}

static bool stance_world(const qrgpu_stance_desc &S) { return S.mode == QRGPU_MODE_WALK || (S.mode == QRGPU_MODE_ADVANCED_TROT && S.force_in_world); }

static int stance_update_check(const qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, qrgpu_stance_desc &S, const float *d_est_in, const float *d_est_out,
                               const float *d_ground_out, const float *d_rpy, const float *d_gait_out, const float *d_gait_state, const float *d_stance_cmd,
                               const float *d_stance_state)
{
    if (!batch_ok(c, n) || !stance_desc(desc, S)) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_ground_out || !d_rpy || !d_gait_out || !d_stance_cmd || !d_stance_state) return QRGPU_ERR_BAD_ARG;
    if ((S.mode == QRGPU_MODE_POSITION || S.mode == QRGPU_MODE_ADVANCED_TROT) && !d_gait_state) return QRGPU_ERR_BAD_ARG;   // allowSwitchLegState
    return QRGPU_OK;
}

static int stance_command_check(const qrgpu_ctx *c, int n, const qrgpu_stance_desc &S, const float *d_vmc_in, const float *d_stance_out, const float *d_tau,
                                const float *d_swing_q, const float *d_swing_flag, const float *d_motor_cmd)
{
    if (!batch_ok(c, n) || !d_tau || !d_motor_cmd) return QRGPU_ERR_BAD_ARG;
    if (S.mode == QRGPU_MODE_WALK && (!d_vmc_in || !d_stance_out)) return QRGPU_ERR_BAD_ARG;             // contacts, N, moveBasePhase
    if ((d_swing_q == nullptr) != (d_swing_flag == nullptr)) return QRGPU_ERR_BAD_ARG;                   // both or neither
    return QRGPU_OK;
}

int qrgpu_stance_update_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset, const float *d_est_in,
                              const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_gait_out, const float *d_gait_state,
                              const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in, float *d_ratio, float *d_stance_out)
{
    qrgpu_stance_desc S;
    const int e = stance_update_check(c, n, desc, S, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state);
    if (e != QRGPU_OK) return e;
    return launch_stage(c, qr_stance_update_kernel, per_robot(n), dim3(64), n, S, current_time, robot_stop ? 1 : 0, reset ? 1 : 0, d_est_in, d_est_out, d_ground_out,
                        d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state, d_vmc_in, d_ratio, d_stance_out, stage_args(c, 1, 1));
}

int qrgpu_stance_command_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, int robot_stop, const float *d_vmc_in, const float *d_stance_out,
                               const float *d_tau, const float *d_swing_q, const float *d_swing_flag, float *d_motor_cmd)
{
    qrgpu_stance_desc S;
    if (!stance_desc(desc, S)) return QRGPU_ERR_BAD_ARG;
    const int e = stance_command_check(c, n, S, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
    if (e != QRGPU_OK) return e;
    return launch_stage(c, qr_stance_command_kernel, per_robot(n), dim3(64), n, S, robot_stop ? 1 : 0, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
}

int qrgpu_stance_tick_batch(qrgpu_ctx *c, int n, const qrgpu_stance_desc *desc, float current_time, int robot_stop, int reset, const int *d_type_id,
                            const float *d_est_in, const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_gait_out,
                            const float *d_gait_state, const float *d_stance_cmd, float *d_stance_state, float *d_vmc_in, float *d_ratio, float *d_stance_out,
                            float *d_force, float *d_tau, int *d_status, const float *d_swing_q, const float *d_swing_flag, float *d_motor_cmd)
{
    qrgpu_stance_desc S;
    int e = stance_update_check(c, n, desc, S, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd, d_stance_state);
    if (e != QRGPU_OK) return e;
    const bool world = stance_world(S);
    if (!d_vmc_in || !d_force || (world && !d_ratio)) return QRGPU_ERR_BAD_ARG;
    e = stance_command_check(c, n, S, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
    if (e != QRGPU_OK) return e;
    if (!(d_type_id ? ready_mask(c->vmc_ready) != 0 : c->vmc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    e = qrgpu_stance_update_batch(c, n, desc, current_time, robot_stop, reset, d_est_in, d_est_out, d_ground_out, d_rpy, d_gait_out, d_gait_state, d_stance_cmd,
                                  d_stance_state, d_vmc_in, d_ratio, d_stance_out);
    if (e != QRGPU_OK) return e;
    const float *d_q = d_est_in + (size_t)17 * n;                                                       // motor angles: rows 17-28 of est_in
    e = launch_vmc(c, n, d_type_id, d_vmc_in, world ? d_ratio : nullptr, d_q, d_force, d_tau, d_status);
    if (e != QRGPU_OK) return e;
    return qrgpu_stance_command_batch(c, n, desc, robot_stop, d_vmc_in, d_stance_out, d_tau, d_swing_q, d_swing_flag, d_motor_cmd);
}

void qrgpu_pose_plan_desc_default(qrgpu_pose_plan_desc *d)
{
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int leg = 0; leg < 4; ++leg) { d->rBH[3 * leg] = leg < 2 ? 0.18f : -0.18f; d->rBH[3 * leg + 1] = (leg & 1) ? 0.047f : -0.047f; }
    d->l_min = 0.22f; d->l_max = 0.35f; d->omega = 0.5f; d->eps = 0.1f; d->body_height = 0.27f; d->loops = QRGPU_POSE_MAX_LOOPS;
}

int qrgpu_pose_plan_batch(qrgpu_ctx *c, int n, const qrgpu_pose_plan_desc *desc, int event, const int *d_event, int reset, const float *d_est_in,
                          const float *d_est_out, const float *d_ground_out, const float *d_rpy, const float *d_walk_out, float *d_pose_state,
                          float *d_stance_cmd, float *d_pose_out, int *d_pose_flags)
{
    if (!batch_ok(c, n) || !desc || event < 0 || event > 3) return QRGPU_ERR_BAD_ARG;
    if (!d_est_in || !d_est_out || !d_ground_out || !d_rpy || !d_walk_out || !d_pose_state || !d_stance_cmd || !d_pose_flags) return QRGPU_ERR_BAD_ARG;
    const bool masked = c->stage_reset.d_mask != nullptr;                                               // a masked robot is reset also where nothing else happens
    if (!d_event && event == 0 && !reset && !masked) return QRGPU_OK;                                   // nothing to do: no launch
    return launch_stage(c, qr_pose_plan_kernel, dim3(8 * ((n + 7) / 8)), dim3(64), n, *desc, event, d_event, reset ? 1 : 0, d_est_in, d_est_out, d_ground_out, d_rpy,
                        d_walk_out, d_pose_state, d_stance_cmd, d_pose_out, d_pose_flags, stage_args(c, 1, 1));
}

int qrgpu_mpc_frontend_batch(qrgpu_ctx *c, int n, int num_horizon_l, float dt_ctrl, float dt_mpc, const float *d_fe_in, float *d_fe_state,
                             float *d_traj, float *d_gait, float *d_wbc_cmd, int *d_mpc_updated)
{
    if (!batch_ok(c, n) || !d_fe_in || !d_fe_state || !d_traj || !d_gait) return QRGPU_ERR_BAD_ARG;
    if (num_horizon_l <= 0 || !(dt_ctrl > 0.f) || !(dt_mpc > 0.f)) return QRGPU_ERR_BAD_ARG;
    // iterationsInaMPC = round(dtMPC / dt) (:51); the cadence takes a remainder by half of it, so the reference cannot run below 2.  The upper
    // bound keeps the period within what the float counter row can hold (include/qrgpu.h).
    const float iterations = roundf(dt_mpc / dt_ctrl);
    if (!(iterations >= 2.f && iterations <= 16777216.f)) return QRGPU_ERR_BAD_ARG;
    if (!c->mpc_ready[0]) return QRGPU_ERR_NOT_SETUP;
    return launch_stage(c, qr_frontend_kernel, per_robot(n), dim3(64, c->mpc.horizon), n, c->mpc.horizon, num_horizon_l, dt_ctrl, dt_mpc, (int)iterations / 2,
                        d_fe_in, d_fe_state, d_traj, d_gait, d_wbc_cmd, d_mpc_updated, stage_args(c, QRGPU_STAGE_RESET_CONSTRUCT, QRGPU_STAGE_RESET_LIVE));
}

void qrgpu_plant_params_default(qrgpu_plant_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->dt = 0.002f; p->substeps = 2;
    p->contact_k = 2e4f; p->contact_a = 1.0f; p->mu = 0.6f; p->v_eps = 0.01f; p->ground_z = 0.f;
    p->tau_max = 33.5f;                                                                                 // a1_description's joint effort limit
    p->contact_threshold = 5.0f;                                                                        // qr_robot_a1_sim.cpp:662
    p->com_offset[0] = -0.008f; p->com_offset[1] = 0.005f; p->com_offset[2] = 0.f;                      // config/a1_sim/a1_sim.yaml (A1's comOffset)
}

// The plant kernels read the model constants the WBC launch reads: the same readiness rule, the same upload.
static int plant_model(qrgpu_ctx *c, const int *d_type_id)
{
    if (!(d_type_id ? ready_mask(c->wbc_ready) != 0 : c->wbc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    return upload_wbc(c);
}
static dim3 per_quad(int n) { return dim3((n + 15) / 16); }      // four lanes per robot, one wavefront per workgroup

int qrgpu_forward_dynamics_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_fb_state, const float *d_tau, const float *d_foot_force,
                                 float *d_nu_dot, int *d_status)
{
    if (!batch_ok(c, n) || !d_fb_state || !d_tau || !d_nu_dot) return QRGPU_ERR_BAD_ARG;
    const int e = plant_model(c, d_type_id);
    if (e != QRGPU_OK) return e;
    return launch_stage(c, qr_fwd_dyn_kernel, per_quad(n), dim3(64), n, (const WbcConst *)c->d_wbc, d_type_id, ready_mask(c->wbc_ready), d_fb_state, d_tau, d_foot_force,
                        d_nu_dot, d_status);
}

int qrgpu_plant_step_batch(qrgpu_ctx *c, int n, const qrgpu_plant_params *params, const int *d_type_id, float *d_fb_state, const float *d_motor_cmd,
                           float *d_plant_out, float *d_mpc_state, float *d_est_in, int *d_status)
{
    if (!batch_ok(c, n) || !params || !d_fb_state || !d_motor_cmd) return QRGPU_ERR_BAD_ARG;
    if (params->substeps < 1 || params->substeps > 64 || !(params->dt > 0.f)) return QRGPU_ERR_BAD_ARG;
    const int e = plant_model(c, d_type_id);
    if (e != QRGPU_OK) return e;
    return launch_stage(c, qr_plant_step_kernel, per_quad(n), dim3(64), n, *params, (const WbcConst *)c->d_wbc, d_type_id, ready_mask(c->wbc_ready), d_fb_state,
                        d_motor_cmd, d_plant_out, d_mpc_state, d_est_in, d_status);
}

int qrgpu_plant_step_terrain_batch(qrgpu_ctx *c, int n, const qrgpu_plant_params *params, const qrgpu_terrain_desc *terrain, const float *d_height,
                                   const int *d_field_id, const float *d_base_push, const int *d_type_id, float *d_fb_state, const float *d_motor_cmd,
                                   float *d_plant_out, float *d_terrain_out, float *d_mpc_state, float *d_est_in, int *d_status)
{
    if (!batch_ok(c, n) || !params || !d_fb_state || !d_motor_cmd || !terrain || !d_height) return QRGPU_ERR_BAD_ARG;
    if (params->substeps < 1 || params->substeps > 64 || !(params->dt > 0.f)) return QRGPU_ERR_BAD_ARG;
    if (terrain->nx < 2 || terrain->ny < 2 || terrain->n_fields < 1 || !(terrain->cell > 0.f) || !std::isfinite(terrain->cell)) return QRGPU_ERR_BAD_ARG;
    if (!std::isfinite(terrain->x0) || !std::isfinite(terrain->y0)) return QRGPU_ERR_BAD_ARG;
    const int e = plant_model(c, d_type_id);
    if (e != QRGPU_OK) return e;
    return launch_stage(c, qr_plant_step_terrain_kernel, per_quad(n), dim3(64), n, *params, *terrain, (const WbcConst *)c->d_wbc, d_type_id, ready_mask(c->wbc_ready),
                        d_height, d_field_id, d_base_push, d_fb_state, d_motor_cmd, d_plant_out, d_terrain_out, d_mpc_state, d_est_in, d_status);
}

void qrgpu_plant_body_desc_default(qrgpu_plant_body_desc *d)
{   // a1_description: the trunk's collision box 0.267 x 0.194 x 0.114 at the base origin; hip +-46 deg, thigh -60..240 deg, calf -154.5..-52.5 deg
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->trunk_half[0] = 0.1335f; d->trunk_half[1] = 0.097f; d->trunk_half[2] = 0.057f;
    d->q_lo[0] = -0.802851455917f; d->q_hi[0] = 0.802851455917f;
    d->q_lo[1] = -1.0471975512f; d->q_hi[1] = 4.18879020479f;
    d->q_lo[2] = -2.69653369433f; d->q_hi[2] = -0.916297857297f;
    d->limit_k = 150.f; d->limit_a = 0.02f;                       // include/qrgpu.h derives them
}

int qrgpu_plant_body_setup(qrgpu_ctx *c, int type_id, const qrgpu_plant_body_desc *desc)
{
    if (!c || type_id < 0 || type_id >= QRGPU_MAX_TYPES || !desc) return QRGPU_ERR_BAD_ARG;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(desc->trunk_half[k]) || !(desc->trunk_half[k] > 0.f) || !std::isfinite(desc->trunk_center[k])) return QRGPU_ERR_BAD_ARG;
        if (!std::isfinite(desc->q_lo[k]) || !std::isfinite(desc->q_hi[k]) || !(desc->q_lo[k] < desc->q_hi[k])) return QRGPU_ERR_BAD_ARG;
    }
    if (!std::isfinite(desc->limit_k) || !(desc->limit_k >= 0.f) || !std::isfinite(desc->limit_a) || !(desc->limit_a >= 0.f)) return QRGPU_ERR_BAD_ARG;
    c->body_host[type_id] = *desc;
    c->body_ready[type_id] = true;
    c->body_dirty = true;
    return QRGPU_OK;
}

int qrgpu_plant_step_body_batch(qrgpu_ctx *c, int n, const qrgpu_plant_params *params, const qrgpu_terrain_desc *terrain, const float *d_height,
                                const int *d_field_id, const float *d_base_push, const int *d_type_id, float *d_fb_state, const float *d_motor_cmd,
                                float *d_plant_out, float *d_terrain_out, float *d_body_out, float *d_mpc_state, float *d_est_in, int *d_status)
{
    if (!batch_ok(c, n) || !params || !d_fb_state || !d_motor_cmd || !terrain || !d_height) return QRGPU_ERR_BAD_ARG;
    if (params->substeps < 1 || params->substeps > 64 || !(params->dt > 0.f)) return QRGPU_ERR_BAD_ARG;
    if (terrain->nx < 2 || terrain->ny < 2 || terrain->n_fields < 1 || !(terrain->cell > 0.f) || !std::isfinite(terrain->cell)) return QRGPU_ERR_BAD_ARG;
    if (!std::isfinite(terrain->x0) || !std::isfinite(terrain->y0)) return QRGPU_ERR_BAD_ARG;
    for (int t = 0; t < QRGPU_MAX_TYPES; ++t) if (c->wbc_ready[t] && !c->body_ready[t]) return QRGPU_ERR_NOT_SETUP;      // a type with a model and no body
    const int e = plant_model(c, d_type_id);
    if (e != QRGPU_OK) return e;
    if (c->body_dirty) {
        HIPCHK(c, hipMemcpyAsync(c->d_body, c->body_host, sizeof(c->body_host), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->body_dirty = false;
    }
    return launch_stage(c, qr_plant_step_body_kernel, per_quad(n), dim3(64), n, *params, *terrain, (const WbcConst *)c->d_wbc, (const qrgpu_plant_body_desc *)c->d_body,
                        d_type_id, ready_mask(c->wbc_ready), d_height, d_field_id, d_base_push, d_fb_state, d_motor_cmd, d_plant_out, d_terrain_out, d_body_out,
                        d_mpc_state, d_est_in, d_status);
}

void qrgpu_episode_desc_default(qrgpu_episode_desc *d)
{   // spawn height, stand pose and settle gains of tools/closed_loop.py
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->status_mask = QRGPU_PL_NONFINITE | QRGPU_PL_QUAT_ZERO | QRGPU_PL_TRUNK_CONTACT; d->status_ticks = 1;
    d->seed = 1u;
    d->tilt_max = 1.0f; d->min_clearance = 0.10f; d->spawn_height = 0.30f;
    for (int l = 0; l < 4; ++l) { d->q_spawn[3 * l] = 0.f; d->q_spawn[3 * l + 1] = 0.8f; d->q_spawn[3 * l + 2] = -1.6f; }
    d->kp = 100.f; d->kd = 2.f;
}

// BAD_ARG with the argument's name in qrgpu_last_error
static int bad_arg(qrgpu_ctx *c, const char *what)
{
    if (c) c->err = std::string("qrgpu_episode_step_batch: ") + what;
    return QRGPU_ERR_BAD_ARG;
}

int qrgpu_episode_step_batch(qrgpu_ctx *c, int n, const qrgpu_episode_desc *desc, int reset_all, const qrgpu_plant_params *params, const qrgpu_terrain_desc *terrain,
                             const float *d_height, const int *d_field_id, const float *d_spawn, int n_spawn, const int *d_plant_status, const int *d_tick_status,
                             const int *d_force_reset, float *d_fb_state, float *d_prev_ori, float *d_motor_cmd, int *d_ep_state, float *d_ep_stats, int *d_done,
                             int *d_done_list, int *d_done_count)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return bad_arg(c, "n");
    if (!desc) return bad_arg(c, "desc");
    if (!d_fb_state) return bad_arg(c, "d_fb_state");
    if (!d_ep_state) return bad_arg(c, "d_ep_state");
    if (!d_ep_stats) return bad_arg(c, "d_ep_stats");
    if (!d_done) return bad_arg(c, "d_done");
    if (!d_spawn) return bad_arg(c, "d_spawn");
    if (n_spawn < 1) return bad_arg(c, "n_spawn");
    if (d_done_list && !d_done_count) return bad_arg(c, "d_done_count");
    qrgpu_terrain_desc T;
    memset(&T, 0, sizeof(T));
    if (terrain) {
        if (terrain->nx < 2 || terrain->ny < 2 || terrain->n_fields < 1 || !(terrain->cell > 0.f) || !std::isfinite(terrain->cell) || !std::isfinite(terrain->x0) ||
            !std::isfinite(terrain->y0)) return bad_arg(c, "terrain");
        if (!d_height) return bad_arg(c, "d_height");
        T = *terrain;
    }
    if (desc->status_ticks < 1) return bad_arg(c, "status_ticks");
    if (desc->max_ticks < 0) return bad_arg(c, "max_ticks");
    const struct { const char *name; float v; } nonneg[] = {{"tilt_max", desc->tilt_max}, {"min_clearance", desc->min_clearance}, {"field_margin", desc->field_margin},
        {"spawn_height", desc->spawn_height}, {"xy_jitter", desc->xy_jitter}, {"yaw_jitter", desc->yaw_jitter}, {"q_jitter", desc->q_jitter},
        {"v_jitter", desc->v_jitter}, {"kp", desc->kp}, {"kd", desc->kd}};
    for (const auto &a : nonneg) if (!std::isfinite(a.v) || !(a.v >= 0.f)) return bad_arg(c, a.name);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(desc->q_spawn[k])) return bad_arg(c, "q_spawn");
    const float ground_z = params ? params->ground_z : 0.f;
    if (!std::isfinite(ground_z)) return bad_arg(c, "params->ground_z");
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    HIPCHK(c, hipSetDevice(c->device));
    if (d_done_count) HIPCHK(c, hipMemsetAsync(d_done_count, 0, sizeof(int), c->stream));
    return launch_stage(c, qr_episode_kernel, per_robot(n), dim3(64), n, *desc, episode::cos_tilt_of(desc->tilt_max), reset_all != 0 ? 1 : 0, ground_z, terrain ? 1 : 0, T,
                        d_height, d_field_id, d_spawn, n_spawn, d_plant_status, d_tick_status, d_force_reset, d_fb_state, d_prev_ori, d_motor_cmd, d_ep_state,
                        d_ep_stats, d_done, d_done_list, d_done_count);
}

int qrgpu_set_stage_reset(qrgpu_ctx *c, const qrgpu_stage_reset *r)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!r) { c->stage_reset = qrgpu_stage_reset{}; return QRGPU_OK; }
    const char *what = nullptr;
    if (!r->d_mask && !r->d_ticks) what = "d_mask and d_ticks are both NULL";
    else if (r->d_mask && r->bits == 0u) what = "bits";
    else if (r->d_mask && r->level != QRGPU_STAGE_RESET_CONSTRUCT && r->level != QRGPU_STAGE_RESET_LIVE) what = "level";
    else if (r->d_ticks && (!std::isfinite(r->tick_dt) || !(r->tick_dt > 0.f))) what = "tick_dt";
    if (what) { c->err = std::string("qrgpu_set_stage_reset: ") + what; return QRGPU_ERR_BAD_ARG; }
    c->stage_reset = *r;
    if (!r->d_mask) { c->stage_reset.bits = 0u; c->stage_reset.level = QRGPU_STAGE_RESET_CONSTRUCT; }       // fields that are not read
    if (!r->d_ticks) c->stage_reset.tick_dt = 0.f;
    return QRGPU_OK;
}

void qrgpu_observe_desc_default(qrgpu_observe_desc *d, int variant)
{   // qr_robot.cpp:30-37 (the windows are the kernel's), qr_robot_a1_sim.cpp:606-670, qr_robot_a1.cpp:140-193; geometry as qrgpu_estimator_desc_default
    if (!d) return;
    memset(d, 0, sizeof(*d));
    const bool hardware = variant == QRGPU_OBS_HARDWARE;
    d->filter_rpy = hardware ? 0 : 1; d->filter_motor_velocity = hardware ? 1 : 0;
    d->hip_l = 0.08505f; d->upper_l = 0.2f; d->lower_l = 0.2f;
    const float ho[12] = {0.1805f, -0.047f, 0.f, 0.1805f, 0.047f, 0.f, -0.1805f, -0.047f, 0.f, -0.1805f, 0.047f, 0.f};
    memcpy(d->hip_offset, ho, sizeof(ho));
    d->base_height = 0.27f; d->tick_ms = 2u; d->seed = 1u;
}

int qrgpu_observe_state_rows(const qrgpu_observe_desc *d) { return !d ? 0 : d->filter_motor_velocity ? QRGPU_OBSERVE_STATE_ROWS_MV : QRGPU_OBSERVE_STATE_ROWS; }

static int observe_bad(qrgpu_ctx *c, const char *what)
{
    if (c) c->err = std::string("qrgpu_observe_batch: ") + what;
    return QRGPU_ERR_BAD_ARG;
}

int qrgpu_observe_batch(qrgpu_ctx *c, int n, const qrgpu_observe_desc *desc, int reset, unsigned step, const float *d_raw, const float *d_est_out_prev,
                        float *d_obs_state, float *d_est_in, float *d_rpy, float *d_ground_in, unsigned *d_tick)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return observe_bad(c, "n");
    if (!desc) return observe_bad(c, "desc");
    if (!d_raw) return observe_bad(c, "d_raw");
    if (!d_obs_state) return observe_bad(c, "d_obs_state");
    if (!d_est_in) return observe_bad(c, "d_est_in");
    if (!d_rpy) return observe_bad(c, "d_rpy");
    if (desc->tick_ms == 0u) return observe_bad(c, "tick_ms");
    const struct { const char *name; float v; } noise[] = {{"acc_noise", desc->acc_noise}, {"gyro_noise", desc->gyro_noise}, {"q_noise", desc->q_noise},
        {"qd_noise", desc->qd_noise}};
    for (const auto &a : noise) if (!std::isfinite(a.v) || !(a.v >= 0.f)) return observe_bad(c, a.name);
    const struct { const char *name; float v; } finite[] = {{"yaw_offset", desc->yaw_offset}, {"base_height", desc->base_height}, {"hip_l", desc->hip_l},
        {"upper_l", desc->upper_l}, {"lower_l", desc->lower_l}};
    for (const auto &a : finite) if (!std::isfinite(a.v)) return observe_bad(c, a.name);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(desc->hip_offset[k])) return observe_bad(c, "hip_offset");
    return launch_stage(c, qr_observe_kernel, per_robot(n), dim3(64), n, *desc, reset != 0 ? 1 : 0, step, stage_mask_args(c), d_raw, d_est_out_prev, d_obs_state,
                        d_est_in, d_rpy, d_ground_in, d_tick);
}

}  // extern "C"
