// One prototype per __global__ kernel of libqrgpu.so, included by the host files that launch the kernels and by the kernel files that define
// them: a kernel's signature is written here and at its definition, nowhere else.
#pragma once
#include "qr_device_types.h"

namespace qrgpu {

// qr_mpc_kernel.hip; the same kernels with the executed-arithmetic counters compiled in: qr_mpc_kernel_fl.hip.
// The launch bounds of the templates are part of the prototype: an instantiation takes them from the FIRST declaration it sees, and one
// declared here without them was compiled for 1024 threads and no register budget (the definitions use the same two macros).
// The macros name the template parameters: wherever they expand, those must be spelled MAXB, BIG, LIST, NTHR and MINW.
#define QR_MAIN_WAVES_PER_SIMD 3     // register budget of the h <= 11 main pass: 3 workgroups per CU (168 VGPRs); the LDS allotment decides how many run
#define QR_MPC_KERNEL_BOUNDS  __launch_bounds__(NTHR, (MINW ? MINW : ((MAXB <= 4 && !LIST && !BIG) ? (NTHR >= 384 ? 4 : QR_MAIN_WAVES_PER_SIMD) : (NTHR >= 512 ? 2 : 1))))
#define QR_MPC_PERSIST_BOUNDS __launch_bounds__(NTHR, (MINW ? MINW : ((MAXB <= 4 && !BIG) ? (NTHR >= 384 ? 4 : QR_MAIN_WAVES_PER_SIMD) : (NTHR >= 512 ? 2 : 1))))
template <int MAXB, bool BIG, bool LIST, int NTHR, int MINW = 0, bool H16 = (MAXB > 4)> __global__ QR_MPC_KERNEL_BOUNDS void qr_mpc_kernel(MpcLaunch P, MpcIO io);
template <int MAXB, bool BIG, bool LIST, int NTHR, int MINW = 0, bool H16 = (MAXB > 4)> __global__ QR_MPC_KERNEL_BOUNDS void qr_mpc_kernel_fl(MpcLaunch P, MpcIO io);
template <int MAXB, bool BIG, int NTHR, int MINW = 0> __global__ QR_MPC_PERSIST_BOUNDS void qr_mpc_persist_kernel(MpcLaunch P, MpcIO io);
#define QR_MPC_INSTANCES(K)                                  \
    extern template __global__ void K<2, false, false, 512>(MpcLaunch, MpcIO);          \
    extern template __global__ void K<4, true, true, 256>(MpcLaunch, MpcIO);            \
    extern template __global__ void K<2, true, false, 512>(MpcLaunch, MpcIO);           \
    extern template __global__ void K<2, true, false, 512, 4, true>(MpcLaunch, MpcIO);  \
    extern template __global__ void K<5, true, false, 512>(MpcLaunch, MpcIO);           \
    extern template __global__ void K<9, true, true, 256>(MpcLaunch, MpcIO);
QR_MPC_INSTANCES(qr_mpc_kernel)
QR_MPC_INSTANCES(qr_mpc_kernel_fl)
#undef QR_MPC_INSTANCES
extern template __global__ void qr_mpc_kernel<4, true, true, 256, 2, true>(MpcLaunch, MpcIO);
extern template __global__ void qr_mpc_persist_kernel<2, false, 512>(MpcLaunch, MpcIO);
extern template __global__ void qr_mpc_persist_kernel<5, true, 512>(MpcLaunch, MpcIO);
__global__ void qr_lpt_order_kernel(int n, const int *cost, int *order, const int *ftime, int *wbc_order);
__global__ void qr_gate_kernel(int *counter, int expected_total, long long max_ticks, int *timed_out, int timed_out_value, int *bump);
__global__ void qr_gate2_kernel(int *c0, int e0, int *c1, int e1, long long max_ticks, long long *stamp);
__global__ void qr_join_kernel(int *counter, int expected_total, long long max_ticks, int *timed_out, int *g0, int e0, int *g1, int e1, int *tick_done,
                               int *lane_done, int lane_expect, long long *dbg);
__global__ void qr_probe_wait_kernel(int *flag, int *out, long long max_ticks, int token);
__global__ void qr_probe_set_kernel(int *flag, int token);
__global__ void qr_selftest_kernel(double *out);

// qr_wbc_kernel.hip; with the inspection outputs and cycle stamps compiled in: qr_wbc_kernel_dbg.hip
__global__ void qr_wbc_kernel(int n, const WbcConst *types, const int *type_id, const float *g_state, const float *g_cmd,
                              float *g_prev, float *g_tau, float *g_qdes, int *g_status, float *g_dbg, int merge_tau, int status_or, long long *dbgT,
                              const float *g_fr, int type_ready, int epilogue, float *g_qp, WbcPipe pipe);
__global__ void qr_wbc_kernel_dbg(int n, const WbcConst *types, const int *type_id, const float *g_state, const float *g_cmd,
                                  float *g_prev, float *g_tau, float *g_qdes, int *g_status, float *g_dbg, int merge_tau, int status_or, long long *dbgT,
                                  const float *g_fr, int type_ready, int epilogue, float *g_qp, WbcPipe pipe);

// The binding of qrgpu_set_stage_reset as a stage kernel takes it, always its last argument: robot i is reset at `level` -- already the stage's own
// number; the front-end takes the QRGPU_STAGE_RESET_* value itself -- where mask[i] & bits, and its clock is ticks[i] * tick_dt.  A null mask resets
// nobody and a null tick array leaves the call's scalar clock: that is every caller that has bound nothing.
struct StageResetArgs {
    const int *mask;      // [n] or null
    unsigned bits;
    int level;
    const int *ticks;     // [n] or null
    float tick_dt;
};
// Robot i's mask word (0 without a mask) and clock (the call's scalar without a tick array): one row load each, issued with the first state loads.
__device__ __forceinline__ bool stage_masked(const StageResetArgs &SR, int i) { return SR.mask && ((unsigned)SR.mask[i] & SR.bits) != 0u; }
__device__ __forceinline__ float stage_time(const StageResetArgs &SR, int i, float scalar)
{
#pragma clang fp contract(off)
    return SR.ticks ? (float)SR.ticks[i] * SR.tick_dt : scalar;
}

// qr_frontend_kernel.hip, qr_vmc_kernel.hip
__global__ void qr_frontend_kernel(int n, int horizon, int numHorizonL, float dt, float dtMPC, int period, const float *fin, float *fst,
                                   float *g_traj, float *g_gait, float *g_cmd, int *g_updated, StageResetArgs SR);
__global__ void qr_vmc_kernel(VmcLaunch P, const int *type_id, const float *g_in, const float *g_q, float *g_force, float *g_tau, int *g_status);

// qr_estimator_kernel.hip
__global__ void qr_estimator_kernel(int n, qrgpu_estimator_desc D, const float *g_in, const unsigned *g_tick, double *st, float *g_out, StageResetArgs SR);
__global__ void qr_pack_state_kernel(int n, float c0, float c1, float c2, const float *g_in, const float *g_est, const float *g_rpy, float *g_mpc, float *g_fb);
__global__ void qr_swing_kernel(int n, qrgpu_estimator_desc D, const float *g_in, float *g_cmd, float *g_tgt_world, float *g_qdes);
__global__ void qr_foothold_kernel(int n, qrgpu_foothold_desc D, const float *g_in, const float *g_gait_state, const float *g_gait_out, float *g_swing);
__global__ void qr_ground_kernel(int n, int fresh, const float *g_in, double *g_st, float *g_out, float *g_est_in, StageResetArgs SR);
__global__ void qr_walk_gait_kernel(int n, WalkDesc D, float currentTime, int stop, int fresh, const float *g_contact, float *st, float *g_out, float *g_ratio,
                                    float *g_vmc_in, StageResetArgs SR);
__global__ void qr_swing_velocity_kernel(int n, qrgpu_estimator_desc D, qrgpu_swing_velocity_desc V, const float *g_in, float *g_out);

// qr_swing_modes_kernel.hip, qr_stance_kernel.hip, qr_pose_plan_kernel.hip
__global__ void qr_swing_update_kernel(int n, qrgpu_swing_mode_desc M, int reset, int stop, const float *g_est_in, const float *g_est_out, const float *g_gait_out,
                                       float *g_st, float *g_swing_in, float *g_swing_vel_in, float *g_fe_in, int *g_flags, StageResetArgs SR);
__global__ void qr_swing_action_kernel(int n, qrgpu_swing_mode_desc M, qrgpu_estimator_desc D, int stop, const float *g_est_in, const float *g_est_out,
                                       const float *g_gait_out, const float *g_gait_state, float *g_st, float *g_out, int *g_flags);
__global__ void qr_stance_update_kernel(int n, qrgpu_stance_desc S, float current_time, int stop, int reset, const float *g_est_in, const float *g_est_out,
                                        const float *g_ground, const float *g_rpy, const float *g_gait_out, const float *g_gait_state, const float *g_cmd,
                                        float *g_st, float *g_vmc_in, float *g_ratio, float *g_out, StageResetArgs SR);
__global__ void qr_stance_command_kernel(int n, qrgpu_stance_desc S, int stop, const float *g_vmc_in, const float *g_stance_out, const float *g_tau,
                                         const float *g_swing_q, const float *g_swing_flag, float *g_cmd);
__global__ void qr_pose_plan_kernel(int n, qrgpu_pose_plan_desc D, int event, const int *g_event, int reset, const float *g_est_in, const float *g_est_out,
                                    const float *g_ground, const float *g_rpy, const float *g_walk, float *g_state, float *g_cmd, float *g_out, int *g_flags,
                                    StageResetArgs SR);

// qr_plant_kernel.hip: four lanes per robot, sixteen robots per workgroup of one wavefront
__global__ void qr_fwd_dyn_kernel(int n, const WbcConst *types, const int *type_id, int type_ready, const float *g_state, const float *g_tau, const float *g_ff,
                                  float *g_nudot, int *g_status);
__global__ void qr_plant_step_kernel(int n, qrgpu_plant_params P, const WbcConst *types, const int *type_id, int type_ready, float *g_state, const float *g_cmd,
                                     float *g_out, float *g_mpc, float *g_est, int *g_status);
__global__ void qr_plant_step_terrain_kernel(int n, qrgpu_plant_params P, qrgpu_terrain_desc T, const WbcConst *types, const int *type_id, int type_ready,
                                             const float *g_height, const int *g_field, const float *g_push, float *g_state, const float *g_cmd, float *g_out,
                                             float *g_tout, float *g_mpc, float *g_est, int *g_status);


// qr_plant_body_kernel.hip: the terrain step with knee and trunk contact and joint limits; bodies [QRGPU_MAX_TYPES] beside types
__global__ void qr_plant_step_body_kernel(int n, qrgpu_plant_params P, qrgpu_terrain_desc T, const WbcConst *types, const qrgpu_plant_body_desc *bodies,
                                          const int *type_id, int type_ready, const float *g_height, const int *g_field, const float *g_push, float *g_state,
                                          const float *g_cmd, float *g_out, float *g_tout, float *g_bout, float *g_mpc, float *g_est, int *g_status);

// qr_episode_kernel.hip: one lane per robot; termination, statistics, spawn, the list of the robots reset
__global__ void qr_episode_kernel(int n, qrgpu_episode_desc D, double cos_tilt, int reset_all, float ground_z, int has_terrain, qrgpu_terrain_desc T,
                                  const float *g_height, const int *g_field, const float *g_spawn, int n_spawn, const int *g_pstatus, const int *g_tstatus,
                                  const int *g_force, float *g_state, float *g_prev, float *g_cmd, int *g_st, float *g_stats, int *g_done, int *g_list,
                                  int *g_count);

// qr_observe_kernel.hip: one lane per robot; ReceiveObservation's filters, yaw logic and quaternion, the inputs of the ground and estimator stages
__global__ void qr_observe_kernel(int n, qrgpu_observe_desc D, int reset, unsigned step, StageResetArgs SR, const float *g_raw, const float *g_prev, float *g_st,
                                  float *g_est_in, float *g_rpy, float *g_ground_in, unsigned *g_tick);

// qr_dataflow_kernel.hip: one lane per robot; the operator's command, the getters between the trot's stages, the motor command of the MPC mode
__global__ void qr_command_kernel(int n, qrgpu_command_desc D, int reset, StageResetArgs SR, const float *g_joy, float *g_st, float *g_des, float *g_fe, float *g_fh,
                                  float *g_sv, float *g_sc);
__global__ void qr_trot_inputs_kernel(int n, const float *g_est_in, const float *g_est_out, const float *g_rpy, const float *g_gait_out, const float *g_gait_state,
                                      float *g_fe, float *g_fh, float *g_sw, float *g_est_w);
__global__ void qr_mpc_command_kernel(int n, qrgpu_mpc_command_desc D, int reset, StageResetArgs SR, const float *g_tau, const float *g_qdes, const float *g_sw,
                                      const float *g_gait_out, const float *g_gait_state, int *g_mem, float *g_cmd);

// qr_cadence_kernel.hip: one lane per robot; between the MPC and the WBC launch of the cadenced tick: the kept base-frame force of the robots just
// solved, the torques and the status word of the others.  The leg geometry per type is the MPC launch's (MpcType).
struct CadenceLegs {
    float hip_l[QRGPU_MAX_TYPES], upper_l[QRGPU_MAX_TYPES], lower_l[QRGPU_MAX_TYPES];
    int type_ready;       // bit t: type t was set up
};
// g_skip (qrgpu_set_mode_route; null: nobody): with it g_due is the masked due', and a robot that is not due and whose word of g_skip is non-zero -- a
// robot that is not on the MPC chain -- is left alone.
__global__ void qr_cadence_kernel(int n, CadenceLegs L, const int *g_type, const int *g_due, const float *g_mpc_state, const float *g_fb_state, const float *g_force,
                                  float *g_hold, float *g_tau, int *g_status, const int *g_skip);

// qr_mode_route_kernel.hip: one lane per robot; the chain each robot's mode selects, the masks of the cadenced tick under it, the chain's motor command
__global__ void qr_mode_route_kernel(int n, qrgpu_mode_route_desc D, const float *g_sel, const int *g_plan, int *g_chain, int *g_flags, int *g_count);
__global__ void qr_mode_masks_kernel(int n, const int *g_updated, const int *g_chain, int *g_due, int *g_skip);
__global__ void qr_mode_command_kernel(int n, const int *g_chain, const float *g_cmd_mpc, const float *g_cmd_fb, const int *g_st_mpc, const int *g_st_fb,
                                       float *g_out, int *g_st_out);

// qr_fsm_kernel.hip: one lane per robot; the control state machine: what runs this tick, the zeroed command of a transition, the command sent
__global__ void qr_fsm_update_kernel(int n, qrgpu_fsm_desc D, int reset, const float *g_msg, const float *g_script, int n_script, const int *g_ticks,
                                     const int *g_done, unsigned bits, float *g_st, float *g_joy, int *g_plan, int *g_stage_mask);
__global__ void qr_fsm_zero_kernel(int n, const int *g_plan, float *g_des, float *g_fe, float *g_fh, float *g_sv, float *g_sc);
__global__ void qr_fsm_command_kernel(int n, qrgpu_fsm_desc D, const int *g_plan, const float *g_est_in, const float *g_loco, float *g_st, float *g_cmd,
                                      float *g_out);

// qr_gait_kernel.hip: one lane per robot; the open-loop gait generator on the call's one gait and on the table entry each robot latched at its last
// reset (the table in device memory, indexed per lane), and the clock that counts from where a mask last said
__global__ void qr_gait_kernel(int n, qrgpu_gait_desc D, float currentTime, int stop, int fresh, const float *g_contact, float *st, float *g_out, float *g_fe,
                               StageResetArgs SR);
__global__ void qr_gait_select_kernel(int n, const qrgpu_gait_desc *g_table, int n_gaits, const float *g_sel, float currentTime, int stop, int fresh,
                                      const float *g_contact, float *st, float *g_out, float *g_fe, float *g_sw, int *g_flags, StageResetArgs SR);
__global__ void qr_stage_clock_kernel(int n, const int *g_mask, unsigned bits, const int *g_ticks, int *g_origin, int *g_local);

// qr_velocity_flow_kernel.hip: one lane per robot; the getters between the stages of the force-balance trot, the entries of its swing command
__global__ void qr_velocity_flow_kernel(int n, int terrain, int reset, StageResetArgs SR, const float *g_est_in, const float *g_est_out, const float *g_ground,
                                        const float *g_gait_out, const float *g_gait_state, const float *g_des, float *g_sv, float *g_est_w, int *g_mem,
                                        float *g_flag);

}  // namespace qrgpu
