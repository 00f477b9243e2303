// ============================================================================
// libqrgpu.so host side: the control state machine (qr_fsm_kernel.hip) and the defaults of its parameter block.
// Every entry point is "check the arguments, one launch on the context's stream" (qrgpu_dataflow.hip).
// ============================================================================
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>

#include "qrgpu_ctx.h"

static int fsm_bad(qrgpu_ctx *c, const char *call, const char *what)
{
    if (c) c->err = std::string(call) + ": " + what;
    return QRGPU_ERR_BAD_ARG;
}

template <typename... KArgs, typename... Args>
static int fsm_launch(qrgpu_ctx *c, void (*kernel)(KArgs...), int n, Args... args)
{
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, args...);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

static bool fsm_positive(float v) { return std::isfinite(v) && v > 0.f; }

// the field of the desc a call refuses, or null
static const char *fsm_desc_bad(const qrgpu_fsm_desc *d)
{
    if (!fsm_positive(d->stand_up_time)) return "desc->stand_up_time";
    if (!fsm_positive(d->stand_up_total)) return "desc->stand_up_total";
    if (!fsm_positive(d->sit_down_time)) return "desc->sit_down_time";
    if (!fsm_positive(d->time_step)) return "desc->time_step";
    if (d->transition_ticks < 1) return "desc->transition_ticks";
    if (!fsm_positive(d->gait_transition_duration)) return "desc->gait_transition_duration";
    if (!fsm_positive(d->stand_transition_duration)) return "desc->stand_transition_duration";
    if (!fsm_positive(d->tau_clip)) return "desc->tau_clip";
    if (d->initial_ctrl_state < 0 || d->initial_ctrl_state > 7) return "desc->initial_ctrl_state";
    return nullptr;
}

extern "C" {

void qrgpu_fsm_desc_default(qrgpu_fsm_desc *d)
{   // qr_robot_a1_sim.cpp:114-126, config/a1_sim; qr_fsm_state_standup.cpp:62, :66; qr_fsm_state_locomotion.cpp:176, :181; qr_safety_checker.cpp:57-60
    if (!d) return;
    memset(d, 0, sizeof(*d));
    const float body_height = 0.28f, upper_l = 0.2f;
    const float hip = std::acos(body_height / 2.f / upper_l), knee = -2.f * hip;
    for (int l = 0; l < 4; ++l) {
        d->stand_up_angles[3 * l] = 0.f; d->stand_up_angles[3 * l + 1] = hip; d->stand_up_angles[3 * l + 2] = knee;
        d->sit_down_angles[3 * l] = -0.167136f; d->sit_down_angles[3 * l + 1] = 0.934969f; d->sit_down_angles[3 * l + 2] = -2.54468f;
        d->kp[3 * l] = d->kp[3 * l + 1] = d->kp[3 * l + 2] = 100.f;
        d->kd[3 * l] = 1.f; d->kd[3 * l + 1] = d->kd[3 * l + 2] = 2.f;
    }
    d->stand_up_time = 2.f; d->stand_up_total = 3.f; d->sit_down_time = 1.5f; d->time_step = 0.001f;
    d->transition_ticks = 1000; d->gait_transition_duration = 2.f; d->stand_transition_duration = 1.f;
    d->tau_clip = 23.f; d->body_height = body_height; d->initial_ctrl_state = 5;
    d->max_velx = 0.2f; d->max_vely = 0.1f; d->max_yawrate = 0.2f;
}

int qrgpu_fsm_update_batch(qrgpu_ctx *c, int n, const qrgpu_fsm_desc *desc, int reset, const float *d_joy_msg, const float *d_script, int n_script,
                           const int *d_ticks, const int *d_done, unsigned bits, float *d_fsm_state, float *d_joy, int *d_plan, int *d_stage_mask)
{
    static const char *const me = "qrgpu_fsm_update_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return fsm_bad(c, me, "n");
    if (!desc) return fsm_bad(c, me, "desc");
    if (const char *f = fsm_desc_bad(desc)) return fsm_bad(c, me, f);
    if (reset != 0 && reset != 1) return fsm_bad(c, me, "reset");
    if (n_script < 0 || n_script > QRGPU_FSM_SCRIPT_MAX) return fsm_bad(c, me, "n_script");
    if (n_script > 0 && !d_script) return fsm_bad(c, me, "d_script");
    if (d_script && n_script > 0 && !d_ticks) return fsm_bad(c, me, "d_ticks");
    if (d_done && bits == 0u) return fsm_bad(c, me, "bits");
    if (!d_fsm_state) return fsm_bad(c, me, "d_fsm_state");
    if (!d_joy) return fsm_bad(c, me, "d_joy");
    if (!d_plan) return fsm_bad(c, me, "d_plan");
    const bool scripted = d_script && n_script > 0;
    return fsm_launch(c, qr_fsm_update_kernel, n, *desc, reset, d_joy_msg, scripted ? d_script : (const float *)nullptr, scripted ? n_script : 0,
                      scripted ? d_ticks : (const int *)nullptr, d_done, bits, d_fsm_state, d_joy, d_plan, d_stage_mask);
}

int qrgpu_fsm_zero_command_batch(qrgpu_ctx *c, int n, const int *d_plan, float *d_state_des, float *d_fe_in, float *d_fh_in, float *d_swing_vel_in,
                                 float *d_stance_cmd)
{
    static const char *const me = "qrgpu_fsm_zero_command_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return fsm_bad(c, me, "n");
    if (!d_plan) return fsm_bad(c, me, "d_plan");
    return fsm_launch(c, qr_fsm_zero_kernel, n, d_plan, d_state_des, d_fe_in, d_fh_in, d_swing_vel_in, d_stance_cmd);
}

int qrgpu_fsm_command_batch(qrgpu_ctx *c, int n, const qrgpu_fsm_desc *desc, const int *d_plan, const float *d_est_in, const float *d_motor_cmd_loco,
                            float *d_fsm_state, float *d_motor_cmd, float *d_fsm_out)
{
    static const char *const me = "qrgpu_fsm_command_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return fsm_bad(c, me, "n");
    if (!desc) return fsm_bad(c, me, "desc");
    if (const char *f = fsm_desc_bad(desc)) return fsm_bad(c, me, f);
    if (!d_plan) return fsm_bad(c, me, "d_plan");
    if (!d_est_in) return fsm_bad(c, me, "d_est_in");
    if (!d_motor_cmd_loco) return fsm_bad(c, me, "d_motor_cmd_loco");
    if (!d_fsm_state) return fsm_bad(c, me, "d_fsm_state");
    if (!d_motor_cmd) return fsm_bad(c, me, "d_motor_cmd");
    return fsm_launch(c, qr_fsm_command_kernel, n, *desc, d_plan, d_est_in, d_motor_cmd_loco, d_fsm_state, d_motor_cmd, d_fsm_out);
}

}  // extern "C"
