// ============================================================================
// libqrgpu.so host side: the trot's command, data-flow and motor-command stages (qr_dataflow_kernel.hip) and the defaults of their parameter blocks.
// Every entry point is "check the arguments, one launch on the context's stream" (qrgpu_stages.hip).
// ============================================================================
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>

#include "qrgpu_ctx.h"

static int dataflow_bad(qrgpu_ctx *c, const char *call, const char *what)
{
    if (c) c->err = std::string(call) + ": " + what;
    return QRGPU_ERR_BAD_ARG;
}

template <typename... KArgs, typename... Args>
static int dataflow_launch(qrgpu_ctx *c, void (*kernel)(KArgs...), int n, Args... args)
{
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, args...);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

extern "C" {

void qrgpu_command_desc_default(qrgpu_command_desc *d)
{   // qr_desired_state_command.hpp:155, :266, :302-337; robot_params.body_height of config/a1_sim
    if (!d) return;
    memset(d, 0, sizeof(*d));
    d->dt = 0.002f; d->filter_factor = 0.02f; d->body_height = 0.28f;
    d->min_velx = -0.15f; d->max_velx = 0.2f; d->min_vely = -0.1f; d->max_vely = 0.1f;
    d->min_yawrate = -0.2f; d->max_yawrate = 0.2f; d->min_pitch = -0.5f; d->max_pitch = 0.5f;
}

int qrgpu_command_update_batch(qrgpu_ctx *c, int n, const qrgpu_command_desc *desc, int reset, const float *d_joy, float *d_cmd_state, float *d_state_des,
                               float *d_fe_in, float *d_fh_in, float *d_swing_vel_in, float *d_stance_cmd)
{
    static const char *const me = "qrgpu_command_update_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return dataflow_bad(c, me, "n");
    if (!desc) return dataflow_bad(c, me, "desc");
    if (reset != 0 && reset != 1) return dataflow_bad(c, me, "reset");
    if (!d_joy) return dataflow_bad(c, me, "d_joy");
    if (!d_cmd_state) return dataflow_bad(c, me, "d_cmd_state");
    return dataflow_launch(c, qr_command_kernel, n, *desc, reset, stage_mask_args(c), d_joy, d_cmd_state, d_state_des, d_fe_in, d_fh_in, d_swing_vel_in,
                           d_stance_cmd);
}

int qrgpu_trot_inputs_batch(qrgpu_ctx *c, int n, const float *d_est_in, const float *d_est_out, const float *d_rpy, const float *d_gait_out,
                            const float *d_gait_state, float *d_fe_in, float *d_fh_in, float *d_swing_in, float *d_est_in_next)
{
    static const char *const me = "qrgpu_trot_inputs_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return dataflow_bad(c, me, "n");
    if (!d_est_in) return dataflow_bad(c, me, "d_est_in");
    if (!d_est_out) return dataflow_bad(c, me, "d_est_out");
    if (!d_rpy) return dataflow_bad(c, me, "d_rpy");
    if (!d_gait_out) return dataflow_bad(c, me, "d_gait_out");
    if (d_fe_in && !d_gait_state) return dataflow_bad(c, me, "d_gait_state");                       // allowSwitchLegState, for the contacts
    return dataflow_launch(c, qr_trot_inputs_kernel, n, d_est_in, d_est_out, d_rpy, d_gait_out, d_gait_state, d_fe_in, d_fh_in, d_swing_in, d_est_in_next);
}

void qrgpu_mpc_command_desc_default(qrgpu_mpc_command_desc *d)
{   // motor gains as qrgpu_stance_desc_default (config/a1_sim); qr_mpc_stance_leg_controller.cpp:145, :149
    if (!d) return;
    memset(d, 0, sizeof(*d));
    for (int l = 0; l < 4; ++l) {
        d->kp[3 * l] = d->kp[3 * l + 1] = d->kp[3 * l + 2] = 100.f;
        d->kd[3 * l] = 1.f; d->kd[3 * l + 1] = d->kd[3 * l + 2] = 2.f;
    }
    d->stance_kd = 3.0f; d->early_contact_abad_kp = 100.0f; d->epilogue = 0;
}

int qrgpu_mpc_command_batch(qrgpu_ctx *c, int n, const qrgpu_mpc_command_desc *desc, int reset, const float *d_tau, const float *d_qdes,
                            const float *d_swing_in, const float *d_gait_out, const float *d_gait_state, int *d_cmd_mem, float *d_motor_cmd)
{
    static const char *const me = "qrgpu_mpc_command_batch";
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return dataflow_bad(c, me, "n");
    if (!desc) return dataflow_bad(c, me, "desc");
    if (reset != 0 && reset != 1) return dataflow_bad(c, me, "reset");
    if (!d_tau) return dataflow_bad(c, me, "d_tau");
    if (!d_qdes) return dataflow_bad(c, me, "d_qdes");
    if (!d_swing_in) return dataflow_bad(c, me, "d_swing_in");
    if (!d_gait_out) return dataflow_bad(c, me, "d_gait_out");
    if (!d_gait_state) return dataflow_bad(c, me, "d_gait_state");
    if (!d_cmd_mem) return dataflow_bad(c, me, "d_cmd_mem");
    if (!d_motor_cmd) return dataflow_bad(c, me, "d_motor_cmd");
    return dataflow_launch(c, qr_mpc_command_kernel, n, *desc, reset, stage_mask_args(c), d_tau, d_qdes, d_swing_in, d_gait_out, d_gait_state, d_cmd_mem,
                           d_motor_cmd);
}

}  // extern "C"
