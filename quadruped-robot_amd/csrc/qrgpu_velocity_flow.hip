// ============================================================================
// libqrgpu.so host side: the data-flow stage of the force-balance trot (qr_velocity_flow_kernel.hip).  "Check the arguments, one launch on the
// context's stream" (qrgpu_dataflow.hip).
// ============================================================================
#include <hip/hip_runtime.h>
#include <string>

#include "qrgpu_ctx.h"

static int velocity_flow_bad(qrgpu_ctx *c, const char *what)
{
    if (c) c->err = std::string("qrgpu_velocity_inputs_batch: ") + what;
    return QRGPU_ERR_BAD_ARG;
}

extern "C" {

int qrgpu_velocity_inputs_batch(qrgpu_ctx *c, int n, int terrain, int reset, const float *d_est_in, const float *d_est_out, const float *d_ground_out,
                                const float *d_gait_out, const float *d_gait_state, const float *d_state_des, float *d_swing_vel_in, float *d_est_in_next,
                                int *d_cmd_mem, float *d_swing_flag)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (!batch_ok(c, n)) return velocity_flow_bad(c, "n");
    if (terrain < 0 || terrain > 4) return velocity_flow_bad(c, "terrain");
    if (reset != 0 && reset != 1) return velocity_flow_bad(c, "reset");
    if (!d_est_in) return velocity_flow_bad(c, "d_est_in");
    if (!d_est_out) return velocity_flow_bad(c, "d_est_out");
    if (terrain >= 2 && !d_ground_out) return velocity_flow_bad(c, "d_ground_out");                // baseRInControlFrame, off the horizontal terrains
    if (!d_gait_out) return velocity_flow_bad(c, "d_gait_out");
    if (!d_gait_state) return velocity_flow_bad(c, "d_gait_state");
    if (!d_state_des) return velocity_flow_bad(c, "d_state_des");
    if (d_swing_flag && !d_cmd_mem) return velocity_flow_bad(c, "d_cmd_mem");                      // the flag is "has an entry and ..."
    c->ov_chain = false;                                             // another launch of the context: the next overlapped tick is not chained
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(qr_velocity_flow_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, terrain, reset, stage_mask_args(c), d_est_in, d_est_out, d_ground_out,
                       d_gait_out, d_gait_state, d_state_des, d_swing_vel_in, d_est_in_next, d_cmd_mem, d_swing_flag);
    HIPCHK(c, hipGetLastError());
    return QRGPU_OK;
}

}  // extern "C"
