// ============================================================================
// qr_command_kernel, qr_trot_inputs_kernel, qr_mpc_command_kernel: the operator's command (qrDesiredStateCommand::Update), the getters between the
// trot's stages and the motor command of the MPC mode (qrgpu_command_update_batch, qrgpu_trot_inputs_batch, qrgpu_mpc_command_batch,
// include/qrgpu.h); the arithmetic is qr_dataflow.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  A lane issues all its loads, then computes, then stores: one memory latency per kernel.  The two kernels with memory
// take the stage-reset binding as an argument always (a null mask: unbound) and read only its mask; the mask word's load is the first of the lane's
// loads, not a gate in front of them (qr_observe_kernel.hip).  g_est_w of the trot inputs may be g_est_in (no __restrict__ on the pair): the rows
// written are not among the rows read, and every row read is in registers before the first store.  No LDS, no barrier, no cross-lane traffic.
// A lane past n does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_dataflow.h"

namespace qrgpu {

// the robot's reset: the call's scalar, or its mask word under a binding; unbound, the lane reads a word of `own` (a column it loads anyway) instead
__device__ __forceinline__ bool dataflow_reset(const StageResetArgs &SR, int reset, const void *own, int i)
{
    const unsigned *mp = SR.mask ? (const unsigned *)SR.mask + i : (const unsigned *)own + i;
    const unsigned bits = SR.mask ? SR.bits : 0u;
    return (reset != 0) | ((*mp & bits) != 0u);
}

__global__ void __launch_bounds__(64) qr_command_kernel(int n, qrgpu_command_desc D, int reset, StageResetArgs SR, const float *__restrict__ g_joy,
                                                        float *__restrict__ g_st, float *__restrict__ g_des, float *__restrict__ g_fe, float *__restrict__ g_fh,
                                                        float *__restrict__ g_sv, float *__restrict__ g_sc)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    const bool rst = dataflow_reset(SR, reset, g_joy, i);
    dataflow::command_update(D, rst, (size_t)n, g_joy + i, g_st + i, g_des ? g_des + i : nullptr, g_fe ? g_fe + i : nullptr, g_fh ? g_fh + i : nullptr,
                             g_sv ? g_sv + i : nullptr, g_sc ? g_sc + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_trot_inputs_kernel(int n, const float *g_est_in, const float *__restrict__ g_est_out, const float *__restrict__ g_rpy,
                                                            const float *__restrict__ g_gait_out, const float *__restrict__ g_gait_state, float *__restrict__ g_fe,
                                                            float *__restrict__ g_fh, float *__restrict__ g_sw, float *g_est_w)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    dataflow::trot_inputs((size_t)n, g_est_in + i, g_est_out + i, g_rpy + i, g_gait_out + i, g_gait_state ? g_gait_state + i : nullptr, g_fe ? g_fe + i : nullptr,
                          g_fh ? g_fh + i : nullptr, g_sw ? g_sw + i : nullptr, g_est_w ? g_est_w + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_mpc_command_kernel(int n, qrgpu_mpc_command_desc D, int reset, StageResetArgs SR, const float *__restrict__ g_tau,
                                                            const float *__restrict__ g_qdes, const float *__restrict__ g_sw, const float *__restrict__ g_gait_out,
                                                            const float *__restrict__ g_gait_state, int *__restrict__ g_mem, float *__restrict__ g_cmd)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    const bool rst = dataflow_reset(SR, reset, g_tau, i);
    dataflow::mpc_command(D, rst, (size_t)n, g_tau + i, g_qdes + i, g_sw + i, g_gait_out + i, g_gait_state + i, g_mem + i, g_cmd + i);
}

}  // namespace qrgpu
