// ============================================================================
// qr_fsm_update_kernel, qr_fsm_zero_kernel, qr_fsm_command_kernel: the control state machine per robot -- joystick, stand-up, transitions
// (qrgpu_fsm_update_batch, qrgpu_fsm_zero_command_batch, qrgpu_fsm_command_batch, include/qrgpu.h); the arithmetic is qr_fsm.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  The script of the update is read at addresses that do not depend on the lane.  g_loco of the command kernel may be
// g_cmd (no __restrict__ on the pair): a lane has its column in registers before its first store.  No LDS, no barrier, no cross-lane traffic.
// A lane past n does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_fsm.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_fsm_update_kernel(int n, qrgpu_fsm_desc D, int reset, const float *__restrict__ g_msg, const float *__restrict__ g_script,
                                                           int n_script, const int *__restrict__ g_ticks, const int *__restrict__ g_done, unsigned bits,
                                                           float *__restrict__ g_st, float *__restrict__ g_joy, int *__restrict__ g_plan,
                                                           int *__restrict__ g_stage_mask)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    fsm::update(D, reset, (size_t)n, g_msg ? g_msg + i : nullptr, g_script, n_script, g_ticks ? g_ticks + i : nullptr, g_done ? g_done + i : nullptr, bits,
                g_st + i, g_joy + i, g_plan + i, g_stage_mask ? g_stage_mask + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_fsm_zero_kernel(int n, const int *__restrict__ g_plan, float *__restrict__ g_des, float *__restrict__ g_fe,
                                                         float *__restrict__ g_fh, float *__restrict__ g_sv, float *__restrict__ g_sc)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    fsm::zero_command((size_t)n, g_plan[i], g_des ? g_des + i : nullptr, g_fe ? g_fe + i : nullptr, g_fh ? g_fh + i : nullptr, g_sv ? g_sv + i : nullptr,
                      g_sc ? g_sc + i : nullptr);
}

__global__ void __launch_bounds__(64) qr_fsm_command_kernel(int n, qrgpu_fsm_desc D, const int *__restrict__ g_plan, const float *__restrict__ g_est_in,
                                                            const float *g_loco, float *__restrict__ g_st, float *g_cmd, float *__restrict__ g_out)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    fsm::command(D, (size_t)n, g_plan[i], g_est_in + i, g_loco + i, g_st + i, g_cmd + i, g_out ? g_out + i : nullptr);
}

}  // namespace qrgpu
