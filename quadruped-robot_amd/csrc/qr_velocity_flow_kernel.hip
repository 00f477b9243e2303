// ============================================================================
// qr_velocity_flow_kernel: the getters between the stages of the force-balance trot and the memory of its swing command
// (qrgpu_velocity_inputs_batch, include/qrgpu.h); what a lane does is qr_velocity_flow.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  A lane issues all its loads, then stores: one memory latency per kernel.  The stage-reset binding is an argument
// always (a null mask: unbound) and only its mask is read; the mask word's load is the first of the lane's loads, not a gate in front of them
// (qr_dataflow_kernel.hip).  g_est_w may be g_est_in (no __restrict__ on the pair): the rows written are not among the rows read, and every row
// read is in registers before the first store.  No LDS, no scratch, no barrier, no cross-lane traffic.  A lane past n does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_velocity_flow.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_velocity_flow_kernel(int n, int terrain, int reset, StageResetArgs SR, const float *g_est_in, const float *__restrict__ g_est_out,
                                                              const float *__restrict__ g_ground, const float *__restrict__ g_gait_out,
                                                              const float *__restrict__ g_gait_state, const float *__restrict__ g_des, float *__restrict__ g_sv,
                                                              float *g_est_w, int *__restrict__ g_mem, float *__restrict__ g_flag)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    // the robot's reset: the call's scalar, or its mask word under a binding; unbound, the lane reads a word of a column it loads anyway
    const unsigned *mp = SR.mask ? (const unsigned *)SR.mask + i : (const unsigned *)g_gait_out + i;
    const unsigned bits = SR.mask ? SR.bits : 0u;
    const bool rst = (reset != 0) | ((*mp & bits) != 0u);
    velocity_flow::velocity_inputs(terrain, rst, (size_t)n, g_est_in + i, g_est_out + i, g_ground ? g_ground + i : nullptr, g_gait_out + i, g_gait_state + i,
                                   g_des + i, g_sv ? g_sv + i : nullptr, g_est_w ? g_est_w + i : nullptr, g_mem ? g_mem + i : nullptr,
                                   g_flag ? g_flag + i : nullptr);
}

}  // namespace qrgpu
