// ============================================================================
// qr_mode_route_kernel, qr_mode_masks_kernel, qr_mode_command_kernel: the locomotion mode per robot -- which chain a robot is on, the masks of the
// cadenced tick under that choice, and the motor command of the robot's own chain (qrgpu_mode_route_batch, qrgpu_tick_cadence_batch under
// qrgpu_set_mode_route, qrgpu_mode_command_batch, include/qrgpu.h); the arithmetic is qr_mode_route.h's.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is
// one coalesced row segment.  The route counts the robots per chain with one ballot and one popcount per chain and wavefront, and lane 0 adds the
// three integers to the call's counters with one atomicAdd each: integer sums, the same in any order.  A lane past n takes part in the ballots with a
// chain nobody counts and does nothing else.  g_out of the command kernel may be either input (no __restrict__ on the three): a lane has both
// columns in registers before its first store.  No LDS, no barrier.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_mode_route.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_mode_route_kernel(int n, qrgpu_mode_route_desc D, const float *__restrict__ g_sel, const int *__restrict__ g_plan,
                                                           int *__restrict__ g_chain, int *__restrict__ g_flags, int *__restrict__ g_count)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    int chain = -1;
    if (i < n) {
        int flags;
        chain = mode_route::route(D, g_sel[i], g_plan != nullptr, g_plan ? g_plan[i] : 0, flags);
        g_chain[i] = chain;
        if (g_flags) g_flags[i] = flags;
    }
    if (!g_count) return;                                       // (uniform: every lane of the wavefront is still here for the ballots)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cnt = __popcll(__ballot(chain == c));
        if (threadIdx.x == 0 && cnt) atomicAdd(g_count + c, cnt);
    }
}

__global__ void __launch_bounds__(64) qr_mode_masks_kernel(int n, const int *__restrict__ g_updated, const int *__restrict__ g_chain, int *__restrict__ g_due,
                                                           int *__restrict__ g_skip)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    int due, skip;
    mode_route::masks(g_updated[i], g_chain[i], due, skip);
    g_due[i] = due;
    g_skip[i] = skip;
}

__global__ void __launch_bounds__(64) qr_mode_command_kernel(int n, const int *__restrict__ g_chain, const float *g_cmd_mpc, const float *g_cmd_fb,
                                                             const int *g_st_mpc, const int *g_st_fb, float *g_out, int *g_st_out)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    mode_route::command((size_t)n, g_chain[i], g_cmd_mpc + i, g_cmd_fb + i, g_st_mpc ? g_st_mpc + i : nullptr, g_st_fb ? g_st_fb + i : nullptr, g_out + i,
                        g_st_out ? g_st_out + i : nullptr);
}

}  // namespace qrgpu
