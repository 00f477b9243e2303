// ============================================================================
// qr_cadence_kernel: what the cadenced tick (qrgpu_tick_cadence_batch, include/qrgpu.h) does between its MPC launch and its WBC launch; the arithmetic
// is qr_cadence.h's.  A robot whose word of g_due is non-zero has just been solved: its base-frame force -R^T f is kept in g_hold.  Every other robot
// was left alone by the MPC launch: its twelve torques are the kept force through the Jacobian of its joint angles of now, and its status word starts
// at zero (no MPC flags, iteration count 0) for the WBC launch to OR its bits into.
//
// One lane per robot, 64 lanes (one wavefront) per workgroup.  Every array is [row][n], robot index fastest: each load and store of a wavefront is one
// coalesced row segment.  The two kinds of robot touch disjoint columns.  No LDS, no barrier, no atomics, no cross-lane traffic.  A lane past n
// does nothing.
// ============================================================================
#include <hip/hip_runtime.h>
#include "qr_device_types.h"
#include "qr_kernels.h"
#include "qr_cadence.h"

namespace qrgpu {

__global__ void __launch_bounds__(64) qr_cadence_kernel(int n, CadenceLegs L, const int *__restrict__ g_type, const int *__restrict__ g_due,
                                                        const float *__restrict__ g_mpc_state, const float *__restrict__ g_fb_state,
                                                        const float *__restrict__ g_force, float *__restrict__ g_hold, float *__restrict__ g_tau,
                                                        int *__restrict__ g_status, const int *__restrict__ g_skip)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= n) return;
    if (g_due[i] != 0) {
        cadence::hold_from_force((size_t)n, g_mpc_state + (size_t)6 * n + i, g_force + i, g_hold + i);
        return;
    }
    // (mode route bound: not due and skipped by the WBC launch is a robot on another chain, or on none -- nothing of it is read or written)
    if (g_skip && g_skip[i] != 0) return;
    // (a type that was never set up: the first valid one, as the MPC and WBC kernels take it; the WBC launch flags the robot)
    int tyid = g_type ? g_type[i] : 0;
    (void)resolve_type(tyid, L.type_ready);
    const int t = tyid & (QRGPU_MAX_TYPES - 1);
    cadence::held_torque(L.hip_l[t], L.upper_l[t], L.lower_l[t], (size_t)n, g_fb_state + (size_t)13 * n + i, g_hold + i, g_tau + i);
    if (g_status) g_status[i] = 0;
}

}  // namespace qrgpu
