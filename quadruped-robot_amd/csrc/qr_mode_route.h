// The mode per robot: which locomotion chain a robot is on this tick, the two masks the cadenced tick's launches take for it, and whose motor command
// it gets -- what qr_mode_route_kernel, qr_mode_masks_kernel and qr_mode_command_kernel (qr_mode_route_kernel.hip) run per lane.  Integer compares and
// copies; the one float is the selection, which is tested and never computed with.  Every function is __host__ __device__: the same text compiles for a
// CPU check against tests/mode_route_ref.py (tests/stubs/mode_route_host.hip).  include/qrgpu.h states the rules.
//   qrFSMStateLocomotion::OnEnter   quadruped/src/fsm/qr_fsm_state_locomotion.cpp:78-158 (JOY_TROT: VELOCITY_LOCOMOTION, JOY_ADVANCED_TROT: the MPC, the
//                                   WBC and the hip compensation, JOY_WALK: WALK_LOCOMOTION)
//   qrFSMStateLocomotion::Run       :162-171 (locomotionController->Update() and GetAction() on the ticks the state runs, and on no other)
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/qrgpu.h"

#ifndef QR_HD
#define QR_HD __host__ __device__ __forceinline__
#endif

namespace qrgpu {
namespace mode_route {

// The selection as an integer in -1..3, or -2: NaN, no integer, outside the range (the cast is made only once the range is known)
QR_HD int mode_of(float sel)
{
    if (!(sel >= -1.f && sel <= 3.f)) return -2;
    const int m = (int)sel;
    return (float)m == sel ? m : -2;
}

// Robot r's chain and flag word.  plan: the robot's QRGPU_FSM_PLAN_* word where has_plan.
QR_HD int route(const qrgpu_mode_route_desc &D, float sel, bool has_plan, int plan, int &flags)
{
    flags = 0;
    if (has_plan && (plan & (QRGPU_FSM_PLAN_RUN | QRGPU_FSM_PLAN_PHASE1)) == 0) return QRGPU_CHAIN_NONE;      // no locomotion controller runs on such a tick
    const int m = mode_of(sel);
    if (m == -1) return QRGPU_CHAIN_NONE;                                                                      // OnEnter has not run yet
    if (m < 0) { flags = QRGPU_ROUTE_BAD_MODE; return D.fallback_chain; }
    // (a select over the four entries, not an indexed read of the by-value struct: no scratch copy of it)
    const int c = m == 0 ? D.chain_of_mode[0] : m == 1 ? D.chain_of_mode[1] : m == 2 ? D.chain_of_mode[2] : D.chain_of_mode[3];
    if (c == QRGPU_CHAIN_NONE) { flags = QRGPU_ROUTE_NO_CHAIN; return D.fallback_chain; }
    return c;
}

// The cadenced tick under the binding: due' = updated && on the MPC chain goes to the MPC launch, skip' = updated || !on the MPC chain to the WBC launch.
QR_HD void masks(int updated, int chain, int &due, int &skip)
{
    const bool on = chain == QRGPU_CHAIN_MPC, up = updated != 0;
    due = (up && on) ? 1 : 0;
    skip = (up || !on) ? 1 : 0;
}

// The merge: robot r's column and status word are its chain's; no chain, zeros.  Both columns are in registers before the first store (out may be either
// input), and the result is selected per word, never blended: what the other chain left -- a NaN included -- does not reach it.
QR_HD void command(size_t S, int chain, const float *cmd_mpc, const float *cmd_fb, const int *st_mpc, const int *st_fb, float *out, int *st_out)
{
    float a[QRGPU_MOTOR_CMD_ROWS], b[QRGPU_MOTOR_CMD_ROWS];
#pragma unroll
    for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) { a[k] = cmd_mpc[(size_t)k * S]; b[k] = cmd_fb[(size_t)k * S]; }
    const int sa = st_mpc ? *st_mpc : 0, sb = st_fb ? *st_fb : 0;
#pragma unroll
    for (int k = 0; k < QRGPU_MOTOR_CMD_ROWS; ++k) out[(size_t)k * S] = chain == QRGPU_CHAIN_MPC ? a[k] : chain == QRGPU_CHAIN_FORCE_BALANCE ? b[k] : 0.f;
    if (st_out) *st_out = chain == QRGPU_CHAIN_MPC ? sa : chain == QRGPU_CHAIN_FORCE_BALANCE ? sb : 0;
}

}  // namespace mode_route
}  // namespace qrgpu
