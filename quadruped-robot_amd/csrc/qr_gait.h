// The open-loop gait generator, written once, and the stage clock that restarts where a mask says: what qr_gait_kernel (one gait for the launch),
// qr_gait_select_kernel (the gait chosen per robot) and qr_stage_clock_kernel (qr_gait_kernel.hip) run per lane.  float32 + - x / with contraction off,
// exact fmodf, every operation in the order of tests/gait_ref.py.  Every function is __host__ __device__: the same text compiles for a CPU check against
// tests/gait_ref.py and tests/gait_select_ref.py (tests/stubs/gait_select_host.hip).  include/qrgpu.h states the rules.
//   qrOpenLoopGaitGenerator::Reset                  quadruped/src/gait/qr_openloop_gait_generator.cpp:77-123 (re-reads the block of `gait`)
//   qrOpenLoopGaitGenerator::Update, Schedule       :126-207, :210-249 (legs with a non-zero duty factor)
//   qrGaitGenerator::Reset, the members' initialisers   quadruped/include/quadruped/gait/qr_gait.h:76-87, :263-294
//   qrLocomotionController::Reset                   quadruped/src/controllers/qr_locomotion_controller.cpp:56-66 (resetTime = GetTimeSinceReset())
// Row k of an array lies at p[k * S]: the kernel passes the robot's column and S = n, a packed record has S = 1.
//
// d_gait_state rows: 0 resetTime, 1 lastTime, 2 cumDt, 3 gaitCycle, then per leg 4 cur, 8 last, 12 desired, 16 legState, 20 allow, 24 firstSwing,
// 28 firstStance, 32 phaseInFullCycle, 36 normalizedPhase, 40 contactStartPhase, 44 swingTimeRemaining; 48 the index of the gait in force (written by
// select_update alone); 49-51 spare.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include "../../include/qrgpu.h"

#ifndef QR_HD
#define QR_HD __host__ __device__ __forceinline__
#endif

namespace qrgpu {
namespace gait {

enum { SWING = 0, STANCE = 1, EARLY_CONTACT = 2 };
enum { S_RESET_TIME = 0, S_LAST_TIME, S_CUM_DT, S_GAIT_CYCLE, S_CUR = 4, S_LAST = 8, S_DESIRED = 12, S_LEG = 16, S_ALLOW = 20, S_FIRST_SWING = 24,
       S_FIRST_STANCE = 28, S_PHASE = 32, S_NPHASE = 36, S_CONTACT_START = 40, S_SWING_REMAINING = 44, S_INDEX = 48 };
static_assert(S_INDEX < QRGPU_GAIT_STATE_FLOATS, "d_gait_state rows");

// Rows 0-47 of a column in registers.
struct Generator {
    float reset_time, last_time, cum_dt, gait_cycle;
    int cur[4], last[4], desired[4], leg[4], allow[4], fsw[4], fst[4];
    float phase[4], nphase[4], csp[4], srem[4];
};

// The integer a float32 holds if it is one of 0 .. n - 1, else -1 (NaN, a fraction, a negative, n or more).
QR_HD int index_of(float v, int n)
{
    if (!(v >= 0.f) || !(v < (float)n)) return -1;
    const int k = (int)v;
    return (float)k == v ? k : -1;
}

QR_HD void load(size_t S, const float *st, Generator &g)
{
    g.reset_time = st[S_RESET_TIME * S]; g.last_time = st[S_LAST_TIME * S]; g.cum_dt = st[S_CUM_DT * S]; g.gait_cycle = st[S_GAIT_CYCLE * S];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        g.cur[l] = (int)st[(S_CUR + l) * S]; g.last[l] = (int)st[(S_LAST + l) * S]; g.desired[l] = (int)st[(S_DESIRED + l) * S];
        g.leg[l] = (int)st[(S_LEG + l) * S]; g.allow[l] = (int)st[(S_ALLOW + l) * S]; g.fsw[l] = (int)st[(S_FIRST_SWING + l) * S];
        g.fst[l] = (int)st[(S_FIRST_STANCE + l) * S]; g.phase[l] = st[(S_PHASE + l) * S]; g.nphase[l] = st[(S_NPHASE + l) * S];
        g.csp[l] = st[(S_CONTACT_START + l) * S]; g.srem[l] = st[(S_SWING_REMAINING + l) * S];
    }
}

// Reset(0) with the block of D: QRGPU_GAIT_RESET_LIVE on the running generator (the members qrGaitGenerator::Reset does not write survive),
// any other non-zero level on a generator as constructed (the members' initialisers first).
QR_HD void reset(const qrgpu_gait_desc &D, int level, Generator &g)
{
    g.reset_time = g.last_time = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) { g.cur[l] = g.last[l] = g.desired[l] = g.leg[l] = D.initial_leg_state[l]; g.nphase[l] = g.csp[l] = 0.f; }
    if (level != QRGPU_GAIT_RESET_LIVE) {
        g.cum_dt = g.gait_cycle = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l) { g.allow[l] = 1; g.fsw[l] = g.fst[l] = 0; g.phase[l] = g.srem[l] = 0.f; }
    }
}

// Update + Schedule of one control tick on the parameters of D; ct: GetFootContact().  swing_duration is Reset's, of D.  The members are worked on in
// arrays of their own, not in G: with two members of one object stored to on the two sides of a branch, the compiler merges the stores into one at a
// selected address, and the object goes to private memory.
QR_HD void update(const qrgpu_gait_desc &D, float current_time, int stop, const float ct[4], Generator &G, float swing_duration[4])
{
#pragma clang fp contract(off)
    float reset_time = G.reset_time, cum_dt = G.cum_dt, gait_cycle = G.gait_cycle;
    const float last_time = G.last_time;
    int cur[4], last[4], desired[4], leg[4], allow[4], fsw[4], fst[4];
    float phase[4], nphase[4], csp[4], srem[4], full[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        cur[l] = G.cur[l]; last[l] = G.last[l]; desired[l] = G.desired[l]; leg[l] = G.leg[l]; fsw[l] = G.fsw[l]; fst[l] = G.fst[l];
        phase[l] = G.phase[l]; nphase[l] = G.nphase[l]; csp[l] = G.csp[l]; srem[l] = G.srem[l];
        full[l] = D.stance_duration[l] / D.duty_factor[l]; swing_duration[l] = full[l] - D.stance_duration[l];
    }
    float tsr = current_time;
    if (reset_time + full[0] < tsr) { reset_time = tsr; gait_cycle += 1.f; }
    tsr -= reset_time;
#pragma unroll
    for (int l = 0; l < 4; ++l) allow[l] = 1;
    if (D.advanced_trot) {
#pragma unroll
        for (int l = 0; l < 4; ++l) if (cur[l] == SWING && desired[l] == STANCE && ct[l] == 0.f) allow[l] = 0;
        if (allow[0] + allow[1] + allow[2] + allow[3] < 4) {
            const float dt_ = current_time - last_time;
            cum_dt += dt_;
            if (cum_dt > D.wait_time) {
#pragma unroll
                for (int l = 0; l < 4; ++l) allow[l] = 1;
            } else reset_time += dt_;
        } else cum_dt = 0.f;
    }
    const bool all_allowed = allow[0] + allow[1] + allow[2] + allow[3] == 4;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (!all_allowed) continue;
        if (!stop || (stop && last[l] == SWING)) { last[l] = cur[l]; cur[l] = desired[l]; }
        const float augmented = D.initial_leg_phase[l] * full[l] + tsr;
        phase[l] = fmodf(augmented, full[l]) / full[l];
        const float ratio = D.duty_factor[l];
        if (phase[l] < ratio) { desired[l] = STANCE; nphase[l] = phase[l] / ratio; }
        else {
            desired[l] = SWING;
            nphase[l] = (phase[l] - ratio) / (1 - ratio);
            if (cur[l] == STANCE) { fsw[l] = 1; csp[l] = 0.f; fst[l] = 0; srem[l] = swing_duration[l]; }
            else { fsw[l] = 0; srem[l] = swing_duration[l] * (1 - nphase[l]); }
        }
        if (leg[l] == EARLY_CONTACT && desired[l] == SWING) continue;
        leg[l] = desired[l];
        if (nphase[l] < D.contact_detection_phase_threshold) continue;
        if (leg[l] == SWING && ct[l] != 0.f) { leg[l] = EARLY_CONTACT; csp[l] = phase[l] - 1.0f; }
        if (cur[l] == SWING && (leg[l] == EARLY_CONTACT || leg[l] == STANCE)) { fst[l] = 1; fsw[l] = 0; }
    }
    G.reset_time = reset_time; G.cum_dt = cum_dt; G.gait_cycle = gait_cycle;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        G.cur[l] = cur[l]; G.last[l] = last[l]; G.desired[l] = desired[l]; G.leg[l] = leg[l]; G.allow[l] = allow[l]; G.fsw[l] = fsw[l]; G.fst[l] = fst[l];
        G.phase[l] = phase[l]; G.nphase[l] = nphase[l]; G.csp[l] = csp[l]; G.srem[l] = srem[l];
    }
}

// One robot's tick on the parameters of D and a loaded generator: Reset where the level says, Update, then everything the tick writes.  Row 1
// (lastTime) receives the call's time.  st, out, fe, sw: the robot's columns (out, fe and sw may be null).  A leg's state rows are stored beside its
// out / fe / sw rows, in one loop: a store pass over the whole generator in front of the output pass keeps every member live across both (183
// against 139 VGPRs in qr_gait_select_kernel).
QR_HD void tick(const qrgpu_gait_desc &D, int level, float current_time, int stop, size_t S, const float ct[4], Generator &g, float *st, float *out,
                float *fe, float *sw)
{
    if (level) reset(D, level, g);
    float swing_duration[4];
    update(D, current_time, stop, ct, g, swing_duration);
    st[S_RESET_TIME * S] = g.reset_time; st[S_LAST_TIME * S] = current_time; st[S_CUM_DT * S] = g.cum_dt; st[S_GAIT_CYCLE * S] = g.gait_cycle;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        st[(S_CUR + l) * S] = (float)g.cur[l]; st[(S_LAST + l) * S] = (float)g.last[l]; st[(S_DESIRED + l) * S] = (float)g.desired[l];
        st[(S_LEG + l) * S] = (float)g.leg[l]; st[(S_ALLOW + l) * S] = (float)g.allow[l]; st[(S_FIRST_SWING + l) * S] = (float)g.fsw[l];
        st[(S_FIRST_STANCE + l) * S] = (float)g.fst[l]; st[(S_PHASE + l) * S] = g.phase[l]; st[(S_NPHASE + l) * S] = g.nphase[l];
        st[(S_CONTACT_START + l) * S] = g.csp[l]; st[(S_SWING_REMAINING + l) * S] = g.srem[l];
        if (out) {
            out[(size_t)l * S] = g.phase[l]; out[(size_t)(4 + l) * S] = g.nphase[l]; out[(size_t)(8 + l) * S] = (float)g.desired[l];
            out[(size_t)(12 + l) * S] = (float)g.leg[l]; out[(size_t)(16 + l) * S] = (float)g.cur[l]; out[(size_t)(20 + l) * S] = g.srem[l];
        }
        if (fe) {            // rows 42-61 of the MPC front-end's input
            fe[(size_t)(42 + l) * S] = g.phase[l]; fe[(size_t)(46 + l) * S] = D.duty_factor[l]; fe[(size_t)(50 + l) * S] = g.nphase[l];
            fe[(size_t)(54 + l) * S] = (float)g.desired[l]; fe[(size_t)(58 + l) * S] = (float)g.leg[l];
        }
        if (sw) sw[(size_t)(8 + l) * S] = swing_duration[l];      // swingDuration of the gait in force
    }
}

// One robot's tick of qrgpu_gait_update_batch: one gait for the whole call.  level: the robot's reset level at this call; contact, st, out, fe: the
// robot's columns (out and fe may be null).  Rows 48-51 of the state are neither read nor written, and swing_in is the caller's.  The state column and
// the contacts are loaded before anything depends on the level; a reset then overrides what its level does not keep.
QR_HD void fixed_update(const qrgpu_gait_desc &D, int level, float current_time, int stop, size_t S, const float *contact, float *st, float *out, float *fe)
{
    Generator g;
    load(S, st, g);
    float ct[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) ct[l] = contact[(size_t)l * S];
    tick(D, level, current_time, stop, S, ct, g, st, out, fe, nullptr);
}

// One robot's tick of qrgpu_gait_select_update_batch.  table [n_gaits] in memory the caller can read with an index of its own; sel: the robot's word of
// d_gait_sel; level: the robot's reset level at this call (0, QRGPU_GAIT_RESET_CONSTRUCT, QRGPU_GAIT_RESET_LIVE); st, out, fe, sw: the robot's columns
// (out, fe, sw and flag may be null).  The state column, the selection and the contacts are loaded before anything depends on the level.
QR_HD void select_update(const qrgpu_gait_desc *table, int n_gaits, float sel, int level, float current_time, int stop, size_t S, const float *contact,
                         float *st, float *out, float *fe, float *sw, int *flag)
{
    Generator g;
    load(S, st, g);
    const int kept = index_of(st[S_INDEX * S], n_gaits), chosen = index_of(sel, n_gaits);
    float ct[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) ct[l] = contact[(size_t)l * S];
    int idx = kept < 0 ? 0 : kept, bad = 0;
    if (level) { idx = chosen < 0 ? 0 : chosen; bad = chosen < 0 ? QRGPU_GAIT_BAD_SEL : 0; }      // the selection counts at a reset and nowhere else
    const qrgpu_gait_desc D = table[idx];
    tick(D, level, current_time, stop, S, ct, g, st, out, fe, sw);
    st[S_INDEX * S] = (float)idx;
    if (flag) *flag = bad;
}

// One robot's word of qrgpu_stage_clock_batch: the origin moves to now where the mask says, the local clock counts from it.
QR_HD void stage_clock(int mask, unsigned bits, int ticks, int *origin, int *local)
{
    const int kept = *origin;
    const int o = ((unsigned)mask & bits) != 0u ? ticks : kept;
    *origin = o;
    *local = ticks - o;
}

}  // namespace gait
}  // namespace qrgpu
