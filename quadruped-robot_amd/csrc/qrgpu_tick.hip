// ============================================================================
// libqrgpu.so host side: the fused tick (MPC launches + WBC launch) in its three forms -- serial, pipelined, overlapped --
// and the switch, fence and counters of the overlapped form; the cadenced tick (per robot the MPC or the WBC, always serial).  The MPC launches
// themselves: qrgpu_mpc.hip.
// ============================================================================
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>

#include "qrgpu_ctx.h"

// The arrays of one qrgpu_tick_batch call.
struct TickArgs {
    int n;
    const int *type_id;
    const float *mpc_state, *traj, *gait, *fb_state, *wbc_cmd;
    float *prev_ori, *force, *tau, *qdes;
    int *status;
};

// May this tick run its WBC launch beside its MPC launches?
static bool tick_is_piped(qrgpu_ctx *c, int n)
{
    if (!(c->pipeline && qr_env().tick_pipeline != 0 && n >= 64 && !c->d_dbg_cycles && !c->d_dbg_cycles_wbc)) return false;
    // (not while the stream is being captured into a graph: the WBC launch lives on a stream of the context's own)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) { cap = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
    return cap == hipStreamCaptureStatusNone;
}

// The hold of an overlapped context: `hold_calls` calls on the plain pipelined tick from the call that finds `trigger`, then it looks again.
// True: this call is one of them.  The only code that touches ov_hold (besides forget_history).
static bool ov_on_hold(qrgpu_ctx *c, int hold_calls, bool trigger)
{
    if (c->ov_hold > 0) { --c->ov_hold; return true; }
    if (hold_calls > 0 && trigger) { c->ov_hold = hold_calls; return true; }
    return false;
}

// Overlapped tick (qrgpu_set_tick_overlap): the tick's launches go on a lane of their own -- stream sets of the context's, alternating -- and the
// context's stream carries only the join.  Does this (pipelined) tick take that form?
static bool tick_overlaps(qrgpu_ctx *c, int n, bool small_h)
{
    if (!c->overlap || c->flops_on) return false;
    if (!(small_h ? (c->lane[1].d_order && c->lane[2].d_order) : (c->lane[3].d_order && c->lane[4].d_order))) return false;
    const Lane &NL = c->lane[(small_h ? 1 : 3) + c->ov_next];
    // h > 11: only the two-workgroups-per-CU form of the main pass overlaps, on the CU-masked lanes; a shard in which most robots stand (the
    // planned list beyond 45 % of the batch) goes back to the plain tick for QRGPU_H16_TWO_HOLD calls
    if (!small_h) return h16_two_allowed(c, n) && !ov_on_hold(c, qr_env().h16_two_hold, list_exceeds_45_percent(NL, n));
    // A population with a PLAN -- robots that want a whole CU on a list launch beside the main pass -- is not for overlapped ticks: on a machine
    // that is never empty a whole-CU workgroup waits until both halves of some CU happen to be free at once, and the half-CU list kernel that
    // needs no such luck (S^-1 in the global scratch) takes 300 us and more for such a robot, which the pipeline then waits for: 3.0-3.3 against
    // 4.2 M ticks/s on the bench's populations with an all-stance robot at a degenerate vertex.  So when the lane that is next finds a plan (its
    // last trailing launch listed somebody) the context goes back to the plain pipelined tick for QRGPU_OV_PLAN_HOLD calls, then looks again.
    return !ov_on_hold(c, qr_env().ov_plan_hold, lane_has_plan(c, NL, n));
}

// What an overlapped tick's lane waits for before its launches: its predecessor's starts (chained) or the context's stream (not).
static int ov_begin(qrgpu_ctx *c, Lane &LN, const TickArgs &a, bool was_chain, bool small_h, unsigned epoch, unsigned prev_epoch, OvLaunch &ov)
{
    const int n = a.n;
    c->ov_next ^= 1;
    const void *outs[4] = {(const void *)a.force, (const void *)a.tau, (const void *)a.qdes, (const void *)a.status};
    bool distinct = true;
    for (int x = 0; x < 4; ++x) if (outs[x]) for (int y = 0; y < 4; ++y) if (outs[x] == c->ov_out[y]) distinct = false;
    // A tick whose lane has a plan is not chained, nor is its successor (see tick_overlaps: only reached with QRGPU_OV_PLAN_HOLD=0).
    ov.plan_tick = small_h && lane_has_plan(c, LN, n);
    ov.chained = was_chain && c->ov_n == n && c->ov_epoch == prev_epoch && c->ov_prev_ori == (const void *)a.prev_ori && distinct && !ov.plan_tick && !c->ov_prev_plan;
    c->ov_prev_plan = ov.plan_tick;
    // What the caller had queued on the context's stream when it made the PREVIOUS tick call -- the join of the tick before that one and whatever
    // consumed its outputs, which are the arrays this tick overwrites when the caller double-buffers -- must be through before this tick writes
    // anything: the event recorded at that call.  (It completed about a tick ago: the wait costs the lane nothing.)  An unchained tick waits for
    // the event recorded now: everything queued on the context's stream so far.
    const int ev_now = (c->ev_call_last + 1) & 1;
    const int ev_prev = c->ev_call_last;
    HIPCHK(c, hipEventRecord(c->ev_call[ev_now], c->stream));
    if (ov.chained && ev_prev >= 0) {
        HIPCHK(c, hipStreamWaitEvent(LN.stream, c->ev_call[ev_prev], 0));
        // ... and not before every workgroup of the previous tick's main pass and planned launch has started (bounded: 50 ms; harmless if it gives up)
        Lane &PL = c->lane[c->ov_lane_last];
        // (h > 11: the planned launches live on reserved CUs, the main pass cannot keep them from starting)
        hipLaunchKernelGGL(qr_gate2_kernel, dim3(1), dim3(64), 0, LN.stream, c->d_main_started, (int)c->ov_main_total, small_h ? PL.d_started : (int *)nullptr, (int)PL.started_total, (long long)5000000,
                           c->d_timeline ? c->d_timeline + QR_TL_GATES + (epoch & 63u) * 2 : (long long *)nullptr);      // (diagnostic: qrgpu_debug_gate2)
        HIPCHK(c, hipGetLastError());
    } else {
        ov.chained = false;
        HIPCHK(c, hipStreamWaitEvent(LN.stream, c->ev_call[ev_now], 0));
    }
    c->ev_call_last = ev_now;
    if (ov.chained) {      // (all of the predecessor's planned workgroups but the ones that wait for a CU held by the tick before's rescuers)
        const Lane &PL = c->lane[c->ov_lane_last];
        ov.prev_started = PL.d_started; ov.prev_started_total = PL.started_total - (PL.last_linger < 8 ? PL.last_linger : 8);
    }
    // (the all-gathers the caller fenced since the last tick -- qrgpu_allgather_fence -- still read output arrays this tick overwrites)
    for (int sl = 0; sl < 2; ++sl)
        if (((c->ov_fence_slots >> sl) & 1) && c->ev_gather[sl]) HIPCHK(c, hipStreamWaitEvent(LN.stream, c->ev_gather[sl], 0));
    c->ov_fence_slots = 0;
    for (int x = 0; x < 4; ++x) c->ov_out[x] = outs[x];
    return QRGPU_OK;
}

static WbcOpts tick_wbc_opts(const qrgpu_ctx *c, const TickArgs &a, float *force)
{
    WbcOpts o;
    o.merge = 1; o.status_or = a.status ? 1 : 0; o.fr = force; o.epilogue = c->epilogue;
    return o;
}

// The WBC launch beside the MPC launches, behind its gate.  Large batches, LABORATORY (QRGPU_LAB=1 QRGPU_WBC_CHUNKS=1; LAB_NOTES A.7: bit-identical,
// 5 % slower at 8192 robots): in launches of 1024 workgroups, each behind its own gate (WbcPipe::slot_base).  The main pass is not persistent at
// h <= 11, so "started" counts workgroups in dispatch order.
static int tick_issue_wbc(qrgpu_ctx *c, Lane &LN, const TickArgs &a, float *force, bool ovl, bool small_h, hipStream_t wbc_stream, unsigned epoch, unsigned wait_epoch,
                          int *gate_abort)
{
    const QrEnv &env = qr_env();
    const int n = a.n;
    const int total_wgs = 8 * ((n + 7) / 8);
    const bool chunked = env.wbc_chunks && !ovl && n >= 4096 && small_h && !c->last_main_persist;
    const int chunk_wgs = chunked ? 1024 : total_wgs;
    const int expect = (int)c->main_started_total;                                      // (launch_mpc has added this tick's main-pass units)
    const int main_before = (int)(c->main_started_total - (unsigned)total_wgs);         // (what the counter stood at before this tick's main pass)
    for (int base = 0; base < total_wgs; base += chunk_wgs) {
        const int wgs = (total_wgs - base < chunk_wgs) ? total_wgs - base : chunk_wgs;
        // (bounded at 50 ms; QRGPU_PIPE_GATE_MS for the tests.  A gate that gives up -- the caller had that much work of its own queued in front of
        //  this tick -- turns the tick into the serial one: WbcPipe::gate_abort)
        // (an overlapped tick has no second pass to fall back on: its gate is patient -- 2 s -- and one that gives up just lets the launch go: every wait
        //  of a WBC workgroup for its robot's forces is bounded and flagged.  What the serial fall-back protects against -- inputs that the caller's stream
        //  has not produced yet -- cannot happen: a chained tick's inputs are ready by contract, an unchained one makes this stream wait for the event too)
        hipLaunchKernelGGL(qr_gate_kernel, dim3(1), dim3(64), 0, wbc_stream, c->d_main_started, chunked ? main_before + base + wgs : expect, ovl ? 200000000LL : env.pipe_gate_ticks,
                           ovl ? (int *)nullptr : gate_abort, (int)epoch, (int *)nullptr);
        HIPCHK(c, hipGetLastError());
        WbcOpts o = tick_wbc_opts(c, a, force);
        o.stream = wbc_stream; o.grid_wgs = chunked ? wgs : 0; o.timed = base == 0;
        o.pipe.flag = LN.d_done_flag; o.pipe.epoch = epoch;
        o.pipe.gate_abort = ovl ? (int *)nullptr : gate_abort;
        o.pipe.finished = c->d_wbc_finished;           // (the tick's join polls it)
        o.pipe.tlr = c->d_tlr; o.pipe.tl = c->d_timeline;
        o.pipe.order = chunked ? LN.order_used : nullptr;
        o.pipe.wbc_done = ovl ? c->d_wbc_done : nullptr; o.pipe.wait_epoch = wait_epoch; o.pipe.wait_ticks = env.ov_wait_ticks;
        o.pipe.wait_list = ovl ? 1 : 0;
        o.pipe.flag_ticks = env.pipe_wait_ticks;
        o.pipe.slot_base = chunked ? base : 0;
        const int rc = launch_wbc(c, n, a.type_id, a.fb_state, a.wbc_cmd, a.prev_ori, a.tau, a.qdes, a.status, o);
        if (rc) return rc;
    }
    return QRGPU_OK;
}

// The second pass (not in an overlapped tick): the robots of the trailing launch's list (there is one at h <= 11) -- or every robot, should the
// gate have given up.
static int tick_issue_second_pass(qrgpu_ctx *c, Lane &LN, const TickArgs &a, float *force, unsigned epoch, int *gate_abort)
{
    const bool have_list = LN.last_rescue_active;
    WbcOpts o = tick_wbc_opts(c, a, force);
    o.pipe.epoch = epoch;
    o.pipe.list = have_list ? LN.d_rescue + 2 : nullptr; o.pipe.list_count = have_list ? LN.d_rescue + LN.last_rescue_parity : nullptr;
    o.pipe.gate_abort = gate_abort;
    o.pipe.second = 1;
    o.pipe.tl = c->d_timeline;
    o.pipe.flag_ticks = qr_env().pipe_wait_ticks;
    return launch_wbc(c, a.n, a.type_id, a.fb_state, a.wbc_cmd, a.prev_ori, a.tau, a.qdes, a.status, o);
}

// The join: a one-thread launch on the context's stream that polls the count of WBC waves whose written-through outputs are in memory
// (... and waits for the all-gathers queued before this tick, so that the fence in front of the next tick need not queue a launch: qr_join_kernel)
static int tick_issue_join(qrgpu_ctx *c, int n)
{
    c->wbc_finished_total += 2u * (unsigned)n;
    int *g0 = c->d_gather_done, *g1 = c->d_gather_done ? c->d_gather_done + 1 : nullptr;
    hipLaunchKernelGGL(qr_join_kernel, dim3(1), dim3(64), 0, c->stream, c->d_wbc_finished, (int)c->wbc_finished_total, (long long)2000000, c->lane[0].d_pre_hint + 2,
                       g0, (int)c->gather_total[0], g1, (int)c->gather_total[1], c->d_tick_done, (int *)nullptr, 0,
                       c->d_join_dbg ? c->d_join_dbg + 8 * (c->tick_done_total & 15u) : (long long *)nullptr);
    HIPCHK(c, hipGetLastError());
    c->gather_joined[0] = c->gather_total[0]; c->gather_joined[1] = c->gather_total[1];
    ++c->tick_done_total; c->last_tick_piped = true;
    return QRGPU_OK;
}

extern "C" {

int qrgpu_tick_batch(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_mpc_state, const float *d_traj,
                     const float *d_gait, const float *d_fb_state, const float *d_wbc_cmd, float *d_prev_ori,
                     float *d_force, float *d_tau, float *d_qdes, int *d_status)
{
    if (!c || !d_fb_state || !d_wbc_cmd || !d_tau || !d_prev_ori) return QRGPU_ERR_BAD_ARG;
    if (n <= 0 || n > c->max_batch) return QRGPU_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    c->last_tick_piped = false;
    const bool piped = tick_is_piped(c, n);
    // When the caller's previous call was an overlapped tick of the same batch that wrote OTHER output arrays, this tick is CHAINED to it: its main
    // pass is released as soon as every workgroup of that tick's MPC launches has started and fills the slots that tick's drain leaves empty; every
    // robot waits for its own previous solve / WBC pass (MpcLaunch::solved, WbcPipe::wbc_done).  Otherwise the lane waits for everything queued on
    // the context's stream so far (an event): no overlap, same results.
    const bool was_chain = c->ov_chain;
    const bool small_h = 4 * c->mpc.horizon <= 44;
    const bool ovl = piped && tick_overlaps(c, n, small_h);
    const int lane_id = ovl ? (small_h ? 1 : 3) + c->ov_next : 0;
    Lane &LN = c->lane[lane_id];
    // wbcData.Fr_des = f (:408): the WBC kernel takes its Fr_des rows from the force array the MPC kernel has just written.
    // The K14 tail, when switched on, is applied by the WBC kernel after the stance / swing merge (the MPC launch leaves d_tau raw).
    float *const force = d_force ? d_force : LN.d_cmd_tick;
    const TickArgs a{n, d_type_id, d_mpc_state, d_traj, d_gait, d_fb_state, d_wbc_cmd, d_prev_ori, d_force, d_tau, d_qdes, d_status};
    const MpcIO mpc_arrays = mpc_io(d_type_id, d_mpc_state, d_traj, d_gait, d_fb_state + (size_t)13 * n, force, d_tau, d_status);
    if (!piped) {
        int rc = launch_mpc(c, n, mpc_arrays);
        if (rc) return rc;
        return launch_wbc(c, n, d_type_id, d_fb_state, d_wbc_cmd, d_prev_ori, d_tau, d_qdes, d_status, tick_wbc_opts(c, a, force));
    }
    // Pipelined tick.  Of a robot's WBC only the relaxation QP at its very end reads the MPC's forces, and the MPC launch spends its last third
    // with most of its slots empty (two rounds of robots of very different length: DESIGN.md 5).  So the WBC launch goes on a stream of its own
    // beside the MPC launches: a gate holds it until every workgroup of the main pass has started (it must never take a CU from a solve it is
    // going to wait for), then its workgroups settle wherever a solve has left, run the rigid-body dynamics, the task set and the kinematic
    // projection, and wait -- bounded -- at the QP for their robot's flag (qr_wbc_kernel.hip, qr_mpc_kernel.hip).  Robots the main pass hands
    // to its trailing list launch are skipped there and taken by a second, list-driven WBC pass queued behind that launch.
    // (No fork event from the context stream: the gate opens only once this tick's main pass -- queued on the context stream behind everything
    //  the caller put there -- is running, and the WBC launch of the previous tick is ahead of this one on the same stream.)
    const unsigned prev_epoch = c->tick_epoch;
    if (++c->tick_epoch >= 0x3fffffffu) c->tick_epoch = 1;        // (below 2^30: bit 31 of a robot's flag word says "its WBC workgroup gave up in this epoch")
    const unsigned epoch = c->tick_epoch;
    // (the give-up word of this tick's WBC gate: a ring indexed by the epoch -- several ticks may be queued behind a backlog)
    int *const gate_abort = c->d_gate_abort + (epoch & (QR_ABORT_RING - 1));
    // (QRGPU_OV_FAULT=1, the give-up tests: chained ticks wait for an epoch nobody ever writes -- a quarter of the epochs' range ahead: "not
    //  reached yet" -- so that every per-robot wait runs into its bound)
    const unsigned waited_epoch = (prev_epoch + (qr_env().ov_fault == 1 ? 0x10000000u : 0u)) & 0x3fffffffu;
    OvLaunch ov{epoch, false, waited_epoch, false, nullptr, 0u};
    if (ovl) { const int rc = ov_begin(c, LN, a, was_chain, small_h, epoch, prev_epoch, ov); if (rc) return rc; }
    MpcOpts mo;
    mo.piped = true; mo.lane_id = lane_id; mo.ov = ovl ? &ov : nullptr;
    int rc = launch_mpc(c, n, mpc_arrays, mo);
    if (rc) return rc;
    // (overlapped ticks: a stream of the highest priority, qrgpu_ctx::wbc_stream_hi)
    const hipStream_t wbc_stream = ovl ? c->wbc_stream_hi : c->wbc_stream;
    if (ovl && !ov.chained) HIPCHK(c, hipStreamWaitEvent(wbc_stream, c->ev_call[c->ev_call_last], 0));
    rc = tick_issue_wbc(c, LN, a, force, ovl, small_h, wbc_stream, epoch, (ovl && ov.chained) ? waited_epoch : 0u, gate_abort);
    if (!rc && !ovl) rc = tick_issue_second_pass(c, LN, a, force, epoch, gate_abort);
    if (!rc) rc = tick_issue_join(c, n);
    if (rc) return rc;
    if (ovl) {
        ++c->ov_stats[ov.chained ? 0 : 1];
        c->ov_chain = true; c->ov_n = n; c->ov_epoch = epoch; c->ov_main_total = c->main_started_total; c->ov_prev_ori = (const void *)d_prev_ori; c->ov_lane_last = lane_id;
    }
    return QRGPU_OK;
}

// The tick on the reference's cadence (include/qrgpu.h): per robot either the MPC (d_mpc_updated[i] != 0) or the WBC.  Always the serial form, on
// the context's stream: the MPC launches with the mask and the context's torque tail (only due robots are solved and write d_tau), the cadence
// kernel (kept force of the due robots; torques and status word of the others), the WBC launch with the same mask as its skip list.  The pipelined
// and overlapped forms rest on every robot's solve raising a flag and on gates that count workgroups: not for a tick in which most robots are
// not solved.  Nothing is read back: which robots are due is known on the device alone.
int qrgpu_tick_cadence_batch(qrgpu_ctx *c, int n, const int *d_type_id, const int *d_mpc_updated, const float *d_mpc_state, const float *d_traj,
                             const float *d_gait, const float *d_fb_state, const float *d_wbc_cmd, float *d_prev_ori, float *d_force, float *d_hold,
                             float *d_tau, float *d_qdes, int *d_status)
{
    if (!c || !d_mpc_updated || !d_force || !d_hold) return QRGPU_ERR_BAD_ARG;
    if (!d_mpc_state || !d_traj || !d_gait || !d_fb_state || !d_wbc_cmd || !d_tau || !d_prev_ori) return QRGPU_ERR_BAD_ARG;
    if (n <= 0 || n > c->max_batch) return QRGPU_ERR_BAD_ARG;
    // (both launches' set-up rules before the first launch: a call that fails has launched nothing)
    if (!(d_type_id ? (ready_mask(c->mpc_ready) != 0 && ready_mask(c->wbc_ready) != 0) : (c->mpc_ready[0] && c->wbc_ready[0]))) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    c->last_tick_piped = false;
    const TickArgs a{n, d_type_id, d_mpc_state, d_traj, d_gait, d_fb_state, d_wbc_cmd, d_prev_ori, d_force, d_tau, d_qdes, d_status};
    // Under qrgpu_set_mode_route only the robots on the MPC chain take part: due' = updated && on_chain goes to the MPC launch, skip' = updated ||
    // !on_chain to the WBC launch, both written by one small launch in front of the MPC launch; the cadence kernel leaves the others alone too.
    const int *due = d_mpc_updated, *skip = d_mpc_updated, *idle = nullptr;
    if (c->mode_chain) {
        if (!c->d_mode_masks) HIPCHK(c, hipMalloc((void **)&c->d_mode_masks, 2 * sizeof(int) * (size_t)c->max_batch));
        int *const d_due = c->d_mode_masks, *const d_skip = c->d_mode_masks + c->max_batch;
        hipLaunchKernelGGL(qr_mode_masks_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_mpc_updated, c->mode_chain, d_due, d_skip);
        HIPCHK(c, hipGetLastError());
        due = d_due; skip = d_skip; idle = d_skip;
    }
    MpcIO io = mpc_io(d_type_id, d_mpc_state, d_traj, d_gait, d_fb_state + (size_t)13 * n, d_force, d_tau, d_status);
    io.due = due;
    MpcOpts mo;
    mo.epilogue = c->epilogue;
    int rc = launch_mpc(c, n, io, mo);
    if (rc) return rc;
    CadenceLegs L{};
    for (int t = 0; t < QRGPU_MAX_TYPES; ++t) { L.hip_l[t] = c->mpc.type[t].hip_l; L.upper_l[t] = c->mpc.type[t].upper_l; L.lower_l[t] = c->mpc.type[t].lower_l; }
    L.type_ready = ready_mask(c->mpc_ready);
    hipLaunchKernelGGL(qr_cadence_kernel, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, L, d_type_id, due, d_mpc_state, d_fb_state, (const float *)d_force, d_hold,
                       d_tau, d_status, idle);
    HIPCHK(c, hipGetLastError());
    WbcOpts o = tick_wbc_opts(c, a, d_force);
    o.pipe.skip = skip;
    return launch_wbc(c, n, d_type_id, d_fb_state, d_wbc_cmd, d_prev_ori, d_tau, d_qdes, d_status, o);
}

}  // extern "C"

// Do the streams of an overlapped context really run side by side in this process?  Probed both ways round: the first `npair` streams of the set
// against each other and against the rest (a launch on one that waits for a launch queued afterwards on the other).
static int probe_streams(qrgpu_ctx *c, hipStream_t *st, int nst, int npair)
{
    DeviceScratch scratch;
    HIPCHK(c, hipMalloc(&scratch.p, 16 * sizeof(int)));
    int *const d_probe = (int *)scratch.p;
    HIPCHK(c, hipMemset(d_probe, 0, 16 * sizeof(int)));
    HIPCHK(c, hipDeviceSynchronize());
    int k = 0, token = 0;
    for (int a = 0; a < nst; ++a)
        for (int b = 0; b < nst; ++b) {
            if (a == b || (a >= npair && b >= npair)) continue;
            // (20 ms, and a pair that fails is asked once more: the waiting launch runs from the moment it is queued, the other one is queued by this
            //  thread right behind it -- on a host busy with something else "right behind" has been seen to take longer than the 2 ms this bound was)
            int res = 0;
            for (int attempt = 0; attempt < 2 && res != 1; ++attempt) {
                ++token;                                   // (the eight flag words go round: every probe has a value of its own)
                hipLaunchKernelGGL(qr_probe_wait_kernel, dim3(1), dim3(64), 0, st[a], d_probe + k, d_probe + 8, (long long)2000000, token);
                hipLaunchKernelGGL(qr_probe_set_kernel, dim3(1), dim3(64), 0, st[b], d_probe + k, token);
                HIPCHK(c, hipStreamSynchronize(st[a]));
                HIPCHK(c, hipStreamSynchronize(st[b]));
                HIPCHK(c, hipMemcpy(&res, d_probe + 8, sizeof(int), hipMemcpyDeviceToHost));
                k = (k + 1) & 7;
            }
            if (res != 1) {
                static char msg[320];
                snprintf(msg, sizeof(msg), "qrgpu_set_tick_overlap: two of the context's streams share a hardware queue in this process (set GPU_MAX_HW_QUEUES=8 before the first HIP call); "
                         "overlapped ticks stay off [a launch on stream %d of the set waited for one queued behind it on stream %d]", a, b);
                c->err = msg;
                c->overlap = 0;
                return QRGPU_ERR_NOT_SETUP;
            }
        }
    return QRGPU_OK;
}

extern "C" {

// Overlapped ticks: see include/qrgpu.h.  Switching them on creates the lanes and PROBES that two of the context's streams really run side
// by side in this process: with fewer hardware queues than streams (GPU_MAX_HW_QUEUES, default 4, against the context's seven) two streams may
// share one, a chained tick would sit out its gates' bounds behind its predecessor, and the mode is refused -- QRGPU_ERR_NOT_SETUP,
// qrgpu_last_error says why, ticks stay as they were.
int qrgpu_set_tick_overlap(qrgpu_ctx *c, int on)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    c->ov_chain = false;
    if (!on) { c->overlap = 0; return QRGPU_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->ev_call[0]) for (int k = 0; k < 2; ++k) HIPCHK(c, hipEventCreateWithFlags(&c->ev_call[k], hipEventDisableTiming));
    if (!c->wbc_stream_hi) HIPCHK(c, create_side_stream(&c->wbc_stream_hi));
    // The stream sets are made for the horizon the context is set up with at this call (a context whose horizon changes class afterwards calls this
    // again; until then its ticks are plain pipelined ticks): every stream wants a hardware queue of its own, and a context that made both sets
    // would own eleven streams against GPU_MAX_HW_QUEUES = 8.
    //   h <= 11: lanes 1 and 2 (a stream each; the planned launches of consecutive ticks share lane 0's side stream, in tick order).
    //   h > 11 (QRGPU_OV16=0 keeps such contexts on the plain tick): lanes 3 and 4 on a machine split in space by CU masks -- the main pass two to a
    //     CU on 192 CUs, the big class's whole-CU workgroups (and whatever the main pass hands on) on 64 reserved ones, eight of every XCD
    //     (the per-XCD count has to be a multiple of four, LAB_NOTES A.2 item 2).
    const bool want16 = 4 * c->mpc.horizon > 44;
    hipStream_t st[6]; int nst = 0, npair = 0;
    if (!want16) {
        for (int l = 1; l <= 2; ++l) {
            if (lane_create(c, c->lane[l], true) != QRGPU_OK) { c->err = "qrgpu_set_tick_overlap: allocation of a lane failed"; return QRGPU_ERR_ALLOC; }
            c->lane[l].side_stream = c->lane[0].side_stream;
        }
        st[0] = c->lane[1].stream; st[1] = c->lane[2].stream; st[2] = c->wbc_stream_hi; st[3] = c->stream; nst = 4; npair = 2;
    } else if (qr_env().ov16) {
        if (!c->ov16_side_cus) {
            int k = (64 * c->num_cu / 256) & ~31;          // (a quarter of the machine)
            if (k < 32) k = 32;
            if (k > c->num_cu / 2) k = (c->num_cu / 2) & ~31;
            c->ov16_side_cus = k;
            for (int b = 0; b < c->num_cu && b < 512; ++b) { if (b < c->num_cu - k) c->mask16_main[b >> 5] |= 1u << (b & 31); else c->mask16_side[b >> 5] |= 1u << (b & 31); }
        }
        for (int l = 3; l <= 4; ++l)
            if (lane_create(c, c->lane[l], true, true) != QRGPU_OK) { c->err = "qrgpu_set_tick_overlap: allocation of a CU-masked lane failed"; return QRGPU_ERR_ALLOC; }
        st[0] = c->lane[3].stream; st[1] = c->lane[4].stream; st[2] = c->lane[3].side_stream; st[3] = c->lane[4].side_stream; st[4] = c->wbc_stream_hi; st[5] = c->stream; nst = 6; npair = 4;
    } else { c->overlap = 1; return QRGPU_OK; }          // (h > 11 with QRGPU_OV16=0: the mode is on, the ticks stay plain)
    const int rc = probe_streams(c, st, nst, npair);
    if (rc) return rc;
    c->overlap = 1;
    return QRGPU_OK;
}
int qrgpu_tick_fence(qrgpu_ctx *c) { if (!c) return QRGPU_ERR_BAD_ARG; c->ov_chain = false; return QRGPU_OK; }
int qrgpu_tick_overlap_stats(const qrgpu_ctx *c, int *chained, int *unchained)
{
    if (!c) return QRGPU_ERR_BAD_ARG;
    if (chained) *chained = c->ov_stats[0];
    if (unchained) *unchained = c->ov_stats[1];
    return QRGPU_OK;
}

}  // extern "C"
