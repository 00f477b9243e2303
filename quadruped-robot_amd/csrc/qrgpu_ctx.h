// Internal: the context behind the opaque qrgpu_ctx of include/qrgpu.h, the environment switches and the declarations the host files share
// (qrgpu_api.hip, qrgpu_stages.hip, qrgpu_debug.hip, qrgpu_mpc.hip, qrgpu_tick.hip, qrgpu_comm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/qrgpu.h"
#include "qr_device_types.h"
#include "qr_kernels.h"

using namespace qrgpu;

// The MPC kernel variants the host launches (the table with their functions, workgroup sizes and persistent forms: qrgpu_mpc.hip).
enum MpcVar {
    MPC_MAIN11,            // h <= 11 main pass: <2, ., ., 512>, eight waves build and sweep (two blocks per thread, 128 VGPRs), two workgroups per CU
    MPC_LIST11,            // h <= 11 list launches: <4, BIG, LIST, 256> striding over a list, whole CU's LDS, 96 rows
    MPC_ONE11,             // h <= 11 one robot per workgroup on a whole CU: <2, BIG, ., 512> (planned list; main pass of batches below 64 robots)
    MPC_HALF_LIST11,       // h <= 11 list launches of an overlapped tick on HALF a CU: <4, BIG, LIST, 256, 2, H16>, S^-1 in the global scratch
    MPC_MAIN16,            // h <= 16 main pass: <5, BIG, ., 512>, one workgroup per CU (also the planned list's one robot per workgroup)
    MPC_LIST16,            // h <= 16 list launches: <9, BIG, LIST, 256>
    MPC_TWO16,             // h <= 16 two to a CU: <2, BIG, ., 512, 4, H16> (also one listed robot per half CU in an overlapped tick at h <= 11)
    MPC_PERSIST11,         // persistent form of MPC_MAIN11 (QRGPU_PERSIST=2)
    MPC_PERSIST16,         // persistent form of MPC_MAIN16
    MPC_VAR_COUNT,
    MPC_VAR_NONE = -1
};

// One "lane" of MPC launch scheduling: everything a sequence of MPC launches on ONE stream carries from launch to launch -- the longest-first
// order, the rescue and planned lists with their ping-pong parities and pinned length hints, the cumulative counters its gates poll, the
// per-robot flags its solves raise for the WBC launch running beside them.  Lane 0 is the context's own stream (every call but an overlapped
// tick).  Lanes 1 and 2 have streams of their own and alternate between consecutive OVERLAPPED ticks (qrgpu_set_tick_overlap): tick t + 1's
// launches are queued on the other lane and start filling the slots tick t's drain leaves empty; what a robot carries from tick to tick
// (warm-start words, cost word, the orientation task's memory) is handed over per robot (MpcLaunch::solved, WbcPipe::wbc_done).
#define QR_LANES 5                 // 0: the context's stream; 1, 2: overlapped ticks at h <= 11; 3, 4: overlapped ticks at h > 11 (CU-masked streams)
#define QR_ABORT_RING 8            // give-up words are rings indexed by epoch: several ticks may be in flight behind a backlog
struct Lane {
    hipStream_t stream = nullptr;             // (lane 0: mirrors qrgpu_ctx::stream)
    bool own_stream = false;
    hipStream_t side_stream = nullptr;        // the planned list launch beside the main pass
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int *d_order = nullptr;                   // [max_batch] longest-first dispatch order of the next MPC launch of this lane
    int lpt_n = 0;                            // batch size d_order is valid for (0 = no history yet)
    int *d_rescue = nullptr;                  // [2] counters (ping-pong by call parity) + [max_batch] robot ids of the MPC rescue pass
    int rescue_parity = 0;
    bool last_rescue_active = false;          // did the last launch_mpc carry a trailing list launch (so that flags may say "on the rescue list")?
    int last_rescue_parity = 0;
    // planned list (launched beside the main pass on side_stream): [4] counters + [max_batch] robot ids; skip flags; batch size the plan is for
    int *d_pre = nullptr;
    unsigned char *d_skip = nullptr;
    int plan_n = 0;
    int *d_pre_hint = nullptr;                // device-side address of h_pre_count
    int *h_pre_count = nullptr;               // pinned: [0], [1] the planned list's length as of the last call, by parity (stale by a call or two at worst)
    int plan_sync_left = 0;                   // calls after a history reset that still end with a stream sync (so that the host sees the first plans' lengths)
    int *d_started = nullptr;                 // workgroups of planned list launches that have started, ever (qr_gate_kernel); never cleared
    unsigned started_total = 0;               // what that counter reaches once every planned launch issued so far has started (wraps like the counter)
    int *d_go = nullptr;                      // [0] "go" count of the planned launches' gates (cumulative); [1 + (plan epoch & 7)]: plan epoch of a gate that gave up
    unsigned go_total = 0;
    int plan_epoch = 0;
    int *d_planned_done = nullptr;            // workgroups of planned launches that are through, ever (polled by the trailing launch of a pipelined tick)
    unsigned planned_done_total = 0;
    int *d_qhead = nullptr;                   // [2][8] queue heads of the persistent main pass, ping-pong (a launch zeroes the other half)
    int qhead_parity = 0;
    int two_hold = 0;                         // h > 11 two to a CU: calls left on one workgroup per CU after the planned list outgrew 45 % of the batch
    bool two_probe = false;                   //   ... and the call after them runs two to a CU whatever the count says, to get a fresh plan
    unsigned *d_done_flag = nullptr;          // [max_batch] (tick epoch << 1) | on-the-rescue-list, raised by this lane's solves for the WBC launch
    float *d_cmd_tick = nullptr;              // [12][max_batch] force scratch of a tick whose caller passes no force array
    bool masked = false;                      // lanes 3, 4: stream = all CUs but the reserved ones, side_stream = the reserved ones (both owned)
    int *d_lane_done = nullptr;               // overlapped ticks of this lane whose tail (second WBC pass) is through, ever (the tick's join polls it)
    int *d_main_done = nullptr; int main_done_total = 0;   // h > 11 overlapped: workgroups of the lane's main passes that have left (cumulative), MpcLaunch::main_done
    int order_parity = 0;                               // which half of d_order the lane's next main pass reads (the trailing launch writes the other)
    const int *order_used = nullptr;                    // ... and what the last main pass read (the chunked WBC launches of that tick read it too)
    bool join_recorded = false;                         // ev_join has been recorded at least once (the lane's next overlapped tick at h > 11 waits for it)
    int last_linger = 0;                                // how many workgroups of the lane's last planned launch stay until its main pass is through
    int *d_rescue_taken = nullptr;                      // ... and the rescue list's second head, per parity (MpcLaunch::rescue_taken)
    unsigned lane_done_total = 0;
};

struct qrgpu_ctx {
    int device = 0;
    int max_batch = 0;
    int horizon_max = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    MpcLaunch mpc{};
    bool mpc_ready[QRGPU_MAX_TYPES] = {false, false, false, false};
    bool wbc_ready[QRGPU_MAX_TYPES] = {false, false, false, false};
    VmcLaunch vmc{};
    bool vmc_ready[QRGPU_MAX_TYPES] = {false, false, false, false};
    WbcConst wbc_host[QRGPU_MAX_TYPES];
    WbcConst *d_wbc = nullptr;
    bool wbc_dirty = true;
    // the plant's body per type (qrgpu_plant_body_setup): a device array of its own beside d_wbc, uploaded like it
    qrgpu_plant_body_desc body_host[QRGPU_MAX_TYPES] = {};
    qrgpu_plant_body_desc *d_body = nullptr;
    bool body_ready[QRGPU_MAX_TYPES] = {false, false, false, false};
    bool body_dirty = true;
    // the stage kernels' per-robot reset and clock (qrgpu_set_stage_reset); all zeros while nothing is bound
    qrgpu_stage_reset stage_reset{};
    // the chain each robot is on (qrgpu_set_mode_route); null while nothing is bound.  d_mode_masks [2][max_batch]: the masked due and skip words
    // of the cadenced tick under the binding (qr_mode_masks_kernel), allocated at the first such call
    const int *mode_chain = nullptr;
    int *d_mode_masks = nullptr;
    // the gait table of qrgpu_gait_select_update_batch: a device copy the kernel's lanes index themselves, allocated at the first call and uploaded
    // when the caller's table differs from the one last uploaded
    qrgpu_gait_desc gait_table_host[QRGPU_MAX_GAITS] = {};
    qrgpu_gait_desc *d_gait_table = nullptr;
    int gait_table_n = 0;
    // scratch for the single-robot calls and the fused tick
    // Staging of the single-robot calls.  Default: ONE block of pinned, mapped host memory that the kernels read and write in place (zero
    // copy: d_* are the device-side addresses of h_*), so a call is "fill h_in1, one launch, wait, read h_out1" with no copy command on the
    // stream.  QRGPU_SINGLE_COPIES=1: device buffers and three hipMemcpyAsync per call (round 2's form, kept for the A/B of INTEGRATION.md).
    float *d_in1 = nullptr;       // staging: single-robot inputs
    float *d_out1 = nullptr;      // staging: single-robot outputs
    int *d_st1 = nullptr;
    float *h_in1 = nullptr, *h_out1 = nullptr;     // host-side addresses of the same memory (zero copy) or null
    int *h_st1 = nullptr;
    void *h_stage = nullptr;      // the pinned block
    bool zero_copy = false;
    int type_stage = 0;           // (copy path) the type word in flight
    Lane lane[QR_LANES];
    // what each robot cost in the last MPC launch: [0] every launch of lane 0, in place; an overlapped tick of epoch e writes [e & 1] and smooths
    // with [(e & 1) ^ 1], its predecessor's (the trailing launch of tick t sorts a buffer that tick t + 1's solves do not write)
    int *d_cost[2] = {nullptr, nullptr};
    int cost_n[2] = {0, 0};       // batch size each holds the costs of a whole overlapped tick for (0: not)
    double *d_sinv_spill = nullptr;   // [max_batch][tri(QR_QH)] S^-1 scratch of the h > 11 variants, allocated at first use
    bool planned = true;
    int big_nls = 0;
    // pipelined tick (qrgpu_set_tick_pipeline, default on): the WBC launch of a tick runs on wbc_stream beside that tick's MPC launches
    bool pipeline = true;
    hipStream_t wbc_stream = nullptr;
    int *d_main_started = nullptr;            // main-pass workgroups started, ever (the WBC launch's gate); never cleared
    unsigned main_started_total = 0;
    unsigned tick_epoch = 0;
    int main_slots[MPC_VAR_COUNT] = {};       // resident workgroups per CU of each persistent variant at the LDS size it was last configured for (0: not asked yet)
    int main_slots_lds[MPC_VAR_COUNT] = {};
    int *d_tick_done = nullptr;               // pipelined ticks complete (bumped by their joins), ever: what qrgpu_allgather_tau_of_tick's gate polls
    unsigned tick_done_total = 0;
    bool last_tick_piped = false;             // the context's most recent qrgpu_tick_batch was a pipelined one with a polling join
    int *d_gather_done = nullptr;             // [2] gathers finished per source-buffer slot, ever (qrgpu_allgather_fence polls it)
    unsigned gather_total[2] = {0, 0};
    unsigned gather_joined[2] = {0, 0};            // ... of which a pipelined tick's join has already made the compute stream wait for
    int *d_gate_abort = nullptr;              // [QR_ABORT_RING] word (epoch & 7): epoch of the pipelined tick whose WBC gate timed out (0: none)
    int *d_wbc_finished = nullptr;            // waves of pipelined WBC launches whose outputs are in memory, ever (the tick's join); never cleared
    unsigned wbc_finished_total = 0;
    // overlapped ticks (qrgpu_set_tick_overlap): consecutive pipelined ticks alternate between lanes 1 and 2
    int overlap = 0;                          // 0 off, 1 on (the caller's promise about inputs and output buffers: include/qrgpu.h)
    int ov_next = 0;                          // which of lanes 1 / 2 the next overlapped tick takes
    bool ov_chain = false;                    // the context's last launch was an overlapped tick (the next one may start under it)
    int ov_n = 0;                             // ... of this batch size
    unsigned ov_epoch = 0, ov_main_total = 0; // ... with this epoch, after which d_main_started reaches this
    const void *ov_out[4] = {nullptr, nullptr, nullptr, nullptr};   // ... writing these output arrays (force, tau, qdes, status)
    const void *ov_prev_ori = nullptr;        // ... and this orientation-task memory
    int ov_lane_last = 0;                     // ... on this lane
    int ov_fence_slots = 0;                   // bit s: qrgpu_allgather_fence(s) was called since the last overlapped tick (that tick's lane waits for the gather too)
    int ov_hold = 0;                          // calls left on the plain pipelined tick after a lane found a plan (a population with whole-CU robots)
    bool ov_prev_plan = false;                // ... with a planned launch (its successor is not chained either)
    // the tail of an overlapped tick -- its second WBC pass and the count its join polls -- runs on a stream of its own behind an event of the lane's
    // stream: on the lane's stream those thousand (empty) workgroups, dispatched one freed slot at a time on a machine that is never empty, stood
    // between the lane's next tick and its gate (60 us per tick)
    // the WBC launches of overlapped ticks: a stream of the highest priority.  Tick k's WBC workgroups and tick k + 1's solves want the same freed
    // slots; at equal priority the solves get most of them, tick k's WBC launch lasts until tick k + 1's main pass is dispatched (tick duration: two
    // periods) and tick k + 2, which waits for tick k's join, starts late every other tick
    hipStream_t wbc_stream_hi = nullptr;
    // overlapped ticks at h > 11: a tenth of a mixed shard wants a whole CU per robot, which a machine that is never empty does not offer -- so the
    // machine is split in space: ov16_side_cus CUs (a multiple of 32 on 256: every XCD's share a multiple of four, or the LDS a queue may use per CU
    // drops to ~100 KB) are reserved for the whole-CU launches (planned list, trailing launch), the main passes run on the others
    int ov16_side_cus = 0;
    uint32_t mask16_main[16] = {}, mask16_side[16] = {};
    // a chained tick waits for what the caller had queued on the context's stream when it made the PREVIOUS tick call (its predecessor's predecessor's
    // join and whatever consumed that tick's outputs: the arrays this tick overwrites), recorded at that call: ring of two
    hipEvent_t ev_call[2] = {nullptr, nullptr};
    int ev_call_last = -1;                    // index of the event recorded at the last overlapped tick call (-1: none)
    long long *d_join_dbg = nullptr;          // diagnostic (qrgpu_debug_counters): what the last joins saw
    int ov_stats[2] = {0, 0};                 // overlapped ticks issued so far: chained to their predecessor / behind an event of the context's stream
    unsigned *d_solved = nullptr;             // [max_batch] epoch of the overlapped tick whose solve of the robot has left its warm-start and cost words in memory
    unsigned *d_wbc_done = nullptr;           // [max_batch] ... whose WBC pass has left the orientation task's memory (prev_ori) in memory
    int *d_tlr = nullptr;                     // diagnostic: [4][max_batch] per-robot WBC moments of the last pipelined tick
    long long *d_timeline = nullptr;          // diagnostic (qrgpu_debug_timeline): [64][8], or null
    int *d_ftime = nullptr;                   // diagnostic, with d_tlr: [max_batch] when each robot's solve ended in the last pipelined tick (100 MHz clock, low word)
    bool lpt = true;
    bool rescue = true;
    int epilogue = 0;             // QRGPU_EPILOGUE_* bits
    double *d_flops = nullptr;    // [max_batch][4], allocated by qrgpu_enable_flop_count
    bool flops_on = false;
    int flops_n = 0;              // robots of the last counted launch
    bool warm = true;             // warm start of the MPC active set from the slot's previous solve
    unsigned char *d_warm = nullptr;   // [max_batch][QR_WARM_STRIDE]
    int warm_n = 0;               // batch size d_warm is valid for (0 = nothing yet)
    bool last_main_persist = false;  // the last main pass took robots off queues (its "started" count is per robot, in no fixed order: no chunked WBC launches)
    void *d_dbg_cycles_wbc = nullptr;
    void *d_dbg_cycles = nullptr; // optional [max_batch][8] int64 phase stamps of the MPC kernel (qrgpu_debug_cycles)
    int lds_per_cu = 0, num_cu = 0;
    std::string name;
    std::string err;
    // multi-GPU: context-owned RCCL communicator and the stream its all-gathers run on (qrgpu_comm.hip)
    void *comm = nullptr;         // ncclComm_t
    bool comm_owned = false;
    int comm_nranks = 0, comm_rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_tick = nullptr;          // compute stream -> comm stream: this tick's torques are complete
    hipEvent_t ev_gather[2] = {nullptr, nullptr};   // comm stream -> compute stream: the gather that read buffer `slot` has landed
    bool ev_gather_pending[2] = {false, false};
    // timing
    bool timing = false;
    bool timing_paused = false;
    int timing_every = 1;          // events bracket every timing_every-th launch of a kernel (qrgpu_enable_timing(ctx, N))
    unsigned ev_calls[2] = {0, 0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[2];
    size_t ev_used[2] = {0, 0};
    std::vector<hipEvent_t> marks;   // qrgpu_mark: caller-indexed events on the context stream
};

// Environment switches.  The SUPPORTED ones are listed in include/qrgpu.h (name, default, effect) and read with getenv.  The LABORATORY ones --
// launch forms kept for a test or a profiling run, LAB_NOTES.md A.1 -- are read through lab_env, which answers only when QRGPU_LAB=1 is set, so
// that a product run cannot be steered by a leftover of an experiment.  qrgpu_create warns once per process about any other QRGPU_* variable
// it finds in the environment.
inline const char *lab_env(const char *name)
{
    static const bool lab = [] { const char *e = getenv("QRGPU_LAB"); return e && atoi(e) != 0; }();
    return lab ? getenv(name) : nullptr;
}
#define QRGPU_SUPPORTED_ENV "QRGPU_TICK_PIPELINE", "QRGPU_PIPE_GATE_MS", "QRGPU_PLAN_GO_MS", "QRGPU_PIPE_WAIT_US", "QRGPU_OV_WAIT_US", "QRGPU_OV_FAULT", "QRGPU_OV_PLAN_HOLD", "QRGPU_OV16", \
                            "QRGPU_COMM_EVENTS", "QRGPU_SINGLE_COPIES", "QRGPU_PERSIST", "QRGPU_H16_TWO", "QRGPU_H16_TWO_HOLD", "QRGPU_H16_BIG_US", "QRGPU_H16_BIG_STAY_US", \
                            "QRGPU_LIB", "QRGPU_EXTRA_FLAGS", "QRGPU_LAB"
#define QRGPU_LAB_ENV "QRGPU_WBC_CHUNKS", "QRGPU_PLANNED_FORK"

// Every switch the library reads, read ONCE per process, at the first call that asks (qr_env): the only getenv / lab_env calls of the host code
// besides lab_env's own.  Times are in ticks of the 100 MHz clock the kernels' bounded waits count.
struct QrEnv {
    static int num(const char *e, int dflt) { return e ? atoi(e) : dflt; }
    static long long ms(const char *e) { return 100000LL * (e ? atoll(e) : 50LL); }
    static long long us(const char *e, long long dflt_ticks) { return e ? 100LL * atoll(e) : dflt_ticks; }
    int tick_pipeline = num(getenv("QRGPU_TICK_PIPELINE"), 1);                   // 0 keeps every tick serial
    long long pipe_gate_ticks = ms(getenv("QRGPU_PIPE_GATE_MS"));                // bound of the gate in front of a pipelined tick's WBC launch
    long long plan_go_ticks = ms(getenv("QRGPU_PLAN_GO_MS"));                    // bound of the planned launch's wait for the "go" of the context's stream
    long long pipe_wait_ticks = us(getenv("QRGPU_PIPE_WAIT_US"), 400000LL);      // bound of a WBC workgroup's wait for its robot's forces (4 ms)
    long long ov_wait_ticks = us(getenv("QRGPU_OV_WAIT_US"), 2000000LL);         // bound of an overlapped tick's per-robot waits for its predecessor (20 ms)
    int ov_fault = num(getenv("QRGPU_OV_FAULT"), 0);                             // fault injection of the give-up tests: 1 chained ticks wait for an epoch nobody writes, 2 nobody lingers
    int ov_plan_hold = num(getenv("QRGPU_OV_PLAN_HOLD"), 31);                    // plain ticks after a lane of an overlapped context found a plan (h <= 11)
    bool ov16 = num(getenv("QRGPU_OV16"), 1) != 0;                               // overlapped ticks at h > 11
    int comm_events = num(getenv("QRGPU_COMM_EVENTS"), -1);                      // (-1: by the communicator's size, qrgpu_comm.hip)
    bool single_copies = num(getenv("QRGPU_SINGLE_COPIES"), 0) != 0;             // device staging and copies for the single-robot calls
    int persist = num(getenv("QRGPU_PERSIST"), 1);                               // 0 never, 1 the h > 11 main pass, 2 the h <= 11 one too
    int h16_two = num(getenv("QRGPU_H16_TWO"), 1);                               // 0 never two to a CU at h > 11, 2 from 64 robots on
    int h16_two_hold = num(getenv("QRGPU_H16_TWO_HOLD"), 31);                    // calls on one workgroup per CU after the list outgrew 45 % of the batch
    int h16_big_us = num(getenv("QRGPU_H16_BIG_US"), 450);                       // the cost rule of the h > 11 planned list: onto a whole CU from this cost on ...
    int h16_big_stay_us = num(getenv("QRGPU_H16_BIG_STAY_US"), 300);             // ... and off it below this one
    int wbc_chunks = num(lab_env("QRGPU_WBC_CHUNKS"), 0);                        // laboratory: the WBC launch of a large batch in launches of 1024 workgroups (LAB_NOTES A.7)
    int planned_fork = num(lab_env("QRGPU_PLANNED_FORK"), 0);                    // laboratory: 1 = the planned launch forks and joins through stream events (counter-collection runs)
};
inline const QrEnv &qr_env() { static const QrEnv env{}; return env; }

#define HIPCHK(ctx, call)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
            return QRGPU_ERR_LAUNCH;                                                         \
        }                                                                                    \
    } while (0)


// ---------------------------------------------------------------------------------------------
// Shared by the host files
// ---------------------------------------------------------------------------------------------
inline int ready_mask(const bool *r) { int m = 0; for (int t = 0; t < QRGPU_MAX_TYPES; ++t) if (r[t]) m |= 1 << t; return m; }

// The check every batched entry point starts with.
inline bool batch_ok(const qrgpu_ctx *c, int n) { return c && n > 0 && n <= c->max_batch; }

// The binding of qrgpu_set_stage_reset as the stage kernels take it: the bound level in the stage's own numbers, the mask and the clock.  With
// nothing bound c->stage_reset is all zeros, and both forms are the unbound struct: a null mask, a null tick array.
inline StageResetArgs stage_args(const qrgpu_ctx *c, int construct, int live)
{
    const qrgpu_stage_reset &b = c->stage_reset;
    return StageResetArgs{b.d_mask, b.bits, b.level == QRGPU_STAGE_RESET_CONSTRUCT ? construct : live, b.d_ticks, b.tick_dt};
}
// The mask alone, for the stages with one reset level and no clock.
inline StageResetArgs stage_mask_args(const qrgpu_ctx *c) { return StageResetArgs{c->stage_reset.d_mask, c->stage_reset.bits, 1, nullptr, 0.f}; }

// A device allocation that lives as long as the scope that made it: freed on every exit path, an early HIPCHK return included.
struct DeviceScratch {
    void *p = nullptr;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { (void)hipFree(p); }
};

// Brackets a launch with a pair of events while timing is on (qrgpu_enable_timing): kernel 0 = the MPC main pass, 1 = the WBC launch.
struct TimerScope {
    qrgpu_ctx *c; int k; bool on; hipStream_t s;
    TimerScope(qrgpu_ctx *ctx, int kernel, hipStream_t stream = nullptr, bool enabled = true) : c(ctx), k(kernel), on(ctx->timing && enabled), s(stream ? stream : ctx->stream)
    {
        if (on && ctx->timing_every > 1 && (ctx->ev_calls[kernel]++ % (unsigned)ctx->timing_every) != 0) on = false;
        if (!on) return;
        if (c->ev_used[k] == c->ev[k].size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            c->ev[k].push_back({a, b});
        }
        hipEventRecord(c->ev[k][c->ev_used[k]].first, s);
    }
    ~TimerScope()
    {
        if (!on) return;
        hipEventRecord(c->ev[k][c->ev_used[k]].second, s);
        c->ev_used[k]++;
    }
};

// What an overlapped tick adds to its MPC launches (qrgpu_tick_batch): the epoch its solves leave in d_solved, whether they wait -- per robot -- for
// the previous tick's (chained), and the cost buffers they read and write.
struct OvLaunch { unsigned epoch; bool chained; unsigned prev_epoch; bool plan_tick; int *prev_started; unsigned prev_started_total; };

// The optional part of an MPC launch: everything but the context, the batch size and the arrays (MpcIO; dbgH / dbgG set: an inspection launch).
struct MpcOpts {
    int epilogue = 0;                 // QRGPU_EPILOGUE_* bits applied by the MPC kernel itself (the MPC-only entry point)
    bool piped = false;               // part of a pipelined tick: the solves raise per-robot flags for the WBC launch running beside them
    int lane_id = 0;
    const OvLaunch *ov = nullptr;     // ... of an overlapped one
};
// ... and of a WBC launch: everything but the context, the batch size and the arrays every launch has.
struct WbcOpts {
    float *dbg = nullptr;             // inspection output of qrgpu_fb_debug_batch (the launch then needs no command, memory or torque array)
    int merge = 0, status_or = 0;     // the tick's stance / swing merge into d_tau, status words OR-ed into what the MPC launch left
    const float *fr = nullptr;        // Fr_des rows: the force array the MPC launch has just written
    int epilogue = 0;
    float *qp = nullptr;              // inspection output of qrgpu_wbc_inspect_batch
    hipStream_t stream = nullptr;     // (null: the context's)
    WbcPipe pipe{};                   // pipelined tick; all zero: every other launch
    int grid_wgs = 0;                 // > 0: one of the launches a large batch's WBC launch is cut into (WbcPipe::slot_base)
    bool timed = true;
};
inline MpcIO mpc_io(const int *type_id, const float *state, const float *traj, const float *gait, const float *q, float *force, float *tau, int *status)
{
    MpcIO io{};
    io.type_id = type_id; io.g_state = state; io.g_traj = traj; io.g_gait = gait; io.g_q = q; io.g_force = force; io.g_tau = tau; io.g_status = status;
    return io;
}
int launch_mpc(qrgpu_ctx *c, int n, const MpcIO &arrays, const MpcOpts &opt = MpcOpts{});                                  // qrgpu_mpc.hip
int launch_wbc(qrgpu_ctx *c, int n, const int *d_type, const float *d_state, const float *d_cmd, float *d_prev, float *d_tau, float *d_qdes, int *d_status,
               const WbcOpts &opt = WbcOpts{});                                                                            // qrgpu_api.hip
int launch_vmc(qrgpu_ctx *c, int n, const int *d_type_id, const float *d_vmc_in, const float *d_ratio, const float *d_q, float *d_force, float *d_tau,
               int *d_status);                                                                                             // qrgpu_api.hip
int upload_wbc(qrgpu_ctx *c);                              // qrgpu_api.hip: the per-type model constants on the device are those of the last qrgpu_wbc_setup
hipError_t create_side_stream(hipStream_t *s);                                                                            // qrgpu_api.hip
int lane_create(qrgpu_ctx *c, Lane &L, bool own_stream, bool masked = false);                                             // qrgpu_api.hip

// The scheduling rules that both the MPC launch and the tick decide by: one definition each.
// The lane has a plan for a batch of n: the list launches are on and its last trailing launch listed somebody (the length comes back through pinned memory).
inline bool lane_has_plan(const qrgpu_ctx *c, const Lane &L, int n)
{
    return c->planned && c->rescue && c->lpt && L.plan_n == n && L.h_pre_count[L.rescue_parity] > 0;
}
// The list the host last saw for a batch of n is more than 45 % of it: a shard in which most robots stand.
inline bool list_exceeds_45_percent(const Lane &L, int n)
{
    return L.plan_n == n && 20 * (long long)L.h_pre_count[L.rescue_parity] > 9 * (long long)n;
}
// h > 11 may run two workgroups to a CU for a batch of n: 3.5 robots per CU and more (QRGPU_H16_TWO=0: never, =2: from 64 robots on), and it needs
// the list launches -- a robot of the big class has nowhere else to go -- and the cost words that carry the plan.
inline bool h16_two_allowed(const qrgpu_ctx *c, int n)
{
    const int two = qr_env().h16_two;
    return two != 0 && n >= (two >= 2 ? 64 : 7 * c->num_cu / 2) && c->rescue && c->planned && c->lpt;
}
