// ============================================================================
// libqrgpu.so host side: the MPC launch.  Which kernel variants a call runs, on how much LDS, on which grids and streams
// (mpc_decide: no HIP call), and the launches themselves in the order the streams need them (launch_mpc and its issue steps).
// ============================================================================
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <mutex>

#include "qrgpu_ctx.h"

// One row per MpcVar (qrgpu_ctx.h), in the enum's order: the kernel, its counting build (qr_mpc_kernel_fl.hip; null: there is none and an
// instrumented launch runs the plain kernel), the threads of a workgroup, and the persistent form of a main pass.
struct MpcVariant { const void *fn, *fn_fl; int threads; MpcVar persistent; };
#define QR_MPC_BOTH(...) (const void *)qr_mpc_kernel<__VA_ARGS__>, (const void *)qr_mpc_kernel_fl<__VA_ARGS__>
static const MpcVariant mpc_variants[MPC_VAR_COUNT] = {
    /* MPC_MAIN11      */ {QR_MPC_BOTH(2, false, false, 512), 512, MPC_PERSIST11},
    /* MPC_LIST11      */ {QR_MPC_BOTH(4, true, true, 256), 256, MPC_VAR_NONE},
    /* MPC_ONE11       */ {QR_MPC_BOTH(2, true, false, 512), 512, MPC_VAR_NONE},
    /* MPC_HALF_LIST11 */ {(const void *)qr_mpc_kernel<4, true, true, 256, 2, true>, nullptr, 256, MPC_VAR_NONE},
    /* MPC_MAIN16      */ {QR_MPC_BOTH(5, true, false, 512), 512, MPC_PERSIST16},
    /* MPC_LIST16      */ {QR_MPC_BOTH(9, true, true, 256), 256, MPC_VAR_NONE},
    /* MPC_TWO16       */ {QR_MPC_BOTH(2, true, false, 512, 4, true), 512, MPC_VAR_NONE},
    /* MPC_PERSIST11   */ {(const void *)qr_mpc_persist_kernel<2, false, 512>, nullptr, 512, MPC_VAR_NONE},
    /* MPC_PERSIST16   */ {(const void *)qr_mpc_persist_kernel<5, true, 512>, nullptr, 512, MPC_VAR_NONE},
};
#undef QR_MPC_BOTH
static const void *mpc_fn(MpcVar var, bool fl) { const MpcVariant &v = mpc_variants[var]; return (fl && v.fn_fl) ? v.fn_fl : v.fn; }

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the function (per device), not to a context: the cache is process-wide and the
// limit is only ever raised, so that a second context asking for less cannot lower it under the first one's launches.
static int mpc_ensure_lds(qrgpu_ctx *c, MpcVar var, bool fl, int bytes)
{
    static std::mutex mu;
    static int configured[16][2][MPC_VAR_COUNT];          // [device][counting build][variant], zero-initialised
    std::lock_guard<std::mutex> lk(mu);
    int &have = configured[c->device & 15][fl ? 1 : 0][var];
    if (have >= bytes) return QRGPU_OK;
    HIPCHK(c, hipFuncSetAttribute(mpc_fn(var, fl), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
    return QRGPU_OK;
}

static int mpc_lds_bytes(const qrgpu_ctx *ctx, int h)
{
    // Packed inverse Hessian for the all-stance worst case plus room for S^-1; two workgroups per CU (80 KB each at h <= 11: every robot
    // fits) when that fits, otherwise the whole CU.
    const size_t fixed = mpc_lds_fixed_bytes(h, true);
    const size_t nmax = 12 * (size_t)h;
    const size_t mp = 8 * (nmax * (nmax + 1) / 2);
    const size_t want = fixed + mp + 8 * (size_t)(24 * 25 / 2);     // at least a 24-row S^-1 in the worst case
    const size_t cu = (size_t)ctx->lds_per_cu;
    return (int)(want <= cu / 2 ? cu / 2 : cu);
}

// What one launch_mpc call is going to run.  Filled by mpc_decide from the context, the lane's history and the list length the host last saw.
struct MpcPlan {
    bool inspect;                   // an inspection launch (dense H / g out): slot order, no lists, no warm start
    bool ovl, ov16;                 // part of an overlapped tick; ... at h > 11: main pass on the lane's (masked) stream, planned launch on its side stream (reserved CUs)
    bool lpt;                       // longest-first dispatch from the previous launch's per-robot cost
    bool small, tiny, two;          // h <= 11 (4 register-resident 3x3 blocks per thread cover tri(44) leg-step pairs; 9 cover h = 16); below 64 robots; h > 11 two to a CU
    bool rescue, planned;           // a trailing list launch behind the main pass; ... which plans the next call's list (needs the cost words: they carry the `big` bit)
    bool have_plan;                 // the last plan listed somebody: a planned launch beside the main pass
    bool half_lists;                // the list launches of an overlapped tick at h <= 11 run on half a CU
    MpcVar main_var, list_var, one_var;        // main pass; striding list kernel (trailing launch, long planned lists); one listed robot per eight-wave workgroup
    int lds_main, lds_list, main_grid, trail_grid;         // (main_grid: before the persistent form caps it)
    int big_nls, big_margin, big_cost, big_cost_stay;      // class and cost rules of the planned list
    // the planned launch (have_plan, or ov16 && rescue)
    bool gate;                      // the main pass waits until the listed robots' workgroups sit on their CUs (not on reserved CUs: nothing to race for)
    bool one_per_wg;                // one robot per workgroup of one_var, or list_var striding over the list
    bool poll_fork, poll_join;      // the side stream learns of this call -- and the trailing launch of the planned launch's end -- by polling a count instead of an event
    int planned_grid, planned_stride, linger;
};

// The decision step: no HIP call, and the only code that touches the lane's two_hold / two_probe.
static MpcPlan mpc_decide(const qrgpu_ctx *c, Lane &LN, int n, bool inspect, bool piped, const OvLaunch *ov)
{
    const QrEnv &env = qr_env();
    const int h = c->mpc.horizon;
    MpcPlan D{};
    D.inspect = inspect;
    D.ovl = ov != nullptr;
    D.ov16 = D.ovl && LN.masked;
    // inspection launches and tiny batches keep slot order
    D.lpt = c->lpt && n >= 64 && !inspect;
    D.small = 4 * h <= 44;
    D.lds_main = mpc_lds_bytes(c, h);
    // Batches below 64 robots (the single-robot drop-in calls among them) have a CU per robot to themselves: they run the whole-CU eight-wave
    // variant <2, BIG, ., 512> (96 working-set positions, the CU's whole LDS) as their main pass, so that nothing is left for a trailing
    // list launch -- one launch instead of two on the single-robot path, and the ping-pong parity of the rescue / planned lists, which
    // belongs to the batched calls' plan, is not touched by calls in between (a solve1 between two planned calls used to flip it and the
    // next planned call read the counters of the plan before last).
    D.tiny = D.small && n < 64 && !inspect;
    if (D.tiny) D.lds_main = c->lds_per_cu;
    // h > 11, batches of 3.5 robots per CU and more (h16_two_allowed): the main pass runs TWO workgroups per CU on half the LDS each.  A trotting
    // robot's inverse Hessian (<= 42 stance leg-steps at h = 16: <= 65 KB) fits, and its 903 blocks are two per thread of the EIGHT-wave build
    // and sweep of the h <= 11 main pass -- <2, BIG, ., 512, 4, H16>, within 128 registers (four waves leave after the sweep).  S^-1 of every
    // robot of the main pass lives in the global scratch (qcap 96 whatever the LDS holds: nobody outgrows the main pass unannounced).  On whole
    // CUs beside the main pass, one robot per eight-wave 256-register workgroup (planned list): the robots whose inverse Hessian does not fit
    // half a CU (three-leg and all-stance gaits: a class known from the gait table, 10 % of the mixed shard) and the tick's long poles --
    // robots whose smoothed cost says 450 us and more two to a CU (60-80 active rows over the spilled S^-1), which stay listed while they
    // cost 300 us and more on a whole CU.
    // Mixed h = 16 shard, one workgroup per CU -> four waves two to a CU -> eight waves two to a CU: 1.37 -> 1.45 -> 1.52 M ticks/s at 1024
    // robots, 1.45 -> 1.68 -> 1.83 M at 2048, 1.50 -> 1.76 -> 1.97 M at 8192; below 3.5 robots per CU one workgroup per CU is faster (1.28
    // against 1.18 M at 768: fewer rounds than slots).
    D.two = !D.small && h16_two_allowed(c, n) && D.lpt;
    if (D.two && !D.ov16) {                         // (ov16: qrgpu_tick_batch has decided -- an overlapped tick IS the two-to-a-CU form)
        // A shard in which most robots stand is a list, not a main pass: all stance is the class that cannot share a CU, and 1024 of them strided over by
        // the planned launch's workgroups (parked waves, three quarters of the CUs) run at 0.59 M ticks/s against 0.94 M one workgroup per CU
        // (60 % standing: 1.16 against 1.29 M; 30 %: 1.96 against 1.56 M; scratch/ab_h16_stand.py).  So when the list the host last saw is more
        // than 45 % of the batch the calls go back to one workgroup per CU for QRGPU_H16_TWO_HOLD calls; nobody plans meanwhile, so the call after
        // them runs two to a CU whatever the old count says (on the old plan: consistent, if stale) and the one after that decides on the fresh count.
        if (LN.two_hold > 0) { --LN.two_hold; D.two = false; }
        else if (LN.two_probe) LN.two_probe = false;
        else if (env.h16_two_hold > 0 && list_exceeds_45_percent(LN, n)) { LN.two_hold = env.h16_two_hold; LN.two_probe = true; D.two = false; }
    }
    if (D.two) D.lds_main = (c->lds_per_cu / 2) & ~15;
    // rescue pass: not for inspection launches or tiny batches (and the whole-CU h > 11 variant holds 96 rows itself)
    D.rescue = c->rescue && !inspect && (D.small || D.two) && !D.tiny;
    D.planned = c->planned && D.rescue && D.lpt;
    D.big_nls = c->big_nls;
    if (D.two) {
        // the class that cannot be solved on half a CU: stance leg-steps whose block-packed inverse Hessian does not fit the main pass's LDS
        const long long room = (long long)D.lds_main - (long long)mpc_lds_fixed_bytes(h, true);
        int k = 1;
        while (k <= 4 * h && (long long)k * (k + 1) / 2 * 72 <= room) ++k;
        if (k > 45) k = 45;                 // (and the eight-wave kernel holds two blocks per thread: 1024 >= tri(44))
        if (D.big_nls <= 0 || D.big_nls > k) D.big_nls = k;        // (a caller's own, stricter class rule stands: qrgpu_set_planned_list)
        // the long poles: a robot whose solve takes most of the tick's span two to a CU (a large working set over the spilled S^-1: 600-800 us
        // against a mean of 200) is planned onto a whole CU, and stays there while its solve costs more than QRGPU_H16_BIG_STAY_US there
        D.big_cost = (int)((long long)env.h16_big_us * 2250 / 256); D.big_cost_stay = (int)((long long)env.h16_big_stay_us * 2250 / 256);
    }
    D.big_margin = D.two ? -1000 : 6;
    D.main_var = D.tiny ? MPC_ONE11 : (D.small ? MPC_MAIN11 : (D.two ? MPC_TWO16 : MPC_MAIN16));
    // Overlapped ticks (h <= 11): the machine is never empty -- a workgroup that asks for a whole CU's LDS waits until both halves of some CU
    // happen to be free at once, behind every half-CU workgroup of the next tick's main pass and every WBC workgroup.  So the list launches of
    // an overlapped tick run on HALF a CU like the main pass, with S^-1 (96 rows) in the global scratch: MPC_HALF_LIST11 striding and
    // MPC_TWO16 one robot per workgroup (the two-to-a-CU main pass of h > 11).
    // A tick whose lane has a PLAN is not chained (qrgpu_tick_batch): it starts on an empty machine, and its planned launch is the whole-CU one.
    D.half_lists = D.small && D.ovl && !ov->plan_tick;
    D.list_var = D.small ? (D.half_lists ? MPC_HALF_LIST11 : MPC_LIST11) : MPC_LIST16;
    D.one_var = D.small ? (D.half_lists ? MPC_TWO16 : MPC_ONE11) : MPC_MAIN16;
    D.lds_list = D.half_lists ? D.lds_main : c->lds_per_cu;
    D.main_grid = 8 * ((n + 7) / 8);
    // the planned launch (and its two stream events) is only worth issuing when the last plan listed somebody: the list's length comes back
    // through pinned memory without a sync.  A stale zero just means the main pass solves everybody (MpcLaunch::skip stays null): consistent either way.
    D.have_plan = D.planned && lane_has_plan(c, LN, n);
    if (D.have_plan || (D.ov16 && D.rescue)) {
        const int listed = D.have_plan ? LN.h_pre_count[LN.rescue_parity] : 0;
        D.gate = !D.ov16;
        // a striding launch over a list of the all-stance twentieth of a batch gets a workgroup per robot
        const int pgrid = n / 16 < 16 ? 16 : (n / 16 > c->num_cu ? c->num_cu : n / 16);
        // (big batches -- hundreds of listed robots at 8192 per launch -- stay on the striding kernel: one workgroup per robot would take every CU
        // from the main pass, and a stale short count would send most of the list to the trailing launch: 4.54 against 4.72 M ticks/s)
        // (h > 11 two to a CU: always the whole-CU kernel, on at most three quarters of the CUs -- a longer list is strided over, MpcLaunch::planned_stride)
        // (... unless most of the batch is listed -- a shard of standing robots: then the list is the launch, and it gets every CU)
        const int g3_cap = D.ov16 ? c->ov16_side_cus : ((D.two && 2 * listed <= n) ? 3 * c->num_cu / 4 : c->num_cu);
        D.one_per_wg = D.two || (n <= 2048 && listed <= (D.small ? c->num_cu / 4 : 3 * c->num_cu / 4));
        // How the side stream learns that the context's stream has reached this call.  An event (QRGPU_PLANNED_FORK=1, and always for the
        // striding kernel and the ungated forms) costs ~10 us before the listed workgroups even launch -- 20 us between a tick's trailing launch and
        // the first workgroup of the next main pass on ticks that have a plan, against 2 on ticks that have none (the kernels' stamps).  Instead: a
        // one-thread launch on the side stream polls a "go" count that the gate in front of the main pass -- a launch on the context's stream --
        // bumps before it waits for the listed workgroups.  Bounded (50 ms, QRGPU_PLAN_GO_MS); a gate that gives up calls the plan off for
        // this call (MpcLaunch::plan_abort): nobody runs on inputs the caller's stream has not produced yet.
        D.poll_fork = !env.planned_fork && D.gate && D.one_per_wg;
        // ... and, in a pipelined tick, how the trailing launch learns that the planned launch is through (MpcLaunch::planned_done)
        D.poll_join = D.poll_fork && piped;
        // grid of the one-robot-per-workgroup launch: the list's length as the host last saw it, plus two
        // (h > 11 two to a CU: the cost rule's share of the list comes and goes with the robots' smoothed costs, a dozen entries a tick -- and a
        //  robot handed to the trailing launch is a whole solve BEHIND the main pass: 1.10 M ticks/s with eight spare workgroups, 1.43 M with 24 or 48)
        int g3 = listed + (D.two ? 24 : 2);
        D.planned_stride = D.ov16 ? (D.have_plan ? 1 : 2) : ((D.two && g3 > g3_cap) ? 1 : 0);      // (2: no list, rescue only)
        g3 = g3 < 1 ? 1 : (g3 > g3_cap ? g3_cap : g3);
        // (how many of its workgroups stay for the hand-overs: all of them while there is no plan -- the whole big class arrives unannounced --
        //  then a few: one or two robots a tick change class, and a workgroup that stays keeps its CU from the next tick's planned launch)
        // (measured on the default configs[4] run, twice each: 16 stay 1.686 M ticks/s, 8: 1.698, 4: 1.715, 2: 1.720, 1: 1.729; four is what is
        //  left of the margin for a tick in which a handful of robots change class at once)
        D.linger = D.ov16 ? (D.have_plan ? (4 < g3_cap ? 4 : g3_cap) : g3_cap) : 0;
        // (QRGPU_OV_FAULT=2, the give-up test of MpcLaunch::main_done: nobody stays, as if every lingering workgroup had run into its bound -- a robot the
        //  main pass hands on afterwards is solved by nobody in that tick, and must carry QRGPU_ST_PIPE_TIMEOUT)
        if (env.ov_fault == 2) D.linger = 0;
        if (D.ov16) g3 = g3_cap;                       // (the reserved CUs are this launch's whatever the list's length: it is also the tick's rescuer)
        D.planned_grid = D.one_per_wg ? g3 : pgrid;
    }
    // (the trailing launch: a grid growing with the batch was tried -- workgroups that ask for a whole CU's LDS are dispatched one every ~2 us,
    //  0.55 ms for an empty pass at 4096 robots; chained ticks: every workgroup of this launch waits for a freed half CU)
    D.trail_grid = (D.half_lists || (D.ov16 && D.rescue)) ? 16 : (64 < n ? 64 : n);
    if (D.trail_grid < 8 && D.lpt) D.trail_grid = 8;
    return D;
}

// One launch_mpc call on its way through the issue steps.
struct MpcCall {
    qrgpu_ctx *c; Lane &LN; int n; bool piped; const OvLaunch *ov;
    MpcPlan D;
    MpcLaunch P;           // the main pass's parameters; the list launches start from a copy
    MpcIO io;
    bool instrumented;     // the kernels with counters, dense H / g and cycle stamps compiled in: only for a launch that asks for one of those
    int *cost_out; int *order_next;
    int main_grid; const void *main_fn;
};

// The parameters every launch of the call shares (and the main pass uses as they are), with the memsets a new batch size needs.
static int mpc_fill_params(MpcCall &M, int epilogue)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D; const int n = M.n; const OvLaunch *ov = M.ov;
    MpcLaunch &P = M.P;
    P = c->mpc;                                    // (horizon, types, Hessian mode; everything a launch sets is zero there)
    P.n = n;
    P.type_ready = ready_mask(c->mpc_ready);
    P.epilogue = epilogue;
    // pipelined tick: the solves raise per-robot flags for the WBC launch that runs beside them (qrgpu_tick_batch)
    P.done_flag = M.piped ? LN.d_done_flag : nullptr;
    P.done_epoch = c->tick_epoch;
    // overlapped tick: per-robot hand-over of the warm-start and cost words between consecutive ticks (MpcLaunch::solved)
    if (!D.ovl) { c->ov_chain = false; c->cost_n[0] = c->cost_n[1] = 0; }      // (any other MPC launch: the next overlapped tick waits for the context's stream)
    M.cost_out = c->d_cost[D.ovl ? (ov->epoch & 1u) : 0];
    const int *const cost_prev = D.ovl ? c->d_cost[(ov->epoch & 1u) ^ 1u] : M.cost_out;
    P.solved = D.ovl ? c->d_solved : nullptr; P.solved_epoch = D.ovl ? ov->epoch : 0u;
    P.prev_solved = (D.ovl && ov->chained) ? c->d_solved : nullptr; P.prev_epoch = D.ovl ? ov->prev_epoch : 0u;
    P.xtick_wait = qr_env().ov_wait_ticks;
    P.main_started = M.piped ? c->d_main_started : nullptr;
    P.tl = M.piped ? c->d_timeline : nullptr;
    P.ftime = (M.piped && c->d_tlr) ? c->d_ftime : nullptr;
    P.wbc_order_out = nullptr;                     // (constant: nobody sorts a WBC order any more, LAB_NOTES A.1)
    P.flops = (c->flops_on && !D.inspect) ? c->d_flops : nullptr;
    if (P.flops) c->flops_n = n;
    // warm start from the slot's previous solve: not for inspection launches; a different batch size starts from nothing
    P.warm = (c->warm && !D.inspect) ? c->d_warm : nullptr;
    if (P.warm && c->warm_n != n) {
        HIPCHK(c, hipMemsetAsync(c->d_warm, 0, (size_t)QR_WARM_STRIDE * (size_t)n, LN.stream));
        c->warm_n = n;
    }
    P.lds_bytes = D.lds_main;
    // (the order is two arrays: this tick's trailing launch sorts the next one into the half this tick's launches -- the chunked WBC launches of a large
    //  batch among them, WbcPipe::slot_base -- do not read)
    M.order_next = LN.d_order + (size_t)(LN.order_parity ^ 1) * (size_t)c->max_batch;
    P.order = (D.lpt && LN.lpt_n == n) ? LN.d_order + (size_t)LN.order_parity * (size_t)c->max_batch : nullptr;
    LN.order_used = P.order;
    P.cost = D.lpt ? M.cost_out : nullptr;
    P.cost_in = cost_prev;
    P.cost_ema = (D.lpt && (D.ovl ? c->cost_n[(ov->epoch & 1u) ^ 1u] == n : LN.lpt_n == n)) ? 1 : 0;      // (smoothed whenever there is a previous cost: no switch any more)
    if (D.ovl) c->cost_n[ov->epoch & 1u] = D.lpt ? n : 0;
    if (!D.small || D.ovl) {            // (overlapped ticks at h <= 11: the list launches run on half a CU with S^-1 in this scratch)
        if (!c->d_sinv_spill) HIPCHK(c, hipMalloc(&c->d_sinv_spill, sizeof(double) * (size_t)c->max_batch * (size_t)(QR_QH * (QR_QH + 1) / 2)));
        if (!D.small) P.sinv_spill = c->d_sinv_spill;
    }
    P.rescue_count = D.rescue ? LN.d_rescue : nullptr;
    P.rescue_list = D.rescue ? LN.d_rescue + 2 : nullptr;
    P.rescue_parity = LN.rescue_parity;
    // rows enter the next tick's guess only when their multiplier exceeds 2 % of the solve's largest (weakly held rows are the ones that do
    // not persist: measured 0.2446 -> 0.2211 ms per launch at h = 10, neutral at h = 5; at h = 16, where a missing row costs 7-13 k cycles
    // to add, every threshold measured worse, so none is applied there)
    P.warm_uthr = D.small ? 0.02 : 0.0;
    P.no_block_drop = 0;                           // (constant)
    P.no_wcache = 0;                               // (constant)
    P.pre_count = D.planned ? LN.d_pre : nullptr;
    // (h > 11 overlapped: the list is two lists, by the parity the counters ping-pong on -- MpcLaunch::pre_list_next)
    P.pre_list = D.planned ? LN.d_pre + 4 + ((D.ov16 && LN.rescue_parity) ? c->max_batch : 0) : nullptr;
    P.pre_list_next = D.ov16 ? (LN.rescue_parity ? -c->max_batch : c->max_batch) : 0;
    P.pre_hint = D.planned ? LN.d_pre_hint : nullptr;
    P.big_nls = D.big_nls; P.big_margin = D.big_margin;
    P.big_cost = D.big_cost; P.big_cost_stay = D.big_cost_stay;
    P.lds_main = P.lds_bytes;
    if (D.planned && LN.plan_n != n) {               // no plan for this batch size yet: nothing is skipped, both counters start at zero
        HIPCHK(c, hipMemsetAsync(LN.d_pre, 0, 4 * sizeof(int), LN.stream));
        HIPCHK(c, hipMemsetAsync(LN.d_skip, 0, (size_t)n, LN.stream));
        // ... and the first two calls (one per parity) end with a stream sync: mpc_finish
        LN.h_pre_count[0] = LN.h_pre_count[1] = 0; LN.plan_sync_left = 2;
    }
    return QRGPU_OK;
}

// Persistent main pass (qr_device_types.h): when the batch is more than the machine holds at once, launch one workgroup per resident slot
// and let them take robots off per-XCD queues.  Default (QRGPU_PERSIST=1): the h > 11 variant only -- 1.31 -> 1.37 M ticks/s on the mixed
// h = 16 shard.  At h <= 11 (QRGPU_PERSIST=2 to try) it loses what it gains and more: the four waves a solve no longer needs after its sweep
// cannot leave a workgroup that has another robot to solve, they have to cross every barrier of the active set with the working ones
// (a live wave counts at s_barrier), and a parked wave's wake-up, look at the exit word and return to the barrier is on the critical
// path of each of the two hundred barriers of a solve: main pass 0.208 -> 0.231 ms at 1024 robots, 1.39 -> 1.46 ms at 8192.
// QRGPU_PERSIST=0: one workgroup per robot everywhere, dispatched by the hardware in launch order.
static int mpc_configure_main(MpcCall &M)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D; MpcLaunch &P = M.P;
    const bool fl = M.instrumented;
    { const int rc_ = mpc_ensure_lds(c, D.main_var, fl, P.lds_bytes); if (rc_) return rc_; }
    if (D.rescue) { const int rc_ = mpc_ensure_lds(c, D.list_var, fl, D.lds_list); if (rc_) return rc_; }
    M.main_grid = D.main_grid;
    M.main_fn = mpc_fn(D.main_var, fl);
    const int persist_on = qr_env().persist;
    const MpcVar pvar = mpc_variants[D.main_var].persistent;
    if (!persist_on || fl || pvar == MPC_VAR_NONE || (D.main_var == MPC_MAIN11 && persist_on < 2)) return QRGPU_OK;
    { const int rc_ = mpc_ensure_lds(c, pvar, false, P.lds_bytes); if (rc_) return rc_; }
    if (c->main_slots[pvar] == 0 || c->main_slots_lds[pvar] != P.lds_bytes) {
        int nb = 0;
        HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, mpc_fn(pvar, false), mpc_variants[pvar].threads, (size_t)P.lds_bytes));
        c->main_slots[pvar] = nb > 0 ? nb : 1; c->main_slots_lds[pvar] = P.lds_bytes;
    }
    const int slots = 8 * ((c->main_slots[pvar] * c->num_cu + 7) / 8);
    if (M.main_grid > slots) {
        P.persist = 1;
        P.qhead = LN.d_qhead + 8 * LN.qhead_parity; P.qhead_next = LN.d_qhead + 8 * (LN.qhead_parity ^ 1);
        LN.qhead_parity ^= 1;
        M.main_grid = slots;
        M.main_fn = mpc_fn(pvar, false);
    }
    return QRGPU_OK;
}

// The planned launch beside the main pass, with its fork and its gates: whole CU's LDS, 96 positions, workgroup b takes entries b, b + grid, ...
// of the list the last call's planning left.
static int mpc_issue_planned(MpcCall &M)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D; MpcLaunch &P = M.P; const OvLaunch *ov = M.ov;
    const bool fl = M.instrumented;
    P.skip = D.have_plan ? LN.d_skip : nullptr;
    MpcLaunch L = P;
    L.persist = 0; L.qhead = nullptr; L.qhead_next = nullptr;
    L.rescue_mode = 2; L.order = nullptr; L.rescue_count = nullptr; L.rescue_list = nullptr;
    L.lds_bytes = D.lds_list;
    L.sinv_spill = c->d_sinv_spill;               // (null at h <= 11; the whole-CU kernels of h > 11 put S^-1 there when an all-stance robot's M leaves no room)
    L.started = (D.gate || D.ov16) ? LN.d_started : nullptr;
    L.planned_stride = D.planned_stride;
    LN.last_linger = D.linger;
    L.linger = D.linger;
    const int g3 = D.planned_grid;                 // (of the one-robot-per-workgroup form)
    bool main_gate_queued = false;
    if (D.poll_fork) {
        ++LN.go_total;
        if (++LN.plan_epoch >= 0x7fffffff) LN.plan_epoch = 1;
        // (the give-up word is a ring indexed by the plan epoch: two planned ticks queued behind a backlog longer than twice the bound must not
        //  overwrite each other's word before their own kernels have read it)
        int *const abort_word = LN.d_go + 1 + (LN.plan_epoch & (QR_ABORT_RING - 1));
        P.plan_abort = abort_word; P.plan_epoch = LN.plan_epoch; L.plan_abort = P.plan_abort; L.plan_epoch = P.plan_epoch;
        // The gate in front of the main pass -- it gives the "go" -- is queued BEFORE the launch that polls for it: should the two streams
        // ever share a hardware queue (more streams in the process than the device has queues), a poller queued in front of what it polls for
        // would sit out its whole bound; this way round the worst case is the 30 us of the main pass's own gate.
        LN.started_total += g3;
        hipLaunchKernelGGL(qr_gate_kernel, dim3(1), dim3(64), 0, LN.stream, LN.d_started, LN.started_total, (long long)3000, (int *)nullptr, 0, LN.d_go);
        HIPCHK(c, hipGetLastError());
        main_gate_queued = true;
        hipLaunchKernelGGL(qr_gate_kernel, dim3(1), dim3(64), 0, LN.side_stream, LN.d_go, LN.go_total, qr_env().plan_go_ticks, abort_word, LN.plan_epoch, (int *)nullptr);
        HIPCHK(c, hipGetLastError());
    } else {
        // (h > 11 overlapped: the lane's previous planned launch is through before anything of this tick runs -- it normally ended a tick ago, the tick's
        //  join having waited for the WBC workgroups of its robots; but a WBC workgroup that GAVE UP on a robot lets the join pass while the robot's
        //  solve is still going, and this tick's main pass clears the counters that launch's workgroups take their work from.  Found by fault injection:
        //  tests/test_gpu_overlap.py::test_h16_hand_overs_nobody_takes_are_never_silent)
        if (D.ov16 && LN.join_recorded) HIPCHK(c, hipStreamWaitEvent(LN.stream, LN.ev_join, 0));
        HIPCHK(c, hipEventRecord(LN.ev_fork, LN.stream));
        HIPCHK(c, hipStreamWaitEvent(LN.side_stream, LN.ev_fork, 0));
        if (D.ov16 && ov->chained && ov->prev_started) {
            // This tick's planned workgroups share the reserved CUs with its predecessor's, and each waits -- per robot -- for that robot's previous
            // solve: not one of them may start before EVERY planned workgroup of the predecessor has (a waiting workgroup holds its CU; one that
            // waits for a robot in the share of a workgroup that cannot start for lack of a CU never sees it: 144 robots timed out a tick, 5.8 ms).
            hipLaunchKernelGGL(qr_gate_kernel, dim3(1), dim3(64), 0, LN.side_stream, ov->prev_started, (int)ov->prev_started_total, (long long)5000000, (int *)nullptr, 0,
                               (int *)nullptr);
            HIPCHK(c, hipGetLastError());
        }
    }
    int gate_expect = 0;
    void *largs[2] = {(void *)&L, (void *)&M.io};
    if (D.one_per_wg) {
        // one robot per workgroup of the eight-wave whole-CU kernel; the grid is the list's length as the host last saw it (the kernel
        // hands a longer list's tail to the trailing launch)
        L.rescue_mode = 3; L.rescue_count = P.rescue_count; L.rescue_list = P.rescue_list;
        { const int rc_ = mpc_ensure_lds(c, D.one_var, fl, D.lds_list); if (rc_) return rc_; }
        if (D.poll_join) { LN.planned_done_total += g3; L.planned_done = LN.d_planned_done; }       // (every workgroup of the launch bumps it once)
        HIPCHK(c, hipExtLaunchKernel(mpc_fn(D.one_var, fl), dim3(g3), dim3(mpc_variants[D.one_var].threads), largs, (size_t)L.lds_bytes, LN.side_stream, nullptr, nullptr, 0));
        gate_expect = g3;
        if (!main_gate_queued) LN.started_total += g3;               // every workgroup of this launch bumps the counter once, sooner or later
    } else {
        L.started = nullptr;                  // (a long list on the striding kernel competes with the main pass as before: gating it would starve the main pass)
        HIPCHK(c, hipExtLaunchKernel(mpc_fn(D.list_var, fl), dim3(D.planned_grid), dim3(mpc_variants[D.list_var].threads), largs, (size_t)L.lds_bytes, LN.side_stream, nullptr,
                                     nullptr, 0));
    }
    HIPCHK(c, hipGetLastError());
    if (!D.poll_join) { HIPCHK(c, hipEventRecord(LN.ev_join, LN.side_stream)); LN.join_recorded = true; }
    // the main pass waits (at most 30 us) until the listed robots' workgroups sit on their CUs
    if (D.gate && gate_expect > 0 && !main_gate_queued) {
        hipLaunchKernelGGL(qr_gate_kernel, dim3(1), dim3(64), 0, LN.stream, LN.d_started, LN.started_total, (long long)3000, (int *)nullptr, 0, (int *)nullptr);
        HIPCHK(c, hipGetLastError());
    }
    return QRGPU_OK;
}

static int mpc_issue_main(MpcCall &M)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D;
    {
        TimerScope ts(c, 0, LN.stream);
        void *kargs[2] = {(void *)&M.P, (void *)&M.io};
        HIPCHK(c, hipExtLaunchKernel(M.main_fn, dim3(M.main_grid), dim3(mpc_variants[D.main_var].threads), kargs, (size_t)M.P.lds_bytes, LN.stream, nullptr, nullptr, 0));
    }
    HIPCHK(c, hipGetLastError());
    if (D.have_plan && !D.poll_join && !D.ov16) HIPCHK(c, hipStreamWaitEvent(LN.stream, LN.ev_join, 0));
    return QRGPU_OK;
}

// The trailing list launch: the robots whose working set outgrew the main pass (normally none: the workgroups sort the next call's dispatch
// order, plan its list and exit) are re-solved with the whole CU's LDS and 96 working-set positions.
// (h > 11 overlapped: it only sorts and plans -- eight small workgroups on the lane's stream, MpcLaunch::plan_only -- and the tick's planned
//  launch takes the robots the main pass hands on, MpcLaunch::main_done.  A whole-CU trailing launch on the reserved CUs was measured first: it
//  queues behind the NEXT tick's planned workgroups, 200-350 us instead of 8 -- and those may be waiting for the very robot it has yet to solve.)
static int mpc_issue_trailing(MpcCall &M)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D;
    const bool plan_only = D.ov16;
    MpcLaunch R = M.P;
    R.persist = 0; R.qhead = nullptr; R.qhead_next = nullptr;
    R.planned_done = D.poll_join ? LN.d_planned_done : nullptr; R.planned_expect = LN.planned_done_total;
    R.rescue_mode = 1; R.order = nullptr; R.cost = nullptr;
    // (its robots go to the WBC pass queued behind it, not to the one running beside the main pass -- except in an overlapped tick, which has no
    //  second pass: there the robot's WBC workgroup waits for the flag this launch raises, WbcPipe::wait_list)
    R.done_flag = D.ovl ? LN.d_done_flag : nullptr; R.main_started = nullptr;
    R.skip = D.planned ? LN.d_skip : nullptr;          // (written by the planning workgroups; only the main pass reads it)
    R.lpt_cost_in = D.lpt ? M.cost_out : nullptr; R.lpt_order_out = D.lpt ? M.order_next : nullptr;
    R.lds_bytes = plan_only ? 16384 : D.lds_list;      // (plan_only: the sort's histogram; MpcLaunch::lds_main still says what the main pass holds)
    R.sinv_spill = c->d_sinv_spill;
    R.plan_only = plan_only ? 1 : 0;
    R.main_done = nullptr; R.rescue_taken = nullptr;
    MpcIO io = M.io;
    io.dbgH = nullptr; io.dbgG = nullptr; io.dbgT = nullptr;
    void *rargs[2] = {(void *)&R, (void *)&io};
    HIPCHK(c, hipExtLaunchKernel(mpc_fn(D.list_var, M.instrumented), dim3(D.trail_grid), dim3(mpc_variants[D.list_var].threads), rargs, (size_t)R.lds_bytes, LN.stream, nullptr,
                                 nullptr, 0));
    HIPCHK(c, hipGetLastError());
    // (the length of the list just planned reaches h_pre_count by itself).  A trailing launch that does not plan still flips the parity the
    // counters ping-pong on: whatever plan there was now sits under the wrong parity and is forgotten (the next planned call starts afresh)
    LN.plan_n = D.planned ? M.n : 0;
    LN.last_rescue_parity = LN.rescue_parity;
    LN.rescue_parity ^= 1;
    return QRGPU_OK;
}

// What the call leaves for the next one: the dispatch order (sorted by workgroups 0-7 of the trailing launch, or by a launch of its own), the
// counts a pipelined tick's gates poll, and -- after a history reset -- a stream sync.
static int mpc_finish(MpcCall &M)
{
    qrgpu_ctx *c = M.c; Lane &LN = M.LN; const MpcPlan &D = M.D; const int n = M.n;
    LN.last_rescue_active = D.rescue;
    c->last_main_persist = M.P.persist != 0;
    if (M.piped) c->main_started_total += M.P.persist ? n : (int)(8 * ((n + 7) / 8));      // (persistent: one count per robot taken off a queue)
    if (D.lpt && !D.rescue) {
        hipLaunchKernelGGL(qr_lpt_order_kernel, dim3(8), dim3(256), 0, LN.stream, n, M.cost_out, M.order_next, (const int *)M.P.ftime, (int *)nullptr);
        HIPCHK(c, hipGetLastError());
    }
    if (D.lpt) { LN.lpt_n = n; LN.order_parity ^= 1; }
    // The list's length reaches the host through pinned memory, unsynchronised: a caller that queues ticks faster than the GPU runs them
    // decides on a count several ticks old -- and on nothing at all for the first ticks of a new batch, whose listed robots then go through
    // the trailing launch, serially behind the main pass (a 20-step run lost a quarter of its rate on populations with an all-stance robot).
    // The first two calls after a history reset (one per parity) therefore end with a stream sync.
    // (Not while the stream is being captured into a graph: a sync is illegal there, and a replayed graph has a fixed launch shape anyway.)
    if (D.planned && LN.plan_sync_left > 0) {
        --LN.plan_sync_left;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(LN.stream, &cap) != hipSuccess) { cap = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
        if (cap == hipStreamCaptureStatusNone) HIPCHK(c, hipStreamSynchronize(LN.stream));
    }
    return QRGPU_OK;
}

int launch_mpc(qrgpu_ctx *c, int n, const MpcIO &arrays, const MpcOpts &opt)
{
    if (!c || n <= 0 || n > c->max_batch || !arrays.g_state || !arrays.g_traj || !arrays.g_gait || !arrays.g_force) return QRGPU_ERR_BAD_ARG;
    if (arrays.g_tau && !arrays.g_q) return QRGPU_ERR_BAD_ARG;
    // without a type array every robot is type 0; with one, the kernel flags robots whose type was never set up (QRGPU_ST_BAD_TYPE)
    if (!(arrays.type_id ? ready_mask(c->mpc_ready) != 0 : c->mpc_ready[0])) return QRGPU_ERR_NOT_SETUP;
    HIPCHK(c, hipSetDevice(c->device));
    Lane &LN = c->lane[opt.lane_id];
    const bool inspect = arrays.dbgH != nullptr;
    const bool fl = (c->flops_on && !inspect && c->d_flops) || arrays.dbgH != nullptr || arrays.dbgG != nullptr || c->d_dbg_cycles != nullptr;
    MpcCall M{c, LN, n, opt.piped, opt.ov, mpc_decide(c, LN, n, inspect, opt.piped, opt.ov), MpcLaunch{}, arrays, fl, nullptr, nullptr, 0, nullptr};
    M.io.force_stride = 51; M.io.dbgT = (long long *)c->d_dbg_cycles;
    const MpcPlan &D = M.D;
    int rc = mpc_fill_params(M, opt.epilogue);
    if (!rc) rc = mpc_configure_main(M);
    if (rc) return rc;
    if (D.ov16 && D.rescue) {
        // (h > 11 overlapped: the planned launch is also the tick's rescuer, plan or no plan -- MpcLaunch::main_done)
        LN.main_done_total += M.main_grid;
        M.P.main_done = LN.d_main_done; M.P.main_done_expect = LN.main_done_total; M.P.rescue_taken = LN.d_rescue_taken;
    }
    if (D.have_plan || (D.ov16 && D.rescue)) rc = mpc_issue_planned(M);
    if (!rc) rc = mpc_issue_main(M);
    if (!rc && D.rescue) rc = mpc_issue_trailing(M);
    if (!rc) rc = mpc_finish(M);
    return rc;
}
