"""-m gpu: the tick on the reference's cadence (qrgpu_tick_cadence_batch): per robot either the MPC or the WBC, from a device mask.

Inputs: the workload generator's trotting populations with mixed contact tables (5 % all stance, 5 % three-leg).  Every output array starts at a
poison pattern.  Base shape A1, h = 10, n = 70: the longest-first order, the trailing launch and the planned launch are live, and 70 is no multiple
of 8.  Every case runs twice in a row on the same context: the second call runs on a sorted order, a plan and a warm start.

What a DUE robot must carry is what qrgpu_mpc_solve_batch gives it on a fresh context with the same torque epilogue, call for call, bit for bit
(force, torque, status word); its kept force d_hold is -R^T f within the bar below; the WBC has not touched it (d_prev_ori as put in, d_qdes poison).
What a HELD robot must carry: d_force and d_hold as put in, bit for bit; the stance-leg torques, d_qdes and d_prev_ori of qrgpu_wbc_run_batch fed the
same Fr_des, call for call, bit for bit (clipped where the epilogue clips: the clip is exact); the swing-leg torques J(q)^T d_hold of
tests/cadence_ref.py, with +-0.9 on the abad and the clip where the epilogue says so, within the bar; the WBC's status word with an MPC part of 0
and an iteration count of 0.  A robot's result does not depend on who else is due: the same two references serve every mask.

The bar (DESIGN 4.6, rows behind transcendental functions): 8 x the gap between cadence_ref evaluated in float32 and in float64 on the same
inputs, never under 2e-6, relative to max(1, |value|).  Measured on the n = 70 base shape: see DESIGN 4.6."""
import numpy as np
import pytest

import cadence_ref as R
import gpu_helpers as G

pytestmark = pytest.mark.gpu

POISON_F, POISON_I = np.float32(-12345.5), 0x7f0000ff
BOTH = R.EPILOGUE_HIP_COMP | R.EPILOGUE_CLIP


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one shape: its inputs and its two references, computed once and shared
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _batch(pkg, n, h, mixed):
    if not mixed:
        b = pkg.make_batch(n, h, "a1", seed=0xCAD + n + h)
        return b, None, np.tile(np.asarray(pkg.model_desc("a1")[:3], np.float64), (n, 1))
    ba, bl = pkg.make_batch(n, h, "a1", seed=0xCAD + n), pkg.make_batch(n, h, "lite3", seed=0xCAE + n)
    tid = (np.arange(n) % 3 == 1).astype(np.int32)
    b = dict(ba)
    for k in ("mpc_state", "traj", "gait", "fb_state", "wbc_cmd", "prev_ori_vel"):
        b[k] = np.where(tid.reshape((n,) + (1,) * (ba[k].ndim - 1)) == 1, bl[k], ba[k])
    legs = np.where(tid[:, None] == 1, np.asarray(pkg.model_desc("lite3")[:3], np.float64), np.asarray(pkg.model_desc("a1")[:3], np.float64))
    return b, tid, legs


def _ctx(pkg, h, n, epilogue, mixed, cold=False):
    ctx = pkg.Context(0, max(n, 64), 16)
    G.setup_a1(ctx, pkg, h)
    if mixed:
        ctx.mpc_setup_packed(1, pkg.mpc_cfg("lite3"), h); ctx.wbc_setup_packed(1, pkg.model_desc("lite3"))
    ctx.set_torque_epilogue(hip_comp=bool(epilogue & 1), clip=bool(epilogue & 2))
    if cold:
        ctx.set_warm_start(False); ctx.set_planned_list(False)
    return ctx


class _Arrays:
    """The device arrays of one shape on one context: inputs uploaded once, outputs poisoned on request."""

    def __init__(self, ctx, pkg, b, tid):
        n, h, S = b["n"], b["horizon"], pkg.to_soa
        self.ctx, self.n = ctx, n
        self.d = dict(state=ctx.alloc((28, n)).upload(S(b["mpc_state"])), traj=ctx.alloc((12 * h, n)).upload(S(b["traj"])), gait=ctx.alloc((4 * h, n)).upload(S(b["gait"])),
                      fb=ctx.alloc((37, n)).upload(S(b["fb_state"])), cmd=ctx.alloc((67, n)).upload(S(b["wbc_cmd"])), prev=ctx.alloc((3, n)), force=ctx.alloc((12, n)),
                      hold=ctx.alloc((12, n)), tau=ctx.alloc((12, n)), qdes=ctx.alloc((24, n)), status=ctx.alloc((n,), np.int32), due=ctx.alloc((n,), np.int32))
        self.tid = ctx.alloc((n,), np.int32).upload(tid) if tid is not None else None

    def poison(self):
        n, d = self.n, self.d
        d["tau"].upload(np.full((12, n), POISON_F, np.float32)); d["qdes"].upload(np.full((24, n), POISON_F, np.float32))
        d["status"].upload(np.full((n,), POISON_I, np.int32))

    def get(self, *names):
        self.ctx.sync()
        return {k: (self.d[k].download() if k in ("status", "due") else self.d[k].download().T.copy()) for k in names}

    def free(self):
        for v in self.d.values():
            v.free()
        if self.tid is not None:
            self.tid.free()


_SHAPES = {}


def _shape(pkg, n, h, epilogue, mixed=False):
    """-> dict: the batch, the memory put in, and per call (two calls) what a due robot and what a held robot must carry."""
    key = (n, h, epilogue, mixed)
    if key in _SHAPES:
        return _SHAPES[key]
    b, tid, legs = _batch(pkg, n, h, mixed)
    rng = np.random.default_rng(7 * n + h)
    prev_in = rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)
    # all due: qrgpu_mpc_solve_batch on a fresh context with the same epilogue, twice
    ctx = _ctx(pkg, h, n, epilogue, mixed)
    A = _Arrays(ctx, pkg, b, tid)
    due = []
    for _ in range(2):
        A.poison(); A.d["force"].upload(np.full((12, n), POISON_F, np.float32))
        ctx.mpc_solve_batch(n, A.d["state"], A.d["traj"], A.d["gait"], A.d["fb"].row(13), A.d["force"], A.d["tau"], A.d["status"], A.tid)
        due.append(A.get("force", "tau", "status"))
    A.free(); ctx.close()
    # the memory every case starts from: the forces of the first solve, and their kept form by the restatement -- with a force on the legs that swing
    # now as well, as a leg that stood at the robot's last solve has it: those are the legs on which a held tick's J(q)^T d_hold reaches the motors
    force_in = due[0]["force"].copy()
    quat = b["mpc_state"][:, 6:10]
    stance = np.repeat(b["wbc_cmd"][:, 63:67] != 0, 3, axis=1)                         # [n][12]
    stood = np.where(stance, force_in, rng.uniform(-1.0, 1.0, (n, 12)).astype(np.float32) * np.tile(np.float32([15, 15, 60]), 4))
    hold_in = R.hold_from_force(quat, stood).astype(np.float32)
    # none due: qrgpu_wbc_run_batch on a fresh context fed the same Fr_des, twice on the same orientation memory
    ctx = _ctx(pkg, h, n, epilogue, mixed)
    cmd = b["wbc_cmd"].copy(); cmd[:, 51:63] = force_in
    A = _Arrays(ctx, pkg, dict(b, wbc_cmd=cmd), tid)
    A.d["prev"].upload(pkg.to_soa(prev_in))
    held = []
    for _ in range(2):
        A.poison()
        ctx.wbc_run_batch(n, A.d["fb"], A.d["cmd"], A.d["prev"], A.d["tau"], A.d["qdes"], A.d["status"], A.tid)
        held.append(A.get("tau", "qdes", "prev", "status"))
    A.free(); ctx.close()
    q = b["fb_state"][:, 13:25]
    swing64 = R.epilogue(R.torque(q, hold_in, legs), ~stance[:, 0::3], epilogue)
    swing32 = R.epilogue(R.torque(q, hold_in, legs, np.float32), ~stance[:, 0::3], epilogue, np.float32)
    gap_t, bar_t = R.bar(swing32, swing64)
    assert (np.abs(swing64[~stance]) > 1.5).mean() > 0.3                               # (the swing legs' torques are no zeros plus the compensation)
    _SHAPES[key] = dict(b=b, tid=tid, legs=legs, n=n, h=h, epilogue=epilogue, mixed=mixed, prev_in=prev_in, force_in=force_in, hold_in=hold_in, quat=quat, due=due,
                        held=held, stance=stance, swing64=swing64, gap_t=gap_t, bar_t=bar_t)
    return _SHAPES[key]


def _run_cadence(pkg, sh, mask, ctx=None):
    """Two cadenced ticks in a row with the mask; -> the outputs of each."""
    n, own = sh["n"], ctx is None
    if own:
        ctx = _ctx(pkg, sh["h"], n, sh["epilogue"], sh["mixed"])
    A = _Arrays(ctx, pkg, sh["b"], sh["tid"])
    try:
        A.d["due"].upload(np.asarray(mask, np.int32))
        A.d["prev"].upload(pkg.to_soa(sh["prev_in"])); A.d["force"].upload(pkg.to_soa(sh["force_in"])); A.d["hold"].upload(pkg.to_soa(sh["hold_in"]))
        outs = []
        for _ in range(2):
            A.poison()
            ctx.tick_cadence_batch(n, A.d["due"], A.d["state"], A.d["traj"], A.d["gait"], A.d["fb"], A.d["cmd"], A.d["prev"], A.d["force"], A.d["hold"], A.d["tau"],
                                   status=A.d["status"], qdes=A.d["qdes"], type_id=A.tid)
            outs.append(A.get("force", "hold", "tau", "qdes", "prev", "status"))
        return outs
    finally:
        A.free()
        if own:
            ctx.close()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _check(sh, mask, outs, what):
    """Every due robot carries its all-due result, every held robot its none-due result, call for call."""
    m = np.asarray(mask) != 0
    clip = (lambda t: np.clip(t, np.float32(-23), np.float32(23))) if sh["epilogue"] & R.EPILOGUE_CLIP else (lambda t: t)
    for k, o in enumerate(outs):
        tag = (what, "call %d" % k)
        d, w = sh["due"][k], sh["held"][k]
        # due robots: the solve's own outputs, the kept force, nothing of the WBC
        assert _same(o["force"][m], d["force"][m]) and _same(o["tau"][m], d["tau"][m]) and np.array_equal(o["status"][m], d["status"][m]), tag
        hold64 = R.hold_from_force(sh["quat"][m], d["force"][m])
        gap_h, bar_h = R.bar(R.hold_from_force(sh["quat"][m], d["force"][m], np.float32), hold64) if m.any() else (0.0, 2e-6)
        worst_h = float(R.rel_err(o["hold"][m], hold64).max()) if m.any() else 0.0
        assert _same(o["prev"][m], sh["prev_in"][m]) and np.all(o["qdes"][m] == POISON_F), tag
        # held robots: the memory as put in, the WBC's rows, the kept force through the Jacobian of now, a status word without an MPC part
        h_ = ~m
        assert _same(o["force"][h_], sh["force_in"][h_]) and _same(o["hold"][h_], sh["hold_in"][h_]), tag
        st = sh["stance"][h_]
        assert _same(o["tau"][h_][st], clip(w["tau"][h_])[st]), tag
        assert _same(o["qdes"][h_], w["qdes"][h_]) and _same(o["prev"][h_], w["prev"][h_]), tag
        worst_t = float(R.rel_err(o["tau"][h_][~st], sh["swing64"][h_][~st]).max()) if (~st).any() else 0.0
        assert np.array_equal(o["status"][h_], w["status"][h_]) and np.all(G.iterations(o["status"][h_]) == 0), tag
        print("%s call %d: due %d held %d | hold gap %.2e bar %.2e worst %.2e | swing torque gap %.2e bar %.2e worst %.2e"
              % (what, k, m.sum(), h_.sum(), gap_h, bar_h, worst_h, sh["gap_t"], sh["bar_t"], worst_t))
        assert worst_h <= bar_h and worst_t <= sh["bar_t"], tag
        assert np.isfinite(o["tau"]).all() and not np.any(o["tau"] == POISON_F) and not np.any(o["status"] == POISON_I), tag


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", [0, BOTH])
def test_all_due_is_the_mpc_solve(pkg, epilogue):
    sh = _shape(pkg, 70, 10, epilogue)
    _check(sh, np.ones(70, np.int32), _run_cadence(pkg, sh, np.ones(70, np.int32)), "all due, epilogue %d" % epilogue)


@pytest.mark.parametrize("epilogue", [0, BOTH])
def test_none_due_is_the_held_force_and_the_wbc(pkg, epilogue):
    sh = _shape(pkg, 70, 10, epilogue)
    assert 0.2 < sh["stance"].mean() < 0.8                                             # both kinds of leg
    _check(sh, np.zeros(70, np.int32), _run_cadence(pkg, sh, np.zeros(70, np.int32)), "none due, epilogue %d" % epilogue)


def _masks(n):
    r = np.arange(n)
    return {"every third": (r % 3 == 0).astype(np.int32), "one due": (r == n // 2).astype(np.int32), "one held": (r != n // 3).astype(np.int32),
            "the word 2": 2 * (r % 2).astype(np.int32)}


@pytest.mark.parametrize("which", ["every third", "one due", "one held", "the word 2"])
def test_mixed_masks(pkg, which):
    sh = _shape(pkg, 70, 10, BOTH)
    mask = _masks(70)[which]
    _check(sh, mask, _run_cadence(pkg, sh, mask), which)


@pytest.mark.parametrize("n,h,mixed", [(5, 10, False), (70, 16, False), (272, 16, False), (70, 10, True)],
                         ids=["whole-CU path n=5", "h=16 n=70", "h=16 n=272 persistent", "A1 and Lite3"])
def test_shapes_where_the_launch_form_changes(pkg, n, h, mixed):
    sh = _shape(pkg, n, h, BOTH, mixed)
    mask = (np.arange(n) % 3 == 0).astype(np.int32)
    _check(sh, mask, _run_cadence(pkg, sh, mask), "n=%d h=%d mixed=%s" % (n, h, mixed))


def test_sequence_driven_by_the_front_end(pkg):
    """36 ticks at n = 70.  The front-end's counter (row 7 of d_fe_state) starts at 50 + r % period, period = round(dt_mpc / dt_ctrl) / 2 = 12, so another
    subset is due on every tick and the share of due robots over the ticks is 1 / period exactly (the restated rule, checked on the CPU).  A second
    context runs the front-end, qrgpu_mpc_solve_batch and qrgpu_wbc_run_batch on everybody every tick; d_force, d_hold, d_tau, d_prev_ori and d_qdes are
    merged on the host by the mask.  Both contexts start every solve cold (warm start and planned list off, gpu_helpers.cold_start): the second one
    solves every robot every tick, the first one a robot every twelfth tick, and a warm start from another tick's working set moves the last bits.
    From tick 18 on the front-end reads another gait phase: legs that stood at a robot's last solve swing now, and their kept force reaches the motors
    through the Jacobian of now until the robot's next solve."""
    n, h, T, dt_ctrl, dt_mpc = 70, 10, 36, 0.002, 0.05
    period = R.period_of(dt_ctrl, dt_mpc)
    assert period == 12
    seq = pkg.make_batch_sequence(n, h, "a1", seed=0x5EC, steps=T, dt=dt_ctrl)
    fe, st = pkg.workload.make_frontend_batch(n, seed=0xFE)
    fe_b = fe.copy()
    fe_b[:, 38:62] = pkg.workload.make_frontend_batch(n, seed=0xFF)[0][:, 38:62]       # contacts, phases and leg states of another moment of the gait
    st[:, 7] = 50 + np.arange(n) % period
    want_due = R.due_schedule(st[:, 7], period, T)
    assert want_due.mean() == 1.0 / period and all(0 < want_due[t].sum() < n for t in range(T))
    legs = np.tile(np.asarray(pkg.model_desc("a1")[:3], np.float64), (n, 1))
    S = pkg.to_soa
    X, Y = _ctx(pkg, h, n, BOTH, False, cold=True), _ctx(pkg, h, n, BOTH, False, cold=True)
    try:
        ax, ay = _Arrays(X, pkg, seq[0], None), _Arrays(Y, pkg, seq[0], None)
        for A, ctx in ((ax, X), (ay, Y)):
            A.fe, A.fst = ctx.alloc((64, n)).upload(S(fe)), ctx.alloc((8, n)).upload(S(st))
            A.d["force"].upload(np.zeros((12, n), np.float32)); A.d["prev"].upload(np.zeros((3, n), np.float32))
        ax.d["hold"].upload(np.zeros((12, n), np.float32))
        force = np.zeros((n, 12), np.float32); hold = np.zeros((n, 12), np.float32); prev = np.zeros((n, 3), np.float32)
        qdes = np.full((n, 24), POISON_F, np.float32)
        ax.poison()
        seen = []
        worst_h = worst_t = bar_hmax = bar_tmax = 0.0
        swing_held = 0
        for t, b in enumerate(seq):
            for A, ctx in ((ax, X), (ay, Y)):
                if t == T // 2:
                    A.fe.upload(S(fe_b))
                A.d["state"].upload(S(b["mpc_state"])); A.d["fb"].upload(S(b["fb_state"]))
                ctx.mpc_frontend_batch(n, A.fe, A.fst, A.d["traj"], A.d["gait"], A.d["cmd"], A.d["due"], dt_ctrl=dt_ctrl, dt_mpc=dt_mpc)
            X.tick_cadence_batch(n, ax.d["due"], ax.d["state"], ax.d["traj"], ax.d["gait"], ax.d["fb"], ax.d["cmd"], ax.d["prev"], ax.d["force"], ax.d["hold"],
                                 ax.d["tau"], status=ax.d["status"], qdes=ax.d["qdes"])
            got = ax.get("due", "force", "hold", "tau", "qdes", "prev", "status")
            m = got["due"] != 0
            assert np.array_equal(m, want_due[t]), t
            seen.append(m)
            # the other context: everybody solved, then the WBC on the merged Fr_des and the merged orientation memory
            ay.poison()
            Y.mpc_solve_batch(n, ay.d["state"], ay.d["traj"], ay.d["gait"], ay.d["fb"].row(13), ay.d["force"], ay.d["tau"], ay.d["status"])
            sol = ay.get("force", "tau", "status", "cmd")
            force = np.where(m[:, None], sol["force"], force)
            hold64 = np.where(m[:, None], R.hold_from_force(b["mpc_state"][:, 6:10], force), hold.astype(np.float64))
            cmd = sol["cmd"].copy(); cmd[:, 51:63] = force
            ay.d["cmd"].upload(S(cmd)); ay.d["prev"].upload(S(prev))
            Y.wbc_run_batch(n, ay.d["fb"], ay.d["cmd"], ay.d["prev"], ay.d["tau"], ay.d["qdes"], ay.d["status"])
            wbc = ay.get("tau", "qdes", "prev", "status")
            stance = np.repeat(cmd[:, 63:67] != 0, 3, axis=1)
            tag = "tick %d" % t
            # due robots
            assert _same(got["force"][m], sol["force"][m]) and _same(got["tau"][m], sol["tau"][m]) and np.array_equal(got["status"][m], sol["status"][m]), tag
            gap, bar = R.bar(R.hold_from_force(b["mpc_state"][m, 6:10], force[m], np.float32), hold64[m])
            e = float(R.rel_err(got["hold"][m], hold64[m]).max())
            worst_h, bar_hmax = max(worst_h, e), max(bar_hmax, bar)
            assert e <= bar, (tag, e, bar)
            assert _same(got["prev"][m], prev[m]) and _same(got["qdes"][m], qdes[m]), tag
            # held robots (the kept force they map is the cadenced context's own float32 one, held bit for bit since its solve)
            h_ = ~m
            assert _same(got["force"][h_], force[h_]) and _same(got["hold"][h_], hold[h_]), tag
            assert _same(got["tau"][h_][stance[h_]], np.clip(wbc["tau"], np.float32(-23), np.float32(23))[h_][stance[h_]]), tag
            assert _same(got["qdes"][h_], wbc["qdes"][h_]) and _same(got["prev"][h_], wbc["prev"][h_]), tag
            assert np.array_equal(got["status"][h_], wbc["status"][h_]) and np.all(G.iterations(got["status"][h_]) == 0), tag
            q = b["fb_state"][:, 13:25]
            sw64 = R.epilogue(R.torque(q, hold, legs), ~stance[:, 0::3], BOTH)
            sw32 = R.epilogue(R.torque(q, hold, legs, np.float32), ~stance[:, 0::3], BOTH, np.float32)
            gap, bar = R.bar(sw32[h_], sw64[h_])
            sel = h_[:, None] & ~stance
            e = float(R.rel_err(got["tau"][sel], sw64[sel]).max()) if sel.any() else 0.0
            worst_t, bar_tmax = max(worst_t, e), max(bar_tmax, bar)
            swing_held += int((np.abs(sw64[sel]) > 1.5).sum())
            assert e <= bar, (tag, e, bar)
            # what the next tick starts from
            hold = np.where(m[:, None], got["hold"], hold)
            prev = np.where(m[:, None], prev, wbc["prev"]); qdes = np.where(m[:, None], qdes, wbc["qdes"])
        print("sequence: hold worst %.2e (largest bar %.2e), swing torque worst %.2e (largest bar %.2e)" % (worst_h, bar_hmax, worst_t, bar_tmax))
        assert np.mean(seen) == 1.0 / period
        assert swing_held > 100                                                        # swing legs that carried a kept force, over the run
        for A in (ax, ay):
            A.fe.free(); A.fst.free(); A.free()
    finally:
        X.close(); Y.close()


def test_bad_arguments_launch_nothing_and_a_valid_call_follows(pkg):
    sh = _shape(pkg, 70, 10, BOTH)
    n = 70
    ctx = pkg.Context(0, n, 16)
    G.setup_a1(ctx, pkg, 10)
    ctx.set_torque_epilogue(hip_comp=True, clip=True)
    A = _Arrays(ctx, pkg, sh["b"], None)
    try:
        mask = (np.arange(n) % 3 == 0).astype(np.int32)
        A.d["due"].upload(mask); A.d["prev"].upload(pkg.to_soa(sh["prev_in"])); A.d["force"].upload(pkg.to_soa(sh["force_in"])); A.d["hold"].upload(pkg.to_soa(sh["hold_in"]))
        A.poison()
        d = A.d

        def call(n_=n, **over):
            a = dict(d, **over)
            return ctx._lib.qrgpu_tick_cadence_batch(ctx._h, n_, None, *[x.ptr if x is not None else None for x in (
                a["due"], a["state"], a["traj"], a["gait"], a["fb"], a["cmd"], a["prev"], a["force"], a["hold"], a["tau"], a["qdes"], a["status"])])
        BAD_ARG = 2                                                                                     # QRGPU_ERR_BAD_ARG
        assert pkg.qrgpu.ERRORS[BAD_ARG] == "BAD_ARG"
        for bad in (dict(due=None), dict(force=None), dict(hold=None)):
            assert call(**bad) == BAD_ARG, bad
        assert call(0) == BAD_ARG and call(n + 1) == BAD_ARG                                            # (the context's max_batch is n)
        got = A.get("tau", "status", "force", "hold")
        assert np.all(got["tau"] == POISON_F) and np.all(got["status"] == POISON_I)                     # nothing was launched
        assert _same(got["force"], sh["force_in"]) and _same(got["hold"], sh["hold_in"])
        assert call() == 0
        o = A.get("force", "hold", "tau", "qdes", "prev", "status")
        _check(sh, mask, [o], "after the refused calls")
    finally:
        A.free(); ctx.close()


def test_after_an_overlapped_tick_on_the_same_context(pkg):
    """The tool's path: Context.tick_cadence_batch right behind an overlapped qrgpu_tick_batch on the same context, no sync in between.  The serial
    call is queued on the context's stream behind that tick's join, so it waits for what the lanes queued: the same results as on a fresh context.
    Every solve starts cold here (gpu_helpers.cold_start: the context's history is the overlapped ticks', not the reference's), so both calls are held
    against the reference's first, cold solve."""
    sh = _shape(pkg, 70, 10, BOTH)
    n = 70
    ctx = _ctx(pkg, 10, n, BOTH, False, cold=True)
    B = _Arrays(ctx, pkg, sh["b"], None)
    try:
        assert ctx.set_tick_overlap(True)
        B.d["prev"].upload(pkg.to_soa(sh["prev_in"])); B.poison()
        ctx.sync()
        for _ in range(2):
            ctx.tick_batch(n, B.d["state"], B.d["traj"], B.d["gait"], B.d["fb"], B.d["cmd"], B.d["prev"], B.d["force"], B.d["tau"], B.d["status"], qdes=B.d["qdes"])
        mask = (np.arange(n) % 3 == 0).astype(np.int32)
        outs = _run_cadence(pkg, sh, mask, ctx=ctx)
    finally:
        B.free(); ctx.close()
    ref = dict(sh, due=[sh["due"][0], sh["due"][0]])
    _check(ref, mask, outs, "behind an overlapped tick")
