"""The control state machine on the device (qrgpu_fsm_update_batch, qrgpu_fsm_zero_command_batch, qrgpu_fsm_command_batch) against tests/fsm_ref.py on
the streams of the host test, at n = 130 (two full waves and a ragged one) and n = 1.  Every comparison is bit for bit.

  * parity over the 264 ticks: the state column, the joy rows, the plan, the stage mask, the motor command, the report; the resets given through d_done
    (n = 130; every robot that is not reset carries a word outside `bits`) and through the scalar (n = 1); a guard row of poison behind every array.
  * the zeroing stage writes +0 into the listed rows of the robots in phase 1 and leaves poison everywhere else.
  * every optional array NULL in turn: the other outputs keep their bits; a NULL input is the input that says nothing.
  * a robot reset at tick k is from k on the robot of a run started fresh at k.
  * d_stage_mask is (d_done & bits) | QRGPU_FSM_ENTERED; a done word outside `bits` is no reset.
  * d_motor_cmd_loco aliased to d_motor_cmd gives the bits of the two apart.
  * PASSIVE -> STAND_UP, which no joystick message reaches, from a state column written into that situation.
  * a machine constructed in HARD_CODE: the joy rows are desc->hard_code_v / hard_code_w until a request moves the state on.
  * refusals: every BAD_ARG case names its argument and leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import fsm_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
POISON, IPOISON, BAD_ARG = R.POISON, i32(0x7fffffff), 2
FOUT = dict(state=R.STATE_ROWS, joy=8, cmd=R.CMD_ROWS, out=R.OUT_ROWS, **R.ZERO_ARRAY_ROWS)
IOUT = ("plan", "mask")
KEYS = tuple(FOUT) + IOUT
ZERO = tuple(R.ZERO_ARRAY_ROWS)


class Arrays:
    """The three stages' device arrays for n robots, every written one with a guard row of poison behind it; the streams uploaded once."""

    def __init__(self, ctx, pkg, n, script=True, r0=0, D=R.SHORT):
        S = R.streams()
        self.ctx, self.n, self.r0, self.zero_msg = ctx, n, r0, None
        self.desc = pkg.fsm_desc(**D)
        self.d = {k: ctx.alloc((r + 1, n)).upload(np.full((r + 1, n), POISON, f32)) for k, r in FOUT.items()}
        self.d.update({k: ctx.alloc((2, n), i32).upload(np.full((2, n), IPOISON, i32)) for k in IOUT})
        cut = lambda a: np.ascontiguousarray(a[..., r0:r0 + n])
        self.msg = ctx.alloc((R.T_REF, R.MSG_ROWS, n)).upload(cut(S["joy_msg"]))
        self.est = ctx.alloc((R.T_REF, 54, n)).upload(cut(S["est_in"]))
        self.loco = ctx.alloc((R.T_REF, R.CMD_ROWS, n)).upload(cut(S["loco"]))
        self.ticks = ctx.alloc((R.T_REF, n), i32).upload(cut(S["ticks"]))
        self.script = ctx.alloc(R.SCRIPT.shape).upload(R.SCRIPT) if script else None
        self.done = ctx.alloc((n,), i32)

    def tick(self, t, reset, mode="done", null=(), alias=False, bits=0xff, done_word=0x40, empty=()):
        """tick t of the streams; reset [N_REF] bool.  null: arguments given as NULL; empty: inputs given as arrays that say nothing"""
        ctx, n, d = self.ctx, self.n, self.d
        reset = reset[self.r0:self.r0 + n]
        for k in ("joy", "cmd", "out") + ZERO:
            d[k].upload(np.full((FOUT[k] + 1, n), POISON, f32))
        for k in IOUT:
            d[k].upload(np.full((2, n), IPOISON, i32))
        g = lambda k, v: None if k in null else v
        msg = self.msg.row(t)
        if "joy_msg" in empty:
            if self.zero_msg is None:
                self.zero_msg = ctx.alloc((R.MSG_ROWS, n)).zero()
            msg = self.zero_msg
        done = None
        if mode == "done":
            self.done.upload(np.where(reset & ("done" not in empty), done_word, 0x01000000).astype(i32))
            done = self.done
        scripted = self.script is not None and "script" not in null
        ctx.fsm_update(n, self.desc, d["state"], d["joy"], d["plan"], stage_mask=g("mask", d["mask"]), joy_msg=g("joy_msg", msg),
                       script=self.script if scripted else None, n_script=R.SCRIPT.shape[1] if scripted and "script" not in empty else 0,
                       ticks=self.ticks.row(t) if scripted else None, done=g("done", done), bits=bits, reset=int(mode == "scalar" and bool(reset.all())))
        ctx.fsm_zero_command(n, d["plan"], **{a: g(k, d[k]) for a, k in (("state_des", "state_des"), ("fe_in", "fe"), ("fh_in", "fh"), ("swing_vel_in", "sv"),
                                                                      ("stance_cmd", "sc"))})
        loco = self.loco.row(t)
        if alias:
            ctx._chk(ctx._lib.qrgpu_memcpy_async(ctx._h, d["cmd"].ptr, loco, R.CMD_ROWS * n * 4, 2))
            loco = d["cmd"]
        ctx.fsm_command(n, self.desc, d["plan"], self.est.row(t), loco, d["state"], d["cmd"], fsm_out=g("out", d["out"]))

    def read(self):
        out = {}
        for k in KEYS:
            a = self.d[k].download()
            assert np.all(a[-1] == (IPOISON if k in IOUT else POISON)), ("guard row", k)
            out[k] = a[0].copy() if k in IOUT else a[:-1].copy()
        return out

    def set_state(self, col):
        self.d["state"].upload(np.concatenate([col[:, self.r0:self.r0 + self.n], np.full((1, self.n), POISON, f32)]))

    def free(self):
        for v in list(self.d.values()) + [self.msg, self.est, self.loco, self.ticks, self.done] + [v for v in (self.script, self.zero_msg) if v is not None]:
            v.free()


def device_run(ctx, pkg, n, first=0, last=R.T_REF, fresh_at=None, mode="done", state0=None, r0=0, **kw):
    """ticks first..last-1 -> [T'] stacked outputs.  state0: the state column to start from (else the first tick must reset everyone)"""
    S = R.streams()
    a = Arrays(ctx, pkg, n, r0=r0)
    if state0 is not None:
        a.set_state(state0)
    out = []
    try:
        for t in range(first, last):
            reset = S["reset"][t] | (t == fresh_at)
            a.tick(t, reset, mode=mode, **kw)
            out.append(a.read())
    finally:
        a.free()
    return {k: np.stack([o[k] for o in out]) for k in KEYS}


@pytest.fixture(scope="module")
def full(gpu_ctx, pkg):
    return device_run(gpu_ctx, pkg, R.N_REF)


def test_parity(full):
    ref = R.reference()
    for t in range(R.T_REF):
        R.compare({k: full[k][t] for k in KEYS}, ref, t, R.N_REF, tag="n=130")


def test_parity_one_robot_scalar_reset(gpu_ctx, pkg):
    """n = 1: robots 5 (X during its stand-up, reset there and again inside a gait transition) and 2 (sits down, goes passive) of the streams, each a
    batch of its own, the resets given by the scalar"""
    full_ref = R.reference()
    for r0 in (5, 2):
        got = device_run(gpu_ctx, pkg, 1, mode="scalar", r0=r0)
        ref = {k: v[..., r0:r0 + 1] for k, v in full_ref.items() if k != "paths"}
        for t in range(R.T_REF):
            R.compare({k: got[k][t] for k in KEYS}, ref, t, 1, tag="n=1, robot %d" % r0, done_word=0)


def test_optional_arrays(gpu_ctx, pkg, full):
    """Ticks 150-155 from the state after tick 149 (robots in every state, a dozen in phase 1): each optional output NULL in turn leaves the others' bits
    alone and keeps its poison; a NULL joy_msg, script or d_done is an array that says nothing."""
    ref, n, k0, k1 = R.reference(), R.N_REF, 150, 156
    assert ref["zeroed"][k0:k1].sum() >= 10
    run = lambda **kw: device_run(gpu_ctx, pkg, n, first=k0, last=k1, state0=ref["state"][k0 - 1], **kw)
    base = run()
    for t in range(k0, k1):
        R.compare({k: base[k][t - k0] for k in KEYS}, ref, t, n, tag="from the state of tick 149")
    for name in ("mask", "out") + ZERO:
        got = run(null=(name,))
        for k in KEYS:
            if k != name:
                assert got[k].tobytes() == base[k].tobytes(), (name, k)
        assert np.all(got[name] == (IPOISON if name in IOUT else POISON)), name
    for name in ("joy_msg", "script", "done"):
        a, b = run(null=(name,)), run(empty=(name,))
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        if name == "joy_msg":                             # the input mattered: a dozen messages arrive in these ticks
            assert a["state"].tobytes() != base["state"].tobytes()


def test_a_robot_reset_at_k_is_the_robot_started_fresh_at_k(gpu_ctx, pkg, full):
    S, seen = R.streams(), 0
    for k in (30, 100):
        robots = np.nonzero(S["reset"][k])[0]
        assert 5 in robots                                # reset in the middle of its stand-up (30) and of a gait transition (100)
        B = device_run(gpu_ctx, pkg, R.N_REF, first=k, last=k + 45, fresh_at=k)
        for key in KEYS:
            a, b = full[key][k:k + 45][..., robots], B[key][..., robots]
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (k, key)
        seen += len(robots)
    assert seen >= 2


def test_stage_mask_and_bits(gpu_ctx, pkg):
    """Tick 150 from the state after 149 with EVERY robot's done word 0x40: under bits 0xff everyone is reset and the mask is 0x40; under bits 0x0f nobody is,
    the tick is the streams' and the mask is QRGPU_FSM_ENTERED alone."""
    ref, n, k = R.reference(), R.N_REF, 150
    assert not R.streams()["reset"][k].any() and (ref["mask"][k] & R.ENTERED).any()
    a = Arrays(gpu_ctx, pkg, n)
    try:
        a.set_state(ref["state"][k - 1]); a.tick(k, np.ones(n, bool), bits=0x0f)
        got = a.read()
        assert np.array_equal(got["mask"], ref["mask"][k] & R.ENTERED)
        got["mask"] = got["mask"] | np.where(ref["mask"][k] & 1, 0x40, 0)
        R.compare(got, ref, k, n, tag="bits 0x0f")
        a.set_state(ref["state"][k - 1]); a.tick(k, np.ones(n, bool), bits=0xff)
        got = a.read()
        quiet = ~ref["paths"][k].any(-1) & (R.streams()["joy_msg"][k, 9] == 0)          # robots that receive nothing at this tick
        assert np.all(got["mask"] == 0x40) and np.all(got["plan"][quiet] == (R.ACTION | R.ACTION_FIRST)) and np.all(got["out"][0][quiet] == R.STAND_UP)
        assert quiet.sum() > 100 and np.all(got["state"][30, quiet] == f32(0.05)) and np.all(got["state"][43:46, quiet] == np.array([[0], [0], [-1]], f32))
    finally:
        a.free()


def test_loco_command_aliased_to_the_output(gpu_ctx, pkg):
    ref, n, k0, k1 = R.reference(), R.N_REF, 150, 156
    got = device_run(gpu_ctx, pkg, n, first=k0, last=k1, state0=ref["state"][k0 - 1], alias=True)
    assert ((ref["plan"][k0:k1] & (R.RUN | R.PHASE1)) != 0).sum() > 100
    for t in range(k0, k1):
        R.compare({k: got[k][t - k0] for k in KEYS}, ref, t, n, tag="aliased")


def test_passive_to_stand_up_from_a_written_state(gpu_ctx, pkg):
    """The one path no joystick reaches (joyCmdExit is never cleared): a PASSIVE robot whose fsmMode is K_STAND_UP.  The state column is the
    restatement's, written by hand into that situation; the next 40 ticks -- the one-tick transition, OnEnter, the stand-up -- are compared."""
    from test_fsm_ref import passive_robot_asked_to_stand_up
    S, n, k0 = R.streams(), R.N_REF, 200
    robots = [passive_robot_asked_to_stand_up(R.SHORT) for _ in range(n)]
    a = Arrays(gpu_ctx, pkg, n, script=False)
    try:
        a.set_state(np.stack([rb.state_rows() for rb in robots], 1))
        seen = set()
        for t in range(k0, k0 + 40):
            a.tick(t, np.zeros(n, bool), null=("joy_msg",))
            got = a.read()
            for r, rb in enumerate(robots):
                o = rb.tick(None, False, S["est_in"][t, 13:17, r], S["est_in"][t, 17:29, r], S["loco"][t, :, r])
                assert got["plan"][r] == o["plan"] and got["mask"][r] == 0, (t, r)
                for k, want in (("cmd", o["cmd"]), ("state", rb.state_rows()), ("joy", o["joy"]), ("out", o["out"])):
                    assert np.array_equal(got[k][:, r].view(np.uint32), want.view(np.uint32)), (t, r, k)
                seen.add(o["plan"])
        assert seen == {R.PLAN_PASSIVE | R.DONE, R.ACTION | R.ACTION_FIRST, R.ACTION}
    finally:
        a.free()


def test_constructed_in_hard_code(gpu_ctx, pkg):
    """desc->initial_ctrl_state HARD_CODE: the joy rows carry desc->hard_code_v / hard_code_w until a request moves the state on (here the streams'
    messages and gaitSwitch flags of ticks 0-79, every robot constructed at tick 0)."""
    D = dict(R.SHORT, initial_ctrl_state=R.HARD_CODE, hard_code_v=[0.125, -0.0625, 0.03125], hard_code_w=[0.5, -0.25, 0.75])
    S, n = R.streams(), R.N_REF
    robots = [R.Robot(D) for _ in range(n)]
    a = Arrays(gpu_ctx, pkg, n, D=D)
    hard = moved = 0
    try:
        for t in range(80):
            a.tick(t, np.full(n, t == 0))
            got = a.read()
            for r, rb in enumerate(robots):
                m, gs, _ = R.message(S, R.SCRIPT, t, r)
                o = rb.tick(m, gs, S["est_in"][t, 13:17, r], S["est_in"][t, 17:29, r], S["loco"][t, :, r])
                assert got["plan"][r] == o["plan"], (t, r)
                for k, want in (("cmd", o["cmd"]), ("state", rb.state_rows()), ("joy", o["joy"]), ("out", o["out"])):
                    assert np.array_equal(got[k][:, r].view(np.uint32), want.view(np.uint32)), (t, r, k)
                if o["joy"][7] == R.HARD_CODE:
                    hard += 1
                    assert list(got["joy"][:7, r]) == [f32(x) for x in D["hard_code_v"] + D["hard_code_w"] + [0.28]]
                else:
                    moved += 1
    finally:
        a.free()
    assert hard > 2000 and moved > 2000, (hard, moved)


def test_refusals(gpu_ctx, pkg):
    """Every BAD_ARG case returns the code, names the argument and launches nothing: the outputs keep what they held."""
    ctx, n = gpu_ctx, 5
    a = Arrays(ctx, pkg, n)
    d, desc = a.d, a.desc
    a.done.upload(np.zeros(n, i32))
    before = a.read()

    def refused(call, name, fn):
        with pytest.raises(pkg.QrgpuError) as e:
            fn()
        assert str(e.value).startswith("BAD_ARG: %s: %s" % (call, name)), (call, name, str(e.value))
        assert ctx.last_error() == "%s: %s" % (call, name)

    def upd(n_=n, desc_=desc, **k):
        kw = dict(stage_mask=d["mask"], joy_msg=a.msg, script=a.script, n_script=R.SCRIPT.shape[1], ticks=a.ticks, done=a.done, bits=0xff, reset=0)
        pos = dict(fsm_state=d["state"], joy=d["joy"], plan=d["plan"])
        for key, v in k.items():
            (pos if key in pos else kw)[key] = v
        return lambda: ctx.fsm_update(n_, desc_, pos["fsm_state"], pos["joy"], pos["plan"], **kw)

    U, Z, M = "qrgpu_fsm_update_batch", "qrgpu_fsm_zero_command_batch", "qrgpu_fsm_command_batch"
    for bad_n in (0, -3, 4097):
        refused(U, "n", upd(n_=bad_n))
    for key in ("fsm_state", "joy", "plan"):
        refused(U, "d_" + key, upd(**{key: None}))
    for bad in (2, -1):
        refused(U, "reset", upd(reset=bad))
    refused(U, "d_ticks", upd(ticks=None))                                   # a script without its clock
    refused(U, "d_script", upd(script=None))                                 # n_script entries of nothing
    for bad in (-1, 65):
        refused(U, "n_script", upd(n_script=bad))
    refused(U, "bits", upd(bits=0))                                          # d_done with no bit to look at
    for field, bad in (("stand_up_time", 0.0), ("stand_up_total", -1.0), ("sit_down_time", 0.0), ("time_step", 0.0), ("time_step", float("nan")),
                       ("transition_ticks", 0), ("transition_ticks", -5), ("gait_transition_duration", 0.0), ("stand_transition_duration", -2.0),
                       ("tau_clip", 0.0), ("initial_ctrl_state", 8)):
        bad_desc = pkg.fsm_desc(**dict(R.SHORT, **{field: bad}))
        refused(U, "desc->" + field, upd(desc_=bad_desc))
        refused(M, "desc->" + field, lambda: ctx.fsm_command(n, bad_desc, d["plan"], a.est, a.loco, d["state"], d["cmd"], fsm_out=d["out"]))

    def cmd(n_=n, **k):
        g = lambda key, v: k[key] if key in k else v
        return lambda: ctx.fsm_command(n_, desc, g("plan", d["plan"]), g("est_in", a.est), g("motor_cmd_loco", a.loco), g("fsm_state", d["state"]),
                                       g("motor_cmd", d["cmd"]), fsm_out=d["out"])
    for bad_n in (0, -3, 4097):
        refused(M, "n", cmd(n_=bad_n))
        refused(Z, "n", lambda: ctx.fsm_zero_command(bad_n, d["plan"], state_des=d["state_des"]))
    for key in ("plan", "est_in", "motor_cmd_loco", "fsm_state", "motor_cmd"):
        refused(M, "d_" + key, cmd(**{key: None}))
    refused(Z, "d_plan", lambda: ctx.fsm_zero_command(n, None, state_des=d["state_des"], fe_in=d["fe"]))
    lib, p = pkg.load_library(), lambda x: C.c_void_p(x.ptr)
    assert lib.qrgpu_fsm_update_batch(ctx._h, n, None, 0, None, None, 0, None, None, 0, p(d["state"]), p(d["joy"]), p(d["plan"]), None) == BAD_ARG
    assert ctx.last_error() == U + ": desc"
    assert lib.qrgpu_fsm_command_batch(ctx._h, n, None, p(d["plan"]), p(a.est), p(a.loco), p(d["state"]), p(d["cmd"]), None) == BAD_ARG
    assert ctx.last_error() == M + ": desc"
    assert lib.qrgpu_fsm_update_batch(None, n, C.byref(desc), 0, None, None, 0, None, None, 0, p(d["state"]), p(d["joy"]), p(d["plan"]), None) == BAD_ARG
    assert lib.qrgpu_fsm_zero_command_batch(None, n, p(d["plan"]), None, None, None, None, None) == BAD_ARG
    assert lib.qrgpu_fsm_command_batch(None, n, C.byref(desc), p(d["plan"]), p(a.est), p(a.loco), p(d["state"]), p(d["cmd"]), None) == BAD_ARG
    ctx.sync()
    after = a.read()
    for k in KEYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    a.free()
