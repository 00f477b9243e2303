"""The trot's command, data-flow and motor-command stages on the device (qrgpu_command_update_batch, qrgpu_trot_inputs_batch, qrgpu_mpc_command_batch)
against tests/dataflow_ref.py on the streams of the host test, at n = 130 (two full waves and a ragged one) and n = 1.

  * parity over the 48 ticks, the streams' per-robot resets given as a stage-reset mask: every row reached by copies and + - x / alone bit for bit, rows
    14-25 of fe_in (behind the quaternion's rotation matrix) under the bar of test_dataflow_host.py (8 x the restatement's float32-to-float64 gap, never
    under 2e-6); every row a stage must leave alone, and a guard row behind every array, keep their poison; once more with both epilogue bits.
  * every optional output NULL in turn: the other outputs' bits do not change.
  * the scalar reset is the mask of every robot; a robot masked at tick k is from k on the robot of a run started fresh at k, bit for bit, for the command
    state and the command memory.
  * refusals: every BAD_ARG case names its argument and leaves the outputs untouched.

Measured on an MI355X (test_parity prints them): foot positions in the world frame, gap 1.6e-7 -> bar 2.0e-6, worst device-vs-restatement distance 0 at
n = 130 and n = 1, with and without the epilogue: the kernel writes the rotation's products in the restatement's order."""
import numpy as np
import pytest

import dataflow_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
POISON = R.POISON
MEM_POISON = i32(0x7fffffff)
BAD_ARG = 2
OUT_ROWS = dict(cmd_state=6, state_des=12, fe=R.FE_ROWS, fh=R.FH_ROWS, sv=R.SV_ROWS, sc=R.SC_ROWS, sw=R.SW_ROWS, est_in=54, motor_cmd=R.MOTOR_CMD_ROWS)
IN_ROWS = dict(joy=8, est_out=42, rpy=3, gait_out=24, gait_state=52, tau=12, qdes=24)
KEYS = tuple(OUT_ROWS) + ("mem",)
SCATTERED = ("state_des", "fe", "fh", "sv", "sc", "sw", "motor_cmd")


class Arrays:
    """The three stages' device arrays for n robots, every written one with a guard row of poison behind it."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.d = {k: ctx.alloc((r + 1, n)).upload(np.full((r + 1, n), POISON, f32)) for k, r in OUT_ROWS.items()}
        self.d.update({k: ctx.alloc((r, n)) for k, r in IN_ROWS.items()})
        self.d["mem"] = ctx.alloc((2, n), i32).upload(np.full((2, n), MEM_POISON, i32))
        self.mask = ctx.alloc((n,), i32).zero()

    def feed(self, S, t):
        """tick t of the streams: the inputs, est_in as it comes, the scattered arrays back at poison (swing_in rows 0-3: the tick's flags)"""
        n = self.n
        for k in IN_ROWS:
            self.d[k].upload(np.ascontiguousarray(S[k][t][:, :n]))
        for k in SCATTERED:
            a = np.full((OUT_ROWS[k] + 1, n), POISON, f32)
            if k == "sw":
                a[0:4] = S["swing_flag"][t][:, :n]
            self.d[k].upload(a)
        self.d["est_in"].upload(np.concatenate([S["est_in"][t][:, :n], np.full((1, n), POISON, f32)]))

    def bind(self, mask):
        """robot r is reset at the next call when mask[r] (None: no binding)"""
        if mask is None:
            self.ctx.clear_stage_reset()
        else:
            self.mask.upload(np.where(mask[:self.n], 0x40, 0x01000000).astype(i32))         # a word outside `bits` is no reset
            self.ctx.set_stage_reset(mask=self.mask, bits=0xff)

    def command(self, desc, reset=0, **null):
        d = dict(self.d, **{k: None for k in null})
        self.ctx.command_update(self.n, desc, d["joy"], d["cmd_state"], state_des=d["state_des"], fe_in=d["fe"], fh_in=d["fh"], swing_vel_in=d["sv"],
                                stance_cmd=d["sc"], reset=reset)

    def inputs(self, **null):
        d = dict(self.d, **{k: None for k in null})
        self.ctx.trot_inputs(self.n, self.d["est_in"], d["est_out"], d["rpy"], d["gait_out"], gait_state=d["gait_state"], fe_in=d["fe"], fh_in=d["fh"],
                             swing_in=d["sw"], est_in_next=d["est_in"])

    def motor(self, desc, reset=0):
        d = self.d
        self.ctx.mpc_command(self.n, desc, d["tau"], d["qdes"], d["sw"], d["gait_out"], d["gait_state"], d["mem"], d["motor_cmd"], reset=reset)

    def read(self):
        out = {}
        for k in KEYS:
            a = self.d[k].download()
            assert np.all(a[-1] == (MEM_POISON if k == "mem" else POISON)), ("guard row", k)
            out[k] = a[0].copy() if k == "mem" else a[:-1].copy()
        return out


def descs(pkg, epilogue=0):
    return pkg.command_desc(**R.COMMAND_DESC), pkg.mpc_command_desc(**dict(R.MPC_COMMAND_DESC, epilogue=epilogue))


def device_run(ctx, pkg, n, epilogue=0, first=0, last=R.T_REF, fresh_at=None):
    """The three stages over ticks first..last-1 of the streams, resets as a mask (fresh_at: that tick resets everyone instead) -> [T'] stacked outputs"""
    S = R.streams()
    cd, md = descs(pkg, epilogue)
    a = Arrays(ctx, n)
    out = []
    try:
        for t in range(first, last):
            a.feed(S, t)
            everyone = t == fresh_at
            a.bind(np.ones(n, bool) if everyone else S["cmd_reset"][t]); a.command(cd)
            a.inputs()
            a.bind(np.ones(n, bool) if everyone else S["mem_reset"][t]); a.motor(md)
            out.append(a.read())
    finally:
        ctx.clear_stage_reset()
    return {k: np.stack([o[k] for o in out]) for k in KEYS}


@pytest.mark.parametrize("n,epilogue", [(130, 0), (1, 0), (130, 3)])
def test_parity(gpu_ctx, pkg, n, epilogue):
    ref = R.reference(epilogue)
    gap, bar = R.foot_world_bar(ref)
    got = device_run(gpu_ctx, pkg, n, epilogue)
    worst = R.compare(got, {k: ref[k][..., :n] for k in KEYS}, KEYS, bar, tag="n=%d epilogue=%d" % (n, epilogue))
    print("n=%d epilogue=%d: foot positions in the world frame: gap %.2e, bar %.2e, worst %.2e" % (n, epilogue, gap, bar, worst))


def test_optional_outputs(gpu_ctx, pkg):
    """Each optional output NULL in turn: the others' bits are those of the full call, the array left out keeps its poison."""
    ctx, n, t = gpu_ctx, 130, 7
    S = R.streams()
    cd, _ = descs(pkg)
    a = Arrays(ctx, n)

    def run(stage, **null):
        a.feed(S, t)
        a.d["cmd_state"].upload(np.full((7, n), POISON, f32))
        if stage == "command":
            a.command(cd, reset=1, **null)
        else:
            a.inputs(**null)
        return a.read()

    for stage, outs in (("command", ("state_des", "fe", "fh", "sv", "sc")), ("inputs", ("fe", "fh", "sw"))):
        full = run(stage)
        for k in outs:
            got = run(stage, **{k: 1})
            for j in KEYS:
                if j != k:
                    assert got[j].tobytes() == full[j].tobytes(), (stage, k, j)
            want = np.full_like(full[k], POISON)
            if k == "sw":
                want[0:4] = S["swing_flag"][t][:, :n]
            assert np.array_equal(got[k], want), (stage, k)
    # est_in_next NULL, or an array of its own: est_in stays as fed, the other array gets rows 41-44 alone
    full = run("inputs")
    a.feed(S, t)
    other = ctx.alloc((55, n)).upload(np.full((55, n), POISON, f32))
    ctx.trot_inputs(n, a.d["est_in"], a.d["est_out"], a.d["rpy"], a.d["gait_out"], gait_state=a.d["gait_state"], fe_in=a.d["fe"], est_in_next=None)
    assert np.array_equal(a.read()["est_in"], S["est_in"][t][:, :n])
    ctx.trot_inputs(n, a.d["est_in"], a.d["est_out"], a.d["rpy"], a.d["gait_out"], gait_state=a.d["gait_state"], est_in_next=other)
    o = other.download()
    assert np.array_equal(o[41:45], full["est_in"][41:45]) and np.all(np.delete(o, np.r_[41:45], axis=0) == POISON)
    # without fe_in the gait state is not needed
    ctx.trot_inputs(n, a.d["est_in"], a.d["est_out"], a.d["rpy"], a.d["gait_out"], gait_state=None, fh_in=a.d["fh"])
    assert a.read()["fh"].tobytes() == full["fh"].tobytes()


def test_scalar_reset_is_the_mask_of_everyone(gpu_ctx, pkg):
    ctx, n = gpu_ctx, 130
    S = R.streams()
    cd, md = descs(pkg)
    masked = device_run(ctx, pkg, n, first=20, last=21, fresh_at=20)
    a = Arrays(ctx, n)
    a.feed(S, 20)
    a.command(cd, reset=1); a.inputs(); a.motor(md, reset=1)
    got = a.read()
    for k in KEYS:
        assert got[k].tobytes() == masked[k][0].tobytes(), k
    # the scalar wins over a mask that names nobody; a cleared binding is ignored
    a.feed(S, 21)
    a.bind(np.zeros(n, bool)); a.command(cd, reset=1); a.inputs(); a.motor(md, reset=1)
    ctx.clear_stage_reset()
    first = a.read()
    a.feed(S, 21)
    a.command(cd, reset=1); a.inputs(); a.motor(md, reset=1)
    second = a.read()
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k
    assert np.all(first["cmd_state"][:, S["joy"][21, 7, :n] == R.JOY_STAND] == 0)


def test_a_robot_reset_at_k_is_the_robot_started_fresh_at_k(gpu_ctx, pkg):
    """Under a stage-reset binding, for the command state and the command memory: run A goes through the streams from tick 0 with their resets; run B
    starts at tick k with everyone reset.  From its reset tick k on, a robot of A that the streams reset at k (in both stages) is B's robot, bit for bit."""
    ctx, n = gpu_ctx, 130
    S = R.streams()
    A = device_run(ctx, pkg, n)
    seen = 0
    for k in (9, 23):
        B = device_run(ctx, pkg, n, first=k, fresh_at=k)
        for stage_keys, reset in ((("cmd_state", "state_des", "fe", "fh", "sv", "sc"), S["cmd_reset"]), (("mem", "motor_cmd"), S["mem_reset"])):
            robots = np.nonzero(reset[k][:n])[0]
            seen += len(robots)
            for key in stage_keys:
                rows = slice(0, 6) if key == "fe" else slice(None)               # fe rows 6-: the data-flow stage, which has no memory
                a_, b_ = A[key][k:], B[key]
                a_, b_ = (a_[:, robots], b_[:, robots]) if key == "mem" else (a_[:, rows][..., robots], b_[:, rows][..., robots])
                # B follows the streams' later resets as A does, so the two agree to the end of the run
                assert np.ascontiguousarray(a_).tobytes() == np.ascontiguousarray(b_).tobytes(), (k, key)
    assert seen >= 8


def test_refusals(gpu_ctx, pkg):
    """Every BAD_ARG case returns the code, names the argument and launches nothing: the outputs keep what they held."""
    ctx, n = gpu_ctx, 5
    S = R.streams()
    cd, md = descs(pkg)
    a = Arrays(ctx, n)
    a.feed(S, 0)
    before = a.read()

    def refused(call, name, fn):
        with pytest.raises(pkg.QrgpuError) as e:
            fn()
        assert str(e.value).startswith("BAD_ARG: %s: %s" % (call, name)), (call, name, str(e.value))
        assert ctx.last_error() == "%s: %s" % (call, name)

    d = a.d
    cmd = lambda n_=n, reset=0, **k: (lambda: ctx.command_update(n_, cd, k.get("joy", d["joy"]), k.get("st", d["cmd_state"]), state_des=d["state_des"], fe_in=d["fe"],
                                                                fh_in=d["fh"], swing_vel_in=d["sv"], stance_cmd=d["sc"], reset=reset))
    for bad_n in (0, -3, 4097):
        refused("qrgpu_command_update_batch", "n", cmd(n_=bad_n))
    for bad_reset in (2, -1):
        refused("qrgpu_command_update_batch", "reset", cmd(reset=bad_reset))
    refused("qrgpu_command_update_batch", "d_joy", cmd(joy=None)); refused("qrgpu_command_update_batch", "d_cmd_state", cmd(st=None))

    def inp(n_=n, **k):
        g = lambda key: k[key] if key in k else d[key]
        return lambda: ctx.trot_inputs(n_, g("est_in"), g("est_out"), g("rpy"), g("gait_out"), gait_state=g("gait_state"), fe_in=d["fe"], fh_in=d["fh"],
                                       swing_in=d["sw"], est_in_next=d["est_in"])
    for bad_n in (0, -3, 4097):
        refused("qrgpu_trot_inputs_batch", "n", inp(n_=bad_n))
    for key in ("est_in", "est_out", "rpy", "gait_out", "gait_state"):
        refused("qrgpu_trot_inputs_batch", "d_" + key, inp(**{key: None}))

    def mot(n_=n, reset=0, **k):
        g = lambda key: k[key] if key in k else d[key]
        return lambda: ctx.mpc_command(n_, md, g("tau"), g("qdes"), g("sw"), g("gait_out"), g("gait_state"), g("mem"), g("motor_cmd"), reset=reset)
    for bad_n in (0, -3, 4097):
        refused("qrgpu_mpc_command_batch", "n", mot(n_=bad_n))
    for bad_reset in (2, -1):
        refused("qrgpu_mpc_command_batch", "reset", mot(reset=bad_reset))
    for key, name in (("tau", "d_tau"), ("qdes", "d_qdes"), ("sw", "d_swing_in"), ("gait_out", "d_gait_out"), ("gait_state", "d_gait_state"), ("mem", "d_cmd_mem"),
                      ("motor_cmd", "d_motor_cmd")):
        refused("qrgpu_mpc_command_batch", name, mot(**{key: None}))
    import ctypes as C
    lib, p = pkg.load_library(), lambda k: C.c_void_p(d[k].ptr)
    assert lib.qrgpu_command_update_batch(ctx._h, n, None, 0, p("joy"), p("cmd_state"), p("state_des"), None, None, None, None) == BAD_ARG
    assert ctx.last_error() == "qrgpu_command_update_batch: desc"
    assert lib.qrgpu_mpc_command_batch(ctx._h, n, None, 0, p("tau"), p("qdes"), p("sw"), p("gait_out"), p("gait_state"), p("mem"), p("motor_cmd")) == BAD_ARG
    assert ctx.last_error() == "qrgpu_mpc_command_batch: desc"
    assert lib.qrgpu_command_update_batch(None, n, C.byref(cd), 0, p("joy"), p("cmd_state"), None, None, None, None, None) == BAD_ARG
    assert lib.qrgpu_trot_inputs_batch(None, n, p("est_in"), p("est_out"), p("rpy"), p("gait_out"), None, None, None, None, None) == BAD_ARG
    assert lib.qrgpu_mpc_command_batch(None, n, C.byref(md), 0, p("tau"), p("qdes"), p("sw"), p("gait_out"), p("gait_state"), p("mem"), p("motor_cmd")) == BAD_ARG
    ctx.sync()
    after = a.read()
    for k in KEYS:
        assert after[k].tobytes() == before[k].tobytes(), k
