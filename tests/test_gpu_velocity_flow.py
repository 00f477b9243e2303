"""The data-flow stage of the force-balance trot on the device (qrgpu_velocity_inputs_batch) against tests/velocity_flow_ref.py on the streams of the host
test, at n = 130 (two full waves and a ragged one) and n = 1, on terrain 0 (PLANE, no ground_out given) and terrain 3 (SLOPE).

  * parity over the 48 ticks, est_in written in place, the streams' masked resets given as a stage-reset mask and their scalar resets as the call's scalar:
    every written row bit for bit (the stage copies and compares, nothing else); every row that is not the stage's -- rows 8-19 of swing_vel_in among
    them -- and a guard row behind every array keep their poison.
  * every optional output NULL in turn: the other outputs' bits do not change; est_in_next as an array of its own; the entries without the flags.
  * the scalar reset is the mask of every robot, and wins over a mask that names nobody.
  * refusals: every BAD_ARG case names its argument and leaves the outputs untouched.
  * the consumer's guard: the stage's swing_vel_in, fed straight into qrgpu_swing_velocity_batch, gives what that kernel gives on an array the host assembled
    from the same values (desired speed in rows 24-26, twisting speed in 27, yaw rate in 23): the row layout is pinned against the kernel that reads it."""
import numpy as np
import pytest

import velocity_flow_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
POISON, MEM_POISON = R.POISON, R.MEM_POISON
BAD_ARG = 2
OUT_ROWS = dict(sv=R.SV_ROWS, est_in=R.EST_IN_ROWS, flag=4)
IN_ROWS = dict(est_out=42, ground_out=32, gait_out=24, gait_state=52, state_des=12)
KEYS = ("sv", "est_in", "mem", "flag")


class Arrays:
    """The stage's device arrays for n robots, every written one with a guard row of poison behind it."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.d = {k: ctx.alloc((r + 1, n)).upload(np.full((r + 1, n), POISON, f32)) for k, r in OUT_ROWS.items()}
        self.d.update({k: ctx.alloc((r, n)) for k, r in IN_ROWS.items()})
        self.d["mem"] = ctx.alloc((2, n), i32).upload(np.full((2, n), MEM_POISON, i32))
        self.mask = ctx.alloc((n,), i32).zero()

    def free(self):
        for v in list(self.d.values()) + [self.mask]:
            v.free()

    def feed(self, S, t):
        """tick t of the streams: the inputs, est_in as it comes, swing_vel_in and swing_flag back at poison; the memory is carried"""
        n = self.n
        for k in IN_ROWS:
            self.d[k].upload(np.ascontiguousarray(S[k][t][:, :n]))
        for k in ("sv", "flag"):
            self.d[k].upload(np.full((OUT_ROWS[k] + 1, n), POISON, f32))
        self.d["est_in"].upload(np.concatenate([S["est_in"][t][:, :n], np.full((1, n), POISON, f32)]))

    def bind(self, mask):
        """robot r is reset at the next call when mask[r] (None: no binding)"""
        if mask is None:
            self.ctx.clear_stage_reset()
        else:
            self.mask.upload(np.where(mask[:self.n], 0x40, 0x01000000).astype(i32))         # a word outside `bits` is no reset
            self.ctx.set_stage_reset(mask=self.mask, bits=0xff)

    def call(self, terrain, reset=0, n=None, **over):
        d = {**self.d, "est_in_next": self.d["est_in"], **over}
        self.ctx.velocity_inputs(self.n if n is None else n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["state_des"],
                                 ground_out=d["ground_out"] if terrain >= 2 else over.get("ground_out"), swing_vel_in=d["sv"], est_in_next=d["est_in_next"],
                                 cmd_mem=d["mem"], swing_flag=d["flag"], terrain=terrain, reset=reset)

    def read(self):
        out = {}
        for k in KEYS:
            a = self.d[k].download()
            assert np.all(a[-1] == (MEM_POISON if k == "mem" else POISON)), ("guard row", k)
            out[k] = a[0].copy() if k == "mem" else a[:-1].copy()
        return out


def device_run(ctx, n, terrain, first=0, last=R.T_REF, everyone_masked_at=None):
    """The stage over ticks first..last-1 of the streams (everyone_masked_at: at that tick the mask names every robot and the scalar is 0) -> [T'] outputs"""
    S = R.streams()
    a = Arrays(ctx, n)
    out = []
    try:
        for t in range(first, last):
            a.feed(S, t)
            if t == everyone_masked_at:
                a.bind(np.ones(n, bool)); a.call(terrain, reset=0)
            else:
                a.bind(S["mask_reset"][t]); a.call(terrain, reset=int(S["scalar_reset"][t]))
            out.append(a.read())
    finally:
        ctx.clear_stage_reset()
        a.free()
    return {k: np.stack([o[k] for o in out]) for k in KEYS}


@pytest.mark.parametrize("n,terrain", [(130, R.PLANE), (130, R.SLOPE), (1, R.PLANE), (1, R.SLOPE)])
def test_parity(gpu_ctx, n, terrain):
    ref = R.reference(terrain)
    got = device_run(gpu_ctx, n, terrain)
    for k in KEYS:
        R.same_bits(got[k], ref[k][..., :n], tag="n=%d terrain=%d %s" % (n, terrain, k))
    assert np.all(got["sv"][:, 8:20] == POISON)                                    # the swing update's rows


def test_optional_outputs(gpu_ctx):
    """Each optional output NULL in turn: the others' bits are those of the full call, the array left out keeps what it held."""
    ctx, n, t, terrain = gpu_ctx, 130, 7, R.SLOPE
    S = R.streams()
    a = Arrays(ctx, n)
    start = (np.arange(n) % 16).astype(i32)

    def run(**over):
        a.feed(S, t)
        a.d["mem"].upload(np.stack([start, np.full(n, MEM_POISON, i32)]))
        a.call(terrain, **over)
        return a.read()

    full = run()
    want = R.velocity_inputs(terrain, S["est_in"][t], S["est_out"][t], S["ground_out"][t], S["gait_out"][t], S["gait_state"][t], S["state_des"][t], start,
                             np.zeros(n, bool))
    R.same_bits(full["sv"], R.fill(R.SV_ROWS, n, want["sv"])); R.same_bits(full["mem"], want["mem"]); R.same_bits(full["flag"], want["flag"])
    untouched = dict(sv=np.full((R.SV_ROWS, n), POISON, f32), est_in=np.array(S["est_in"][t]), mem=start, flag=np.full((4, n), POISON, f32))
    for name, key in (("sv", "sv"), ("est_in_next", "est_in"), ("flag", "flag")):
        got = run(**{name: None})
        for j in KEYS:
            R.same_bits(got[j], untouched[j] if j == key else full[j], tag="%s NULL: %s" % (name, j))
    got = run(mem=None, flag=None)                                                 # neither the entries nor the flags
    for j in KEYS:
        R.same_bits(got[j], untouched[j] if j in ("mem", "flag") else full[j], tag="mem, flag NULL: %s" % j)
    # est_in_next as an array of its own: est_in stays as fed, the other array gets rows 41-44 alone
    other = ctx.alloc((55, n)).upload(np.full((55, n), POISON, f32))
    got = run(est_in_next=other)
    o = other.download()
    assert np.array_equal(got["est_in"], S["est_in"][t]) and np.array_equal(o[41:45], full["est_in"][41:45])
    assert np.all(np.delete(o, np.r_[41:45], axis=0) == POISON)
    for j in ("sv", "mem", "flag"):
        R.same_bits(got[j], full[j], tag="est_in_next apart: %s" % j)
    # on the horizontal terrains ground_out is not read: given or not, the same bits
    a.feed(S, t); a.call(R.PLUM_PILES, ground_out=None); flat = a.read()
    a.feed(S, t); a.call(R.PLUM_PILES, ground_out=a.d["ground_out"]); given = a.read()
    for j in ("sv", "flag"):
        R.same_bits(flat[j], given[j], tag="ground_out on terrain 1: %s" % j)
    assert np.all(flat["sv"][28] == 1) and np.all(flat["sv"][29] == 0) and np.all(flat["sv"][37] == 1) and np.all(flat["sv"][38:41] == 0)
    other.free(); a.free()


def test_scalar_reset_is_the_mask_of_everyone(gpu_ctx):
    ctx, n, terrain = gpu_ctx, 130, R.PLANE
    S = R.streams()
    t = 23
    assert not S["scalar_reset"][t] and 0 < S["mask_reset"][t].sum() < n
    A = device_run(ctx, n, terrain, last=t + 1)                                    # the streams' own resets: some robots masked at t
    M = device_run(ctx, n, terrain, last=t + 1, everyone_masked_at=t)              # everyone masked at t
    # everyone reset by the scalar at t, from the memory tick t - 1 left, under no binding and under a mask that names nobody
    for mask in (None, np.zeros(n, bool)):
        a = Arrays(ctx, n)
        try:
            a.feed(S, t)
            a.d["mem"].upload(np.stack([A["mem"][t - 1], np.full(n, MEM_POISON, i32)]))
            a.bind(mask); a.call(terrain, reset=1)
            got = a.read()
        finally:
            ctx.clear_stage_reset(); a.free()
        for k in KEYS:
            R.same_bits(got[k], M[k][t], tag="scalar against the mask of everyone: %s" % k)
    assert np.any(M["mem"][t] != A["mem"][t])                                      # the reset of the others shows
    masked = S["mask_reset"][t][:n]
    assert np.array_equal(M["mem"][t][masked], A["mem"][t][masked])                # a robot the streams mask at t is the robot of a run reset at t


def test_refusals(gpu_ctx, pkg):
    """Every BAD_ARG case returns the code, names the argument and launches nothing: the outputs keep their poison."""
    ctx, n = gpu_ctx, 5
    S = R.streams()
    a = Arrays(ctx, n)
    a.feed(S, 0)
    before = a.read()
    d = a.d

    def refused(name, terrain=R.SLOPE, reset=0, n_=n, **over):
        with pytest.raises(pkg.QrgpuError) as e:
            a.call(terrain, reset=reset, n=n_, **over)
        assert str(e.value).startswith("BAD_ARG: qrgpu_velocity_inputs_batch: %s" % name), (name, str(e.value))
        assert ctx.last_error() == "qrgpu_velocity_inputs_batch: %s" % name

    for bad_n in (0, -3, 4097):
        refused("n", n_=bad_n)
    for bad_reset in (2, -1):
        refused("reset", reset=bad_reset)
    for bad_terrain in (-1, 5):
        refused("terrain", terrain=bad_terrain)
    for key in ("est_in", "est_out", "gait_out", "gait_state", "state_des"):
        refused("d_" + key, **{key: None})
    refused("d_ground_out", terrain=R.STAIRS, ground_out=None)
    refused("d_cmd_mem", mem=None)                                                 # the flags need the entries
    import ctypes as C
    lib, p = pkg.load_library(), lambda k: C.c_void_p(d[k].ptr)
    assert lib.qrgpu_velocity_inputs_batch(None, n, 0, 0, p("est_in"), p("est_out"), None, p("gait_out"), p("gait_state"), p("state_des"), p("sv"), p("est_in"),
                                           p("mem"), p("flag")) == BAD_ARG
    ctx.sync()
    after = a.read()
    for k in KEYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert np.all(after["sv"] == POISON) and np.all(after["flag"] == POISON) and np.all(after["mem"] == MEM_POISON)
    a.free()


@pytest.mark.parametrize("terrain", [R.PLANE, R.SLOPE])
def test_the_output_is_what_the_swing_velocity_kernel_reads(gpu_ctx, pkg, terrain):
    """X is a swing_vel_in as the consumer's own tests assemble it on the host (workload.make_swing_velocity_batch: yaw rate in row 23, desired speed in
    24-26, twisting speed in 27).  Its values are handed to the stage where the stage reads them -- est_out 6-8, est_in 6-9, 12 and 17-28, state_des 6, 7, 8,
    11, ground_out 22-30, normalizedPhase, leg states that give X's flags -- and the stage writes into an array that holds X's rows 8-19 and poison
    elsewhere.  qrgpu_swing_velocity_batch on that array and on X must write the same bits."""
    ctx, W, n = gpu_ctx, pkg.workload, 130
    X = W.make_swing_velocity_batch(n, seed=77).T.copy()                           # [53][n]
    if terrain < 2:                                                                # what the reference feeds the formula on horizontal terrain
        X[28:37] = np.eye(3, dtype=f32).reshape(9, 1); X[37:41] = np.array([1, 0, 0, 0], f32)[:, None]
    assert np.abs(X[24] - X[23]).min() > 0 and np.abs(X[27] - X[26]).min() > 0     # a row shifted by one would show
    rng = np.random.default_rng(5)
    est_in, est_out, ground = rng.uniform(-1, 1, (54, n)).astype(f32), rng.uniform(-1, 1, (42, n)).astype(f32), rng.uniform(-1, 1, (32, n)).astype(f32)
    gait_out, gait_state, des = rng.uniform(0, 1, (24, n)).astype(f32), np.ones((52, n), f32), rng.uniform(-1, 1, (12, n)).astype(f32)
    est_out[6:9] = X[20:23]; est_in[12] = X[23]; des[6:9] = X[24:27]; des[11] = X[27]; ground[22:31] = X[28:37]; est_in[6:10] = X[37:41]; est_in[17:29] = X[41:53]
    gait_out[4:8] = X[4:8]
    gait_out[12:16] = np.where(X[0:4] != 0, R.SWING, R.STANCE)                     # allowSwitchLegState 1: a stance leg is out of swingFootIds
    gait_out[8:12] = gait_out[12:16]
    sv0 = np.full((53, n), POISON, f32); sv0[8:20] = X[8:20]
    vdesc = W.swing_velocity_cfg("a1")
    ecfg = W.estimator_cfg("a1")
    up = lambda a, dt=f32: ctx.alloc(a.shape, dt).upload(a)
    d = dict(est_in=up(est_in), est_out=up(est_out), ground=up(ground), gait_out=up(gait_out), gait_state=up(gait_state), des=up(des), sv=up(sv0), X=up(X),
             out_stage=up(np.full((48, n), POISON, f32)), out_host=up(np.full((48, n), POISON, f32)))
    try:
        ctx.velocity_inputs(n, d["est_in"], d["est_out"], d["gait_out"], d["gait_state"], d["des"], ground_out=d["ground"] if terrain >= 2 else None,
                            swing_vel_in=d["sv"], terrain=terrain)
        ctx.swing_velocity_batch(n, ecfg, vdesc, d["sv"], d["out_stage"])
        ctx.swing_velocity_batch(n, ecfg, vdesc, d["X"], d["out_host"])
        ctx.sync()
        R.same_bits(d["sv"].download(), X, tag="swing_vel_in")
        a, b = d["out_stage"].download(), d["out_host"].download()
        R.same_bits(a, b, tag="the consumer's output")
        flagged = np.repeat(X[0:4] != 0, 3, axis=0)                                # [12][n]
        assert flagged.any() and np.all(a[24:36][~flagged] == POISON) and np.isfinite(a[24:36][flagged]).all()
    finally:
        for v in d.values():
            v.free()
