"""The sensor stage on the device (qrgpu_observe_batch) against tests/observe_ref.py, against its own scalar reset, and in the chain plant -> observe ->
ground -> estimator -> pack.

  * parity on both variants (and the sim class under yaw offsets beyond 2 pi) at n = 1, 63, 64, 65, 130 over the 48-tick streams: rows reached by
    + - x / alone bit for bit, rows behind a transcendental function under the bars of test_observe_host.py (8 x the reference's float32-vs-float64 gap,
    never under 2e-6); est_in aliasing the raw rows and apart, bits identical between the two; rows 41-53 of est_in and a guard row on every array
    untouched; once with noise.
  * the optional arrays left out: the other outputs' bits do not change; a reset robot's base position is (0, 0, base_height).
  * reset, bit for bit, the oracle being the stage's own scalar path: after 25 unbound ticks one bound call with scalar reset 0 equals, robot by robot,
    the unbound call with reset = 1 (masked robots) or 0 (the others) on copies of the same arrays; mask patterns; the scalar wins; a cleared binding
    is ignored; a robot masked at tick k is from k on the robot of a run started fresh at k.
  * chain: 64 robots dropped onto the plant's PD hold, 40 ticks, no controller: pipeline A keeps every array on the device, pipeline B puts the same
    plant rows through observe_ref on the host; est_out, mpc_state and fb_state agree within 1e-5 (2e-5 on est_out rows 36-41).
  * refusals: every BAD_ARG case names its argument and launches nothing.

Measured on an MI355X (worst device-vs-reference distance over the cases; bars in test_observe_host.py): rpy 9.5e-7 (bar 3.2e-6 .. 7.1e-6), quaternion
5.1e-7 (2.0e-6 .. 3.5e-6), foot positions 1.2e-7 (2.0e-6), rpy filter state 3.8e-6 (3.8e-5 .. 4.0e-5); chain A vs B at the last tick: est_out 2.4e-7,
mpc_state 2.4e-7, fb_state 1.5e-7.  The distance of both pipelines from the plant's truth after the 40 ticks of the drop is printed (velocity 0.39 m/s,
feet 4.8e-3 m, rpy 3.2e-3 rad; the quaternion's 2.0 is the sign: rpyToQuat gives w >= 0), not asserted."""
import numpy as np
import pytest

import observe_ref as OR

pytestmark = pytest.mark.gpu

f32, f64, i32, u32 = np.float32, np.float64, np.int32, np.uint32
POISON = f32(-12345.5)
TICK_POISON = u32(0xDEADBEEF)
BITS, OUTSIDE = 0xff, 0x01000000
BAD_ARG = 2


class Arrays:
    """The stage's device arrays for n robots, each with a guard row of poison behind it; raw apart from est_in or (alias) inside it."""

    def __init__(self, ctx, n, rows, alias):
        self.ctx, self.n, self.rows, self.alias = ctx, n, rows, alias
        mk = lambda r, dt=f32, fill=POISON: ctx.alloc((r + 1, n), dt).upload(np.full((r + 1, n), fill, dt))
        self.st, self.est, self.rpy, self.gin, self.prev = mk(rows), mk(54), mk(3), mk(23), mk(42)
        self.tick = mk(1, u32, TICK_POISON)
        self.raw = self.est if alias else mk(41)
        self.est_host = np.full((55, n), POISON, f32)

    def feed(self, x_raw, prev=None):
        """x_raw [n, 41] of this tick (prev [n, 3]) -> the device"""
        if self.alias:
            self.est_host[0:41] = x_raw.T
            self.est.upload(self.est_host)
        else:
            self.raw.upload(np.concatenate([x_raw.T, np.full((1, self.n), POISON, f32)]))
        if prev is not None:
            p = np.full((43, self.n), POISON, f32); p[36:39] = prev.T
            self.prev.upload(p)

    def call(self, desc, reset, step, gin=True, tick=True, prev=False):
        self.ctx.observe_batch(self.n, desc, self.raw, self.st, self.est, self.rpy, ground_in=self.gin if gin else None, tick=self.tick if tick else None,
                               est_out_prev=self.prev if prev else None, reset=reset, step=step)

    def read(self):
        """-> dict of the arrays as [n, rows], guard rows checked"""
        st, est, rpy, gin, tick = self.st.download(), self.est.download(), self.rpy.download(), self.gin.download(), self.tick.download()
        for a in (st, est, rpy, gin):
            assert np.all(a[-1] == POISON), "guard row"
        assert np.all(tick[-1] == TICK_POISON) and np.all(est[41:54] == POISON), "guard row / rows 41-53 of est_in"
        if not self.alias:
            assert np.all(self.raw.download()[-1] == POISON)
        self.est_host = est
        return dict(st_raw=st[:-1].copy(), est=est[:54].T.copy(), rpy=rpy[:3].T.copy(), gin=gin[:23].T.copy(), tick=tick[0].copy(), state=st[:-1].T.copy(),
                    count=st[0].view(u32).copy())

    def snapshot(self):
        return dict(st=self.st.download(), est=self.est.download(), rpy=self.rpy.download(), gin=self.gin.download(), tick=self.tick.download())

    def restore(self, s):
        self.st.upload(s["st"]); self.est.upload(s["est"]); self.rpy.upload(s["rpy"]); self.gin.upload(s["gin"]); self.tick.upload(s["tick"])
        self.est_host = s["est"].copy()


def device_run(ctx, pkg, d, raw, alias, steps=None, first=0, last=None, prev=None):
    """the stage over ticks first..last-1 of raw [T, n, 41], the first call with reset = 1 -> per-tick dicts stacked [T', n, rows]"""
    n = raw.shape[1]
    last = raw.shape[0] if last is None else last
    desc = OR.to_struct(pkg, d)
    rows = ctx.observe_state_rows(desc)
    assert rows == (OR.ROWS_MV if d["filter_motor_velocity"] else OR.ROWS)
    a = Arrays(ctx, n, rows, alias)
    out = []
    for t in range(first, last):
        a.feed(raw[t], None if prev is None else prev[t])
        a.call(desc, t == first, t if steps is None else int(steps[t]), prev=prev is not None)
        out.append(a.read())
    return {k: np.stack([o[k] for o in out]) for k in out[0]}, a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


KEYS = ("est", "rpy", "gin", "tick", "state")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("case", list(OR.CASES))
def test_parity_with_observe_ref(gpu_ctx, pkg, case, n):
    raw, _ = OR.streams(OR.N_REF)
    ref = OR.reference(case)
    want = {k: ref[k][:, :n] for k in ("est", "rpy", "gin", "tick", "count")}
    want["state"] = ref["state"][:, :n].astype(f32)
    rows = want["state"].shape[2]
    apart, _ = device_run(gpu_ctx, pkg, OR.CASES[case], raw[:, :n], alias=False)
    alias, _ = device_run(gpu_ctx, pkg, OR.CASES[case], raw[:, :n], alias=True)
    for k in KEYS:
        assert same_bits(apart[k], alias[k]), ("est_in aliasing d_raw changed bits", k)
    worst = OR.compare(apart, want, case, rows, tag="n=%d" % n)
    print("%s n=%d " % (case, n) + "  ".join("%s %.2e" % kv for kv in worst.items()))


@pytest.mark.parametrize("case", ["sim", "hardware"])
def test_parity_with_noise(gpu_ctx, pkg, case):
    raw, _ = OR.streams(OR.N_REF)
    d = dict(OR.CASES[case], **OR.NOISE)
    ref = OR.reference(case, f32, True)
    want = dict(ref, state=ref["state"].astype(f32))
    got, _ = device_run(gpu_ctx, pkg, d, raw, alias=True)
    OR.compare(got, want, case, want["state"].shape[2], tag="noise")
    # the drawn values: row = raw + amplitude * s, one float32 product and one float32 sum of floats exact on both sides
    for t in (0, 20, 47):
        s = OR.noise_of(d, OR.N_REF, t).astype(f32)
        assert same_bits(got["est"][t, :, 0:3], raw[t, :, 0:3] + f32(d["acc_noise"]) * s[:, 0, 0:3])
        assert same_bits(got["est"][t, :, 17:29], raw[t, :, 17:29] + f32(d["q_noise"]) * s[:, 2:5].reshape(-1, 12))
    # the noise does not depend on n or on the history: 7 robots alone, started 9 ticks later with the same loop counts
    few, _ = device_run(gpu_ctx, pkg, d, raw[:, :7], alias=False, first=9)
    for rows in (slice(0, 3), slice(17, 29)):
        assert same_bits(few["est"][:, :, rows], got["est"][9:, :7, rows])
    # an amplitude of 0 leaves the row's bits alone
    clean, _ = device_run(gpu_ctx, pkg, dict(d, q_noise=0.0, acc_noise=0.0), raw[:3], alias=False)
    assert same_bits(clean["est"][:, :, 0:3], raw[:3, :, 0:3]) and same_bits(clean["est"][:, :, 17:29], raw[:3, :, 17:29])


def test_optional_arrays_left_out(gpu_ctx, pkg):
    raw, _ = OR.streams(OR.N_REF)
    n, T = 65, 12
    d = OR.CASES["sim"]
    desc = OR.to_struct(pkg, d)
    rng = np.random.default_rng(3)
    prev = rng.uniform(-2, 2, (T, n, 3)).astype(f32)
    full, a = device_run(gpu_ctx, pkg, d, raw[:T, :n], alias=False, prev=prev)
    assert np.all(full["gin"][0, :, 16:19] == np.array([0, 0, 0.27], f32)) and same_bits(full["gin"][1:, :, 16:19], prev[1:])
    # no ground_in, no tick, no previous estimate: est_in, rpy and the state have the same bits, the arrays left out keep their poison
    b = Arrays(gpu_ctx, n, a.rows, alias=False)
    for t in range(T):
        b.feed(raw[t, :n])
        b.call(desc, t == 0, t, gin=False, tick=False, prev=False)
        got = b.read()
        for k in ("est", "rpy", "state"):
            assert same_bits(got[k], full[k][t]), (k, t)
        assert np.all(got["gin"] == POISON) and np.all(got["tick"] == TICK_POISON)
    # without the previous estimate the base position is (0, 0, base_height) at every tick; a robot reset by the scalar gets it with the array given
    none, _ = device_run(gpu_ctx, pkg, d, raw[:T, :n], alias=True)
    assert np.all(none["gin"][:, :, 16:19] == np.array([0, 0, 0.27], f32))
    for k in ("est", "rpy", "state", "tick"):
        assert same_bits(none[k], full[k]), k
    a.feed(raw[T, :n], prev[0])
    a.call(desc, True, T, prev=True)
    assert np.all(a.read()["gin"][:, 16:19] == np.array([0, 0, 0.27], f32))


def masks(n):
    r = np.arange(n)
    one = lambda j: np.where(r == j, 0x10, OUTSIDE).astype(i32)
    return dict(none=np.zeros(n, i32), all=np.full(n, 0x80, i32), alternating=np.where(r % 2 == 1, 0x01, OUTSIDE).astype(i32), r63=one(63), r64=one(64), r129=one(129),
                outside=np.full(n, OUTSIDE, i32))


@pytest.fixture(scope="module")
def built_up(gpu_ctx, pkg):
    """variant -> the arrays after T = 25 unbound ticks, their snapshot, and the scalar path's answers to tick 25 with reset = 1 and reset = 0"""
    raw, _ = OR.streams(OR.N_REF)
    T = 25
    rng = np.random.default_rng(11)
    prev = rng.uniform(-2, 2, (T + 1, OR.N_REF, 3)).astype(f32)
    out = {}
    gpu_ctx.clear_stage_reset()
    for case in ("sim", "hardware"):
        d = dict(OR.CASES[case], **OR.NOISE)
        desc = OR.to_struct(pkg, d)
        _, a = device_run(gpu_ctx, pkg, d, raw, alias=True, last=T, prev=prev)
        snap = a.snapshot()
        ans = {}
        for reset in (1, 0):
            a.restore(snap); a.feed(raw[T], prev[T]); a.call(desc, bool(reset), T, prev=True)
            ans[reset] = a.read()
        assert not same_bits(ans[0]["state"], ans[1]["state"])
        out[case] = dict(a=a, snap=snap, ans=ans, desc=desc, x=raw[T], prev=prev[T], T=T)
    return out


@pytest.mark.parametrize("pattern", list(masks(OR.N_REF)))
@pytest.mark.parametrize("case", ["sim", "hardware"])
def test_a_masked_robot_is_reset_as_by_the_scalar(gpu_ctx, pkg, built_up, case, pattern):
    b = built_up[case]
    a, n = b["a"], OR.N_REF
    mask = masks(n)[pattern]
    d_mask = gpu_ctx.alloc((n,), i32).upload(mask)
    m = (mask.astype(np.int64) & BITS) != 0
    try:
        gpu_ctx.set_stage_reset(mask=d_mask, bits=BITS)
        a.restore(b["snap"]); a.feed(b["x"], b["prev"]); a.call(b["desc"], False, b["T"], prev=True)
        got = a.read()
        for k in KEYS:                                                                # every array is [n] or [n, rows] here
            want = np.where(m if got[k].ndim == 1 else m[:, None], b["ans"][1][k], b["ans"][0][k])
            assert same_bits(got[k], want), (case, pattern, k)
        # the scalar reset wins over the mask; with the binding cleared the mask is ignored
        a.restore(b["snap"]); a.feed(b["x"], b["prev"]); a.call(b["desc"], True, b["T"], prev=True)
        got = a.read()
        assert all(same_bits(got[k], b["ans"][1][k]) for k in KEYS)
        gpu_ctx.clear_stage_reset()
        a.restore(b["snap"]); a.feed(b["x"], b["prev"]); a.call(b["desc"], False, b["T"], prev=True)
        got = a.read()
        assert all(same_bits(got[k], b["ans"][0][k]) for k in KEYS)
    finally:
        gpu_ctx.clear_stage_reset()
        d_mask.free()


@pytest.mark.parametrize("case", ["sim", "hardware"])
def test_a_masked_robot_forgets_its_history(gpu_ctx, pkg, case):
    """Robots masked at tick k = 17 are, from k on, bit for bit the robots of a run started fresh at k on the same inputs and loop counts."""
    raw, _ = OR.streams(OR.N_REF)
    n, k, T = OR.N_REF, 17, 40
    d = dict(OR.CASES[case], **OR.NOISE)
    desc = OR.to_struct(pkg, d)
    mask = masks(n)["alternating"]
    m = (mask & BITS) != 0
    d_mask = gpu_ctx.alloc((n,), i32).upload(np.zeros(n, i32))
    a = Arrays(gpu_ctx, n, gpu_ctx.observe_state_rows(desc), alias=True)
    bound = []
    try:
        gpu_ctx.set_stage_reset(mask=d_mask, bits=BITS)
        for t in range(T):
            d_mask.upload(mask if t == k else np.full(n, OUTSIDE, i32))
            a.feed(raw[t]); a.call(desc, t == 0, t)
            bound.append(a.read())
    finally:
        gpu_ctx.clear_stage_reset()
        d_mask.free()
    fresh, _ = device_run(gpu_ctx, pkg, d, raw, alias=True, first=k, last=T)
    for key in KEYS:
        got = np.stack([o[key] for o in bound[k:]])
        assert same_bits(got[:, m], fresh[key][:, m]), key
    assert not same_bits(np.stack([o["state"] for o in bound[k:]])[:, ~m], fresh["state"][:, ~m])


def test_chain_from_the_plant_to_the_packed_state(gpu_ctx, pkg):
    """A: plant -> observe_batch -> ground_update_batch -> estimator_update_batch -> pack_state_batch, no host copy between the stages.  B: the same plant
    rows downloaded each tick, put through observe_ref on the host, uploaded, then the same three library stages.  The robots are dropped from 0.30 m
    onto the joint PD hold at the stand pose, headings all round the circle, no controller: nothing rests on stability."""
    ctx, W = gpu_ctx, pkg.workload
    n, T, win = 64, 40, 16
    ctx.clear_stage_reset()
    ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
    cfg = W.estimator_cfg("a1", window=win)
    com = np.asarray(W.ROBOTS["a1"]["com_offset"], f32)
    d = OR.desc("sim")
    desc = OR.to_struct(pkg, d)
    rng = np.random.default_rng(8)
    yaw = np.linspace(-3.1, 3.1, n)
    fb0 = np.zeros((37, n), f32); fb0[0] = np.cos(yaw / 2); fb0[3] = np.sin(yaw / 2); fb0[6] = 0.30; fb0[13:25] = np.tile([0.0, 0.8, -1.6], 4)[:, None]
    fb0[10:12] = rng.uniform(-0.3, 0.3, (2, n))
    cmd0 = np.zeros((60, n), f32); cmd0[0:12] = fb0[13:25]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
    d_fb, d_cmd, d_truth = ctx.alloc((37, n)).upload(fb0), ctx.alloc((60, n)).upload(cmd0), ctx.alloc((28, n))
    params = pkg.plant_params(dt=0.002, substeps=2)
    est0 = np.zeros((54, n), f32); est0[41:45] = 1.0                                  # STANCE, uploaded once
    nd = ctx.estimator_state_doubles(win)

    def pipeline():
        return dict(raw=ctx.alloc((54, n)).upload(est0), est_in=ctx.alloc((54, n)).upload(est0), rpy=ctx.alloc((3, n)), gin=ctx.alloc((23, n)), tick=ctx.alloc((n,), u32),
                    gst=ctx.alloc((13, n), f64).upload(np.full((13, n), np.nan)), est_state=ctx.alloc((nd, n), f64).upload(np.zeros((nd, n))),
                    est_out=ctx.alloc((42, n)).upload(np.zeros((42, n), f32)), mpc=ctx.alloc((28, n)), fb=ctx.alloc((37, n)))

    def tail(p, k):
        ctx.ground_update_batch(n, p["gin"], p["gst"], None, p["est_in"], reset=k == 0)
        ctx.estimator_update_batch(n, cfg, p["est_in"], p["tick"], p["est_state"], p["est_out"])
        ctx.pack_state_batch(n, com, p["est_in"], p["est_out"], p["rpy"], p["mpc"], p["fb"])

    A, B = pipeline(), pipeline()
    obs_state = ctx.alloc((ctx.observe_state_rows(desc), n)).upload(np.full((OR.ROWS, n), np.nan, f32))
    ob = OR.Observer(n, d)
    for k in range(T):
        ctx.plant_step_batch(n, params, d_fb, d_cmd, mpc_state=d_truth, est_in=A["raw"])
        ctx.observe_batch(n, desc, A["raw"], obs_state, A["est_in"], A["rpy"], ground_in=A["gin"], tick=A["tick"], est_out_prev=A["est_out"], reset=k == 0, step=k)
        tail(A, k)
        x = A["raw"].download()[0:41].T                                               # B: the host's observe on the same plant rows
        o = ob.tick(x, np.full(n, k == 0), k, B["est_out"].download()[36:39].T)
        e = est0.copy(); e[0:41] = o["est"].T
        e[45:54] = B["est_in"].download()[45:54]                                      # the ground stage's rows stay the device's
        B["est_in"].upload(e); B["rpy"].upload(o["rpy"].T); B["gin"].upload(o["gin"].T); B["tick"].upload(o["tick"])
        tail(B, k)
        ea, eb = A["est_out"].download(), B["est_out"].download()
        ma, mb, fa, fb_ = A["mpc"].download(), B["mpc"].download(), A["fb"].download(), B["fb"].download()
        assert np.isfinite(ma).all() and np.isfinite(fa).all()
        e1 = np.abs(ea[0:36] - eb[0:36]).max(); m1 = np.abs(ma - mb).max(); f1 = np.abs(fa - fb_).max()
        assert np.allclose(ea[36:42], eb[36:42], rtol=0, atol=2e-5, equal_nan=True), (k, np.nanmax(np.abs(ea[36:42] - eb[36:42])))
        assert e1 <= 1e-5 and m1 <= 1e-5 and f1 <= 1e-5, (k, e1, m1, f1)
    truth = d_truth.download()
    names = dict(position=slice(0, 3), velocity=slice(3, 6), quaternion=slice(6, 10), omega=slice(10, 13), feet=slice(13, 25), rpy=slice(25, 28))
    print("after %d ticks, |estimated - true| max:  " % T + "  ".join("%s A %.2e B %.2e" % (nm, np.abs(ma[s] - truth[s]).max(), np.abs(mb[s] - truth[s]).max())
                                                                      for nm, s in names.items()))
    print("A vs B at the last tick: est_out %.2e  mpc_state %.2e  fb_state %.2e" % (e1, m1, f1))


def test_refusals(gpu_ctx, pkg):
    """Every BAD_ARG case returns the code, names the argument and launches nothing: the outputs keep their poison."""
    ctx, n = gpu_ctx, 5
    a = Arrays(ctx, n, OR.ROWS_MV, alias=False)
    x = OR.streams(OR.N_REF)[0][0, :n]
    a.feed(x)
    before = a.snapshot()
    good = pkg.observe_desc("hardware")

    def refused(name, desc=good, n_=n, **null):
        arr = dict(raw=a.raw, st=a.st, est=a.est, rpy=a.rpy)
        arr.update({k: None for k in null})
        with pytest.raises(pkg.QrgpuError) as e:
            ctx.observe_batch(n_, desc, arr["raw"], arr["st"], arr["est"], arr["rpy"], ground_in=a.gin, tick=a.tick, reset=True, step=0)
        assert str(e.value).startswith("BAD_ARG: qrgpu_observe_batch: " + name), (name, str(e.value))
        assert ctx.last_error() == "qrgpu_observe_batch: " + name

    refused("n", n_=0); refused("n", n_=-3); refused("n", n_=4097)
    refused("d_raw", raw=1); refused("d_obs_state", st=1); refused("d_est_in", est=1); refused("d_rpy", rpy=1)
    refused("tick_ms", desc=pkg.observe_desc("sim", tick_ms=0))
    for k in ("acc_noise", "gyro_noise", "q_noise", "qd_noise"):
        for v in (-0.1, float("nan"), float("inf")):
            refused(k, desc=pkg.observe_desc("sim", **{k: v}))
    for k in ("yaw_offset", "base_height", "hip_l", "upper_l", "lower_l"):
        for v in (float("nan"), float("-inf")):
            refused(k, desc=pkg.observe_desc("sim", **{k: v}))
    ho = list(OR.HIP_OFFSET); ho[7] = float("nan")
    refused("hip_offset", desc=pkg.observe_desc("sim", hip_offset=ho))
    lib = pkg.load_library()
    import ctypes as C
    rc = lib.qrgpu_observe_batch(ctx._h, n, None, 1, 0, C.c_void_p(a.raw.ptr), None, C.c_void_p(a.st.ptr), C.c_void_p(a.est.ptr), C.c_void_p(a.rpy.ptr), None, None)
    assert rc == BAD_ARG and "qrgpu_observe_batch: desc" in ctx.last_error()
    assert lib.qrgpu_observe_batch(None, n, C.byref(good), 1, 0, C.c_void_p(a.raw.ptr), None, C.c_void_p(a.st.ptr), C.c_void_p(a.est.ptr), C.c_void_p(a.rpy.ptr), None, None) == BAD_ARG
    assert lib.qrgpu_observe_state_rows(None) == 0 and ctx.observe_state_rows(good) == OR.ROWS_MV and ctx.observe_state_rows(pkg.observe_desc("sim")) == OR.ROWS
    ctx.sync()
    after = a.snapshot()
    assert all(same_bits(before[k], after[k]) for k in before)
    # and the call that is accepted does launch
    ctx.observe_batch(n, good, a.raw, a.st, a.est, a.rpy, ground_in=a.gin, tick=a.tick, reset=True, step=0)
    assert np.all(a.read()["tick"] == 2)
