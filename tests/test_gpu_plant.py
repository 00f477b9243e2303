"""-m gpu: the batched plant -- qrgpu_forward_dynamics_batch and qrgpu_plant_step_batch -- against the float64 mechanics of tests/plant_ref.py,
standing on joint PD, and in closed loop with the MPC + WBC tick, entirely on the device.

Bars: 1e-6 * max(1, |ref|) per component, the float32 output's rounding (6e-8) with the margin the project gives its torque bar."""
import ctypes as C

import numpy as np
import pytest

import gpu_helpers as G
import plant_ref as PR
import rigid_body_ref as M

pytestmark = pytest.mark.gpu

BAR = 1e-6


def _setup_both(ctx, pkg):
    for t, robot in enumerate(PR.ROBOTS):
        ctx.mpc_setup_packed(t, pkg.mpc_cfg(robot), PR.HORIZON); ctx.wbc_setup_packed(t, pkg.model_desc(robot))


def _interleave(a, b):
    out = np.empty((len(a) + len(b),) + a.shape[1:], a.dtype)
    out[0::2] = a; out[1::2] = b
    return out


def _worst(got, ref):
    """max over components of |got - ref| / max(1, |ref|), and where."""
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float(e.max()), np.unravel_index(int(e.argmax()), e.shape)


def _fwd(ctx, pkg, state, tau, ff, tid):
    """qrgpu_forward_dynamics_batch on robot-major host arrays.  -> nu_dot [n, 18] float32, status [n]"""
    n = len(state)
    S = pkg.to_soa
    d = dict(s=ctx.alloc((37, n)).upload(S(state)), t=ctx.alloc((12, n)).upload(S(tau)), f=None if ff is None else ctx.alloc((12, n)).upload(S(ff)),
             o=ctx.alloc((18, n)).upload(np.full((18, n), np.nan, np.float32)), st=ctx.alloc((n,), np.int32).upload(np.full(n, -1, np.int32)),
             tid=ctx.alloc((n,), np.int32).upload(tid))
    ctx.forward_dynamics_batch(n, d["s"], d["t"], d["o"], foot_force=d["f"], status=d["st"], type_id=d["tid"])
    ctx.sync()
    out = d["o"].download().T.copy(), d["st"].download()
    for v in d.values():
        if v is not None:
            v.free()
    return out


@pytest.fixture(scope="module")
def fd(gpu_ctx, pkg):
    """One mixed batch, A1 = type 0 at even places and Lite3 = type 1 at odd ones, the stand, wide and edge families of each (the batch of
    test_gpu_rigid_body.py: n = 239), random torques and foot forces; the kernel's nu_dot with and without the forces, and the model's."""
    _setup_both(gpu_ctx, pkg)
    states = {}
    for robot in PR.ROBOTS:
        f = M.families(pkg, robot)
        if robot == "a1":
            f["stand"] = np.concatenate([f["stand"], pkg.make_batch(1, 10, "a1", seed=M.SEEDS["a1"]["stand"] + 1)["fb_state"]])
        states[robot] = np.concatenate([f["stand"], f["wide"], f["edge"]])
    st = _interleave(states["a1"], states["lite3"])
    n = len(st)
    assert n == 239 and n % 2 == 1 and n > 64
    tid = (np.arange(n) % 2).astype(np.int32)
    rng = np.random.default_rng(4401)
    tau = rng.uniform(-20, 20, (n, 12)).astype(np.float32)
    ff = rng.uniform(-50, 50, (n, 12)).astype(np.float32); ff[:, 2::3] = rng.uniform(0, 150, (n, 4)).astype(np.float32)
    edge0 = len(states["a1"]) - 23                    # first edge row of A1 in its own list; its place in the batch is twice that
    pair = (2 * (edge0 + M.NEG_PAIR[0]), 2 * (edge0 + M.NEG_PAIR[1]))
    tau[pair[1]] = tau[pair[0]]; ff[pair[1]] = ff[pair[0]]
    got, status = _fwd(gpu_ctx, pkg, st, tau, ff, tid)
    got0, status0 = _fwd(gpu_ctx, pkg, st, tau, None, tid)
    ref = np.zeros((n, 18)); ref0 = np.zeros((n, 18))
    for t, robot in enumerate(PR.ROBOTS):
        s64 = M.normalised(st[t::2]); rb = M.compute(pkg.model_desc(robot), s64)
        ref[t::2] = PR.forward_dynamics(None, s64, tau[t::2], ff[t::2], rb=rb)
        ref0[t::2] = PR.forward_dynamics(None, s64, tau[t::2], None, rb=rb)
    yield dict(n=n, state=st, tau=tau, ff=ff, tid=tid, got=got, got0=got0, status=status, status0=status0, ref=ref, ref0=ref0, pair=pair)
    G.setup_a1(gpu_ctx, pkg, 10)


def test_forward_dynamics_against_mechanics(fd):
    """nu_dot against solve(H, [0; tau] + sum Jc' f - C - G) of the first-principles model on the normalised state, every robot of the mixed
    batch, with foot forces and (d_foot_force = NULL) without: 1e-6 * max(1, |ref|) per component.
    Measured worst: 5.8e-8 * max(1, |ref|) with the forces and without, at max |ref| 1.5e4: the float32 output's rounding (LAB_NOTES A.13)."""
    for what, got, ref, status in (("with forces", fd["got"], fd["ref"], fd["status"]), ("no forces  ", fd["got0"], fd["ref0"], fd["status0"])):
        w, at = _worst(got, ref)
        print("forward dynamics %s: worst %.3e of its bar at robot %d row %d (max |ref| %.3g)" % (what, w / BAR, at[0], at[1], np.abs(ref).max()))
        assert np.all(status == 0)
        assert np.all(np.abs(got - ref) <= BAR * np.maximum(1.0, np.abs(ref)))


def test_forward_dynamics_is_even_in_the_quaternion(fd):
    a, b = fd["pair"]
    assert np.array_equal(fd["state"][a, 0:4], -fd["state"][b, 0:4]) and np.array_equal(fd["state"][a, 4:], fd["state"][b, 4:])
    assert np.array_equal(fd["got"][a].view(np.uint32), fd["got"][b].view(np.uint32))
    assert np.array_equal(fd["got0"][a].view(np.uint32), fd["got0"][b].view(np.uint32))


@pytest.mark.parametrize("n", [1, 17, 239])
def test_forward_dynamics_batch_edges(gpu_ctx, pkg, fd, n):
    """The first n robots on their own give the bits they give three places further on inside a batch of n + 8, and inside the batch of 239:
    n = 1, 17 and 239 each leave quads of the last workgroup idle."""
    _setup_both(gpu_ctx, pkg)
    pre = 3                                                     # the same robots at another place in a larger batch
    pick = lambda x: np.concatenate([x[:pre], x[:n], x[:5]])
    big, sel = pick(fd["state"]), slice(pre, pre + n)
    alone, st = _fwd(gpu_ctx, pkg, fd["state"][:n], fd["tau"][:n], fd["ff"][:n], fd["tid"][:n])
    inside, _ = _fwd(gpu_ctx, pkg, big, pick(fd["tau"]), pick(fd["ff"]), pick(fd["tid"]))
    assert np.all(st == 0)
    assert np.array_equal(alone.view(np.uint32), inside[sel].view(np.uint32))
    assert np.array_equal(alone.view(np.uint32), fd["got"][:n].view(np.uint32))
    G.setup_a1(gpu_ctx, pkg, 10)


class Plant:
    """Device arrays of one batch of simulated robots."""

    def __init__(self, ctx, pkg, state, cmd, tid=None):
        self.ctx, self.pkg, self.n = ctx, pkg, len(state)
        n = self.n
        self.fb = ctx.alloc((37, n)).upload(pkg.to_soa(state)); self.cmd = ctx.alloc((60, n)).upload(pkg.to_soa(cmd))
        self.out = ctx.alloc((PR.PLANT_OUT_ROWS, n)); self.mpc = ctx.alloc((28, n)); self.est = ctx.alloc((54, n))
        self.status = ctx.alloc((n,), np.int32)
        self.tid = None if tid is None else ctx.alloc((n,), np.int32).upload(tid)

    def step(self, params, status=None):
        self.ctx.plant_step_batch(self.n, params, self.fb, self.cmd, plant_out=self.out, mpc_state=self.mpc, est_in=self.est,
                                  status=self.status if status is None else status, type_id=self.tid)

    def get(self):
        self.ctx.sync()
        return dict(fb_state=self.fb.download().T.copy(), plant_out=self.out.download().T.copy(), mpc_state=self.mpc.download().T.copy(),
                    est_in=self.est.download().T.copy(), status=self.status.download())

    def free(self):
        for v in (self.fb, self.cmd, self.out, self.mpc, self.est, self.status, self.tid):
            if v is not None:
                v.free()


@pytest.mark.parametrize("substeps", PR.STEP_SUBSTEPS)
def test_step_against_plant_ref(gpu_ctx, pkg, substeps):
    """One control tick of 48 A1 + Lite3 robots near the ground (tests/plant_ref.step_cases: feet that penetrate, hover and slide, gains that
    saturate tau_max) against the float64 restatement: fb_state, plant_out, mpc_state and rows 0-40 of est_in within 1e-6 * max(1, |ref|);
    contact flags equal except where the reference's f_n is within 1e-6 of the threshold (at most 2 of 192 feet: none, test_plant_ref.py);
    rows 41-53 of est_in as uploaded.  Measured worst, in units of the bar, at 1 / 2 / 8 sub-steps: fb_state 0.058 / 0.059 / 0.058, plant_out
    0.058 / 0.057 / 0.058, mpc_state 0.137 / 0.091 / 0.160 (yaw: float32 atan2f), est_in 0.058 / 0.059 / 0.059."""
    _setup_both(gpu_ctx, pkg)
    s, c, tid = PR.step_cases()
    p = PR.params(substeps=substeps)
    ref = PR.step_mixed([pkg.model_desc(r) for r in PR.ROBOTS], tid, p, s, c)
    pl = Plant(gpu_ctx, pkg, s, c, tid)
    marker = np.arange(54 * len(s), dtype=np.float32).reshape(54, len(s)) + 0.5
    pl.est.upload(marker)
    pl.step(pkg.plant_params(substeps=substeps))
    got = pl.get()
    pl.free()
    G.setup_a1(gpu_ctx, pkg, 10)
    assert np.all(got["status"] == 0)
    loose = PR.near_threshold(p, ref["fn"])
    assert loose.sum() <= 2
    flag_rows = {"plant_out": slice(24, 28), "est_in": slice(13, 17)}
    for k, rows in (("fb_state", 37), ("plant_out", PR.PLANT_OUT_ROWS), ("mpc_state", 28), ("est_in", 41)):
        g, r = got[k][:, :rows].astype(np.float64), ref[k].copy()
        if k in flag_rows:
            assert np.array_equal(g[:, flag_rows[k]][~loose], r[:, flag_rows[k]][~loose]), k
            g[:, flag_rows[k]] = r[:, flag_rows[k]]
        w, at = _worst(g, r)
        print("substeps %d %-9s worst %.3e of its bar at robot %d row %d" % (substeps, k, w / BAR, at[0], at[1]))
        assert np.all(np.abs(g - r) <= BAR * np.maximum(1.0, np.abs(r))), k
    assert np.array_equal(got["est_in"][:, 41:], marker.T[:, 41:])


def _rpy(fb):
    return PR.quat_to_rpy(fb[:, 0:4].astype(np.float64))


def test_stand_on_joint_pd(gpu_ctx, pkg):
    """32 robots dropped from z = 0.30 onto joint PD at the stand pose (Kp 100, Kd 2), 1500 ticks of 1 ms at 4 sub-steps: every robot ends on
    four feet carrying its weight within 3 % (the float64 prototype: 0.7 %), z in 0.25..0.29, level within 0.03 rad, status 0 on every tick.
    Measured: sum f_z 0.65 % under m g, z 0.2685, |roll|, |pitch| <= 0.0088."""
    G.setup_a1(gpu_ctx, pkg, 10)
    n, ticks = 32, 1500
    pl = Plant(gpu_ctx, pkg, PR.stand_state(n), PR.stand_cmd(n))
    status = gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32))
    params = pkg.plant_params(dt=0.001, substeps=4)
    for k in range(ticks):
        pl.step(params, status=status.row(k))
    got = pl.get()
    st = status.download()
    pl.free(); status.free()
    fz = got["plant_out"][:, 2:12:3].sum(1)
    mg = M.total_mass() * 9.81
    rpy = _rpy(got["fb_state"])
    print("stand: sum fz / m g - 1 = %.4f .. %.4f, z %.4f .. %.4f, |roll| |pitch| <= %.4f" % ((fz / mg - 1).min(), (fz / mg - 1).max(), got["fb_state"][:, 6].min(),
                                                                                         got["fb_state"][:, 6].max(), np.abs(rpy[:, :2]).max()))
    assert np.all(st == 0)
    assert np.all(got["plant_out"][:, 24:28] == 1)
    assert np.all(np.abs(fz - mg) <= 0.03 * mg)
    assert np.all((got["fb_state"][:, 6] >= 0.25) & (got["fb_state"][:, 6] <= 0.29))
    assert np.all(np.abs(rpy[:, :2]) <= 0.03)


def test_closed_loop_with_mpc_and_wbc(gpu_ctx, pkg):
    """The point of the plant: 64 A1 robots settle on joint PD (400 ticks of 1 ms, 1 sub-step), are shoved by up to 0.3 m/s in x and y, and are
    then held by plant -> qrgpu_tick_batch -> plant for 500 ticks of 2 ms at 2 sub-steps with no host copy in the loop: the plant writes the
    tick's mpc_state and fb_state, the tick writes its torque into rows 48-59 of the motor command.  No status flag on any tick or robot, and
    the end state inside the stand band (|z - 0.27| <= 0.01, |x|, |y| <= 0.03, |roll|, |pitch| <= 0.03) that tests/test_plant_ref.py shows
    the float64 chain with the oracle tick to reach for the shoves at the corners of that square.
    Measured: |x| <= 0.0025, |y| <= 0.0017, |z - 0.27| <= 0.0031, |roll|, |pitch| <= 0.0063; the +x shove ends at x 0.0002, z 0.2671."""
    G.setup_a1(gpu_ctx, pkg, PR.HORIZON)
    n, ticks, h = 64, 500, PR.HORIZON
    S = pkg.to_soa
    pl = Plant(gpu_ctx, pkg, PR.stand_state(n), PR.stand_cmd(n))
    pd = pkg.plant_params(dt=0.001, substeps=1)
    for _ in range(400):
        pl.step(pd)
    got = pl.get()
    assert np.all(got["status"] == 0)
    rng = np.random.default_rng(5150)
    shove = rng.uniform(-PR.SHOVE_MAX, PR.SHOVE_MAX, (n, 2))
    shove[0] = (PR.SHOVE_MAX, 0.0)                                    # the prototype's case
    fb = got["fb_state"]; fb[:, 10:12] += shove.astype(np.float32)
    pl.fb.upload(S(fb)); pl.cmd.upload(np.zeros((60, n), np.float32))
    traj, gait, wcmd, prev = PR.stand_tick_inputs(n)
    d = dict(traj=gpu_ctx.alloc((12 * h, n)).upload(S(traj)), gait=gpu_ctx.alloc((4 * h, n)).upload(S(gait)), cmd=gpu_ctx.alloc((67, n)).upload(S(wcmd)),
             prev=gpu_ctx.alloc((3, n)).upload(S(prev)), force=gpu_ctx.alloc((12, n)),
             tick_status=gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32)),
             plant_status=gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32)))
    params = pkg.plant_params(dt=0.002, substeps=2)
    gpu_ctx.set_warm_start(True)
    pl.mpc.upload(S(PR.truth_mpc_state(pkg.model_desc("a1"), PR.params(), M.normalised(fb))))       # the first tick's; the plant writes the rest
    for k in range(ticks):
        gpu_ctx.tick_batch(n, pl.mpc, d["traj"], d["gait"], pl.fb, d["cmd"], d["prev"], d["force"], pl.cmd.row(48), d["tick_status"].row(k))
        pl.step(params, status=d["plant_status"].row(k))
    got = pl.get()
    tick_status, plant_status = d["tick_status"].download(), d["plant_status"].download()
    pl.free()
    for v in d.values():
        v.free()
    rpy = _rpy(got["fb_state"])
    pos = got["fb_state"][:, 4:7]
    print("closed loop: |x| <= %.4f, |y| <= %.4f, |z - 0.27| <= %.4f, |roll| |pitch| <= %.4f; robot 0 (x shove): x %.4f z %.4f"
          % (np.abs(pos[:, 0]).max(), np.abs(pos[:, 1]).max(), np.abs(pos[:, 2] - 0.27).max(), np.abs(rpy[:, :2]).max(), pos[0, 0], pos[0, 2]))
    assert np.all(G.flags(tick_status) == 0), np.unique(G.flags(tick_status))
    assert np.all(plant_status == 0)
    assert np.all(np.abs(pos[:, 2] - 0.27) <= 0.01)
    assert np.all(np.abs(pos[:, 0:2]) <= 0.03)
    assert np.all(np.abs(rpy[:, 0:2]) <= 0.03)


def test_error_returns_and_bad_type_flag(gpu_ctx, pkg):
    """QRGPU_ERR_BAD_ARG for n outside 1..max_batch, null required pointers, substeps outside 1..64 and dt <= 0; QRGPU_ERR_NOT_SETUP on a
    context with no WBC type; a bad type beside a valid one is computed with the first valid type and flagged, robot by robot."""
    G.setup_a1(gpu_ctx, pkg, 10)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    n = 5
    s, c = PR.stand_state(n), PR.stand_cmd(n)
    pl = Plant(gpu_ctx, pkg, s, c)
    nud = gpu_ctx.alloc((18, n))
    P = pkg.plant_params
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    BAD, NOT_SETUP = 2, 3
    fwd = lambda n_, st, tau, out: lib.qrgpu_forward_dynamics_batch(h, n_, None, vp(st), vp(tau), None, vp(out), None)
    stp = lambda n_, par, st, cmd: lib.qrgpu_plant_step_batch(h, n_, None if par is None else C.byref(par), None, vp(st), vp(cmd), None, None, None, None)
    tau = pl.cmd            # any [12][n] rows
    assert fwd(0, pl.fb, tau, nud) == BAD and fwd(gpu_ctx.max_batch + 1, pl.fb, tau, nud) == BAD
    assert fwd(n, None, tau, nud) == BAD and fwd(n, pl.fb, None, nud) == BAD and fwd(n, pl.fb, tau, None) == BAD
    assert fwd(n, pl.fb, tau, nud) == 0
    assert stp(0, P(), pl.fb, pl.cmd) == BAD and stp(gpu_ctx.max_batch + 1, P(), pl.fb, pl.cmd) == BAD
    assert stp(n, None, pl.fb, pl.cmd) == BAD and stp(n, P(), None, pl.cmd) == BAD and stp(n, P(), pl.fb, None) == BAD
    assert stp(n, P(substeps=0), pl.fb, pl.cmd) == BAD and stp(n, P(substeps=65), pl.fb, pl.cmd) == BAD
    assert stp(n, P(dt=0.0), pl.fb, pl.cmd) == BAD and stp(n, P(dt=-0.001), pl.fb, pl.cmd) == BAD
    gpu_ctx.sync()
    assert np.array_equal(pl.fb.download(), pkg.to_soa(s))                       # nothing was launched by the refused calls
    assert stp(n, P(substeps=64), pl.fb, pl.cmd) == 0
    # a bad type beside a valid one
    tid = np.array([0, 4, -1, 0, 7], np.int32)
    d_tid = gpu_ctx.alloc((n,), np.int32).upload(tid)
    pl.fb.upload(pkg.to_soa(s))
    st = gpu_ctx.alloc((n,), np.int32).upload(np.full(n, -1, np.int32))
    gpu_ctx.forward_dynamics_batch(n, pl.fb, tau, nud, status=st, type_id=d_tid)
    gpu_ctx.sync()
    flags = st.download()
    assert np.array_equal(flags != 0, tid != 0) and np.all(flags[tid != 0] == pkg.qrgpu.PL_BAD_TYPE)
    out = nud.download()
    assert np.array_equal(out[:, 1].view(np.uint32), out[:, 0].view(np.uint32))   # ... computed with type 0: the same state, the same bits
    gpu_ctx.plant_step_batch(n, P(), pl.fb, pl.cmd, status=st, type_id=d_tid)
    gpu_ctx.sync()
    assert np.array_equal(st.download() != 0, tid != 0)
    # a zero quaternion is flagged, not propagated
    z = s.copy(); z[2, 0:4] = 0
    pl.fb.upload(pkg.to_soa(z))
    gpu_ctx.plant_step_batch(n, P(), pl.fb, pl.cmd, status=st)
    gpu_ctx.sync()
    assert np.array_equal(st.download(), np.where(np.arange(n) == 2, pkg.qrgpu.PL_QUAT_ZERO, 0))
    assert np.all(np.isfinite(pl.fb.download()))
    # no type set up at all
    fresh = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
    try:
        a = fresh.alloc((60, n)); b = fresh.alloc((18, n))
        par = P()
        assert fresh._lib.qrgpu_forward_dynamics_batch(fresh._h, n, None, vp(a), vp(a), None, vp(b), None) == NOT_SETUP
        assert fresh._lib.qrgpu_plant_step_batch(fresh._h, n, C.byref(par), None, vp(a), vp(a), None, None, None, None) == NOT_SETUP
        a.free(); b.free()
    finally:
        fresh.close()
    for v in (nud, d_tid, st):
        v.free()
    pl.free()
