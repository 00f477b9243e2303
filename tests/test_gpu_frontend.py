"""GPU parity of the batched MPC front-end (qrgpu_mpc_frontend_batch) against the oracle restatement of
MPCStanceLegController::SetupCommand / Run / UpdateMPC (qr_mpc_stance_leg_controller.cpp:158-382).

Bar: bit-exact float32, except the three outputs that carry std::sin (height / pitch compensation: bodyHeight, rpyComp[1]),
where libm and the device library may differ in the last bit of a double sine -> at most 1 float ulp.

The second half holds the kernel to tests/frontend_ref.py, the reference restated statement by statement, on every tick of every robot of its
families at the same bar, and pins the two things that model found: the float tick counter at 2^24 and the re-plan period of zero."""
import numpy as np

import frontend_ref as R
import gpu_helpers as G
import pytest

from gpu_helpers import setup_a1, tau_tol

pytestmark = pytest.mark.gpu
SIN_CMD_ROWS = [2, 10]            # pBody_des z (bodyHeight), pBody_RPY_des pitch
SIN_TRAJ_COLS = [1, 5]


def _run_gpu(ctx, pkg, fe, st, h, L=2, prev_traj=None):
    n = fe.shape[0]
    S = pkg.to_soa
    d_in = ctx.alloc((64, n)).upload(S(fe)); d_st = ctx.alloc((8, n)).upload(S(st))
    t0 = np.full((n, 12 * h), np.nan, np.float32) if prev_traj is None else prev_traj
    d_traj = ctx.alloc((12 * h, n)).upload(S(t0)); d_gait = ctx.alloc((4 * h, n))
    d_cmd = ctx.alloc((67, n)).upload(np.full((67, n), np.nan, np.float32)); d_upd = ctx.alloc((n,), np.int32)
    ctx.mpc_frontend_batch(n, d_in, d_st, d_traj, d_gait, d_cmd, d_upd, num_horizon_l=L)
    ctx.sync()
    out = dict(traj=d_traj.download().T.copy(), gait=d_gait.download().T.copy(), cmd=d_cmd.download().T.copy(),
               state=d_st.download().T.copy(), updated=d_upd.download())
    for v in (d_in, d_st, d_traj, d_gait, d_cmd, d_upd):
        v.free()
    return out


def _ulp_close(a, b, ulps=1):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))))


def frontend_parity(ctx, pkg, oracle, h, L, n=1000, seed=None):
    """Every robot of one qrgpu_mpc_frontend_batch call against the oracle: bit-exact but for the sin rows (1 ulp)."""
    setup_a1(ctx, pkg, h)
    fe, st = pkg.workload.make_frontend_batch(n, seed=h if seed is None else seed)
    g = _run_gpu(ctx, pkg, fe, st, h, L)
    exact_cmd = [r for r in list(range(15)) + [63, 64, 65, 66] if r not in SIN_CMD_ROWS]
    exact_traj = [c for c in range(12) if c not in SIN_TRAJ_COLS]
    n_upd = 0
    for i in range(n):
        o = oracle.mpc_frontend(h, L, fe[i], st[i])
        assert g["updated"][i] == o["updated"]
        assert np.array_equal(g["state"][i], o["state"]), i
        assert np.array_equal(g["gait"][i], o["gait"]), i
        assert np.array_equal(g["cmd"][i, exact_cmd[:13]], o["wbc15"][exact_cmd[:13]]), i
        assert np.array_equal(g["cmd"][i, 63:67], o["contact"])
        assert _ulp_close(g["cmd"][i, SIN_CMD_ROWS], o["wbc15"][SIN_CMD_ROWS])
        assert np.isnan(g["cmd"][i, 15:63]).all()                       # foot tasks / Fr_des rows are not the front-end's
        tg = g["traj"][i].reshape(h, 12)
        if o["updated"]:
            n_upd += 1
            to = o["traj"].reshape(h, 12)
            assert np.array_equal(tg[:, exact_traj], to[:, exact_traj]), i
            assert _ulp_close(tg[:, SIN_TRAJ_COLS], to[:, SIN_TRAJ_COLS])
        else:
            assert np.isnan(tg).all()                                   # no re-plan: trajectory left alone
    assert 0 < n_upd < n


@pytest.mark.parametrize("h,L", [(10, 2), (5, 2), (16, 3)])
def test_frontend_parity(gpu_ctx, pkg, oracle, h, L):
    frontend_parity(gpu_ctx, pkg, oracle, h, L, n=1000)          # (1000: not a multiple of the block size, a ragged tail)


def test_frontend_sequence_feeds_tick(gpu_ctx, pkg, oracle):
    """Thirty consecutive ticks with persistent fe_state, then the trajectory / table / wbc rows the front-end wrote drive one
    full MPC+WBC tick whose torques match the oracle fed with the oracle front-end's outputs."""
    h, n = 10, 64
    setup_a1(gpu_ctx, pkg, h)
    b = pkg.make_batch(n, horizon=h, robot="a1", seed=77, excite=0.3)
    fe, st = pkg.workload.make_frontend_batch(n, seed=21)
    st[:, 7] = 40                                                       # crosses the 50-tick boundary of the cadence
    # tie the front-end's robot state to the MPC batch (position, attitude, contacts of step 0)
    shift = b["mpc_state"][:, 0:2] - fe[:, 6:8]
    for l in range(4):
        fe[:, 14 + 3 * l:16 + 3 * l] += shift; fe[:, 26 + 3 * l:28 + 3 * l] += shift
    fe[:, 62:64] += shift
    fe[:, 6:9] = b["mpc_state"][:, 0:3]; fe[:, 10:14] = b["mpc_state"][:, 6:10]; fe[:, 9] = b["mpc_state"][:, 27]
    fe[:, 38:42] = b["gait"][:, 0:4]
    fe[:, 0] = b["traj"][:, 5]; fe[:, 2] = 0
    st[:, 3] = b["mpc_state"][:, 27]; st[:, 4:6] = b["mpc_state"][:, 0:2]
    fe[:, 3:6] *= 0.3
    S = pkg.to_soa
    d_in = gpu_ctx.alloc((64, n)).upload(S(fe)); d_st = gpu_ctx.alloc((8, n)).upload(S(st))
    d_traj = gpu_ctx.alloc((12 * h, n)).upload(S(b["traj"])); d_gait = gpu_ctx.alloc((4 * h, n))
    d_cmd = gpu_ctx.alloc((67, n)).upload(S(b["wbc_cmd"])); d_upd = gpu_ctx.alloc((n,), np.int32)
    o_st = st.copy(); o_traj = b["traj"].copy(); o_gait = np.zeros((n, 4 * h), np.float32); o_cmd = b["wbc_cmd"].copy()
    upd_hist = []
    for k in range(30):
        gpu_ctx.mpc_frontend_batch(n, d_in, d_st, d_traj, d_gait, d_cmd, d_upd)
        for i in range(n):
            o = oracle.mpc_frontend(h, 2, fe[i], o_st[i])
            o_st[i] = o["state"]; o_gait[i] = o["gait"]; o_cmd[i, :15] = o["wbc15"]; o_cmd[i, 63:67] = o["contact"]
            if o["updated"]:
                o_traj[i] = o["traj"]
        upd_hist.append(int(d_upd.download().sum()))
    gpu_ctx.sync()
    # counters 40..49 re-plan every tick (< 50); of 50..69 only 60 does (% 15)
    assert upd_hist[:10] == [n] * 10 and upd_hist[20] == n and sum(upd_hist[10:]) == n
    assert np.array_equal(d_st.download().T, o_st)
    assert np.array_equal(d_gait.download().T, o_gait)
    g_traj = d_traj.download().T.copy(); g_gait = d_gait.download().T.copy(); g_cmd = d_cmd.download().T.copy()
    assert np.allclose(g_traj, o_traj, rtol=0, atol=1e-6)
    assert np.allclose(g_cmd, o_cmd, rtol=0, atol=1e-6)
    # one full tick on what the front-end produced (device buffers handed straight to qrgpu_tick_batch)
    d = dict(state=gpu_ctx.alloc((28, n)).upload(S(b["mpc_state"])), fb=gpu_ctx.alloc((37, n)).upload(S(b["fb_state"])),
             prev=gpu_ctx.alloc((3, n)).upload(S(b["prev_ori_vel"])), force=gpu_ctx.alloc((12, n)), tau=gpu_ctx.alloc((12, n)),
             status=gpu_ctx.alloc((n,), np.int32))
    gpu_ctx.tick_batch(n, d["state"], d_traj, d_gait, d["fb"], d_cmd, d["prev"], d["force"], d["tau"], d["status"])
    gpu_ctx.sync()
    tau = d["tau"].download().T; status = d["status"].download()
    assert np.all(G.flags(status) == 0), np.unique(G.flags(status))
    f_o, tau_o, st_o, _, _ = oracle.tick_batch(1, pkg.mpc_cfg("a1"), h, pkg.model_desc("a1")[:3], pkg.model_desc("a1"), b["mpc_state"],
                                               g_traj, g_gait, b["fb_state"], g_cmd, b["prev_ori_vel"].copy(), nthreads=4)
    assert np.all(st_o == 0)
    assert np.all(np.abs(tau - tau_o) <= tau_tol(tau_o, 1e-4)), np.abs(tau - tau_o).max()
    for v in list(d.values()) + [d_in, d_st, d_traj, d_gait, d_cmd, d_upd]:
        v.free()


# ----------------------------------------------------------------------------- the kernel against tests/frontend_ref.py
def kernel_sequence(ctx, pkg, f, idx=None, guard=None):
    """qr_frontend_kernel on a family of frontend_ref: the controller memory and the trajectory stay on the device from tick to tick.
    -> outs[tick] = dict of [n][...] arrays in the oracle's layout"""
    setup_a1(ctx, pkg, f["h"])
    idx = np.arange(f["st"].shape[0]) if idx is None else idx
    n, h, S = len(idx), f["h"], pkg.to_soa
    d_in = ctx.alloc((64, n)); d_st = ctx.alloc((8, n)).upload(S(f["st"][idx]))
    d_traj = ctx.alloc((12 * h, n)).upload(np.full((12 * h, n), np.nan, np.float32)); d_gait = ctx.alloc((4 * h, n))
    d_cmd = ctx.alloc((67, n)).upload(np.full((67, n), np.nan, np.float32)); d_upd = ctx.alloc((n,), np.int32)
    outs = []
    for k in range(f["ticks"]):
        if k < f["fe"].shape[0]:
            d_in.upload(S(f["fe"][k][idx]))
        ctx.mpc_frontend_batch(n, d_in, d_st, d_traj, d_gait, d_cmd, d_upd, num_horizon_l=f["L"], dt_ctrl=f["dt"], dt_mpc=f["dt_mpc"])
        cmd = d_cmd.download().T
        assert np.isnan(cmd[:, 15:63]).all()
        outs.append(dict(traj=d_traj.download().T.copy(), gait=d_gait.download().T.copy(), wbc15=cmd[:, :15].copy(), contact=cmd[:, 63:67].copy(),
                         state=d_st.download().T.copy(), updated=d_upd.download().copy()))
    for v in (d_in, d_st, d_traj, d_gait, d_cmd, d_upd):
        v.free()
    return outs


@pytest.mark.parametrize("name", R.NAMES)
def test_kernel_is_the_model_on_every_tick(gpu_ctx, pkg, name):
    """Every tick of every robot of every family of tests/frontend_ref.py: bit for bit, the sine rows to 1 ulp, the counter row as
    include/qrgpu.h states it."""
    f, want, _ = R.expected(pkg, name)
    period = R.iterations_in_a_mpc(f["dt"], f["dt_mpc"]) // 2
    got = kernel_sequence(gpu_ctx, pkg, f)
    for k in range(f["ticks"]):
        for r in range(R.N_ROBOTS):
            R.compare({key: v[r] for key, v in got[k].items()}, want[r][k], period, (name, r, k))


@pytest.mark.parametrize("ratio", [30, 25, 3])
def test_counter_started_below_2p24_replans_like_an_integer(gpu_ctx, pkg, ratio):
    """The counter row is a float: started at 2^24 - 3 it must go on re-planning on the ticks on which an integer counter does."""
    f, _, _ = R.expected(pkg, "counter_2p24_%d" % ratio)
    got = kernel_sequence(gpu_ctx, pkg, f)
    integer = (((1 << 24) - 3 + np.arange(f["ticks"])) % (ratio // 2) == 0).astype(np.int32)
    upd = np.stack([o["updated"] for o in got])                       # [tick][robot]
    assert np.array_equal(upd, np.repeat(integer[:, None], R.N_ROBOTS, axis=1))
    rows = np.stack([o["state"][:, 7] for o in got])
    assert np.all(rows < 1 << 24) and np.all(rows[3:] >= 50)
    # the fold tick stores the SMALLEST value >= 50 of 2^24's residue class, and the row counts on from it
    assert np.all(rows[1] == (1 << 24) - 1) and np.all(rows[2] == R.folded(1 << 24, ratio // 2)) and R.folded(1 << 24, ratio // 2) - ratio // 2 < 50
    assert np.array_equal(rows[2:], rows[2:3] + np.arange(rows.shape[0] - 2)[:, None])


def test_period_of_zero_is_refused_and_nothing_is_written(gpu_ctx, pkg):
    """round(dt_mpc / dt_ctrl) < 2 (the reference's remainder by zero) or beyond 2^24: QRGPU_ERR_BAD_ARG, no launch."""
    setup_a1(gpu_ctx, pkg, 10)
    n, S = 65, pkg.to_soa
    fe, st = pkg.workload.make_frontend_batch(n, seed=4)
    poison = lambda rows: np.full((rows, n), -7.5, np.float32)
    d_in = gpu_ctx.alloc((64, n)).upload(S(fe)); d_st = gpu_ctx.alloc((8, n)).upload(S(st))
    d_traj = gpu_ctx.alloc((120, n)).upload(poison(120)); d_gait = gpu_ctx.alloc((40, n)).upload(poison(40)); d_cmd = gpu_ctx.alloc((67, n)).upload(poison(67))
    for dt, dt_mpc in ((0.002, 0.002), (0.002, 0.0029), (0.002, 0.0005), (0.06, 0.002), (0.002, 40000.0)):
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            gpu_ctx.mpc_frontend_batch(n, d_in, d_st, d_traj, d_gait, d_cmd, None, dt_ctrl=dt, dt_mpc=dt_mpc)
    gpu_ctx.sync()
    assert np.array_equal(d_st.download(), S(st))
    assert np.all(d_traj.download() == -7.5) and np.all(d_gait.download() == -7.5) and np.all(d_cmd.download() == -7.5)
    # round = 2 and 3 are the smallest that run: a period of 1, a re-plan on every tick
    d_upd = gpu_ctx.alloc((n,), np.int32)
    for dt_mpc in (0.004, 0.006):
        gpu_ctx.mpc_frontend_batch(n, d_in, d_st, d_traj, d_gait, d_cmd, d_upd, dt_mpc=dt_mpc)
        assert np.all(d_upd.download() == 1)
    for v in (d_in, d_st, d_traj, d_gait, d_cmd, d_upd):
        v.free()
