"""CPU: tests/frontend_ref.py (the MPC front-end written from the reference statement by statement) against closed forms, and
oracle/qr_oracle_frontend.cpp against frontend_ref on every tick of every robot of every family of frontend_ref.NAMES: bit for bit, the sine rows
to 1 ulp.  The two findings this model turned up are tests of their own at the end: the float tick counter at 2^24 and the re-plan period of zero."""
import numpy as np
import pytest

import frontend_ref as R


def oracle_sequence(oracle, f, robot):
    """The oracle on one robot of a family, its controller memory and trajectory carried from tick to tick.  -> list of per-tick dicts"""
    st = f["st"][robot].copy(); traj = np.full(12 * f["h"], np.nan, np.float32)
    outs = []
    for k in range(f["ticks"]):
        o = oracle.mpc_frontend(f["h"], f["L"], f["fe"][min(k, f["fe"].shape[0] - 1), robot], st, dt=f["dt"], dt_mpc=f["dt_mpc"])
        st = o["state"]
        if o["updated"]:
            traj = o["traj"]
        else:
            assert np.isnan(o["traj"]).all()                                    # no re-plan: trajAll is not written
        o["traj"] = traj.copy()
        outs.append(o)
    return outs


@pytest.mark.parametrize("name", R.NAMES)
def test_oracle_is_the_model_on_every_tick(pkg, oracle, name):
    f, want, seen = R.expected(pkg, name)
    assert R.COVERS.get(name, set()) <= seen, (name, R.COVERS[name] - seen)
    period = R.iterations_in_a_mpc(f["dt"], f["dt_mpc"]) // 2
    n_upd = 0
    for r in range(R.N_ROBOTS):
        got = oracle_sequence(oracle, f, r)
        for k in range(f["ticks"]):
            R.compare(got[k], want[r][k], period, (name, r, k))
            n_upd += want[r][k]["updated"]
    if period > 1:
        assert 0 < n_upd < R.N_ROBOTS * f["ticks"], name                        # both sides of the cadence


def test_integer_division_of_the_period():
    assert R.iterations_in_a_mpc(0.002, 0.06) // 2 == 15 and R.iterations_in_a_mpc(0.002, 0.05) // 2 == 12 and R.iterations_in_a_mpc(0.002, 0.006) // 2 == 1
    assert R.iterations_in_a_mpc(0.5, 1.25) == 3 and R.iterations_in_a_mpc(0.5, 1.2) == 2               # 2.5 (exact in float32) rounds away from zero


def _quiet_robot(pkg, seed=9):
    """One robot in stance on all four legs, level, yaw 0: nothing but the filters and the plan moves."""
    fe, _ = pkg.workload.make_frontend_batch(1, seed=seed)
    f = fe[0].copy()
    f[3:6] = (0.5, 0.1, 0.2); f[9] = 0.0; f[10:14] = (1, 0, 0, 0); f[54:62] = 1; f[38:42] = 1
    return f


def test_low_pass_filters_in_closed_form(pkg):
    """Constant command: x_k = c (1 - (1 - a)^k) for a = 0.01, 0.005, 0.03, and the yaw plan is dt times the running sum of the turn rate."""
    f = _quiet_robot(pkg)
    m = R.MPCStanceLegController(10, 2, np.zeros(8, np.float32))
    K = 300
    yaw = 0.0
    for k in range(1, K + 1):
        s = m.Run(f)["state"]
        yaw += 0.002 * 0.2 * (1 - 0.97 ** k)
        # k float32 steps, each rounding a value below the command: k ulps of the command at the most
        assert abs(s[0] - 0.5 * (1 - 0.99 ** k)) <= 2 * k * np.spacing(np.float32(0.5))
        assert abs(s[1] - 0.1 * (1 - 0.995 ** k)) <= 2 * k * np.spacing(np.float32(0.1))
        assert abs(s[2] - 0.2 * (1 - 0.97 ** k)) <= 2 * k * np.spacing(np.float32(0.2))
        assert abs(s[3] - yaw) <= 2 * k * np.spacing(np.float32(yaw)) + 0.002 * 2 * k * np.spacing(np.float32(0.2))
        assert s[7] == k
    # the clips hold the filtered command, not the command
    f[3], f[4] = 50.0, -50.0
    for _ in range(400):
        s = m.Run(f)["state"]
    assert s[0] == 2.0 and s[1] == np.float32(-0.6)


def test_contact_table_is_the_phase_indicator(pkg):
    """Column j of rows 1 .. h-1 is [frac(phase_j + i / (L h)) < duty_j] for legs that are not EARLY_CONTACT; row 0 is the measured contact.
    Entries whose phase lies within 1e-6 of the duty factor or of 1 (ties of the float32 sum) are left out."""
    n_checked = 0
    for h, L in ((10, 2), (16, 3), (1, 2)):
        fe, st = pkg.workload.make_frontend_batch(R.N_ROBOTS, seed=0x7AB + h)
        for r in range(R.N_ROBOTS):
            g = R.MPCStanceLegController(h, L, st[r]).Run(fe[r])["gait"].reshape(h, 4)
            assert np.array_equal(g[0], (fe[r, 38:42] != 0).astype(np.float32))
            for j in range(4):
                ph = fe[r, 42 + j].astype(np.float64) + np.arange(1, h) / (L * h)
                fr = ph - np.floor(ph)
                clear = (np.abs(fr - fe[r, 46 + j]) > 1e-6) & (np.abs(ph - 1.0) > 1e-6)
                if int(fe[r, 58 + j]) == R.EARLY_CONTACT:
                    assert g[1:, j].all()
                else:
                    assert np.array_equal(g[1:, j][clear], (fr < fe[r, 46 + j])[clear].astype(np.float32)), (h, L, r, j)
                    n_checked += int(clear.sum())
    assert n_checked > 4000


def test_trajectory_ramps_are_linear(pkg):
    """A re-planned trajectory: yaw, x and y of row i are row 0 plus i dtMPC times the turn rate and the world-frame velocity (float32 running
    sums: i roundings at the magnitude of the row), every other column constant, x and y of row 0 within 0.1 of the base."""
    h = 16
    fe, st = pkg.workload.make_frontend_batch(R.N_ROBOTS, seed=0x7AC)
    st[:, 7] = 0
    for r in range(R.N_ROBOTS):
        o = R.MPCStanceLegController(h, 2, st[r], dtMPC=0.05).Run(fe[r])
        assert o["updated"] == 1
        tr = o["traj"].reshape(h, 12).astype(np.float64)
        i = np.arange(h)
        for col, rate in ((2, o["state"][2]), (3, o["wbc15"][3]), (4, o["wbc15"][4])):
            tol = (i + 1) * np.spacing(np.float32(np.abs(tr[:, col]).max() + 1))
            assert np.all(np.abs(tr[:, col] - (tr[0, col] + i * float(np.float32(0.05)) * float(rate))) <= tol), (r, col)
        assert np.all(tr[:, [0, 1, 5, 6, 7, 8, 9, 10, 11]] == tr[0, [0, 1, 5, 6, 7, 8, 9, 10, 11]])
        assert np.all(tr[0, [0, 6, 7, 11]] == 0) and tr[0, 8] == o["state"][2] and tr[0, 2] == o["state"][3]
        assert abs(tr[0, 3] - fe[r, 6]) <= 0.1 + 1e-6 and abs(tr[0, 4] - fe[r, 7]) <= 0.1 + 1e-6


def test_body_height_plan_is_a_99_percent_filter(pkg):
    f = _quiet_robot(pkg)
    m = R.MPCStanceLegController(10, 2, np.zeros(8, np.float32))
    z = 0.0
    for _ in range(50):
        s = m.Run(f)["state"]
        z = 0.99 * (2 * float(f[0]) - float(f[8])) + 0.01 * z
        assert abs(s[6] - z) <= 2 * np.spacing(np.float32(z))


# ----------------------------------------------------------------------------- the two findings
@pytest.mark.parametrize("ratio", [30, 25, 3])
def test_counter_started_below_2p24_replans_like_an_integer(pkg, oracle, ratio):
    """A robot whose counter row starts at 2^24 - 3 re-plans on exactly the ticks on which an integer counter does.  (A float row that goes on
    adding 1 sticks at 2^24, which is 1 modulo 15: it never re-plans again.)"""
    f, want, _ = R.expected(pkg, "counter_2p24_%d" % ratio)
    period = ratio // 2
    c0 = (1 << 24) - 3
    ticks = np.arange(f["ticks"])
    integer = ((c0 + ticks) % period == 0).astype(int)
    assert integer.sum() >= 2 and integer[3:].sum() >= 1                          # re-plans on both sides of 2^24
    for r in (0, 31, 64):
        assert np.array_equal([o["updated"] for o in want[r]], integer)          # the model counts in an integer
        got = oracle_sequence(oracle, f, r)
        assert np.array_equal([o["updated"] for o in got], integer), (ratio, r)
        rows = np.array([o["state"][7] for o in got])
        assert np.all(rows < 1 << 24) and np.all(rows[3:] >= 50)                  # the row never reaches the value it cannot leave
        # the fold tick stores the SMALLEST value >= 50 of 2^24's residue class, and the row counts on from it
        assert rows[1] == (1 << 24) - 1 and rows[2] == R.folded(1 << 24, period) and R.folded(1 << 24, period) - period < 50
        assert np.array_equal(rows[2:], rows[2] + np.arange(rows.size - 2))


@pytest.mark.parametrize("dt,dt_mpc", [(0.002, 0.002), (0.002, 0.0029), (0.002, 0.0005), (0.06, 0.002), (0.002, 40000.0)])
def test_period_of_zero_is_refused(pkg, oracle, dt, dt_mpc):
    """round(dt_mpc / dt) < 2: the reference would take a remainder by zero.  Model and oracle refuse; nothing is computed.  (Beyond 2^24 too: the
    period must fit under the float counter row.)"""
    fe, st = pkg.workload.make_frontend_batch(1, seed=4)
    with pytest.raises(ValueError):
        R.MPCStanceLegController(10, 2, st[0], dt, dt_mpc)
    with pytest.raises(ValueError):
        oracle.mpc_frontend(10, 2, fe[0], st[0], dt=dt, dt_mpc=dt_mpc)


def test_period_of_one_replans_every_tick(pkg, oracle):
    fe, st = pkg.workload.make_frontend_batch(4, seed=4)
    st[:, 7] = (60, 61, 62, 1000)
    for r in range(4):
        for dt_mpc in (0.004, 0.006):                                           # round = 2 and 3: period 1
            assert oracle.mpc_frontend(10, 2, fe[r], st[r], dt_mpc=dt_mpc)["updated"] == 1
            assert R.MPCStanceLegController(10, 2, st[r], dtMPC=dt_mpc).Run(fe[r])["updated"] == 1
