"""CPU: the float64 plant of tests/plant_ref.py on its own -- the integrator's order, the contact law's continuity, the seeded cases the GPU
file relies on, and the closed loop with the project's oracle tick."""
import numpy as np
import pytest

import plant_ref as PR
import rigid_body_ref as M


def _a1(pkg):
    return pkg.model_desc("a1")


def test_free_flight_energy_drift_is_first_order(pkg):
    """Base at z = 5 (no contact), three wide_states seeds, zero gains, 20 ms of flight: T + V is conserved by the mechanics, so what drifts is
    the integrator's error, and semi-implicit Euler's is first order: halving h halves it.  Ratio in 1.8..2.2 (measured 1.995..2.005)."""
    s0 = np.concatenate([M.wide_states(1, seed) for seed in (11, 12, 13)])
    s0[:, 6] = 5.0
    cmd = np.zeros((3, 60), np.float32)
    e0 = PR.energy(_a1(pkg), s0)
    drift = []
    for h in (5e-5, 2.5e-5):
        p = dict(PR.params(), dt=h, substeps=1)
        s = s0.copy()
        for _ in range(int(round(0.02 / h))):
            s, aux = PR.substep(_a1(pkg), p, s, cmd, h)
            assert not aux["fn"].any()
        drift.append(PR.energy(_a1(pkg), s) - e0)
    ratio = drift[0] / drift[1]
    print("energy drift at h = 5e-5:", drift[0], " at 2.5e-5:", drift[1], " ratio:", ratio)
    assert np.all((ratio > 1.8) & (ratio < 2.2)), ratio


def test_no_contact_force_above_the_ground():
    p = PR.params()
    rng = np.random.default_rng(3)
    pos = rng.uniform(-1, 1, (200, 3)); pos[:, 2] = rng.uniform(0.0, 0.5, 200); pos[0, 2] = 0.0
    f, fn = PR.contact_force(p, pos, rng.uniform(-2, 2, (200, 3)))
    assert not f.any() and not fn.any()


def test_contact_force_is_continuous():
    """Across delta = 0 and across v_t = 0: a step of eps in the state moves the force by O(eps), not by a jump."""
    p = PR.params()
    eps = 1e-9
    for vz in (-0.5, 0.0, 0.5):
        for vt in ((0.3, -0.2), (0.0, 0.0)):
            v = np.array([vt[0], vt[1], vz])
            above, _ = PR.contact_force(p, np.array([0.0, 0.0, +eps]), v)
            below, _ = PR.contact_force(p, np.array([0.0, 0.0, -eps]), v)
            assert np.abs(below - above).max() <= 2 * p["contact_k"] * eps * 2          # k delta (1 + |a v_z|), friction below that
    pos = np.array([0.0, 0.0, -0.01])
    for d in ((1.0, 0.0), (0.0, 1.0), (0.6, -0.8)):
        plus, _ = PR.contact_force(p, pos, np.array([eps * d[0], eps * d[1], 0.0]))
        minus, _ = PR.contact_force(p, pos, np.array([-eps * d[0], -eps * d[1], 0.0]))
        zero, _ = PR.contact_force(p, pos, np.zeros(3))
        assert np.abs(plus - minus).max() <= 2 * p["mu"] * p["contact_k"] * 0.01 * eps / p["v_eps"] * 1.01
        assert zero[0] == 0.0 and zero[1] == 0.0 and zero[2] == p["contact_k"] * 0.01


def test_step_cases_exercise_the_contact_and_motor_laws(pkg):
    """The seeded batch of the GPU step test, on the reference alone: feet that penetrate, feet that hover, feet that slide, torques that
    saturate -- and at most 2 of its 192 feet with a normal force within 1e-6 (relative) of the contact threshold, at every sub-step count."""
    s, c, tid = PR.step_cases()
    models = [pkg.model_desc(r) for r in PR.ROBOTS]
    for sub in PR.STEP_SUBSTEPS:
        p = PR.params(substeps=sub)
        r = PR.step_mixed(models, tid, p, s, c)
        fn = r["fn"]
        assert fn.size == 192
        assert PR.near_threshold(p, fn).sum() <= 2
        print('substeps', sub, 'feet in contact at the last sub-step', (fn > 0).sum(), 'near the threshold', PR.near_threshold(p, fn).sum())
        assert (fn > 0).sum() >= 10 and (fn == 0).sum() >= 20          # (deep feet are thrown clear within a tick: fewer touch at 8 sub-steps)
        assert (np.abs(r["plant_out"][:, 28:40]) == p["tau_max"]).sum() >= 12
        assert np.all(np.isfinite(r["fb_state"]))
        sliding = np.hypot(r["plant_out"][:, 0:12:3], r["plant_out"][:, 1:12:3]) > 0.5 * p["mu"] * fn
        assert (sliding & (fn > 0)).sum() >= 5


@pytest.fixture(scope="module")
def closed_loop(pkg, oracle):
    """One robot per shove -- +x, +y and three diagonals at the full 0.3 m/s -- settled on joint PD (400 ticks of 1 ms, 1 sub-step), shoved,
    then 500 ticks of 2 ms at 2 sub-steps of plant -> oracle.tick_batch -> plant in float64 (the tick takes float32 rows, as on the device)."""
    md = _a1(pkg)
    shove = PR.SHOVE_MAX * np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0]])
    n = len(shove)
    p1 = PR.params(dt=0.001, substeps=1)
    s = M.normalised(PR.stand_state(1))
    for _ in range(400):
        s, aux = PR.substep(md, p1, s, PR.stand_cmd(1), p1["dt"])
    settle = dict(z=float(s[0, 6]), fz=float(aux["force"][0, :, 2].sum()))
    s = np.repeat(s, n, 0)
    s[:, 10:12] += shove
    p2 = PR.params(dt=0.002, substeps=2)
    traj, gait, wcmd, prev = PR.stand_tick_inputs(n)
    mcmd = np.zeros((n, 60), np.float32)
    flags, tau_peak = 0, 0.0
    for _ in range(500):
        mpc = PR.truth_mpc_state(md, p2, s)
        _, tau, st, _, prev = oracle.tick_batch(1, pkg.mpc_cfg("a1"), PR.HORIZON, md[:3], md, mpc.astype(np.float32), traj, gait, s.astype(np.float32), wcmd, prev)
        flags |= int(np.bitwise_or.reduce(st.astype(np.int64) & 0xff0000ff))
        tau_peak = max(tau_peak, float(np.abs(tau).max()))
        mcmd[:, 48:60] = tau
        for _ in range(p2["substeps"]):
            s, aux = PR.substep(md, p2, s, mcmd, p2["dt"] / p2["substeps"])
    return dict(shove=shove, state=s, flags=flags, tau_peak=tau_peak, settle=settle)


def test_closed_loop_with_the_oracle_raises_no_flag(closed_loop):
    assert closed_loop["flags"] == 0


def test_closed_loop_with_the_oracle_ends_inside_the_stand_band(closed_loop):
    """The band of the GPU closed-loop test, for the x, y and diagonal shoves at the full 0.3 m/s: the GPU test draws its shoves inside that
    square.  Measured: |x| <= 0.0026, |y| <= 0.0019, z 0.2670, |roll|, |pitch| <= 0.0061, peak torque 23.6 N m (the first ticks after the shove)."""
    s = closed_loop["state"]
    rpy = PR.quat_to_rpy(s[:, 0:4])
    print("settle", closed_loop["settle"], "end x", s[:, 4], "y", s[:, 5], "z", s[:, 6], "rpy", np.abs(rpy).max(0), "peak tau", closed_loop["tau_peak"])
    assert np.all(PR.in_band(s[:, 4:7], rpy))
    assert closed_loop["tau_peak"] < PR.DEFAULTS["tau_max"]
