"""CPU: what tests/cadence_ref.py restates is held against first principles, so that the host and GPU comparisons built on it are worth something:
the leg Jacobian against a central difference of the leg's forward kinematics, the kept force against the rotation's defining property, the
cadence's share of re-planning ticks, and the state machine's memory."""
import numpy as np

import cadence_ref as R


def _foot(angles, leg, legs=R.A1_LEGS):
    """FootPositionInHipFrame (qr_robot.cpp:104-126): the position the analytical Jacobian differentiates."""
    hip, lu, ll = legs
    sh = hip * (-1) ** (leg + 1)
    t0, t1, t2 = angles[:, 0], angles[:, 1], angles[:, 2]
    lEff = np.sqrt(lu * lu + ll * ll + 2 * lu * ll * np.cos(t2))
    tEff = t1 + t2 / 2
    x = -lEff * np.sin(tEff)
    z = -lEff * np.cos(tEff)
    return np.stack([x, np.cos(t0) * sh - np.sin(t0) * z, np.sin(t0) * sh + np.cos(t0) * z], 1)


def test_leg_jacobian_is_the_derivative_of_the_foot_position():
    q = R.poses()["q"].astype(np.float64).reshape(-1, 4, 3)
    eps = 1e-6
    for leg in range(4):
        J = R.leg_jacobian(q[:, leg], leg)
        for j in range(3):
            d = np.zeros(3); d[j] = eps
            fd = (_foot(q[:, leg] + d, leg) - _foot(q[:, leg] - d, leg)) / (2 * eps)
            assert np.abs(J[:, :, j] - fd).max() < 1e-8, (leg, j)


def test_hold_is_the_negated_force_in_the_base_frame():
    P = R.poses()
    Rm = R.rotation(P["quat"])
    assert np.abs(np.einsum("nij,nkj->nik", Rm, Rm) - np.eye(3)).max() < 1e-6           # (the quaternions are unit to float32)
    hold = R.hold_from_force(P["quat"], P["force"]).reshape(-1, 4, 3)
    back = -np.einsum("nij,nlj->nli", Rm, hold)                                         # base -> world of -f_ff gives f back
    assert np.abs(back - P["force"].astype(np.float64).reshape(-1, 4, 3)).max() < 1e-4
    # a level base facing +x keeps the force's components
    level = R.hold_from_force(np.array([[1.0, 0, 0, 0]]), np.arange(12.0)[None])
    assert np.array_equal(level, -np.arange(12.0)[None])


def test_share_of_due_ticks_is_one_in_a_period():
    period = R.period_of(0.002, 0.06)
    assert period == 15 and R.period_of(0.002, 0.05) == 12
    for period, ticks in ((12, 36), (15, 45)):
        c0 = 50 + np.arange(70) % period
        S = R.due_schedule(c0, period, ticks)
        assert S.mean() == 1.0 / period and np.all(S.sum(0) == ticks // period)
        assert all(0 < S[t].sum() < 70 for t in range(ticks))                          # another subset every tick, never all or none
    assert R.due(np.arange(50), 12).all() and not R.due(np.array([50, 59, 61]), 12).any() and R.due(np.array([60]), 12).all()


def test_state_machine_keeps_force_and_hold_between_solves():
    P = R.poses(8, 1)
    n = 8
    m = R.Cadence(np.zeros((n, 12)), np.zeros((n, 12)))
    d0 = np.arange(n) % 2 == 0
    tau0, wbc0 = m.tick(d0, P["force"], P["quat"], P["q"])
    assert np.array_equal(wbc0, ~d0) and np.all(m.force[~d0] == 0) and np.all(tau0[~d0] == 0)
    assert np.array_equal(m.hold[d0], R.hold_from_force(P["quat"][d0], P["force"][d0]))
    kept = m.hold.copy()
    q1 = P["q"][::-1].copy()
    tau1, wbc1 = m.tick(np.zeros(n, bool), 2 * P["force"], P["quat"][::-1], q1)        # nobody due: another attitude and force change nothing kept
    assert wbc1.all() and np.array_equal(m.hold, kept)
    assert np.array_equal(tau1, R.torque(q1, kept))                                    # ... and the kept force goes through the Jacobian of NOW
    both = R.epilogue(tau1, ~d0[:, None].repeat(4, 1), R.EPILOGUE_HIP_COMP | R.EPILOGUE_CLIP)
    assert np.abs(both).max() <= 23 and np.all(both[d0] == np.clip(tau1[d0], -23, 23))
