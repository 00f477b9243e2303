"""CPU: tests/stage_ref.py (leg chain, Kalman filter, windows, pose) against mechanics and closed forms, and the oracle's estimator and leg
kinematics (oracle/qr_oracle_estimator.cpp, qr_oracle_math.cpp, qr_oracle_swing.cpp) against stage_ref on the wide families.

Bars of the oracle-against-model comparisons are the project's existing ones (tests/test_gpu_estimator.py, tests/test_oracle_swing.py): foot
positions 2e-6 m, J qd 2e-5 max(1, max|J qd|), filtered acceleration 2e-6, velocities and omega 1e-5, pose rows 2e-5 with equal NaN pattern,
IK residual 5e-6 m.  The model is float64; the oracle is the reference's float32 statement: float32 rounding is all that separates them.
Measured worst cases: LAB_NOTES.md, "Stage kernels against an independent model"."""
import numpy as np
import pytest

import rigid_body_ref as RB
import stage_ref as S

EPS = np.finfo(np.float64).eps
ROBOTS = ("a1", "lite3")


def _cfg(pkg, robot, window=120):
    return pkg.workload.estimator_cfg(robot, window=window)


def _geom(cfg):
    return cfg[:3], cfg[7:19]


# ----------------------------------------------------------------------------- the model obeys mechanics
@pytest.mark.parametrize("robot", ROBOTS)
def test_jacobian_is_the_derivative_of_the_chain(pkg, robot):
    """J = d FK / d q by central differences, h = 1e-5 rad.  A foot coordinate is sinusoidal in each joint angle with an amplitude of at most
    the reach L = hip_l + upper_l + lower_l, which bounds its third derivative too; |FK| <= |hip_offset| + L.
    Bar: h^2/6 L + 64 eps (|hip_offset| + L) / h = 1.1e-9."""
    geom, ho = _geom(_cfg(pkg, robot))
    q, _ = S.wide_joints(200, 11)
    q = q.astype(np.float64)
    h = 1e-5
    L = float(np.sum(S.widen(geom)))
    bar = h * h / 6 * L + 64 * EPS * (np.linalg.norm(S.widen(ho).reshape(4, 3), axis=1).max() + L) / h
    assert bar < 2e-9
    J = S.leg_jacobians(geom, ho, q)
    for k in range(12):
        dq = np.zeros(12); dq[k] = h
        fd = (S.foot_positions(geom, ho, q + dq) - S.foot_positions(geom, ho, q - dq)) / (2 * h)       # [n, 4, 3]
        for leg in range(4):
            want = J[:, leg, :, k % 3] if k // 3 == leg else 0.0
            assert np.abs(fd[:, leg] - want).max() <= bar, (k, leg)


def test_chain_equals_the_rigid_body_model_a1(pkg):
    """stage_ref's feet are the knee links' end points of rigid_body_ref.bodies (written for the WBC quantities, from the same mechanics but
    other code), seen from the base -- where that model's abad joint locations are the same data as hip_offset.  They are for A1.  For Lite3
    they are not: rigid_body_ref holds A1's (0.1805, 0.047) for both robots, as the reference's BuildDynamicModel does, while Lite3's
    hip_offset is (0.175, 0.062); that comparison is not made (LAB_NOTES.md)."""
    W = pkg.workload
    loc = np.array([RB.ABAD_LOC * np.array([sx, sy, 1.0]) for sx, sy in RB.LEG_SIGNS])
    assert np.array_equal(loc, S.widen(W.ROBOTS["a1"]["hip_offset"]))
    assert not np.array_equal(loc, S.widen(W.ROBOTS["lite3"]["hip_offset"]))
    cfg = _cfg(pkg, "a1")
    geom, ho = _geom(cfg)
    q, _ = S.wide_joints(100, 12)
    q = q.astype(np.float64)
    rng = np.random.default_rng(13)
    quat = rng.standard_normal((100, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    pos = rng.uniform(-2, 2, (100, 3))
    bs, feet = RB.bodies(W.model_desc("a1"), quat, pos, q)
    Rb = RB.quat_to_rot(quat)
    ll = float(S.widen(geom)[2])
    p = S.foot_positions(geom, ho, q)
    for leg, (knee, _) in enumerate(feet):
        tip = bs[knee]["p"] + np.einsum("nij,j->ni", bs[knee]["R"], np.array([0.0, 0.0, -ll]))        # without the model's +-4 mm contact-point offset
        in_base = np.einsum("nji,nj->ni", Rb, tip - pos)
        assert np.abs(in_base - p[:, leg]).max() <= 64 * EPS * 3.0, leg


@pytest.mark.parametrize("robot", ROBOTS)
def test_fk_of_ik_is_the_identity_on_the_ik_domain(pkg, robot):
    """On |t1 + t2/2| <= 1.4, knee -2.6..-0.3: IK(FK(q)) = q and FK(IK(p)) = p.  The inverse's condition is 1/sin|t2| <= 3.4 (knee from the
    distance) times 1/cos(t1 + t2/2) <= 5.9 (hip from the forward coordinate): 20 x a few float64 roundings of numbers below 1 -> bar 1e-12."""
    geom, ho = _geom(_cfg(pkg, robot))
    q = S.ik_joints(300, 21).astype(np.float64)
    p = S.foot_positions(geom, ho, q)
    for leg in range(4):
        a = S.leg_ik(geom, ho, p[:, leg], leg)
        assert np.abs(a - q[:, 3 * leg:3 * leg + 3]).max() <= 1e-12, leg
        q2 = q.copy(); q2[:, 3 * leg:3 * leg + 3] = a
        assert np.abs(S.foot_positions(geom, ho, q2)[:, leg] - p[:, leg]).max() <= 1e-12, leg


def test_ik_of_an_unreachable_point_is_nan(pkg):
    geom, ho = _geom(_cfg(pkg, "a1"))
    hof = S.widen(ho).reshape(4, 3)
    far = S.leg_ik(geom, ho, hof[1] + np.array([0.5, 0.0, -0.3]), 1)                 # 0.58 m from the hip: beyond hip_l + 0.4
    assert np.all(np.isnan(far))
    inside = S.leg_ik(geom, ho, hof[1] + np.array([0.15, 0.03, -0.04]), 1)          # 0.05 m from the abad axis: inside the hip_l cylinder
    assert np.isnan(inside[0]) and np.isnan(inside[1]) and np.isfinite(inside[2])


# ----------------------------------------------------------------------------- the filter against closed forms
def _quiet_input(n, qd):
    """A level robot at the stand pose whose accelerometer reads gravity alone: deltaV = 0; all feet in contact."""
    x = np.zeros((n, 54), np.float32)
    x[:, 2] = 9.81; x[:, 6] = 1.0; x[:, 13:17] = 1; x[:, 41:45] = 1
    x[:, 17:29] = np.tile(S.STAND, 4); x[:, 29:41] = qd
    x[:, 45:54] = np.eye(3).reshape(-1)
    return x


@pytest.mark.parametrize("qv,rv", [(0.1, 0.1), (0.02, 0.5)])
def test_kalman_gain_converges_to_the_scalar_riccati_fixed_point(pkg, qv, rv):
    """Constant observation z, deltaV = 0, F = H = I, Q = q I, R = r I: the covariance stays a multiple of I and obeys the scalar
    recursion P <- (P + q) r / (P + q + r), whose fixed point is P = (-q + sqrt(q^2 + 4 q r)) / 2; the gain is K = (P + q) / (P + q + r) and
    the state closes in on z by the factor (1 - K) per tick."""
    cfg = pkg.workload.estimator_cfg("a1", window=1, accelerometer_variance=qv, sensor_variance=rv)
    qv, rv = float(np.float32(qv)), float(np.float32(rv))
    e = S.Estimator(cfg, 1)
    x = _quiet_input(1, np.tile([0.0, 2.0, -1.0], 4))
    geom, ho = _geom(cfg)
    z = -np.mean(np.einsum("lij,lj->li", S.leg_jacobians(geom, ho, x[0, 17:29].astype(np.float64)), x[0, 29:41].astype(np.float64).reshape(4, 3)), axis=0)
    assert np.abs(z).max() > 0.1
    # (the accelerometer's float32(9.81) is 2e-7 off the 9.81 that is subtracted: deltaV_z = that times deltaTime, 4e-10 per tick)
    g_off = float(np.float32(9.81)) - 9.81
    P, xs = 0.0, np.zeros(3)
    for k in range(300):
        e.update(x, np.array([1 + 2 * k], np.uint32))
        xs = xs + np.array([0.0, 0.0, g_off * (float(np.float32(0.002)) if k == 0 else 0.002)])
        Pp = P + qv; K = Pp / (Pp + rv); P = (1 - K) * Pp; xs = xs + K * (z - xs)
        assert np.abs(e.P[0] - P * np.eye(3)).max() <= 1e-15
        assert np.abs(e.x[0] - xs).max() <= 1e-13
    Pinf = (-qv + np.sqrt(qv * qv + 4 * qv * rv)) / 2
    assert abs(e.P[0, 0, 0] - Pinf) <= 1e-14
    assert np.abs(e.x[0, :2] - z[:2]).max() <= 1e-12 and abs(e.x[0, 2] - z[2]) <= 1e-8      # (z axis: the 4e-10 per tick above, times (1 - K) / K)


def test_windows_are_plain_means(pkg):
    """The acceleration output is the mean of the last min(k + 1, 20) samples; the W = 8 velocity is the sliding mean of the W = 1 velocity
    (= float32 of the Kalman state) over the last min(k + 1, 8) ticks -- on robots whose feet never all leave the ground, where the Kalman
    state does not depend on W."""
    n, ticks = 12, 40
    x, stamp = S.wide_sensor_streams(n, ticks, 31)
    trot = np.arange(n) % 3 == 0
    o1 = S.estimator_run(_cfg(pkg, "a1", 1), x, stamp)
    o8 = S.estimator_run(_cfg(pkg, "a1", 8), x, stamp)
    a = x[:, :, 3:6].astype(np.float64)
    for k in range(ticks):
        assert np.abs(o1[k, :, 0:3] - a[max(0, k - 19):k + 1].mean(axis=0)).max() <= 1e-14
        assert np.abs(o8[k, trot, 3:6] - o1[max(0, k - 7):k + 1][:, trot, 3:6].mean(axis=0)).max() <= 1e-14
    assert np.array_equal(o1[:, :, 3:6], o1[:, :, 3:6].astype(np.float32).astype(np.float64))           # the window holds float32(x)


def test_delta_time_rule(pkg):
    """time_step while the stored stamp is 0 -- so a stream that starts at stamp 0 takes time_step twice -- else the stamp difference mod 2^32."""
    cfg = pkg.workload.estimator_cfg("a1", window=1, time_step=0.005)
    x = _quiet_input(3, 0.0)
    x[:, 12] = 1.0                                                   # yaw rate 1 rad/s: the yaw output integrates deltaTime
    e = S.Estimator(cfg, 3)
    stamps = np.array([[0, 1, 2 ** 32 - 3], [2, 3, 2 ** 32 - 1], [4, 5, 1], [7, 8, 4]], np.uint64).astype(np.uint32)
    yaw = np.stack([e.update(x, s)[:, 41] for s in stamps])
    dt = np.diff(np.concatenate([np.zeros((1, 3)), yaw]), axis=0)
    ts = float(np.float32(0.005))
    assert np.allclose(dt, [[ts, ts, ts], [ts, 0.002, 0.002], [0.002, 0.002, 0.002], [0.003, 0.003, 0.003]], rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------- the oracle agrees with the model
@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for k in sorted(w):
        print("stage_ref worst case  %-40s %.3e" % (k, w[k]))


_note = S.note


@pytest.mark.parametrize("robot", ROBOTS)
def test_oracle_kinematics_on_the_wide_family(pkg, oracle, worst, robot):
    cfg = _cfg(pkg, robot)
    geom, ho = _geom(cfg)
    q, qd = S.wide_joints(400, 41)
    p = S.foot_positions(geom, ho, q); J = S.leg_jacobians(geom, ho, q)
    v = np.einsum("nlij,nlj->nli", J, qd.astype(np.float64).reshape(-1, 4, 3))
    for r in range(q.shape[0]):
        po = oracle.foot_positions(geom, ho, q[r]).reshape(4, 3)
        ep = np.abs(po - p[r]).max()
        _note(worst, robot + " foot position", ep)
        assert ep <= 2e-6, (r, ep)
        for leg in range(4):
            Jo = oracle.leg_jacobian(geom, q[r, 3 * leg:3 * leg + 3], leg)
            vo = Jo.astype(np.float32) @ qd[r, 3 * leg:3 * leg + 3]
            ev = np.abs(vo - v[r, leg]).max() / max(1.0, np.abs(v[r, leg]).max())
            _note(worst, robot + " J qd (relative)", ev)
            _note(worst, robot + " Jacobian entry", np.abs(Jo - J[r, leg]).max())
            assert ev <= 2e-5, (r, leg, ev)


@pytest.mark.parametrize("robot", ROBOTS)
def test_oracle_ik_on_the_ik_domain(pkg, oracle, worst, robot):
    cfg = _cfg(pkg, robot)
    geom, ho = _geom(cfg)
    q = S.ik_joints(300, 51)
    x = S.ik_swing_in(cfg, q)
    ang = np.stack([oracle.swing_targets(geom, ho, x[r])[48:60] for r in range(x.shape[0])])
    assert np.all(np.isfinite(ang))
    S.check_ik(cfg, x, ang, worst, robot + " IK residual")
    _note(worst, robot + " IK angle", np.abs(ang - q).max())
    # the two unreachable targets: NaN angles are replaced by the current ones, the others are kept
    xu, cur = S.unreachable_swing_in(cfg)
    a0 = oracle.swing_targets(geom, ho, xu[0])[48:60]
    a1 = oracle.swing_targets(geom, ho, xu[1])[48:60]
    assert np.array_equal(a0[3:6], cur[3:6])
    assert np.array_equal(a1[3:5], cur[3:5]) and a1[5] != cur[5]
    want = S.leg_ik(geom, ho, xu[1, 15:18], 1)
    assert np.isnan(want[0]) and np.isnan(want[1]) and abs(a1[5] - want[2]) <= 2e-6
    for a in (a0, a1):                                                               # the other legs are ordinary
        assert np.abs(np.delete(a, [3, 4, 5]) - np.delete(np.tile(S.STAND, 4), [3, 4, 5])).max() <= 2e-5


@pytest.mark.parametrize("window,ticks", S.STREAM_CASES)
@pytest.mark.parametrize("robot", ROBOTS)
def test_oracle_estimator_on_the_wide_streams(pkg, oracle, worst, robot, window, ticks):
    cfg = _cfg(pkg, robot, window)
    x, stamp = S.wide_sensor_streams(S.STREAM_N, ticks, 60 + window)
    m = S.estimator_run(cfg, x, stamp)
    o = np.stack([oracle.estimator_run(cfg, x[:, r], stamp[:, r]) for r in range(S.STREAM_N)], axis=1)
    assert np.isnan(m[:, :, 39]).any() and np.isfinite(m[:, :, 39]).any()            # both height branches
    if ticks > 75:
        assert (np.diff(stamp.astype(np.int64), axis=0) < 0).any()                   # the stamp wraps
    for k in range(ticks):
        S.check_stream(o[k], m[k], "%s W=%d" % (robot, window), worst)
