"""TEST INFRASTRUCTURE -- swing-leg selection, the foothold heuristic and the swing trajectories in float64 with vectors and matrices, a second
statement beside oracle/qr_oracle_swing.cpp and the kernels (qr_foothold_kernel, qr_swing_velocity_kernel, qr_swing_kernel):

  * qrRaibertSwingLegController::Update, default branch (quadruped/src/controllers/qr_swing_leg_controller.cpp:211-236): a leg is planned unless
    it is STANCE with allowSwitchLegState, or EARLY_CONTACT;
  * qrFootholdPlanner::ComputeHeuristicFootHold (quadruped/src/planner/qr_foothold_planner.cpp:112-239) on flat ground: the hip's horizontal
    velocity R (v + omega x hipOffset) with np.cross, the Raibert expression target * swingRemainTime - swingKp (target - hip) taken back to the
    base frame and clipped at +-0.2, the hip offset, the abad link turned by the roll angle (stage_ref.rot_x), the body height along the base's
    vertical; the held-leg branch (allowSwitchLegState false) with its lateral trim of 0.005 beyond +-0.01 and the 0.02 drop;
  * the VELOCITY case of GetAction (qr_swing_leg_controller.cpp:285-309, 408-424): the same heuristic through baseRInControlFrame with
    stanceDuration / 2, and the trajectory at the warped phase 0.8 sin(pi phi) for phi <= 0.5, else 0.8 + 0.4 (phi - 0.5);
  * the trajectory as closed forms: XY linear in the phase, Z the parabola through the lift-off point at 0, max(z0, z1) + 0.1 at 0.5 (the apex the
    reference uses) and the target at 1, written as Lagrange interpolation.  The same generator at phaseModule = false (the phase as it is) is the
    trajectory of qrgpu_swing_targets_batch, whose points then go to the world frame.

Rotations are stage_ref.quat_to_rot_raw of the raw float32 quaternion.  The backwards-command lines that write past a 3-vector in the reference
(qr_foothold_planner.cpp:222-225) stay as the project documents them (oracle/qr_oracle_swing.cpp): not mirrored.

THRESHOLD TIES.  A (robot, leg) whose deciding quantity -- the held leg's lateral offset against +-0.01, a clipped component against +-0.2, the
phase against 0.5 -- sits within 4 float32 ulps of its threshold is compared on its flags only; footholds() and swing_velocity() return those pairs
and the check_* functions cap their share at 0.5 % per family.
"""
import numpy as np

import stage_ref as SR

N_ROBOTS = 65
ROBOTS = ("a1", "lite3")
TIE_CAP = 0.005
SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT = 0, 1, 2, 3
SIDE = np.array([-1.0, 1.0, -1.0, 1.0])


def near(v, threshold, ulps=4):
    return abs(v - threshold) <= ulps * float(np.spacing(np.float32(abs(threshold))))


def lever(ho):
    return np.array([-ho[1], ho[0], 0.0])


def footholds(desc29, in46):
    """One robot.  -> flag [4] (leg is in swingFootIds), phase [4] and foothold [4][3] (base frame; NaN rows for legs that are not planned),
    tie [4] (bool); footholds.clipped counts the (robot, leg) pairs whose Raibert step met the +-0.2 clip since it was last set to 0"""
    d = SR.widen(desc29); x = SR.widen(in46)
    hipOffset, hipPos, hip_l, kp, clearance = d[0:12].reshape(4, 3), d[12:24].reshape(4, 3), d[24], d[25:28], d[28]
    legState, allow, remain, nphase = x[0:4].astype(int), x[4:8] != 0, x[8:12], x[12:16]
    vdes, wdes, hdes = x[16:19], x[19], x[20]
    footB, roll, v, w = x[21:33].reshape(4, 3), x[37], x[40:43], x[43:46]
    R = SR.quat_to_rot_raw(x[33:37])
    flag = np.zeros(4); phase = np.full(4, np.nan); ftp = np.full((4, 3), np.nan); tie = np.zeros(4, bool)
    for leg in range(4):
        if (legState[leg] == STANCE and allow[leg]) or legState[leg] == EARLY_CONTACT:
            continue
        flag[leg] = 1
        if not allow[leg]:
            t = R @ (footB[leg] - hipPos[leg])
            tie[leg] = near(t[1], 0.01) or near(t[1], -0.01)
            if t[1] > 0.01:
                t[1] -= 0.005
            elif t[1] < -0.01:
                t[1] += 0.005
            t[2] -= 0.02
            ftp[leg] = R.T @ t + hipPos[leg]
            phase[leg] = 1.0
        else:
            hip_v = R @ (v + np.cross(w, hipOffset[leg])); hip_v[2] = 0
            target_v = vdes + wdes * lever(hipOffset[leg])
            dP = R.T @ (target_v * remain[leg] - kp * (target_v - hip_v))
            tie[leg] = any(near(dP[i], s * 0.2) for i in (0, 1) for s in (1, -1))
            footholds.clipped += int(abs(dP[0]) > 0.2 or abs(dP[1]) > 0.2)
            dP = np.array([np.clip(dP[0], -0.2, 0.2), np.clip(dP[1], -0.2, 0.2), 0.0])
            abad = SR.rot_x(roll).T @ np.array([0.0, hip_l * SIDE[leg], 0.0])
            ftp[leg] = dP + np.array([hipOffset[leg, 0], hipOffset[leg, 1], 0.0]) + abad - R.T @ np.array([0.0, 0.0, hdes - clearance])
            phase[leg] = nphase[leg]
    return flag, phase, ftp, tie


footholds.clipped = 0


def warp(phi):
    return 0.8 * np.sin(np.pi * phi) if phi <= 0.5 else 0.8 + 0.4 * (phi - 0.5)


def trajectory(p0, p1, s):
    """XY linear, Z the parabola through (0, z0), (0.5, max(z0, z1) + 0.1), (1, z1)."""
    xy = (1 - s) * p0[:2] + s * p1[:2]
    apex = max(p0[2], p1[2]) + 0.1
    z = p0[2] * (s - 0.5) * (s - 1) / 0.5 + apex * s * (s - 1) / -0.25 + p1[2] * s * (s - 0.5) / 0.5
    return np.array([xy[0], xy[1], z])


def swing_velocity(desc20, in53):
    """One robot.  -> flag [4], footTargetPosition [4][3], footPositionInBaseFrame [4][3] (base frame; NaN rows for legs not flagged), tie [4]"""
    d = SR.widen(desc20); x = SR.widen(in53)
    hipPos, stanceDuration, kp, height = d[0:12].reshape(4, 3), d[12:16], d[16:19], d[19]
    flag, nphase, liftoff = x[0:4] != 0, x[4:8], x[8:20].reshape(4, 3)
    v, yawDot, speed, twist, dR = x[20:23], x[23], x[24:27], x[27], x[28:37].reshape(3, 3)
    Rb = SR.quat_to_rot_raw(x[37:41])
    tgt = np.full((4, 3), np.nan); pos = np.full((4, 3), np.nan); tie = np.zeros(4, bool)
    for leg in np.nonzero(flag)[0]:
        hip_v = dR @ (v + yawDot * lever(hipPos[leg])); hip_v[2] = 0
        target_v = speed + twist * lever(hipPos[leg])
        tgt[leg] = dR.T @ (hip_v * stanceDuration[leg] / 2 - kp * (target_v - hip_v)) + np.array([hipPos[leg, 0], hipPos[leg, 1], 0.0]) \
            - Rb.T @ np.array([0.0, 0.0, height])
        tie[leg] = near(nphase[leg], 0.5)
        pos[leg] = trajectory(liftoff[leg], tgt[leg], warp(nphase[leg]))
    return flag.astype(float), tgt, pos, tie


def swing_targets(in58):
    """The trajectory part of the MPC/WBC mode's swing targets (phaseModule = false, horizontal terrain): -> flag [4], pFoot_des [4][3] (world),
    footTargetPositionsInWorldFrame [4][3], the trajectory point in the base-aligned frame the IK is given [4][3]"""
    x = SR.widen(in58)
    flag, phase, liftoff, foothold, bp = x[0:4] != 0, x[4:8], x[12:24].reshape(4, 3), x[24:36].reshape(4, 3), x[36:39]
    R = SR.quat_to_rot_raw(x[39:43])
    p_w = np.full((4, 3), np.nan); t_w = np.full((4, 3), np.nan); p_b = np.full((4, 3), np.nan)
    for leg in np.nonzero(flag)[0]:
        p_b[leg] = trajectory(liftoff[leg], foothold[leg], phase[leg])
        p_w[leg] = R @ p_b[leg] + bp
        t_w[leg] = R @ foothold[leg] + bp
    return flag.astype(float), p_w, t_w, p_b


# ----------------------------------------------------------------------------- families
def _raw_quat(rng, n, tilt=0.6):
    rpy = np.stack([rng.uniform(-tilt, tilt, n), rng.uniform(-tilt, tilt, n), rng.uniform(-np.pi, np.pi, n)], 1)
    q = SR._quat_from_rpy(rpy) * rng.uniform(0.99, 1.01, (n, 1))                 # raw: not normalised
    return q.astype(np.float32), rpy


def foothold_family(pkg, robot, n=N_ROBOTS):
    """fh_in [n][46]: wide raw attitudes (roll, pitch +-0.6), omega +-4, v +-2, commands +-1.5 with twist +-2 (the clip active on a known share),
    swingTimeRemaining 0 .. 0.4, leg states STANCE / SWING / EARLY_CONTACT / LOSE_CONTACT, commands on both sides of -0.01, and on a third of
    the robots held legs whose lateral offset is placed at +-0.01 -+ 1e-4, 1e-3 and well inside / outside."""
    W = pkg.workload
    rng = np.random.default_rng(0xF007 + ROBOTS.index(robot))
    x = W.make_foothold_batch(n, robot, seed=0xF0 + ROBOTS.index(robot))
    d = SR.widen(W.foothold_cfg(robot))
    hipPos = d[12:24].reshape(4, 3)
    q, rpy = _raw_quat(rng, n)
    x[:, 33:37] = q; x[:, 37:40] = rpy
    x[:, 0:4] = rng.choice([SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT], (n, 4), p=[0.45, 0.35, 0.1, 0.1])
    x[:, 4:8] = rng.random((n, 4)) > 0.1
    x[:, 8:12] = rng.uniform(0, 0.4, (n, 4))
    x[:, 16:19] = rng.uniform(-1.5, 1.5, (n, 3)); x[:, 18] = 0
    x[::5, 16] = np.resize(np.float32([-0.01, -0.0101, -0.0099, -0.011, -0.009]), x[::5].shape[0])
    x[:, 19] = rng.uniform(-2, 2, n)
    x[:, 40:43] = rng.uniform(-2, 2, (n, 3)); x[:, 43:46] = rng.uniform(-4, 4, (n, 3))
    lateral = np.array([0.01 + 1e-4, 0.01 - 1e-4, -0.01 + 1e-4, -0.01 - 1e-4, 0.011, 0.009, -0.011, -0.009, 0.05, -0.05, 0.0])
    for r in range(0, n, 3):
        x[r, 33:37] /= np.linalg.norm(x[r, 33:37].astype(np.float64))               # (a unit quaternion here, so that the offset lands where it is put)
        R = SR.quat_to_rot_raw(x[r, 33:37].astype(np.float64))
        for leg in range(4):
            x[r, 4 + leg] = 0
            t = np.array([rng.uniform(-0.05, 0.05), lateral[(r // 3 + leg) % lateral.size], rng.uniform(-0.3, -0.2)])
            x[r, 21 + 3 * leg:24 + 3 * leg] = hipPos[leg] + R.T @ t
    return x


def velocity_family(pkg, robot, n=N_ROBOTS):
    """swing_vel_in [n][53] on the same ranges; phases on both sides of 0.5 (0.4999, 0.5001, 0.49, 0.51, 0 and 1 included);
    dR is the rotation of a second wide attitude, as baseRInControlFrame is on a slope."""
    W = pkg.workload
    rng = np.random.default_rng(0x5E10 + ROBOTS.index(robot))
    x = W.make_swing_velocity_batch(n, robot, seed=0x5F + ROBOTS.index(robot))
    x[:, 0:4] = rng.random((n, 4)) > 0.25
    x[:, 4:8] = rng.uniform(0, 1, (n, 4))
    edge = np.float32([0.4999, 0.5001, 0.49, 0.51, 0.0, 1.0])
    x[::4, 4] = np.resize(edge, x[::4].shape[0])
    x[:, 20:23] = rng.uniform(-2, 2, (n, 3)); x[:, 23] = rng.uniform(-4, 4, n)
    x[:, 24:27] = rng.uniform(-1.5, 1.5, (n, 3)); x[:, 26] = 0; x[:, 27] = rng.uniform(-2, 2, n)
    q2, _ = _raw_quat(rng, n, 0.4)
    Rc = SR.quat_to_rot_raw((q2 / np.linalg.norm(q2, axis=1, keepdims=True)).astype(np.float64))
    x[:, 28:37] = Rc.reshape(n, 9)
    x[:, 37:41], _ = _raw_quat(rng, n)
    return x


def targets_family(pkg, robot, n=N_ROBOTS):
    """swing_in [n][58] for the trajectory of qrgpu_swing_targets_batch: the workload's batch with wide raw attitudes and phases over [0, 1]
    with its ends, and the two unreachable targets of stage_ref.unreachable_swing_in in the last two rows."""
    W = pkg.workload
    rng = np.random.default_rng(0x7A60 + ROBOTS.index(robot))
    cfg = W.estimator_cfg(robot)
    x = W.make_swing_batch(n - 2, seed=0x7A + ROBOTS.index(robot))
    x[:, 39:43], _ = _raw_quat(rng, n - 2)
    x[:, 4:8] = rng.uniform(0, 1, (n - 2, 4)); x[::6, 4] = 0; x[1::6, 5] = 1
    return np.concatenate([x, SR.unreachable_swing_in(cfg)[0]])


def tie_share(tie, flag):
    return float(tie[flag != 0].sum()) / max(1, int((flag != 0).sum()))


# ----------------------------------------------------------------------------- comparisons shared by the CPU and the -m gpu tests
SENTINEL = np.float32(-777.0)


def check_footholds(desc29, x, got58, tag, worst=None):
    """got58 [n][58] (oracle or kernel, started from SENTINEL rows) against footholds(): flags and phases exact, the same rows written, footholds
    1e-6 m; tie pairs on their flags only.  -> tie share"""
    ties = planned = 0
    for i in range(x.shape[0]):
        flag, phase, ftp, tie = footholds(desc29, x[i])
        g = got58[i]
        assert np.array_equal(g[0:4], flag), (tag, i)
        for leg in range(4):
            rows = np.r_[4 + leg, 24 + 3 * leg:27 + 3 * leg]
            if not flag[leg]:
                assert np.all(g[rows] == SENTINEL), (tag, i, leg)
                continue
            planned += 1
            assert np.all(g[rows] != SENTINEL), (tag, i, leg)
            if tie[leg]:
                ties += 1
                continue
            assert g[4 + leg] == np.float32(phase[leg]), (tag, i, leg)
            e = np.abs(g[24 + 3 * leg:27 + 3 * leg] - ftp[leg]).max()
            if worst is not None:
                SR.note(worst, tag + " foothold", e)
            assert e <= 1e-6, (tag, i, leg, e)
        other = np.setdiff1d(np.arange(58), np.r_[0:8, 24:36])
        assert np.all(g[other] == SENTINEL), (tag, i)
    share = ties / max(1, planned)
    assert share <= TIE_CAP, (tag, share)
    return share


def _check_angles(cfg, p, ang, leg, current, tag, where, worst):
    """Joint targets as stage_ref.check_ik judges them: the model's forward kinematics of the angles lands on the point, 5e-6 m, on the IK
    domain (|t1 + t2 / 2| <= 1.4, knee in -2.6 .. -0.3); where the model's angle does not exist the current angle is kept."""
    geom, ho = cfg[:3], cfg[7:19]
    want = SR.leg_ik(geom, ho, p, leg)
    for k in range(3):
        if np.isnan(want[k]):
            assert ang[k] == current[k], (tag, where, k)
    if np.isnan(want).any() or abs(want[1] + want[2] / 2) > 1.4 or not -2.6 <= want[2] <= -0.3:
        return
    q12 = np.zeros(12); q12[3 * leg:3 * leg + 3] = ang
    e = np.abs(SR.foot_positions(geom, ho, q12)[leg] - p).max()
    if worst is not None:
        SR.note(worst, tag + " FK(angles) - point", e)
    assert e <= 5e-6, (tag, where, e)


def check_velocity(cfg, desc20, x, got48, tag, worst=None):
    """got48 [n][48] (from SENTINEL rows) against swing_velocity(): legs not flagged untouched, targets 1e-6 m, trajectory points 2e-6 m, joint
    targets through the forward kinematics.  -> tie share"""
    ties = flagged = 0
    for i in range(x.shape[0]):
        flag, tgt, pos, tie = swing_velocity(desc20, x[i])
        g = got48[i]
        for leg in range(4):
            rows = np.concatenate([np.arange(12 * b + 3 * leg, 12 * b + 3 * leg + 3) for b in range(4)])
            if not flag[leg]:
                assert np.all(g[rows] == SENTINEL), (tag, i, leg)
                continue
            flagged += 1
            if tie[leg]:
                ties += 1
                continue
            e1 = np.abs(g[3 * leg:3 * leg + 3] - tgt[leg]).max(); e2 = np.abs(g[12 + 3 * leg:15 + 3 * leg] - pos[leg]).max()
            if worst is not None:
                SR.note(worst, tag + " target", e1); SR.note(worst, tag + " trajectory point", e2)
            assert e1 <= 1e-6 and e2 <= 2e-6, (tag, i, leg, e1, e2)
            _check_angles(cfg, g[12 + 3 * leg:15 + 3 * leg].astype(np.float64), g[24 + 3 * leg:27 + 3 * leg], leg, x[i, 41 + 3 * leg:44 + 3 * leg], tag, (i, leg),
                          worst)
    share = ties / max(1, flagged)
    assert share <= TIE_CAP, (tag, share)
    return share


def check_targets(x, got, tag, worst=None):
    """got [n][48]: pFoot_des[12], vFoot_des[12], aFoot_des[12], footTargetPositionsInWorldFrame[12] (from SENTINEL rows) against swing_targets():
    trajectory points and world-frame targets 2e-6 m (scaled by max(1, |p|): the world positions reach 5 m)."""
    for i in range(x.shape[0]):
        flag, p_w, t_w, _ = swing_targets(x[i])
        for leg in range(4):
            s = slice(3 * leg, 3 * leg + 3)
            if not flag[leg]:
                assert np.all(got[i, 0:12][s] == SENTINEL) and np.all(got[i, 36:48][s] == SENTINEL), (tag, i, leg)
                continue
            e1 = (np.abs(got[i, 0:12][s] - p_w[leg]) / np.maximum(1, np.abs(p_w[leg]))).max()
            e2 = (np.abs(got[i, 36:48][s] - t_w[leg]) / np.maximum(1, np.abs(t_w[leg]))).max()
            if worst is not None:
                SR.note(worst, tag + " pFoot_des", e1); SR.note(worst, tag + " foot target (world)", e2)
            assert e1 <= 2e-6 and e2 <= 2e-6, (tag, i, leg, e1, e2)
