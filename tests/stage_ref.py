"""TEST INFRASTRUCTURE -- the first-generation stage kernels (leg kinematics, velocity and pose estimator, state packing) as an independent
float64 numpy model, batched over a leading robot axis.

It shares no formulation with qr_estimator_kernel.hip / qr_wave_helpers.h or with oracle/qr_oracle_estimator.cpp (both restate the reference's
closed forms in its operation order): the leg is a three-link chain of rotation matrices, the Jacobian is `axis x lever`, the filter is the
textbook linear Kalman recursion solved by numpy.linalg, the windows are plain means over kept samples.  What the three agree on is
mechanics and filtering, not a restatement.  The reference (quadruped/src/robots/qr_robot.cpp, estimators/qr_robot_velocity_estimator.cpp,
estimators/qr_robot_pose_estimator.cpp) is consulted only for WHAT is modelled: which frames, which samples, which rule for the time step.

Leg chain, foot in the base frame (legs FR, FL, RR, RL; abad about x, hip and knee about y):

    p_foot = hip_offset + Rx(t0) ([0, sh, 0] + Ry(t1) ([0, 0, -lu] + Ry(t2) [0, 0, -ll])),      sh = -hip_l on legs 0, 2 and +hip_l on legs 1, 3

    J[:, k] = axis_k x (p_foot - p_joint_k)         joints at hip_offset (axis e_x), at the end of the hip link and at the knee (axis Rx(t0) e_y)

The reference's closed forms (FootPositionInHipFrame, AnalyticalLegJacobian) go through an "effective leg" of length lEff at the angle
t1 + t2/2.  That is exact only for upper_l == lower_l, which both supported robots have; with 0.20 / 0.21 the chain and the closed form are
7.8 mm apart.  This model is the chain.  The difference is the reference's behaviour and is not "fixed" anywhere: for equal link lengths the
two are the same function (1.7e-16 on positions and all nine Jacobian entries).  The inverse kinematics here inverts the chain for any
link lengths; it agrees with the reference's wherever |t1 + t2/2| < pi/2, the half space the reference's asin can return.

Estimator, per tick (rows of est_in / est_out: include/qrgpu.h):
  * attitude R (base -> world) from the RAW quaternion, not normalised: R = I + 2 w [v]x + 2 [v]x^2
  * deltaTime = time_step while the stored stamp is 0, else ((tick - stored) mod 2^32) / 1000; the stamp is then stored
  * filtered acceleration: mean of the last min(k + 1, 20) samples of baseLinearAcceleration
  * observation: mean over the feet in contact of -R (J qd + omega x p); with no foot in contact the previous base-frame velocity
  * Kalman step with F = H = I, Q = q I, R = r I, P0 = 0 (the reference's TinyEKF constructor ignores initialVariance, TinyEKF.h:50-70)
  * velocity: mean of the last min(k + 1, W) samples of float32(x)
  * pose: stance-foot height in the world (body_height with no stance leg) and in the ground frame (NaN with no stance leg), planar
    odometry and yaw integration with the velocity just estimated, absolute height
"""
import numpy as np

_f = np.float32
GRAVITY = 9.81
ACC_WINDOW = 20
EX = np.array([1.0, 0.0, 0.0])
EY = np.array([0.0, 1.0, 0.0])


def widen(x):
    """A parameter as the kernels hold it: rounded to float32, widened to float64."""
    return np.asarray(x, _f).astype(np.float64)


def rot_x(t):
    t = np.asarray(t, np.float64)
    c, s = np.cos(t), np.sin(t)
    R = np.zeros(t.shape + (3, 3))
    R[..., 0, 0] = 1; R[..., 1, 1] = c; R[..., 1, 2] = -s; R[..., 2, 1] = s; R[..., 2, 2] = c
    return R


def rot_y(t):
    t = np.asarray(t, np.float64)
    c, s = np.cos(t), np.sin(t)
    R = np.zeros(t.shape + (3, 3))
    R[..., 1, 1] = 1; R[..., 0, 0] = c; R[..., 0, 2] = s; R[..., 2, 0] = -s; R[..., 2, 2] = c
    return R


def _mv(R, v):
    return np.einsum("...ij,...j->...i", R, v)


def side(leg):
    return -1.0 if leg in (0, 2) else 1.0


def leg_chain(geom, hip_offset, q3, leg):
    """One leg's chain for joint angles q3 [..., 3].  -> joint positions [3] of [..., 3], joint axes [3] of [..., 3], foot [..., 3] (base frame)."""
    hip_l, lu, ll = (float(x) for x in widen(geom)[:3])
    ho = widen(hip_offset).reshape(4, 3)[leg]
    q3 = np.asarray(q3, np.float64)
    Ra = rot_x(q3[..., 0])
    Rh = Ra @ rot_y(q3[..., 1])
    Rk = Rh @ rot_y(q3[..., 2])
    p0 = np.broadcast_to(ho, q3.shape).copy()
    p1 = p0 + _mv(Ra, np.array([0.0, side(leg) * hip_l, 0.0]))
    p2 = p1 + _mv(Rh, np.array([0.0, 0.0, -lu]))
    foot = p2 + _mv(Rk, np.array([0.0, 0.0, -ll]))
    ay = _mv(Ra, EY)
    return [p0, p1, p2], [np.broadcast_to(EX, q3.shape), ay, ay], foot


def foot_positions(geom, hip_offset, q12):
    """[..., 12] joint angles -> [..., 4, 3] feet in the base frame."""
    q12 = np.asarray(q12, np.float64)
    return np.stack([leg_chain(geom, hip_offset, q12[..., 3 * l:3 * l + 3], l)[2] for l in range(4)], axis=-2)


def leg_jacobians(geom, hip_offset, q12):
    """[..., 12] -> [..., 4, 3, 3]: d foot / d q of each leg, column k = axis_k x (foot - joint_k)."""
    q12 = np.asarray(q12, np.float64)
    out = []
    for l in range(4):
        joints, axes, foot = leg_chain(geom, hip_offset, q12[..., 3 * l:3 * l + 3], l)
        out.append(np.stack([np.cross(a, foot - p) for p, a in zip(joints, axes)], axis=-1))
    return np.stack(out, axis=-3)


def leg_ik(geom, hip_offset, p, leg):
    """Joint angles [..., 3] that put leg `leg`'s foot at p [..., 3] (base frame): knee bent backwards (t2 <= 0), leg below the hip axis.
    An angle that does not exist is NaN: all three beyond the leg's reach, abad and hip for a point inside the cylinder of radius hip_l about
    the abad axis."""
    hip_l, lu, ll = (float(x) for x in widen(geom)[:3])
    sh = side(leg) * hip_l
    d = np.asarray(p, np.float64) - widen(hip_offset).reshape(4, 3)[leg]
    with np.errstate(invalid="ignore"):
        t2 = -np.arccos((np.sum(d * d, axis=-1) - (sh * sh + lu * lu + ll * ll)) / (2 * lu * ll))      # law of cosines on |foot - hip joint|
        vz = -np.sqrt(d[..., 1] ** 2 + d[..., 2] ** 2 - sh * sh)                                          # the leg plane's coordinate, below the axis
        t0 = np.arctan2(d[..., 2], d[..., 1]) - np.arctan2(vz, sh)                                        # (y, z) = Rot(t0) (sh, vz)
        t0 = np.where(np.isnan(t2), np.nan, (t0 + np.pi) % (2 * np.pi) - np.pi)
        t1 = np.arctan2(-d[..., 0], -vz) - np.arctan2(ll * np.sin(t2), lu + ll * np.cos(t2))
    return np.stack([t0, t1, t2], axis=-1)


def quat_to_rot_raw(q):
    """R = I + 2 w [v]x + 2 [v]x^2 of a quaternion (w, x, y, z) taken as it is (for a unit quaternion: its base -> world rotation)."""
    q = np.asarray(q, np.float64)
    w, v = q[..., 0], q[..., 1:4]
    S = np.zeros(q.shape[:-1] + (3, 3))
    S[..., 0, 1] = -v[..., 2]; S[..., 0, 2] = v[..., 1]; S[..., 1, 0] = v[..., 2]
    S[..., 1, 2] = -v[..., 0]; S[..., 2, 0] = -v[..., 1]; S[..., 2, 1] = v[..., 0]
    return np.eye(3) + 2 * w[..., None, None] * S + 2 * (S @ S)


class Estimator:
    """n robots' velocity + pose estimators from construction.  cfg20 = workload.estimator_cfg()."""

    def __init__(self, cfg20, n):
        c = widen(cfg20)
        self.geom, self.time_step, self.qvar, self.rvar, self.W = c[:3], c[3], c[4], c[5], int(c[6])
        self.hip_offset, self.body_height = c[7:19], c[19]
        self.n = n
        self.stamp = np.zeros(n, np.uint32)
        self.x = np.zeros((n, 3)); self.P = np.zeros((n, 3, 3))
        self.acc, self.vel = [], []
        self.vb = np.zeros((n, 3))
        self.pose = np.zeros((n, 4))                    # x, y, yaw, absolute height

    def update(self, est_in, tick):
        """est_in [n, 54] float32, tick [n] uint32 -> est_out [n, 42] float64."""
        u = np.asarray(est_in, _f).astype(np.float64)
        tick = np.asarray(tick, np.uint32)
        n = self.n
        q, qd, omega, contact = u[:, 17:29], u[:, 29:41], u[:, 10:13], u[:, 13:17] != 0
        p = foot_positions(self.geom, self.hip_offset, q)
        v = np.einsum("nlij,nlj->nli", leg_jacobians(self.geom, self.hip_offset, q), qd.reshape(n, 4, 3))
        self.acc = (self.acc + [u[:, 3:6]])[-ACC_WINDOW:]
        facc = np.mean(self.acc, axis=0)
        dt = np.where(self.stamp == 0, self.time_step, (tick - self.stamp).astype(np.float64) / 1000.0)      # uint32 difference: mod 2^32
        self.stamp = tick.copy()
        R = quat_to_rot_raw(u[:, 6:10])
        dv = (_mv(R, u[:, 0:3]) - np.array([0, 0, GRAVITY])) * dt[:, None]
        obs = -_mv(R[:, None], v + np.cross(omega[:, None, :], p))                                             # [n, 4, 3]
        cnt = contact.sum(axis=1)
        z = np.where(cnt[:, None] > 0, (obs * contact[:, :, None]).sum(axis=1) / np.maximum(cnt, 1)[:, None], self.vb)
        # linear Kalman step, F = H = I
        I3 = np.eye(3)
        xp = self.x + dv
        Pp = self.P + self.qvar * I3
        K = np.swapaxes(np.linalg.solve(Pp + self.rvar * I3, np.swapaxes(Pp, 1, 2)), 1, 2)                   # Pp S^-1, S symmetric
        self.x = xp + _mv(K, z - xp)
        self.P = (I3 - K) @ Pp
        self.vel = (self.vel + [self.x.astype(_f).astype(np.float64)])[-self.W:]
        vw = np.mean(self.vel, axis=0)
        self.vb = _mv(np.swapaxes(R, 1, 2), vw)
        out = np.zeros((n, 42))
        out[:, 0:3] = facc; out[:, 3:6] = vw; out[:, 6:9] = self.vb; out[:, 9:12] = _mv(R, omega)
        out[:, 12:24] = p.reshape(n, 12); out[:, 24:36] = v.reshape(n, 12)
        # pose estimator
        stance = u[:, 41:45].astype(np.int64) == 1
        ns = stance.sum(axis=1)
        pw = _mv(R[:, None], p)                                                                              # feet, world axes
        G = u[:, 45:54].reshape(n, 3, 3)
        pg = _mv(np.swapaxes(G, 1, 2)[:, None], pw)                                                          # feet, ground axes
        with np.errstate(invalid="ignore", divide="ignore"):
            height = np.where(ns > 0, -(pw[:, :, 2] * stance).sum(axis=1) / ns, self.body_height)
            hground = np.where(ns > 0, -(pg[:, :, 2] * stance).sum(axis=1) / ns, np.nan)
        th = self.pose[:, 2]
        self.pose[:, 0] += (self.vb[:, 0] * np.cos(th) - self.vb[:, 1] * np.sin(th)) * dt
        self.pose[:, 1] += (self.vb[:, 0] * np.sin(th) + self.vb[:, 1] * np.cos(th)) * dt
        self.pose[:, 3] += self.vb[:, 2] * dt
        self.pose[:, 2] = th + omega[:, 2] * dt
        out[:, 36] = self.pose[:, 0]; out[:, 37] = self.pose[:, 1]; out[:, 38] = height; out[:, 39] = hground
        out[:, 40] = self.pose[:, 3]; out[:, 41] = self.pose[:, 2]
        return out


def estimator_run(cfg20, x, stamp):
    """x [ticks, n, 54], stamp [ticks, n] -> [ticks, n, 42] from fresh estimators."""
    e = Estimator(cfg20, x.shape[1])
    return np.stack([e.update(x[k], stamp[k]) for k in range(x.shape[0])])


def pack_state(est_in, est_out, rpy, com_offset):
    """-> mpc_state [n, 28], fb_state [n, 37] (float64) from est_in [n, 54], est_out [n, 42], rpy [n, 3], com_offset [3]:
    mpc_state = position, world velocity, quaternion, world angular velocity, R (foot - com_offset) per leg, rpy;
    fb_state = quaternion, position, body angular rate, base-frame velocity, q, qd."""
    u = np.asarray(est_in, _f).astype(np.float64); e = np.asarray(est_out, _f).astype(np.float64)
    n = u.shape[0]
    R = quat_to_rot_raw(u[:, 6:10])
    lever = _mv(R[:, None], e[:, 12:24].reshape(n, 4, 3) - widen(com_offset))
    mpc = np.concatenate([e[:, 36:39], e[:, 3:6], u[:, 6:10], e[:, 9:12], lever.reshape(n, 12), np.asarray(rpy, _f).astype(np.float64)], axis=1)
    fb = np.concatenate([u[:, 6:10], e[:, 36:39], u[:, 10:13], e[:, 6:9], u[:, 17:29], u[:, 29:41]], axis=1)
    return mpc, fb


# ----------------------------------------------------------------------------- input families (tests/test_stage_ref.py, the -m gpu tests)
STAND = np.array([0.0, 0.9, -1.8])
Q_LO = np.array([-1.0, -1.0, -2.6])
Q_HI = np.array([1.0, 2.5, -0.3])
QD_MAX = 15.0
IK_EFF_MAX = 1.4
EDGE_ROWS = 4            # rest, the stand pose, t0 = 0, t2 = -pi/2


def wide_joints(n, seed):
    """q [n, 12], qd [n, 12] (float32): abad +-1.0, hip -1.0..2.5, knee -2.6..-0.3, qd +-15 on every leg; rows 0-3 are the edge rows: rest
    (stand pose, qd = 0), the stand pose, t0 = 0, t2 = -pi/2."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(np.tile(Q_LO, 4), np.tile(Q_HI, 4), (n, 12))
    qd = rng.uniform(-QD_MAX, QD_MAX, (n, 12))
    q[0] = np.tile(STAND, 4); qd[0] = 0
    q[1] = np.tile(STAND, 4)
    q[2, 0::3] = 0.0
    q[3, 2::3] = -np.pi / 2
    return q.astype(_f), qd.astype(_f)


def ik_joints(n, seed):
    """The wide family restricted to |t1 + t2/2| <= 1.4 (the hip angle is redrawn inside the band; nothing else is excluded)."""
    q, _ = wide_joints(n, seed)
    q = q.astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    for leg in range(4):
        t2 = q[:, 3 * leg + 2]
        lo = np.maximum(Q_LO[1], -IK_EFF_MAX - t2 / 2); hi = np.minimum(Q_HI[1], IK_EFF_MAX - t2 / 2)
        bad = np.abs(q[:, 3 * leg + 1] + t2 / 2) > IK_EFF_MAX
        q[bad, 3 * leg + 1] = rng.uniform(lo, hi)[bad]
    q = q.astype(_f)
    assert np.all(np.abs(q[:, 1::3].astype(np.float64) + q[:, 2::3].astype(np.float64) / 2) <= IK_EFF_MAX + 1e-6)
    return q


def _quat_from_rpy(rpy):
    hr, hp, hy = rpy[:, 0] / 2, rpy[:, 1] / 2, rpy[:, 2] / 2
    cr, sr, cp, sp, cy, sy = np.cos(hr), np.sin(hr), np.cos(hp), np.sin(hp), np.cos(hy), np.sin(hy)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)


FIRST_STAMPS = (0, 1, 2 ** 32 - 150)


def wide_sensor_streams(n, ticks, seed, dt_ms=2):
    """Sensor streams [ticks][n][54] float32 + stamps [ticks][n] uint32 in the manner of workload.make_estimator_sequence, widened: joints sweep the
    wide family (a smooth path between two wide draws, rates up to +-15), roll and pitch up to +-0.6, omega +-4; robot i's contacts are a
    trot (i % 3 == 0), all four feet in flight from tick 5 on (i % 3 == 1) or exactly one foot in contact (i % 3 == 2); its first stamp is
    FIRST_STAMPS[(i // 3) % 3]: 0, 1, or 2^32 - 150 so that the stamp wraps in mid-sequence; 5 % of the ticks carry a late sample (+1 ms).
    Every fifth robot stands on a pitched ground frame."""
    rng = np.random.default_rng(seed)
    x = np.zeros((ticks, n, 54), _f)
    idx = np.arange(n)
    gp = np.where(idx % 5 == 2, 0.2, 0.0)
    gmat = np.zeros((n, 9)); gmat[:, 0] = np.cos(gp); gmat[:, 2] = np.sin(gp); gmat[:, 4] = 1; gmat[:, 6] = -np.sin(gp); gmat[:, 8] = np.cos(gp)
    qa, _ = wide_joints(n, seed + 11); qb, _ = wide_joints(n, seed + 12)
    qa, qb = qa.astype(np.float64), qb.astype(np.float64)
    qd_amp = rng.uniform(-QD_MAX, QD_MAX, (n, 12))
    t0 = np.array(FIRST_STAMPS, np.uint64)[(idx // 3) % 3]
    phase0 = rng.uniform(0, 1, n); yaw0 = rng.uniform(-np.pi, np.pi, n)
    amp = rng.uniform(-0.6, 0.6, (n, 2)); wamp = rng.uniform(-4, 4, (n, 3))
    stamp = np.zeros((ticks, n), np.uint32)
    T =ticks * dt_ms * 1e-3
    for k in range(ticks):
        t = k * dt_ms * 1e-3
        s = 0.5 - 0.5 * np.cos(np.pi * t / T)                                 # 0 -> 1 over the sequence
        rpy = np.stack([amp[:, 0] * np.sin(9 * t + phase0), amp[:, 1] * np.cos(7 * t + phase0), yaw0 + 0.8 * t], 1)
        x[k, :, 6:10] = _quat_from_rpy(rpy)
        x[k, :, 10:13] = wamp * np.cos(11 * t + phase0)[:, None] + 0.02 * rng.standard_normal((n, 3))
        acc = np.stack([1.5 * np.sin(5 * t + phase0), 1.0 * np.cos(4 * t + phase0), 9.81 + 0.8 * np.sin(7 * t + phase0)], 1)
        x[k, :, 0:3] = acc + 0.1 * rng.standard_normal((n, 3))
        x[k, :, 3:6] = acc - np.array([0, 0, 9.81]) + 0.1 * rng.standard_normal((n, 3))
        ph = (phase0 + t / 0.1) % 1.0
        c = np.stack([ph < 0.6, (ph + 0.5) % 1 < 0.6, (ph + 0.5) % 1 < 0.6, ph < 0.6], 1).astype(_f)
        if k >= 5:
            c[idx % 3 == 1] = 0
        one = np.zeros((n, 4), _f); one[idx, (idx + k // 20) % 4] = 1
        c[idx % 3 == 2] = one[idx % 3 == 2]
        x[k, :, 13:17] = c
        x[k, :, 41:45] = c
        x[k, :, 45:54] = gmat
        x[k, :, 17:29] = qa + s * (qb - qa)
        x[k, :, 29:41] = qd_amp * np.cos(20 * t + phase0)[:, None]
        stamp[k] = ((t0 + np.uint64(k * dt_ms) + (rng.uniform(0, 1, n) < 0.05).astype(np.uint64)) % np.uint64(2 ** 32)).astype(np.uint32)
    return x, stamp


STREAM_CASES = ((1, 60), (8, 90), (120, 150))            # (window W, ticks)
STREAM_N = 65


# ----------------------------------------------------------------------------- comparisons shared by the CPU and the -m gpu tests
def note(worst, key, v):
    worst[key] = max(worst.get(key, 0.0), float(v))


def ik_swing_in(cfg, q, current=None):
    """swing_in [n, 58] that makes the swing-target stage solve the IK of FK(q) for every leg: all four legs flagged, phase 0, lift-off point =
    foothold = the foot position, so the trajectory point is that position itself; the current motor angles are `current`."""
    geom, ho = cfg[:3], cfg[7:19]
    n = q.shape[0]
    p = foot_positions(geom, ho, q).reshape(n, 12).astype(np.float32)
    x = np.zeros((n, 58), np.float32)
    x[:, 0:4] = 1; x[:, 8:12] = 0.2
    x[:, 12:24] = p; x[:, 24:36] = p
    x[:, 39] = 1.0
    x[:, 46:58] = np.tile(STAND, 4) if current is None else current
    return x


def unreachable_swing_in(cfg):
    """Two rows: leg 1's target 0.58 m from its hip (beyond the leg's reach: all three angles NaN) and 0.05 m from its abad axis (inside the
    hip_l cylinder: abad and hip NaN, knee finite).  The current angles are distinct numbers, so a fall-back is recognisable."""
    ho = widen(cfg[7:19]).reshape(4, 3)
    cur = (0.01 * np.arange(1, 13)).astype(np.float32)
    x = ik_swing_in(cfg, np.tile(STAND, (2, 4)), current=cur)
    x[0, 15:18] = x[0, 27:30] = (ho[1] + np.array([0.5, 0.0, -0.3])).astype(np.float32)
    x[1, 15:18] = x[1, 27:30] = (ho[1] + np.array([0.15, 0.03, -0.04])).astype(np.float32)
    return x, cur


def check_ik(cfg, x, ang, worst=None, key=""):
    """|FK64(angles) - p| <= 5e-6 m for the targets p in rows 12-23 of swing_in x.

    Why 5e-6 holds on the IK domain: the float32 evaluation makes relative errors of a few 6e-8 in d^2 = |p - hip|^2 <= 0.19 and in the
    products that follow.  The knee comes from acos of a cosine: d t2 = d(cos) / sin|t2|, amplified by 1/sin|t2| <= 3.4 on -2.6..-0.3; the foot
    moves by at most lu ll sin|t2| / l per unit of t2, which cancels that factor again.  The hip comes from asin(-x / l):
    d t1 = d(x / l) / cos(t1 + t2/2), amplified by 1/cos <= 5.9 on |t1 + t2/2| <= 1.4, and the foot moves by l <= 0.4 per unit of t1.  With
    |x / l| <= 1 and an error of 3 roundings (1.8e-7) in it: 0.4 * 5.9 * 1.8e-7 = 4e-7 m, the same again from acos / asin / atan2 themselves:
    below 1e-6 m, inside the 5e-6 bar by a factor of five."""
    geom, ho = cfg[:3], cfg[7:19]
    fk = foot_positions(geom, ho, np.asarray(ang, np.float32)).reshape(-1, 12)
    e = np.abs(fk - x[:, 12:24].astype(np.float64)).max()
    if worst is not None:
        note(worst, key, e)
    assert e <= 5e-6, e


def check_stream(o, m, tag, worst=None):
    """est_out rows of one tick, o (float32, the code under test) against m (float64, stage_ref): [n, 42] each, at the issue's bars."""
    def rec(key, v):
        if worst is not None:
            note(worst, tag + " " + key, v)
    o = np.asarray(o, np.float64)
    e = np.abs(o[:, 12:24] - m[:, 12:24]).max(); rec("foot position", e); assert e <= 2e-6, (tag, e)
    sc = np.maximum(1.0, np.abs(m[:, 24:36]).max(axis=1))
    e = (np.abs(o[:, 24:36] - m[:, 24:36]).max(axis=1) / sc).max(); rec("J qd (relative)", e); assert e <= 2e-5, (tag, e)
    e = np.abs(o[:, 0:3] - m[:, 0:3]).max(); rec("filtered acceleration", e); assert e <= 2e-6, (tag, e)
    e = np.abs(o[:, 3:12] - m[:, 3:12]).max(); rec("velocities, omega", e); assert e <= 1e-5, (tag, e)
    assert np.array_equal(np.isnan(o[:, 36:42]), np.isnan(m[:, 36:42])), tag
    e = np.nanmax(np.abs(o[:, 36:42] - m[:, 36:42])); rec("pose rows", e); assert e <= 2e-5, (tag, e)
