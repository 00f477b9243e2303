"""The sensor stage (qrgpu_observe_batch, include/qrgpu.h) restated in numpy from the reference's text, independent of csrc/qr_observe.h:

  qrRobotA1Sim::ReceiveObservation   quadruped/src/robots/qr_robot_a1_sim.cpp:606-670
  qrRobotA1::ReceiveObservation      quadruped/src/robots/qr_robot_a1.cpp:140-193
  the filters and their Reset        quadruped/src/robots/qr_robot.cpp:30-37, :55-58
  qrMovingWindowFilter<T, N>         quadruped/include/quadruped/estimators/qr_moving_window_filter.hpp:139-189
  quatToRPY, rpyToQuat               quadruped/include/quadruped/utils/qr_se3.h:71-116, 145-178, 209-235
  FootPositionsInBaseFrame           quadruped/src/robots/qr_robot.cpp:127-146, 174-183

run(..., dtype=np.float32) is float32 where the reference is float32, with its double literals promoting where they do there; run(...,
dtype=np.float64) is the same arithmetic with every float a double: the distance between the two is the yardstick of the rows that lie behind a
transcendental function (gaps()).  The filter is a class over n robots at once, each robot with a deque of its own (oldest first, pop_front is a
shift); the ring the library keeps its samples in is bookkeeping beside it, carried only so that the state rows can be compared.  Philox is
episode_ref's."""
import functools

import numpy as np

import episode_ref as ER
import stage_ref as SR

f32, f64 = np.float32, np.float64
M_PI = 3.14159265358979323846
M_2PI = 6.28318530718                      # qr_ctypes.h:51, not 2 pi
COUNT, YAW, ACC, GYRO, RPY, QD, ROWS, ROWS_MV = 0, 1, 2, 25, 48, 71, 71, 337
NOISE_TAG = 0x0b5e7
HIP_OFFSET = (0.1805, -0.047, 0.0, 0.1805, 0.047, 0.0, -0.1805, -0.047, 0.0, -0.1805, 0.047, 0.0)


def desc(variant="sim", **over):
    """qrgpu_observe_desc as a dict: the library's defaults of the variant, with any field overridden"""
    hw = variant == "hardware"
    d = dict(filter_rpy=0 if hw else 1, filter_motor_velocity=1 if hw else 0, yaw_offset=0.0, hip_l=0.08505, upper_l=0.2, lower_l=0.2, hip_offset=HIP_OFFSET,
             base_height=0.27, tick_ms=2, seed=1, acc_noise=0.0, gyro_noise=0.0, q_noise=0.0, qd_noise=0.0)
    assert set(over) <= set(d), set(over) - set(d)
    d.update(over)
    d["variant"] = variant
    return d


def to_struct(pkg, d):
    return pkg.observe_desc(d["variant"], **{k: v for k, v in d.items() if k != "variant"})


class MovingWindowFilter:
    """qrMovingWindowFilter<T, D>(W) of n robots: sum, correction and a deque per robot (buf[r, :length[r]], oldest first)."""

    def __init__(self, n, D, W, dtype):
        self.n, self.D, self.W, self.dt = n, D, W, dtype
        self.sum = np.zeros((n, D), dtype); self.correction = np.zeros((n, D), dtype)
        self.buf = np.zeros((n, W, D), dtype); self.length = np.zeros(n, np.int64)
        self.ring = np.zeros((n, W, D), dtype); self.head = np.zeros(n, np.int64)           # bookkeeping: where the library keeps the samples
        self.taken = np.zeros(2, np.int64)                                                  # how often each branch of NeumaierSum was taken

    def Reset(self, who):
        self.sum[who] = 0; self.correction[who] = 0; self.length[who] = 0
        self.head[who] = 0

    def construct(self, who):
        """a fresh filter; the library's column is zero"""
        self.Reset(who); self.ring[who] = 0

    def NeumaierSum(self, value, who):
        newSum = self.sum + value
        bigger = np.abs(self.sum) >= np.abs(value)
        c = np.where(bigger, (self.sum - newSum) + value, (value - newSum) + self.sum)
        self.taken += [int((bigger & who[:, None]).sum()), int((~bigger & who[:, None]).sum())]
        self.correction = np.where(who[:, None], self.correction + c, self.correction)
        self.sum = np.where(who[:, None], newSum, self.sum)

    def CalculateAverage(self, newValue):
        newValue = np.asarray(newValue, self.dt)
        r = np.arange(self.n)
        full = self.length >= self.W
        self.NeumaierSum(-self.buf[:, 0], full)
        self.buf[full, :-1] = self.buf[full, 1:]                                           # pop_front
        self.length[full] -= 1
        self.NeumaierSum(newValue, np.ones(self.n, bool))
        self.buf[r, self.length] = newValue                                                 # push_back
        out = (self.sum + self.correction) / (self.length + 1).astype(self.dt)[:, None]
        self.length += 1
        self.ring[r, self.head] = newValue; self.head = (self.head + 1) % self.W
        return out

    def rows(self):
        """[n, 2 D + 2 + W D]: the library's rows of this filter"""
        return np.concatenate([self.sum, self.correction, self.length[:, None].astype(self.dt), self.head[:, None].astype(self.dt),
                               self.ring.reshape(self.n, -1)], axis=1)


def fold(y, dt):
    """if (y >= M_PI) y -= M_2PI; else if (y <= -M_PI) y += M_2PI;  -- a float against double constants"""
    y64 = y.astype(f64)
    return np.where(y64 >= M_PI, (y64 - M_2PI).astype(dt), np.where(y64 <= -M_PI, (y64 + M_2PI).astype(dt), y))


def quat_to_rpy(q, dt):
    q0, q1, q2, q3 = (q[:, k] for k in range(4))
    as_ = np.minimum(-2. * (q1 * q3 - q0 * q2).astype(f64), .99999).astype(dt)
    yaw = np.arctan2(2 * (q1 * q2 + q0 * q3), q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3)
    pitch = np.arcsin(as_)
    roll = np.arctan2(2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3)
    return np.stack([roll, pitch, yaw], axis=1).astype(dt)


def _mul3(A, B):
    """[n, 3, 3] products, an entry is (a0 b0 + a1 b1) + a2 b2"""
    return (A[:, :, 0, None] * B[:, None, 0, :] + A[:, :, 1, None] * B[:, None, 1, :]) + A[:, :, 2, None] * B[:, None, 2, :]


def rpy_to_rotmat(rpy, dt):
    n = len(rpy)
    one, zero = np.ones(n, dt), np.zeros(n, dt)
    s, c = np.sin(rpy).astype(dt), np.cos(rpy).astype(dt)
    m = lambda rows: np.stack([np.stack(r, axis=1) for r in rows], axis=1)
    X = m([[one, zero, zero], [zero, c[:, 0], s[:, 0]], [zero, -s[:, 0], c[:, 0]]])
    Y = m([[c[:, 1], zero, -s[:, 1]], [zero, one, zero], [s[:, 1], zero, c[:, 1]]])
    Z = m([[c[:, 2], s[:, 2], zero], [-s[:, 2], c[:, 2], zero], [zero, zero, one]])
    return _mul3(_mul3(X, Y), Z)


def rotmat_to_quat(R1, dt):
    """rotationMatrixToQuaternion: Scalar arithmetic, the literals 0.0, 1.0, 2.0 and 0.25 doubles"""
    r = np.swapaxes(R1, 1, 2)
    d = lambda x: x.astype(f64)
    tr = (r[:, 0, 0] + r[:, 1, 1]) + r[:, 2, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        S0 = (np.sqrt(d(tr) + 1.0) * 2.0).astype(dt)
        S1 = (np.sqrt(1.0 + d(r[:, 0, 0]) - d(r[:, 1, 1]) - d(r[:, 2, 2])) * 2.0).astype(dt)
        S2 = (np.sqrt(1.0 + d(r[:, 1, 1]) - d(r[:, 0, 0]) - d(r[:, 2, 2])) * 2.0).astype(dt)
        S3 = (np.sqrt(1.0 + d(r[:, 2, 2]) - d(r[:, 0, 0]) - d(r[:, 1, 1])) * 2.0).astype(dt)
        q = lambda S: (0.25 * d(S)).astype(dt)
        b0 = np.stack([q(S0), (r[:, 2, 1] - r[:, 1, 2]) / S0, (r[:, 0, 2] - r[:, 2, 0]) / S0, (r[:, 1, 0] - r[:, 0, 1]) / S0], axis=1)
        b1 = np.stack([(r[:, 2, 1] - r[:, 1, 2]) / S1, q(S1), (r[:, 0, 1] + r[:, 1, 0]) / S1, (r[:, 0, 2] + r[:, 2, 0]) / S1], axis=1)
        b2 = np.stack([(r[:, 0, 2] - r[:, 2, 0]) / S2, (r[:, 0, 1] + r[:, 1, 0]) / S2, q(S2), (r[:, 1, 2] + r[:, 2, 1]) / S2], axis=1)
        b3 = np.stack([(r[:, 1, 0] - r[:, 0, 1]) / S3, (r[:, 0, 2] + r[:, 2, 0]) / S3, (r[:, 1, 2] + r[:, 2, 1]) / S3, q(S3)], axis=1)
    k = np.where(d(tr) > 0.0, 0, np.where((r[:, 0, 0] > r[:, 1, 1]) & (r[:, 0, 0] > r[:, 2, 2]), 1, np.where(r[:, 1, 1] > r[:, 2, 2], 2, 3)))
    return np.choose(k[:, None], [b0, b1, b2, b3]).astype(dt), k


def foot_positions(d, q, dt):
    """[n, 12] FootPositionsInBaseFrame of q [n, 12]"""
    out = np.zeros((len(q), 12), dt)
    lu, ll = dt(d["upper_l"]), dt(d["lower_l"])
    ho = np.asarray(d["hip_offset"], dt)
    for leg in range(4):
        t0, t1, t2 = q[:, 3 * leg], q[:, 3 * leg + 1], q[:, 3 * leg + 2]
        sh = dt(d["hip_l"]) * dt(1 if leg & 1 else -1)
        legDist = np.sqrt(lu * lu + ll * ll + 2 * lu * ll * np.cos(t2))
        eff = t1 + t2 / 2
        offX, offZ, offY = -legDist * np.sin(eff), -legDist * np.cos(eff), sh
        out[:, 3 * leg] = offX + ho[3 * leg]
        out[:, 3 * leg + 1] = np.cos(t0) * offY - np.sin(t0) * offZ + ho[3 * leg + 1]
        out[:, 3 * leg + 2] = np.sin(t0) * offY + np.cos(t0) * offZ + ho[3 * leg + 2]
    return out


@functools.lru_cache(maxsize=None)
def noise_words(seed, robot, step):
    """[8, 4] uint32: blocks 0-7 of robot `robot` at loop count `step`"""
    return np.array([ER.philox((step, k, NOISE_TAG, 0), (seed, robot)) for k in range(8)], np.uint32)


def symmetric(w):
    """s = 2 u - 1, u = (w >> 8) 2^-24: exact in float32"""
    return 2.0 * ER.uniform(w) - 1.0


def noise_of(d, n, step, robots=None):
    """[n, 8, 4] float64 s of every robot at `step` (robot indices: robots, default 0..n-1)"""
    idx = range(n) if robots is None else robots
    return symmetric(np.stack([noise_words(int(d["seed"]), int(r), int(step)) for r in idx]))


def add_noise(x, amplitude, s, dt):
    """row += amplitude * s: one product, one sum, in dt; amplitude 0 leaves the row alone"""
    if amplitude == 0:
        return x
    return x + dt(f32(amplitude)) * s.astype(dt)


class Observer:
    """The stage of n robots, tick by tick: d a desc(); robots: the robots' indices in their batch (the noise's key), default 0..n-1."""

    def __init__(self, n, d, dtype=f32, robots=None):
        self.n, self.d, self.dt, self.robots = n, d, dtype, robots
        self.mv = bool(d["filter_motor_velocity"])
        self.acc_f, self.gyro_f, self.rpy_f = (MovingWindowFilter(n, 3, 5, dtype) for _ in range(3))
        self.v_f = MovingWindowFilter(n, 12, 20, dtype)
        self.yaw_prev = np.zeros(n, dtype); self.count = np.zeros(n, np.uint32)
        self.rows = ROWS_MV if self.mv else ROWS

    def tick(self, x_raw, rs, step, prev=None):
        """x_raw [n, 41]; rs [n] bool: the robots reset at this call; step: the loop count; prev [n, 3]: rows 36-38 of the previous est_out or None.
        -> dict of est [n, 41], rpy [n, 3], gin [n, 23], tick [n] uint32, state [n, rows] with count [n] uint32 beside it (row 0 of state is left 0),
        and what the claims need: the yaw before each fold, the jump metric, which branches were taken"""
        d, dt, n = self.d, self.dt, self.n
        rs = np.asarray(rs, bool)
        for f in (self.acc_f, self.gyro_f, self.rpy_f, self.v_f):
            f.construct(rs)
        self.yaw_prev[rs] = 0; self.count[rs] = 0
        x = np.asarray(x_raw).astype(dt)
        acc, quat, gyro, ct, q, qd = x[:, 0:3], x[:, 6:10], x[:, 10:13], x[:, 13:17], x[:, 17:29], x[:, 29:41]
        if any(d[k] != 0 for k in ("acc_noise", "gyro_noise", "q_noise", "qd_noise")):
            s = noise_of(d, n, step, self.robots)
            acc = add_noise(acc, d["acc_noise"], s[:, 0, 0:3], dt); gyro = add_noise(gyro, d["gyro_noise"], s[:, 1, 0:3], dt)
            q = add_noise(q, d["q_noise"], s[:, 2:5].reshape(n, 12), dt); qd = add_noise(qd, d["qd_noise"], s[:, 5:8].reshape(n, 12), dt)
        o = {}
        facc = self.acc_f.CalculateAverage(acc)
        rpy = quat_to_rpy(quat, dt)                                                         # state.imu.rpy
        cy_pre = rpy[:, 2] - dt(f32(d["yaw_offset"]))
        cy = fold(cy_pre, dt)
        o["cy_pre"] = cy_pre.astype(f64); o["fold1"] = np.sign(cy_pre.astype(f64) - cy.astype(f64)).astype(np.int8)
        o["jump"] = np.zeros(n); o["cleared"] = np.zeros(n, bool); o["avg_pre"] = np.zeros(n); o["fold2"] = np.zeros(n, np.int8)
        if d["filter_rpy"]:
            jump = np.abs(self.yaw_prev - cy)                                               # std::abs(float)
            clear = jump.astype(f64) >= M_PI
            self.rpy_f.Reset(clear)
            brpy = self.rpy_f.CalculateAverage(np.stack([rpy[:, 0], rpy[:, 1], cy], axis=1))
            o["jump"] = jump.astype(f64); o["cleared"] = clear; o["avg_pre"] = brpy[:, 2].astype(f64)
            folded = fold(brpy[:, 2], dt)
            o["fold2"] = np.sign(brpy[:, 2].astype(f64) - folded.astype(f64)).astype(np.int8)
            brpy = np.stack([brpy[:, 0], brpy[:, 1], folded], axis=1)
        else:
            brpy = np.stack([rpy[:, 0], rpy[:, 1], cy], axis=1)
        self.yaw_prev = brpy[:, 2].copy()
        fgyro = self.gyro_f.CalculateAverage(gyro)
        bq, o["quat_branch"] = rotmat_to_quat(rpy_to_rotmat(brpy, dt), dt)                  # baseOrientation = rpyToQuat(baseRollPitchYaw)
        fqd = self.v_f.CalculateAverage(qd) if self.mv else qd
        self.count = self.count + np.uint32(1)
        e = np.zeros((n, 41), dt)
        e[:, 0:3] = acc; e[:, 3:6] = facc; e[:, 6:10] = bq; e[:, 10:13] = fgyro; e[:, 13:17] = ct; e[:, 17:29] = q; e[:, 29:41] = fqd
        g = np.zeros((n, 23), dt)
        g[:, 0:4] = ct; g[:, 4:16] = foot_positions(d, q, dt); g[:, 19:23] = bq
        bp = np.tile(np.array([0, 0, f32(d["base_height"])], dt), (n, 1))                   # qrRobot::Reset
        if prev is not None:
            bp = np.where(rs[:, None], bp, np.asarray(prev).astype(dt))
        g[:, 16:19] = bp
        st = np.zeros((n, self.rows), dt)
        st[:, YAW] = self.yaw_prev
        st[:, ACC:GYRO] = self.acc_f.rows(); st[:, GYRO:RPY] = self.gyro_f.rows(); st[:, RPY:QD] = self.rpy_f.rows()
        if self.mv:
            st[:, QD:] = self.v_f.rows()
        o.update(est=e, rpy=brpy, gin=g, tick=self.count * np.uint32(d["tick_ms"]), state=st, count=self.count.copy())
        return o


def run(raw, d, dtype=f32, resets=None, steps=None, prev=None, robots=None):
    """raw [T, n, 41] float32 (rows 0-40 as the plant writes them); resets [T, n] bool (the first tick resets every robot); steps [T] loop counts
    (default 0..T-1); prev [T, n, 3] or None.  -> Observer.tick's dict with a leading tick axis, and how often each branch of NeumaierSum was taken"""
    T, n = raw.shape[:2]
    ob = Observer(n, d, dtype, robots)
    resets = np.zeros((T, n), bool) if resets is None else np.asarray(resets, bool).copy()
    resets[0] = True
    steps = np.arange(T) if steps is None else steps
    ticks = [ob.tick(raw[t], resets[t], steps[t], None if prev is None else prev[t]) for t in range(T)]
    o = {k: np.stack([x[k] for x in ticks]) for k in ticks[0]}
    o["neumaier_taken"] = dict(acc=ob.acc_f.taken, gyro=ob.gyro_f.taken, rpy=ob.rpy_f.taken, qd=ob.v_f.taken)
    return o


def state_bits(o, t):
    """[rows, n] float32: d_obs_state after tick t, the counter in row 0's bits"""
    s = np.ascontiguousarray(o["state"][t].T.astype(f32))
    s[COUNT] = o["count"][t].view(f32)
    return s


# ---- streams ------------------------------------------------------------------------------------------------------------------------------------
T_STREAM = 48
YAW_KINDS = ("up", "down", "across", "level")


def quat_of_rpy(roll, pitch, yaw):
    """the ZYX quaternion whose quatToRPY is (roll, pitch, yaw), float64"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=-1)


@functools.lru_cache(maxsize=None)
def streams(n, T=T_STREAM, seed=4136):
    """raw [T, n, 41] float32 and the yaw kind of each robot.  By construction: robot r's true yaw ramps up through +pi (r % 4 == 0), down through -pi
    (1), swings across +-pi several times in both directions (2) or stays level (3); the accelerometer and the gyro alternate in sign with magnitudes
    from 1e-4 to 1e3, so that a sum meets both a smaller and a larger sample; contacts toggle; joints and joint velocities are stage_ref.wide_joints
    (its edge rows at tick 0, robots 0-3)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    r = np.arange(n)[None, :]
    kind = r % 4
    ph = rng.uniform(0, 1, (1, n))
    yaw = np.where(kind == 0, 2.55 + 0.2 * ph + 0.047 * t, np.where(kind == 1, -2.55 - 0.2 * ph - 0.047 * t,
                   np.where(kind == 2, np.pi + 0.5 * np.sin(0.29 * t + 6.28 * ph) + 0.013, 0.8 * np.sin(0.05 * t + 6.28 * ph))))
    roll = 0.25 * np.sin(0.13 * t + 5 * ph); pitch = 0.2 * np.cos(0.11 * t + 3 * ph)
    raw = np.zeros((T, n, 41), f32)
    raw[:, :, 6:10] = quat_of_rpy(roll, pitch, yaw).astype(f32)
    sign = np.where((np.arange(T) % 2 == 0)[:, None, None], 1.0, -1.0)
    mag = 10.0 ** rng.integers(-4, 4, (T, n, 6)) * rng.uniform(1, 9.9, (T, n, 6))
    raw[:, :, 0:3] = (sign * mag[:, :, 0:3]).astype(f32); raw[:, :, 3:6] = raw[:, :, 0:3]
    raw[:, :, 10:13] = (-sign * mag[:, :, 3:6] * 0.01).astype(f32)
    raw[:, :, 13:17] = (rng.uniform(0, 1, (T, n, 4)) < 0.7).astype(f32)
    raw[:, 0, 13:17] = 1.0
    q, qd = SR.wide_joints(T * n, seed + 1)
    raw[:, :, 17:29] = q.reshape(T, n, 12); raw[:, :, 29:41] = qd.reshape(T, n, 12)
    return raw, np.array(YAW_KINDS)[kind[0]]


# The cases every comparison runs: both variants, and the sim class under yaw offsets beyond 2 pi, where one fold of the calibrated yaw leaves it
# outside (-pi, pi) and the fold of the averaged yaw fires (with an offset inside (-pi, pi) it cannot).
CASES = dict(sim=desc("sim", yaw_offset=0.35), sim_far_neg=desc("sim", yaw_offset=-7.1), sim_far_pos=desc("sim", yaw_offset=7.1),
             hardware=desc("hardware", yaw_offset=-0.35))
NOISE = dict(seed=20266, acc_noise=0.3, gyro_noise=0.05, q_noise=0.01, qd_noise=0.2)
N_REF = 130
GROUPS = dict(rpy=("rpy", slice(0, 3)), quat=("est", slice(6, 10)), foot=("gin", slice(4, 16)), rpy_state=("state", slice(RPY, QD)), yaw_state=("state", slice(YAW, YAW + 1)))
FLOOR = 2e-6                                # the project's standing bar for device sinf / cosf against libm (test_gpu_estimator.py)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=f32, noise=False):
    """run() of a case on the streams of N_REF robots, computed once"""
    d = dict(CASES[case], **NOISE) if noise else CASES[case]
    return run(streams(N_REF)[0], d, dtype)


@functools.lru_cache(maxsize=None)
def gaps(case):
    """group -> max |float32 run - float64 run| over the streams: the reference's own rounding, the yardstick of the barred rows"""
    a, b = reference(case, f32), reference(case, f64)
    return {g: float(np.abs(a[k][:, :, s].astype(f64) - b[k][:, :, s]).max()) for g, (k, s) in GROUPS.items()}


def bars(case):
    """group -> 8 x the gap, never tighter than FLOOR"""
    return {g: max(8.0 * v, FLOOR) for g, v in gaps(case).items()}


def split(rows):
    """the state rows compared exactly (reached by + - x / alone; the counter, row 0, apart: it is an integer in the row's bits) and those under a bar
    (the rpy filter's sums, corrections and samples, group rpy_state; the previous yaw, group yaw_state): -> (exact, rpy_state, yaw_state) row indices"""
    rpy_rows = list(range(RPY, RPY + 6)) + list(range(RPY + 8, QD))
    return [k for k in range(1, rows) if k != YAW and k not in rpy_rows], rpy_rows, [YAW]


def compare(got, want, case, rows, tag=""):
    """got, want: dicts of est [.., n, 41+], rpy [.., n, 3], gin [.., n, 23] or None, tick [.., n] or None, state [.., n, rows] (float32) and count
    [.., n] (uint32), robot index second to last.  Rows reached by + - x / alone are compared bit for bit, rows behind a transcendental function
    under bars(case).  -> the worst distance per barred group; raises on the first group that fails"""
    b = bars(case)
    bits = lambda a: np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)
    ex_rows, rpy_rows, yaw_rows = split(rows)
    exact = dict(acc=("est", slice(0, 6)), gyro=("est", slice(10, 13)), contacts=("est", slice(13, 17)), q_qd=("est", slice(17, 41)),
                 ground_contacts=("gin", slice(0, 4)), base_position=("gin", slice(16, 19)), state=("state", ex_rows))
    for name, (k, s) in exact.items():
        if got.get(k) is None:
            continue
        if not np.array_equal(bits(got[k][..., s]), bits(want[k][..., s])):
            bad = np.argwhere(bits(got[k][..., s]) != bits(want[k][..., s]))
            raise AssertionError((tag, case, name, "first differences (.., robot, row)", bad[:4].tolist()))
    if got.get("tick") is not None:
        assert np.array_equal(got["tick"], want["tick"]), (tag, case, "tick")
    assert np.array_equal(got["count"], want["count"]), (tag, case, "count")
    worst = {}
    barred = dict(rpy=("rpy", slice(0, 3), "rpy"), quat=("est", slice(6, 10), "quat"), ground_quat=("gin", slice(19, 23), "quat"), foot=("gin", slice(4, 16), "foot"),
                  rpy_state=("state", rpy_rows, "rpy_state"), yaw_state=("state", yaw_rows, "yaw_state"))
    for name, (k, s, group) in barred.items():
        if got.get(k) is None:
            continue
        e = float(np.abs(np.asarray(got[k][..., s], f64) - np.asarray(want[k][..., s], f64)).max())
        worst[name] = e
        assert e <= b[group], (tag, case, name, e, b[group])
    return worst
