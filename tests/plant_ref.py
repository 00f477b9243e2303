"""TEST INFRASTRUCTURE -- the plant (qrgpu_forward_dynamics_batch, qrgpu_plant_step_batch) restated in float64 numpy on the first-principles
model of rigid_body_ref.py, batched over robots.

It shares no formulation with qr_plant_kernel.hip: forward dynamics here is np.linalg.solve(H, rhs) on the 18 x 18 mass matrix summed over 25
bodies in world coordinates; the kernel runs an articulated-body recursion in link coordinates.  The motor law, the contact law and the
integrator are the ones include/qrgpu.h states for qrgpu_plant_step_batch.

  state37 = quat_wxyz, pos, omega_body, v_body, q[12], qd[12];  nu = [omega_body, v_body, qd];  arrays here are robot-major [n, rows]
"""
import numpy as np

import rigid_body_ref as M

_f = np.float32
PLANT_OUT_ROWS = 58
DEFAULTS = dict(dt=0.002, substeps=2, contact_k=2e4, contact_a=1.0, mu=0.6, v_eps=0.01, ground_z=0.0, tau_max=33.5, contact_threshold=5.0,
                com_offset=(-0.008, 0.005, 0.0))


def params(**kw):
    """The plant's parameters as the device holds them: float32 values widened (substeps an int)."""
    p = dict(DEFAULTS); p.update(kw)
    out = {k: float(np.float64(_f(v))) for k, v in p.items() if k not in ("substeps", "com_offset")}
    out["substeps"] = int(p["substeps"])
    out["com_offset"] = np.asarray(p["com_offset"], _f).astype(np.float64)
    return out


def forward_dynamics(model, state, tau, foot_force=None, rb=None):
    """nu_dot [n, 18] = solve(H, [0; tau] + sum_leg Jc' f - C - G) at state [n, 37] (quaternion normalised by the model); foot_force [n, 12]
    in the world frame, 3 * leg + axis.  rb: rigid_body_ref.compute(model, state) when the caller has it."""
    rb = M.compute(model, state) if rb is None else rb
    rhs = -rb["C"] - rb["G"]
    rhs[:, 6:] += tau
    if foot_force is not None:
        rhs += np.einsum("nlak,nla->nk", rb["Jc"], np.asarray(foot_force, np.float64).reshape(-1, 4, 3))
    return np.linalg.solve(rb["H"], rhs[..., None])[..., 0]


def contact_force(p, foot_pos, foot_vel):
    """The contact law: -> force [..., 3] (world), f_n [...]."""
    depth = p["ground_z"] - foot_pos[..., 2]
    fn = np.where(depth > 0, np.maximum(0.0, p["contact_k"] * depth * (1.0 - p["contact_a"] * foot_vel[..., 2])), 0.0)
    s = -p["mu"] * fn / np.sqrt(foot_vel[..., 0] ** 2 + foot_vel[..., 1] ** 2 + p["v_eps"] ** 2)
    return np.stack([s * foot_vel[..., 0], s * foot_vel[..., 1], fn], -1), fn


def motor_torque(p, cmd, q, qd):
    """The joint controller's law on cmd [n, 60] = p, Kp, d, Kd, tua."""
    c = np.asarray(cmd, np.float64)
    return np.clip(c[:, 12:24] * (c[:, 0:12] - q) + c[:, 36:48] * (c[:, 24:36] - qd) + c[:, 48:60], -p["tau_max"], p["tau_max"])


def quat_mul(a, b):
    w1, v1, w2, v2 = a[..., 0:1], a[..., 1:], b[..., 0:1], b[..., 1:]
    return np.concatenate([w1 * w2 - np.sum(v1 * v2, -1, keepdims=True), w1 * v2 + w2 * v1 + np.cross(v1, v2)], -1)


def quat_exp(w):
    """The unit quaternion of the rotation vector w."""
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    safe = np.where(th < 1e-8, 1.0, th)
    sc = np.where(th < 1e-8, 0.5, np.sin(0.5 * safe) / safe)
    return np.concatenate([np.cos(0.5 * th), sc * w], -1)


def quat_to_rpy(q):
    """quatToRPY of the reference (asin's argument capped at .99999)."""
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    a = np.minimum(-2.0 * (q1 * q3 - q0 * q2), 0.99999)
    return np.stack([np.arctan2(2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3), np.arcsin(a),
                     np.arctan2(2 * (q1 * q2 + q0 * q3), q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3)], -1)


def substep(model, p, s, cmd, h):
    """One sub-step of length h on the float64 state s [n, 37] (unit quaternion).  -> new state, dict of the sub-step's force [n,4,3], fn [n,4],
    tau [n,12], nu_dot [n,18], acc [n,3] (specific force at the base origin, base frame)."""
    rb = M.compute(model, s)
    f, fn = contact_force(p, rb["pGC"], rb["vGC"])
    tau = motor_torque(p, cmd, s[:, 13:25], s[:, 25:37])
    nud = forward_dynamics(model, s, tau, f.reshape(-1, 12), rb=rb)
    R = M.quat_to_rot(s[:, 0:4])
    acc = nud[:, 3:6] + np.cross(s[:, 7:10], s[:, 10:13]) + np.einsum("nji,j->ni", R, np.array([0.0, 0.0, 9.81]))
    o = s.copy()
    o[:, 7:13] += h * nud[:, 0:6]
    o[:, 25:37] += h * nud[:, 6:18]
    o[:, 13:25] += h * o[:, 25:37]
    o[:, 4:7] += h * np.einsum("nij,nj->ni", R, o[:, 10:13])
    qn = quat_mul(s[:, 0:4], quat_exp(h * o[:, 7:10]))
    o[:, 0:4] = qn / np.linalg.norm(qn, axis=-1, keepdims=True)
    return o, dict(force=f, fn=fn, tau=tau, nu_dot=nud, acc=acc)


def step(model, p, state32, cmd32, state64=None):
    """One control tick.  state32 [n, 37], cmd32 [n, 60]: the float32 rows a device is given (state64: a float64 state to go on from instead,
    for a chain of ticks that keeps its state in float64).  -> dict fb_state [n,37], plant_out [n,58], mpc_state [n,28], est_in [n,41], fn [n,4],
    all float64 and unrounded."""
    s = M.normalised(state32) if state64 is None else state64
    h = p["dt"] / p["substeps"]
    for _ in range(p["substeps"]):
        s, aux = substep(model, p, s, cmd32, h)
    n = len(s)
    rb = M.compute(model, s)
    out = np.zeros((n, PLANT_OUT_ROWS))
    out[:, 0:12] = aux["force"].reshape(n, 12); out[:, 12:24] = rb["pGC"].reshape(n, 12)
    out[:, 24:28] = aux["fn"] > p["contact_threshold"]; out[:, 28:40] = aux["tau"]; out[:, 40:58] = aux["nu_dot"]
    mpc = truth_mpc_state(model, p, s)
    est = np.zeros((n, 41))
    est[:, 0:3] = aux["acc"]; est[:, 3:6] = aux["acc"]; est[:, 6:10] = s[:, 0:4]; est[:, 10:13] = s[:, 7:10]
    est[:, 13:17] = out[:, 24:28]; est[:, 17:29] = s[:, 13:25]; est[:, 29:41] = s[:, 25:37]
    return dict(fb_state=s, plant_out=out, mpc_state=mpc, est_in=est, fn=aux["fn"])


def truth_mpc_state(model, p, s):
    """mpc_state [n, 28] of the float64 state s: qrgpu_pack_state_batch's conventions on the ground truth."""
    rb = M.compute(model, s)
    R = M.quat_to_rot(s[:, 0:4])
    n = len(s)
    mpc = np.zeros((n, 28))
    mpc[:, 0:3] = s[:, 4:7]; mpc[:, 3:6] = np.einsum("nij,nj->ni", R, s[:, 10:13]); mpc[:, 6:10] = s[:, 0:4]
    mpc[:, 10:13] = np.einsum("nij,nj->ni", R, s[:, 7:10])
    mpc[:, 13:25] = (rb["pGC"] - s[:, None, 4:7] - np.einsum("nij,j->ni", R, p["com_offset"])[:, None, :]).reshape(n, 12)
    mpc[:, 25:28] = quat_to_rpy(s[:, 0:4].astype(_f).astype(np.float64))
    return mpc


def energy(model, s):
    """T + V of state s [n, 37]."""
    rb = M.compute(model, s)
    return rb["T"] + rb["V"]


def stand_cmd(n, kp=100.0, kd=2.0, pose=None):
    """Joint PD to the stand pose: motor command rows [n, 60] float32."""
    c = np.zeros((n, 60), _f)
    c[:, 0:12] = M.STAND_POSE if pose is None else pose
    c[:, 12:24] = kp; c[:, 36:48] = kd
    return c


def stand_state(n, z=0.30):
    """At rest at the stand pose, level, base height z: float32 [n, 37]."""
    s = np.zeros((n, 37), _f)
    s[:, 0] = 1.0; s[:, 6] = z; s[:, 13:25] = M.STAND_POSE
    return s


# ---- shared cases (seeded; the CPU file checks what the GPU file relies on)
ROBOTS = ("a1", "lite3")
STEP_N, STEP_SEED, STEP_SUBSTEPS = 48, 9102, (1, 2, 8)


def step_cases(seed=STEP_SEED, n=STEP_N):
    """n robots near the ground, A1 at even places and Lite3 at odd ones: base z in 0.20..0.33 (some feet penetrate, some hover), v_body in
    +-1 m/s horizontally (feet slide), random gains and torques, a quarter of the robots with gains that saturate tau_max.
    -> state [n, 37], cmd [n, 60] float32, type_id [n] int32."""
    rng = np.random.default_rng(seed)
    U = rng.uniform
    s = np.zeros((n, 37))
    rpy = np.stack([U(-0.15, 0.15, n), U(-0.15, 0.15, n), U(-np.pi, np.pi, n)], 1)
    hr, hp, hy = rpy[:, 0] / 2, rpy[:, 1] / 2, rpy[:, 2] / 2
    cr, sr, cp, sp, cy, sy = np.cos(hr), np.sin(hr), np.cos(hp), np.sin(hp), np.cos(hy), np.sin(hy)
    s[:, 0:4] = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
    s[:, 4:6] = U(-1, 1, (n, 2)); s[:, 6] = U(0.20, 0.33, n)
    s[:, 7:10] = U(-1, 1, (n, 3)); s[:, 10:12] = U(-1, 1, (n, 2)); s[:, 12] = U(-0.3, 0.3, n)
    s[:, 13:25] = M.STAND_POSE + U(-0.2, 0.2, (n, 12)); s[:, 25:37] = U(-2, 2, (n, 12))
    c = np.zeros((n, 60))
    c[:, 0:12] = M.STAND_POSE + U(-0.3, 0.3, (n, 12)); c[:, 12:24] = U(0, 150, (n, 12)); c[:, 24:36] = U(-1, 1, (n, 12))
    c[:, 36:48] = U(0, 4, (n, 12)); c[:, 48:60] = U(-15, 15, (n, 12))
    c[0::4, 12:24] = 600.0                                             # 0.3 rad off the command at Kp 600: beyond tau_max
    return s.astype(_f), c.astype(_f), (np.arange(n) % 2).astype(np.int32)


def step_mixed(models, type_id, p, state32, cmd32):
    """step() on a batch of several robot types: models[t] is the model of type t."""
    out = None
    for t, model in enumerate(models):
        k = np.nonzero(type_id == t)[0]
        r = step(model, p, state32[k], cmd32[k])
        if out is None:
            out = {key: np.zeros((len(type_id),) + v.shape[1:]) for key, v in r.items()}
        for key, v in r.items():
            out[key][k] = v
    return out


def near_threshold(p, fn, rel=1e-6):
    """Feet whose normal force is within `rel` (relative) of the contact threshold: their flag may differ between two correct evaluations."""
    return np.abs(fn - p["contact_threshold"]) <= rel * p["contact_threshold"]


HORIZON = 10
SHOVE_MAX = 0.3
BAND = dict(z=0.01, xy=0.03, tilt=0.03, height=0.27)


def stand_tick_inputs(n, horizon=HORIZON):
    """The tick's constant inputs of the closed-loop tests: all-stance gait, a trajectory that holds the origin at height 0.27, a WBC command
    for the same with four contacts.  -> traj [n, 12 h], gait [n, 4 h], wbc_cmd [n, 67], prev_ori [n, 3] float32."""
    traj = np.zeros((n, horizon, 12), _f); traj[:, :, 5] = BAND["height"]
    cmd = np.zeros((n, 67), _f); cmd[:, 2] = BAND["height"]; cmd[:, 63:67] = 1
    return traj.reshape(n, -1), np.ones((n, 4 * horizon), _f), cmd, np.zeros((n, 3), _f)


def in_band(pos, rpy):
    """The stand band of the closed-loop tests: |z - 0.27| <= 0.01, |x|, |y| <= 0.03, |roll|, |pitch| <= 0.03.  -> bool [n]"""
    return ((np.abs(pos[:, 2] - BAND["height"]) <= BAND["z"]) & (np.abs(pos[:, 0:2]).max(1) <= BAND["xy"]) & (np.abs(rpy[:, 0:2]).max(1) <= BAND["tilt"]))
