"""TEST INFRASTRUCTURE -- the plant with a body (qrgpu_plant_step_body_batch) restated in float64 numpy from the comment of include/qrgpu.h: sixteen
contact points a robot (four feet, four knees, eight trunk corners) under terrain_ref's sampler and law, the joints' stops, the push.  Forward
dynamics is plant_ref's np.linalg.solve(H, rhs) on the first-principles model; the knees' and corners' positions, velocities and Jacobians come
from rigid_body_ref.bodies / velocities by linearity.  Nothing is shared with the kernel's recursion.

  body = dict(trunk_half[3], trunk_center[3], q_lo[3], q_hi[3], limit_k, limit_a) with the float32 values widened (body_of)
  points are ordered feet 0-3, knees 4-7, corners 8-15 at 8 + 2 * leg + top;  arrays are robot-major [n, rows].
"""
import numpy as np

import plant_ref as PR
import rigid_body_ref as M
import terrain_ref as TR

_f = np.float32
BODY_OUT_ROWS = 36
N_POINTS = 16
PL_TRUNK_CONTACT, PL_KNEE_CONTACT, PL_JOINT_LIMIT = 0x10, 0x20, 0x40
FEET, KNEES, CORNERS = slice(0, 4), slice(4, 8), slice(8, 16)
TOP = np.arange(16) % 2 == 1
TOP[:8] = False


def body_of(desc):
    """A qrgpu_plant_body_desc (ctypes) as the dict of this module: float32 values widened."""
    w = lambda v: np.asarray(list(v), _f).astype(np.float64)
    return dict(trunk_half=w(desc.trunk_half), trunk_center=w(desc.trunk_center), q_lo=w(desc.q_lo), q_hi=w(desc.q_hi),
                limit_k=float(np.float64(_f(desc.limit_k))), limit_a=float(np.float64(_f(desc.limit_a))))


def corners_in_base(body):
    """The eight trunk corners in the base frame, [8, 3] at 2 * leg + top: trunk_center + (sx hx, sy hy, -+hz)."""
    hx, hy, hz = body["trunk_half"]
    return np.array([body["trunk_center"] + np.array([sx * hx, sy * hy, sz * hz]) for sx, sy in M.LEG_SIGNS for sz in (-1.0, 1.0)])


def points(model, body, s):
    """The sixteen points of the states s [n, 37] (unit quaternion): -> position [n, 16, 3], velocity [n, 16, 3] (world), J [n, 16, 3, 18] (world-frame
    linear velocity over nu)."""
    n = len(s)
    nu = np.concatenate([s[:, 7:13], s[:, 25:37]], 1)
    bs, feet = M.bodies(model, s[:, 0:4], s[:, 4:7], s[:, 13:25])
    w, v = M.velocities(bs, nu)
    e = lambda x: None if x is None else x[..., None, :]
    bs1 = [dict(b, R=b["R"][..., None, :, :], r=e(b["r"]), axis=e(b["axis"])) for b in bs]
    wu, vu = M.velocities(bs1, np.broadcast_to(np.eye(18), (n, 18, 18)))                  # [n, 18 (unit velocity), 3]
    P = np.zeros((n, N_POINTS, 3)); V = np.zeros((n, N_POINTS, 3)); J = np.zeros((n, N_POINTS, 3, 18))

    def put(i, k, r):            # the point at r (world) from the origin of body k
        P[:, i] = bs[k]["p"] + r
        V[:, i] = v[k] + np.cross(w[k], r)
        J[:, i] = np.swapaxes(vu[k] + np.cross(wu[k], r[:, None, :]), -1, -2)

    for leg, (k, r) in enumerate(feet):
        put(leg, k, r)
        put(4 + leg, k, np.zeros((n, 3)))
    Rb = bs[0]["R"]
    for c, cb in enumerate(corners_in_base(body)):
        put(8 + c, 0, np.einsum("nij,j->ni", Rb, cb))
    return P, V, J


def limit_torque(body, q, qd):
    """tau_lim [n, 12] of the joints at q, qd [n, 12]."""
    lo, hi = np.tile(body["q_lo"], 4), np.tile(body["q_hi"], 4)
    k, a = body["limit_k"], body["limit_a"]
    over = -np.maximum(0.0, k * (q - hi) * (1.0 + a * qd))
    under = np.maximum(0.0, k * (lo - q) * (1.0 - a * qd))
    return np.where(q > hi, over, np.where(q < lo, under, 0.0))


def point_forces(p, D, height, fid, P, V):
    """The terrain law on every point: -> force [n, 16, 3] (world), f_n [n, 16], outside-the-grid [n, 16]."""
    z, zx, zy, off = TR.sample(D, height, np.asarray(fid)[:, None], P[..., 0], P[..., 1])
    f, fn = TR.contact_force(p, z + p["ground_z"], TR.normal(zx, zy), P, V)
    return f, fn, off


def substep(model, body, p, D, height, fid, push, s, cmd, h):
    """One sub-step of length h on the float64 state s [n, 37].  The feet and the motor go through plant_ref.forward_dynamics as in terrain_ref; what
    this call adds -- knees, corners, stops -- and the push enter one more solve on the same H, so that with all of them zero the result is
    terrain_ref.substep's to the bit."""
    rb = M.compute(model, s)
    P, V, J = points(model, body, s)
    f, fn, off = point_forces(p, D, height, fid, P, V)
    tau = PR.motor_torque(p, cmd, s[:, 13:25], s[:, 25:37])
    tlim = limit_torque(body, s[:, 13:25], s[:, 25:37])
    nud = PR.forward_dynamics(model, s, tau, f[:, FEET].reshape(-1, 12), rb=rb)
    extra = TR.push_rhs(s, push) + np.einsum("npak,npa->nk", J[:, 4:], f[:, 4:])
    extra[:, 6:] += tlim
    nud = nud + np.linalg.solve(rb["H"], extra[..., None])[..., 0]
    R = M.quat_to_rot(s[:, 0:4])
    acc = nud[:, 3:6] + np.cross(s[:, 7:10], s[:, 10:13]) + np.einsum("nji,j->ni", R, np.array([0.0, 0.0, 9.81]))
    o = s.copy()
    o[:, 7:13] += h * nud[:, 0:6]
    o[:, 25:37] += h * nud[:, 6:18]
    o[:, 13:25] += h * o[:, 25:37]
    o[:, 4:7] += h * np.einsum("nij,nj->ni", R, o[:, 10:13])
    qn = PR.quat_mul(s[:, 0:4], PR.quat_exp(h * o[:, 7:10]))
    o[:, 0:4] = qn / np.linalg.norm(qn, axis=-1, keepdims=True)
    return o, dict(force=f, fn=fn, tau=tau, tlim=tlim, nu_dot=nud, acc=acc, off=off, points=P, J=J, H=rb["H"], C=rb["C"], G=rb["G"])


def status_of(p, aux):
    """The status bits the last sub-step gives: OFF_FIELD over all sixteen points, TRUNK_CONTACT, KNEE_CONTACT, JOINT_LIMIT.  -> [n]"""
    fn, thr = aux["fn"], p["contact_threshold"]
    return (np.where((aux["off"] & (fn > 0)).any(1), TR.PL_OFF_FIELD, 0) | np.where((fn[:, CORNERS] > thr).any(1), PL_TRUNK_CONTACT, 0)
            | np.where((fn[:, KNEES] > thr).any(1), PL_KNEE_CONTACT, 0) | np.where((aux["tlim"] != 0).any(1), PL_JOINT_LIMIT, 0))


def step(model, body, p, D, height, field_id, push, state32, cmd32, state64=None):
    """One control tick: terrain_ref.step's outputs plus body_out [n, 36], fn [n, 16], off [n, 16], tlim [n, 12]; status with the three new bits and
    OFF_FIELD over all sixteen points.  float64 and unrounded."""
    s = M.normalised(state32) if state64 is None else state64
    n = len(s)
    fid = np.zeros(n, np.int64) if field_id is None else np.asarray(field_id, np.int64)
    bad = (fid < 0) | (fid >= D["n_fields"])
    fid = np.where(bad, 0, fid)
    h = p["dt"] / p["substeps"]
    for _ in range(p["substeps"]):
        s, aux = substep(model, body, p, D, height, fid, push, s, cmd32, h)
    rb = M.compute(model, s)
    f, fn, thr = aux["force"], aux["fn"], p["contact_threshold"]
    out = np.zeros((n, PR.PLANT_OUT_ROWS))
    out[:, 0:12] = f[:, FEET].reshape(n, 12); out[:, 12:24] = rb["pGC"].reshape(n, 12)
    out[:, 24:28] = fn[:, FEET] > thr; out[:, 28:40] = aux["tau"]; out[:, 40:58] = aux["nu_dot"]
    z_g, nrm, _ = TR.ground(p, D, height, fid, rb["pGC"])
    tout = np.concatenate([z_g, nrm.reshape(n, 12)], 1)
    bout = np.zeros((n, BODY_OUT_ROWS))
    bout[:, 0:12] = f[:, KNEES].reshape(n, 12); bout[:, 12:16] = fn[:, KNEES] > thr; bout[:, 16:24] = fn[:, CORNERS]; bout[:, 24:36] = aux["tlim"]
    est = np.zeros((n, 41))
    est[:, 0:3] = aux["acc"]; est[:, 3:6] = aux["acc"]; est[:, 6:10] = s[:, 0:4]; est[:, 10:13] = s[:, 7:10]
    est[:, 13:17] = out[:, 24:28]; est[:, 17:29] = s[:, 13:25]; est[:, 29:41] = s[:, 25:37]
    status = np.where(bad, TR.PL_BAD_FIELD, 0) | status_of(p, aux)
    return dict(fb_state=s, plant_out=out, terrain_out=tout, body_out=bout, mpc_state=PR.truth_mpc_state(model, p, s), est_in=est, fn=fn, off=aux["off"],
                tlim=aux["tlim"], status=status.astype(np.int32))


def step_mixed(models, bodies, type_id, p, D, height, field_id, push, state32, cmd32):
    """step() on a batch of several robot types: models[t], bodies[t] are those of type t."""
    out = None
    for t, model in enumerate(models):
        k = np.nonzero(type_id == t)[0]
        r = step(model, bodies[t], p, D, height, None if field_id is None else field_id[k], None if push is None else push[k], state32[k], cmd32[k])
        if out is None:
            out = {key: np.zeros((len(type_id),) + v.shape[1:], v.dtype) for key, v in r.items()}
        for key, v in r.items():
            out[key][k] = v
    return out


def status_masks(p, fn, rel=1e-6):
    """Which status bits of each robot may differ between two correct evaluations: a point whose f_n is within rel of the contact threshold
    (plant_ref.near_threshold) loosens its group's bit.  -> loose flags [n, 16], loose status bits [n] int32"""
    loose = PR.near_threshold(p, fn, rel)
    bits = np.where(loose[:, CORNERS].any(1), PL_TRUNK_CONTACT, 0) | np.where(loose[:, KNEES].any(1), PL_KNEE_CONTACT, 0)
    return loose, bits.astype(np.int32)


# ---- the step case: terrain_ref.step_case's fields, pushes, ids and motor commands under 48 robots drawn from five families
STEP_SEED = 9131
FAMILIES = ("standing", "belly", "kneeling", "back", "wide")


def _quat_rpy(r, p, y):
    hr, hp, hy = r / 2, p / 2, y / 2
    cr, sr, cp, sp, cy, sy = np.cos(hr), np.sin(hr), np.cos(hp), np.sin(hp), np.cos(hy), np.sin(hy)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)


_case_cache = {}


def step_case(pkg):
    """terrain_ref.step_case with the states of robots 8.. replaced, family = (robot // 2) % 5 so that every family holds both types and both
    fields: standing (terrain_ref's own draw), belly (base 0.02-0.07 above the ground under it, legs tucked), kneeling (pitched forward by 0.6-0.9, low:
    front knees under the ground), back (rolled by pi +- 0.2, low: top corners under the ground), wide (rigid_body_ref.wide_states' joint ranges,
    which exceed A1's limits, attitude and rates as standing).  The robots are placed over the grid; x, y of some lie near or beyond the y border,
    as in the terrain case.  -> terrain_ref.step_case's dict plus family [48].  Computed once and shared (callers must not modify it)."""
    if _case_cache:
        return _case_cache
    c = dict(TR.step_case(pkg))
    s = c["state"].astype(np.float64).copy()
    n = len(s)
    rng = np.random.default_rng(STEP_SEED)
    U = rng.uniform
    fam = (np.arange(n) // 2) % 5
    p = PR.params(**TR.STEP_PARAMS)
    zg = TR.sample(c["D"], c["height"], c["fid"], s[:, 4], s[:, 5])[0] + p["ground_z"]           # the ground under each base origin
    wide = M.wide_states(n, STEP_SEED + 1)
    for i in range(n):
        f = FAMILIES[fam[i]]
        yaw = U(-np.pi, np.pi)
        if f == "belly":
            s[i, 0:4] = _quat_rpy(U(-0.1, 0.1), U(-0.1, 0.1), yaw); s[i, 6] = zg[i] + U(0.02, 0.07)
            s[i, 13:25] = np.tile([0.0, 1.3, -2.5], 4) + U(-0.1, 0.1, 12)
        elif f == "kneeling":
            s[i, 0:4] = _quat_rpy(U(-0.1, 0.1), U(0.6, 0.9), yaw); s[i, 6] = zg[i] + U(0.10, 0.16)
            s[i, 13:25] = np.tile([0.0, 0.3, -2.2], 4) + U(-0.1, 0.1, 12)
        elif f == "back":
            s[i, 0:4] = _quat_rpy(np.pi + U(-0.2, 0.2), U(-0.2, 0.2), yaw); s[i, 6] = zg[i] + U(0.0, 0.05)
        elif f == "wide":
            s[i, 13:25] = wide[i, 13:25]; s[i, 25:37] = U(-4, 4, 12); s[i, 6] = zg[i] + U(0.25, 0.4)
    c["state"] = s.astype(_f); c["family"] = fam
    _case_cache.update(c)
    return _case_cache


def models_and_bodies(pkg):
    return [pkg.model_desc(r) for r in PR.ROBOTS], [body_of(pkg.plant_body_desc(r)) for r in PR.ROBOTS]


CLEAR_HEIGHT = 0.29


def clear_case(pkg):
    """terrain_ref.step_case with every base origin CLEAR_HEIGHT above the ground under it: feet at the ground (some in it, some over it), knees and
    trunk well above it, joints inside their limits (the stand pose +- 0.2).  -> the case's dict with the state replaced"""
    c = dict(TR.step_case(pkg))
    s = c["state"].copy()
    p = PR.params(**TR.STEP_PARAMS)
    s[:, 6] = (TR.sample(c["D"], c["height"], c["fid"], s[:, 4].astype(np.float64), s[:, 5].astype(np.float64))[0] + p["ground_z"] + CLEAR_HEIGHT).astype(_f)
    c["state"] = s
    return c


# ---- scenario chains on the flat field: one A1 robot each, all gains and torques zero
SCENARIOS = ("limp", "back")
# 1400 ticks, not 800: the limp robot is still bouncing at 800 (its trunk touches on some ticks and not on others: at tick 800 the float64 chain
# has TRUNK_CONTACT clear) and has come to rest on knees and trunk from tick 1200 on.  The two chains run as one batch of two, in 40 s.
FALL_TICKS, FALL_TAIL = 1400, 350
FALL_PARAMS = dict(dt=0.001, substeps=2)
FALL_GRID = dict(half=1.0, cell=0.125)


def fall_case(pkg, n):
    """-> D, height [1, ny, nx] (all zero), state [n, 37], cmd [n, 60] float32, scenario [n]: dropped from z = 0.30 at the stand pose, even robots
    level ("limp"), odd ones rolled by pi ("back"); the motor command is all zero."""
    T = pkg.terrain
    g = T.Grid.centred(FALL_GRID["half"], FALL_GRID["cell"])
    height = T.stack([T.flat(g)])
    s = PR.stand_state(n)
    s[1::2, 0] = np.cos(0.5 * np.pi); s[1::2, 1] = np.sin(0.5 * np.pi)
    return TR.desc(n_fields=1, **g.desc()), height, s, np.zeros((n, 60), _f), np.arange(n) % 2


def fall_measures(body, state, plant_out, body_out, fz=None):
    """What the fall tests band, [n, 3]: base height, sum f_z over the sixteen points / (m g), largest joint excursion beyond a limit [rad].  The
    outputs give the corners' forces by their f_n only; on the flat field f_z = f_n.  (fz: the sum when the caller has it.)"""
    s = np.asarray(state, np.float64)
    if fz is None:
        po, bo = np.asarray(plant_out, np.float64), np.asarray(body_out, np.float64)
        fz = po[:, 2:12:3].sum(1) + bo[:, 2:12:3].sum(1) + bo[:, 16:24].sum(1)
    q = s[:, 13:25]
    exc = np.maximum(np.maximum(q - np.tile(body["q_hi"], 4), np.tile(body["q_lo"], 4) - q), 0.0).max(1)
    return np.stack([s[:, 6], fz / (M.total_mass() * 9.81), exc], 1)


_chain_cache = {}


def fall_chains(pkg):
    """The float64 chains of the two scenarios, run as a batch of two: step()'s sub-steps without the outputs nobody reads here.  -> per scenario a
    dict: end measures, residual swing (max - min over the last FALL_TAIL ticks), OR of the status words, status at the end, whether every state
    was finite, final state.  Computed once and shared."""
    if _chain_cache:
        return _chain_cache
    D, height, s32, cmd, _ = fall_case(pkg, 2)
    model, body = pkg.model_desc("a1"), body_of(pkg.plant_body_desc("a1"))
    p = PR.params(**FALL_PARAMS)
    s = M.normalised(s32)
    fid = np.zeros(2, np.int64)
    h = p["dt"] / p["substeps"]
    tail, seen, finite = [], np.zeros(2, np.int64), np.ones(2, bool)
    for k in range(FALL_TICKS):
        for _ in range(p["substeps"]):
            s, aux = substep(model, body, p, D, height, fid, None, s, cmd, h)
        status = status_of(p, aux)
        seen |= status; finite &= np.isfinite(s).all(1)
        if k >= FALL_TICKS - FALL_TAIL:
            tail.append(fall_measures(body, s, None, None, fz=aux["force"][:, :, 2].sum(1)))
    tail = np.array(tail)
    for i, name in enumerate(SCENARIOS):
        _chain_cache[name] = dict(end=tail[-1, i], swing=tail[:, i].max(0) - tail[:, i].min(0), seen=int(seen[i]), status=int(status[i]), finite=bool(finite[i]),
                                  state=s[i])
    return _chain_cache


# End values and residual swing of fall_chains (test_body_contact_ref.py asserts that the chains give them), in fall_measures' order: base height [m],
# sum f_z / (m g), largest excursion beyond a joint limit [rad].  The GPU test's bands are end +- 3 swing.
# Measured: the limp robot rests on its knees (75 N), its trunk (61 N) and its feet (5 N) with the abad joints 0.03 rad beyond their stops; the robot on
# its back rests on its four top corners (108 N) with its legs still swinging (no joint damping anywhere: all gains are zero).  sum f_z still
# chatters by about one m g from tick to tick in both: the contact springs at 0.5 ms.
FALL_END = dict(limp=(0.0562348, 1.06890837, 0.0301807), back=(0.05565016, 0.99575552, 0.0))
FALL_SWING = dict(limp=(0.00210126, 1.08313663, 0.01236915), back=(0.00189158, 1.24975312, 0.03827553))
