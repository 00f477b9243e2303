"""TEST INFRASTRUCTURE -- the terrain plant (qrgpu_plant_step_terrain_batch) restated in float64 numpy from the comment of include/qrgpu.h: the
Catmull-Rom sampler of a stack of height fields, the contact law on the sampled surface, the push on the base.  Motor law, forward dynamics and
the integrator's pieces are plant_ref's; the shared seeded cases of the CPU and GPU files live here.

  desc = dict(nx, ny, n_fields, x0, y0, cell) with the float32 values widened;  height [n_fields, ny, nx] float32;  field_id [n] or None;
  push [n, 6] = world-frame force at the base origin, world-frame moment, or None;  arrays are robot-major [n, rows].
"""
import numpy as np

import plant_ref as PR
import rigid_body_ref as M

_f = np.float32
TERRAIN_OUT_ROWS = 16
PL_BAD_FIELD, PL_OFF_FIELD = 0x4, 0x8


def desc(nx, ny, n_fields, x0, y0, cell):
    w = lambda v: float(np.float64(_f(v)))
    return dict(nx=int(nx), ny=int(ny), n_fields=int(n_fields), x0=w(x0), y0=w(y0), cell=w(cell))


def _axis(x, x0, cell, nx):
    """One axis of the sampler: -> clamped node indices [4, ...], weights [4, ...], derivative weights per unit of u [4, ...], outside [...]."""
    ur = (np.asarray(x, np.float64) - x0) / cell
    off = ~((ur >= 0) & (ur <= nx - 1))
    u = np.clip(np.where(np.isnan(ur), 0.0, ur), 0.0, nx - 1.0)
    i = np.minimum(np.floor(u), nx - 2).astype(np.int64)
    t = u - i
    w = 0.5 * np.stack([-t ** 3 + 2 * t ** 2 - t, 3 * t ** 3 - 5 * t ** 2 + 2, -3 * t ** 3 + 4 * t ** 2 + t, t ** 3 - t ** 2])
    d = 0.5 * np.stack([-3 * t ** 2 + 4 * t - 1, 9 * t ** 2 - 10 * t, -9 * t ** 2 + 8 * t + 1, 3 * t ** 2 - 2 * t])
    idx = np.clip(np.stack([i - 1, i, i + 1, i + 2]), 0, nx - 1)
    return idx, w, d, off


def sample(D, height, fid, x, y):
    """The surface of field fid [...] at (x, y) [...]: -> z, dz/dx, dz/dy, outside-the-grid [...] (sampled height only: ground_z not added)."""
    H = np.asarray(height, _f).astype(np.float64).reshape(D["n_fields"], D["ny"], D["nx"])
    ix, wx, dx, ox = _axis(x, D["x0"], D["cell"], D["nx"])
    iy, wy, dy, oy = _axis(y, D["y0"], D["cell"], D["ny"])
    fid = np.broadcast_to(np.asarray(fid, np.int64), np.shape(x))
    nodes = H[fid[None, None], iy[:, None], ix[None, :]]                     # [4 (y), 4 (x), ...]
    z = np.einsum("j...,i...,ji...->...", wy, wx, nodes)
    zx = np.einsum("j...,i...,ji...->...", wy, dx, nodes) / D["cell"]
    zy = np.einsum("j...,i...,ji...->...", dy, wx, nodes) / D["cell"]
    return z, zx, zy, ox | oy


def normal(zx, zy):
    n = np.stack([-zx, -zy, np.ones_like(zx)], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def contact_force(p, z_g, n, foot_pos, foot_vel):
    """The contact law on a surface of height z_g [...] and unit normal n [..., 3] under the foot: -> force [..., 3] (world), f_n [...]."""
    delta = (z_g - foot_pos[..., 2]) * n[..., 2]
    vn = np.sum(foot_vel * n, -1)
    vt = foot_vel - vn[..., None] * n
    fn = np.where(delta > 0, np.maximum(0.0, p["contact_k"] * delta * (1.0 - p["contact_a"] * vn)), 0.0)
    f = fn[..., None] * n - (p["mu"] * fn / np.sqrt(np.sum(vt * vt, -1) + p["v_eps"] ** 2))[..., None] * vt
    return f, fn


def ground(p, D, height, fid, foot_pos):
    """-> z_g [n, 4] (ground_z included), n [n, 4, 3], outside [n, 4] under the feet foot_pos [n, 4, 3] of robots on fields fid [n]."""
    z, zx, zy, off = sample(D, height, np.asarray(fid)[:, None], foot_pos[..., 0], foot_pos[..., 1])
    return z + p["ground_z"], normal(zx, zy), off


def push_rhs(s, push):
    """What the push adds to the right-hand side of H nu_dot + C + G = ...: [R^T moment; R^T force; 0]  [n, 18]."""
    R = M.quat_to_rot(s[:, 0:4])
    w = np.zeros((len(s), 18))
    if push is not None:
        push = np.asarray(push, np.float64)
        w[:, 0:3] = np.einsum("nji,nj->ni", R, push[:, 3:6]); w[:, 3:6] = np.einsum("nji,nj->ni", R, push[:, 0:3])
    return w


def substep(model, p, D, height, fid, push, s, cmd, h):
    """One sub-step of length h on the float64 state s [n, 37]: plant_ref.substep with the terrain's contact law and the push."""
    rb = M.compute(model, s)
    z_g, n, off = ground(p, D, height, fid, rb["pGC"])
    f, fn = contact_force(p, z_g, n, rb["pGC"], rb["vGC"])
    tau = PR.motor_torque(p, cmd, s[:, 13:25], s[:, 25:37])
    nud = PR.forward_dynamics(model, s, tau, f.reshape(-1, 12), rb=rb)
    if push is not None:
        nud = nud + np.linalg.solve(rb["H"], push_rhs(s, push)[..., None])[..., 0]
    R = M.quat_to_rot(s[:, 0:4])
    acc = nud[:, 3:6] + np.cross(s[:, 7:10], s[:, 10:13]) + np.einsum("nji,j->ni", R, np.array([0.0, 0.0, 9.81]))
    o = s.copy()
    o[:, 7:13] += h * nud[:, 0:6]
    o[:, 25:37] += h * nud[:, 6:18]
    o[:, 13:25] += h * o[:, 25:37]
    o[:, 4:7] += h * np.einsum("nij,nj->ni", R, o[:, 10:13])
    qn = PR.quat_mul(s[:, 0:4], PR.quat_exp(h * o[:, 7:10]))
    o[:, 0:4] = qn / np.linalg.norm(qn, axis=-1, keepdims=True)
    return o, dict(force=f, fn=fn, tau=tau, nu_dot=nud, acc=acc, off=off)


def step(model, p, D, height, field_id, push, state32, cmd32, state64=None):
    """One control tick: plant_ref.step's outputs plus terrain_out [n, 16] and status [n] (BAD_FIELD, OFF_FIELD), float64 and unrounded."""
    s = M.normalised(state32) if state64 is None else state64
    n = len(s)
    fid = np.zeros(n, np.int64) if field_id is None else np.asarray(field_id, np.int64)
    bad = (fid < 0) | (fid >= D["n_fields"])
    fid = np.where(bad, 0, fid)
    h = p["dt"] / p["substeps"]
    for _ in range(p["substeps"]):
        s, aux = substep(model, p, D, height, fid, push, s, cmd32, h)
    rb = M.compute(model, s)
    out = np.zeros((n, PR.PLANT_OUT_ROWS))
    out[:, 0:12] = aux["force"].reshape(n, 12); out[:, 12:24] = rb["pGC"].reshape(n, 12)
    out[:, 24:28] = aux["fn"] > p["contact_threshold"]; out[:, 28:40] = aux["tau"]; out[:, 40:58] = aux["nu_dot"]
    z_g, nrm, _ = ground(p, D, height, fid, rb["pGC"])
    tout = np.concatenate([z_g, nrm.reshape(n, 12)], 1)
    est = np.zeros((n, 41))
    est[:, 0:3] = aux["acc"]; est[:, 3:6] = aux["acc"]; est[:, 6:10] = s[:, 0:4]; est[:, 10:13] = s[:, 7:10]
    est[:, 13:17] = out[:, 24:28]; est[:, 17:29] = s[:, 13:25]; est[:, 29:41] = s[:, 25:37]
    status = np.where(bad, PL_BAD_FIELD, 0) | np.where((aux["off"] & (aux["fn"] > 0)).any(1), PL_OFF_FIELD, 0)
    return dict(fb_state=s, plant_out=out, terrain_out=tout, mpc_state=PR.truth_mpc_state(model, p, s), est_in=est, fn=aux["fn"], off=aux["off"],
                status=status.astype(np.int32))


def step_mixed(models, type_id, p, D, height, field_id, push, state32, cmd32):
    """step() on a batch of several robot types: models[t] is the model of type t."""
    out = None
    for t, model in enumerate(models):
        k = np.nonzero(type_id == t)[0]
        r = step(model, p, D, height, None if field_id is None else field_id[k], None if push is None else push[k], state32[k], cmd32[k])
        if out is None:
            out = {key: np.zeros((len(type_id),) + v.shape[1:], v.dtype) for key, v in r.items()}
        for key, v in r.items():
            out[key][k] = v
    return out


# ---- shared cases (seeded; test_terrain_ref.py checks what test_gpu_terrain.py relies on)
STEP_GRID = dict(nx=24, ny=20, x0=-1.2, y0=-0.9, cell=0.11)          # not square: a swapped stride shows; some feet lie beyond the y border
STEP_FIELD_SEED, STEP_PUSH_SEED = 8821, 8822
# A softer ground and a shorter tick than the defaults, and the ground a little lower: at contact_k 2e4 and 2 ms this draw's deep feet (up to 0.3 m
# under field 0) are thrown clear by the first sub-step, and the last sub-step of the 2-sub-step run is left with 12 feet in contact, none off the
# grid.  With these the conditions of test_terrain_ref.py hold at 1, 2 and 8 sub-steps.
STEP_PARAMS = dict(dt=0.0005, contact_k=5e3, ground_z=-0.02)


def step_case(pkg):
    """The 48 mixed robots of plant_ref.step_cases() on two stacked fields -- 0: a plane of slopes (0.2, -0.1) plus a roughness of 0.03, 1: stairs
    -- with field ids that alternate in pairs (0 0 1 1 ...: not in step with the type ids 0 1 0 1) and a push of +-40 N, +-10 N m.
    -> dict state, cmd, tid, D, height [2, 20, 24] float32, fid [48] int32, push [48, 6] float32, grid"""
    T = pkg.terrain
    s, c, tid = PR.step_cases()
    g = T.Grid(**STEP_GRID)
    height = T.stack([T.plane(g, 0.2, -0.1) + T.rough(g, 0.03, STEP_FIELD_SEED), T.stairs(g, 0.05, 0.3, 4)])
    rng = np.random.default_rng(STEP_PUSH_SEED)
    n = len(s)
    push = np.concatenate([rng.uniform(-40, 40, (n, 3)), rng.uniform(-10, 10, (n, 3))], 1).astype(_f)
    fid = ((np.arange(n) // 2) % 2).astype(np.int32)
    return dict(state=s, cmd=c, tid=tid, D=desc(n_fields=2, **STEP_GRID), height=height, fid=fid, push=push, grid=g)


def near_border(D, foot_pos, rel=1e-6):
    """Feet within rel * cell of one of the grid's four border lines: their OFF_FIELD bit may differ between two correct evaluations."""
    x, y = foot_pos[..., 0], foot_pos[..., 1]
    tol = rel * D["cell"]
    x1, y1 = D["x0"] + (D["nx"] - 1) * D["cell"], D["y0"] + (D["ny"] - 1) * D["cell"]
    return (np.abs(x - D["x0"]) <= tol) | (np.abs(x - x1) <= tol) | (np.abs(y - D["y0"]) <= tol) | (np.abs(y - y1) <= tol)


# ---- standing on a slope: 32 A1 robots aligned with plane(tan 0.2, 0) on joint PD
SLOPE_ANGLE, SLOPE_TICKS, SLOPE_TAIL = 0.2, 1500, 500
SLOPE_PARAMS = dict(dt=0.001, substeps=4)


def slope_case(pkg, n):
    """-> D, height [1, ny, nx], state [n, 37], cmd [n, 60] float32: attitude a rotation of -SLOPE_ANGLE about y, position 0.30 n."""
    T = pkg.terrain
    g = T.Grid.centred(1.0, 0.125)
    height = T.stack([T.plane(g, np.tan(SLOPE_ANGLE), 0.0)])
    s = PR.stand_state(n)
    s[:, 0] = np.cos(-0.5 * SLOPE_ANGLE); s[:, 2] = np.sin(-0.5 * SLOPE_ANGLE)
    s[:, 4] = -0.30 * np.sin(SLOPE_ANGLE); s[:, 6] = 0.30 * np.cos(SLOPE_ANGLE)
    return desc(n_fields=1, **g.desc()), height, s, PR.stand_cmd(n)


def slope_measures(state, plant_out):
    """What the slope tests band, [n, 3]: |total contact force - (0, 0, m g)| / (m g), height of the base along the slope's normal, pitch."""
    nrm = np.array([-np.sin(SLOPE_ANGLE), 0.0, np.cos(SLOPE_ANGLE)])
    mg = M.total_mass() * 9.81
    f = np.asarray(plant_out, np.float64)[:, 0:12].reshape(-1, 4, 3).sum(1) - np.array([0.0, 0.0, mg])
    s = np.asarray(state, np.float64)
    return np.stack([np.linalg.norm(f, axis=1) / mg, s[:, 4:7] @ nrm, PR.quat_to_rpy(s[:, 0:4])[:, 1]], 1)


def slope_chain(pkg):
    """The float64 chain of the slope scenario for one robot.  -> end measures, residual swing (max - min over the last SLOPE_TAIL ticks) of each,
    contact flags at the end, worst status."""
    D, height, s32, cmd = slope_case(pkg, 1)
    model = pkg.model_desc("a1")
    p = PR.params(**SLOPE_PARAMS)
    s = M.normalised(s32)
    tail = []
    status = 0
    for k in range(SLOPE_TICKS):
        r = step(model, p, D, height, None, None, None, cmd, state64=s)
        s = r["fb_state"]; status |= int(r["status"][0])
        if k >= SLOPE_TICKS - SLOPE_TAIL:
            tail.append(slope_measures(s, r["plant_out"])[0])
    tail = np.array(tail)
    return dict(end=tail[-1], swing=tail.max(0) - tail.min(0), contact=r["plant_out"][0, 24:28], status=status, state=s,
                fz=float(r["plant_out"][0, 2:12:3].sum()))


# End values and residual swing of slope_chain (test_terrain_ref.py asserts that the chain gives them), in slope_measures' order:
# |sum f - (0, 0, m g)| / (m g), height along the normal [m], pitch [rad].  The GPU test's bands are end +- 3 swing.
# Measured: sum f_z 1.3 % under m g, |sum f - m g z| 8.7 % of m g (the robot still rocks: sum f_x = -11.3 N at the last tick).
SLOPE_END = (0.08654587, 0.26506717, -0.24958452)
SLOPE_SWING = (0.02533288, 0.00162774, 0.01206631)
