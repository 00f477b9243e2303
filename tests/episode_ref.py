"""TEST INFRASTRUCTURE -- the episode step (qrgpu_episode_step_batch) restated in float64 numpy from the comment of include/qrgpu.h: termination,
the counter-based random numbers, the spawn, the bookkeeping.  It shares nothing with csrc/qr_episode.h: its own Philox-4x32-10 (on Python
integers), its own attitude (a rotation MATRIX from the normal by Rodrigues' formula times the yaw matrix, turned into a quaternion by Shepperd's
method, where the header multiplies two quaternions), and terrain_ref.sample for the ground.

  desc = dict of the fields of qrgpu_episode_desc (desc(**over): the library's defaults, float fields as the float32 values widened)
  ground = None (flat) or dict(D=terrain_ref.desc(...), height [n_fields, ny, nx], fid [n] or None);  ground_z a float
  arrays are robot-major: fb [n, 37], ep_state [n, 6] int, ep_stats [n, 9], table [4, n_spawn] float32
"""
import numpy as np

import terrain_ref as TR

_f = np.float32
EP_STATUS, EP_TICK_STATUS, EP_NONFINITE, EP_TILT, EP_HEIGHT, EP_OFF_FIELD, EP_TIMEOUT, EP_FORCED = (1 << k for k in range(8))
EP_REASONS, EP_BAD_FIELD = 0xff, 0x01000000
STATE_ROWS, STATS_ROWS = 6, 9
PL_NONFINITE, PL_QUAT_ZERO, PL_TRUNK_CONTACT, PL_KNEE_CONTACT = 0x1, 0x2, 0x10, 0x20
_FLOATS = ("tilt_max", "min_clearance", "field_margin", "spawn_height", "xy_jitter", "yaw_jitter", "q_jitter", "v_jitter", "kp", "kd")


def desc(**over):
    d = dict(status_mask=PL_NONFINITE | PL_QUAT_ZERO | PL_TRUNK_CONTACT, status_ticks=1, tick_mask=0, max_ticks=0, seed=1, align_to_slope=0, tilt_max=1.0,
             min_clearance=0.10, field_margin=0.0, spawn_height=0.30, xy_jitter=0.0, yaw_jitter=0.0, q_jitter=0.0, v_jitter=0.0,
             q_spawn=[0.0, 0.8, -1.6] * 4, kp=100.0, kd=2.0)
    d.update(over)
    for k in _FLOATS:
        d[k] = float(np.float64(_f(d[k])))
    d["q_spawn"] = np.asarray(d["q_spawn"], _f).astype(np.float64)
    return d


# ---- Philox-4x32-10 on Python integers
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox(counter, key):
    """counter (4 words), key (2 words) -> 4 words"""
    c = [int(x) & _MASK for x in counter]
    k = [int(x) & _MASK for x in key]
    for rnd in range(10):
        if rnd:
            k = [(k[0] + _W0) & _MASK, (k[1] + _W1) & _MASK]
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & _MASK]
    return c


def words(seed, robot, epi):
    """The twenty words of one robot's spawn: blocks 0..4 -> [5, 4] uint32"""
    return np.array([philox((epi, k, 0, 0), (seed, robot)) for k in range(5)], np.uint32)


def uniform(w):
    return (np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0


def cos_tilt(d):
    """What R_zz is held against: a tilt_max of pi (as a float) or more bounds nothing."""
    return -2.0 if d["tilt_max"] >= float(np.float64(_f(np.pi))) else float(np.cos(d["tilt_max"]))


def _field_ids(ground, n):
    """-> fid [n] as used, bad [n]"""
    if ground is None:
        return np.zeros(n, np.int64), np.zeros(n, bool)
    fid = np.zeros(n, np.int64) if ground.get("fid") is None else np.asarray(ground["fid"], np.int64)
    bad = (fid < 0) | (fid >= ground["D"]["n_fields"])
    return np.where(bad, 0, fid), bad


def ground_at(ground, ground_z, fid, x, y):
    """-> height (ground_z included), unit normal [n, 3]"""
    if ground is None:
        n = np.zeros(np.shape(x) + (3,)); n[..., 2] = 1.0
        return np.full(np.shape(x), float(ground_z)), n
    z, zx, zy, _ = TR.sample(ground["D"], ground["height"], fid, x, y)
    n = np.stack([-zx, -zy, np.ones_like(zx)], -1)
    return z + ground_z, n / np.sqrt((n * n).sum(-1))[..., None]


def margin_distance(D, margin, x, y):
    """Signed distance of (x, y) to the nearest line of the grid shrunk by margin: < 0 outside."""
    x1, y1 = D["x0"] + (D["nx"] - 1) * D["cell"], D["y0"] + (D["ny"] - 1) * D["cell"]
    return np.minimum(np.minimum(x - (D["x0"] + margin), (x1 - margin) - x), np.minimum(y - (D["y0"] + margin), (y1 - margin) - y))


def criteria(d, ground, ground_z, fb):
    """The continuous criteria of the state fb [n, 37] (float32 values): finite [n], R_zz, clearance, margin distance (NaN where not judged)."""
    s = np.asarray(fb, _f).astype(np.float64)
    n = len(s)
    finite = np.isfinite(s).all(1)
    t = np.where(finite[:, None], s, 0.0)
    q = t[:, 0:4]
    n2 = (q * q).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rzz = np.where(n2 > 0, 1.0 - 2.0 * (q[:, 1] ** 2 + q[:, 2] ** 2) / n2, 1.0)
    fid, _ = _field_ids(ground, n)
    zg, _ = ground_at(ground, ground_z, fid, t[:, 4], t[:, 5])
    clr = t[:, 6] - zg
    mar = margin_distance(ground["D"], d["field_margin"], t[:, 4], t[:, 5]) if ground is not None else np.full(n, np.nan)
    nan = np.where(finite, 0.0, np.nan)
    return finite, rzz + nan, clr + nan, mar + nan


def _quat_from_matrix(R):
    """Shepperd: the largest of the four candidates -> (w, x, y, z), unit, w >= 0."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    c = [tr, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(c))
    if k == 0:
        w = 0.5 * np.sqrt(1.0 + tr); q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
    elif k == 1:
        x = 0.5 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]); q = [(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)]
    elif k == 2:
        y = 0.5 * np.sqrt(1.0 - R[0, 0] + R[1, 1] - R[2, 2]); q = [(R[0, 2] - R[2, 0]) / (4 * y), (R[0, 1] + R[1, 0]) / (4 * y), y, (R[1, 2] + R[2, 1]) / (4 * y)]
    else:
        z = 0.5 * np.sqrt(1.0 - R[0, 0] - R[1, 1] + R[2, 2]); q = [(R[1, 0] - R[0, 1]) / (4 * z), (R[0, 2] + R[2, 0]) / (4 * z), (R[1, 2] + R[2, 1]) / (4 * z), z]
    q = np.array(q)
    q /= np.sqrt((q * q).sum())
    return -q if q[0] < 0 else q


def attitude(normal, yaw, align):
    """The spawn attitude: R = R_tilt R_z(yaw), R_tilt the rotation about e_z x normal that takes e_z onto normal (identity when not aligned)."""
    c, s = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    Rt = np.eye(3)
    ax = np.array([-normal[1], normal[0], 0.0])
    sn = np.sqrt((ax * ax).sum())
    if align and sn > 0:
        ax = ax / sn
        ang = np.arctan2(sn, normal[2])
        K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
        Rt = np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)
    return _quat_from_matrix(Rt @ Rz)


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def spawn(d, ground, ground_z, table, robot, epi):
    """The spawn of robots `robot` [m] at episode indices `epi` [m] -> dict fb [m, 37] (float64, unrounded), yaw [m], row [m], words [m, 5, 4],
    ground [m] (height under the spawn point), normal [m, 3]."""
    table = np.asarray(table, _f).astype(np.float64)
    ns = table.shape[1]
    robot, epi = np.asarray(robot, np.int64), np.asarray(epi, np.int64)
    m = len(robot)
    W = np.stack([words(d["seed"], int(r), int(e)) for r, e in zip(robot, epi)]) if m else np.zeros((0, 5, 4), np.uint32)
    u = uniform(W)
    s = 2.0 * u - 1.0
    row = np.minimum(np.floor(u[:, 0, 0] * ns).astype(np.int64), ns - 1)
    x = table[0, row] + d["xy_jitter"] * s[:, 0, 1]
    y = table[1, row] + d["xy_jitter"] * s[:, 0, 2]
    yaw = table[2, row] + d["yaw_jitter"] * s[:, 0, 3]
    fid_all, _ = _field_ids(ground, int(robot.max()) + 1 if m else 0)
    zg, nrm = ground_at(ground, ground_z, fid_all[robot] if m else fid_all, x, y)
    fb = np.zeros((m, 37))
    fb[:, 4] = x + d["spawn_height"] * nrm[:, 0]; fb[:, 5] = y + d["spawn_height"] * nrm[:, 1]; fb[:, 6] = zg + d["spawn_height"] * nrm[:, 2]
    for i in range(m):
        fb[i, 0:4] = attitude(nrm[i], yaw[i], d["align_to_slope"])
    fb[:, 10] = d["v_jitter"] * s[:, 1, 0]; fb[:, 11] = d["v_jitter"] * s[:, 1, 1]
    fb[:, 13:25] = d["q_spawn"][None] + d["q_jitter"] * s[:, 2:5, :].reshape(m, 12)
    return dict(fb=fb, yaw=yaw, row=row, words=W, ground=zg, normal=nrm)


def step(d, ground, ground_z, table, fb, ep_state, ep_stats, plant_status=None, tick_status=None, force_reset=None, reset_all=False, prev_ori=None,
         motor_cmd=None):
    """One call.  fb [n, 37], ep_stats [n, 9], prev_ori [n, 3], motor_cmd [n, 60]: float32 values as the device holds them; -> dict of the arrays
    after the call (floats float64, unrounded where the call computes them), done [n], reset [n] bool, and the criteria judged."""
    fb = np.asarray(fb, _f).astype(np.float64)
    n = len(fb)
    st = np.asarray(ep_state, np.int64).copy()
    stats = np.asarray(ep_stats, _f).astype(np.float64)
    zero = np.zeros(n, np.int64)
    ps = zero if plant_status is None else np.asarray(plant_status, np.int64)
    ts = zero if tick_status is None else np.asarray(tick_status, np.int64)
    fr = zero if force_reset is None else np.asarray(force_reset, np.int64)
    _, bad = _field_ids(ground, n)
    flags = np.where(bad, EP_BAD_FIELD, 0)
    finite, rzz, clr, mar = criteria(d, ground, ground_z, fb)
    if reset_all:
        st[:] = 0; stats[:] = 0.0
        reason = np.full(n, EP_FORCED)
    else:
        st[:, 2] = np.where((ps & d["status_mask"]) != 0, np.minimum(st[:, 2] + 1, 0x7fffffff), 0)
        st[:, 0] = np.minimum(st[:, 0] + 1, 0x7fffffff)
        with np.errstate(invalid="ignore"):
            reason = (np.where(st[:, 2] >= d["status_ticks"], EP_STATUS, 0) | np.where((ts & d["tick_mask"]) != 0, EP_TICK_STATUS, 0)
                      | np.where(~finite, EP_NONFINITE, 0) | np.where(rzz < cos_tilt(d), EP_TILT, 0) | np.where(clr < d["min_clearance"], EP_HEIGHT, 0)
                      | np.where(mar < 0, EP_OFF_FIELD, 0) | np.where((d["max_ticks"] > 0) & (st[:, 0] >= d["max_ticks"]), EP_TIMEOUT, 0) | np.where(fr != 0, EP_FORCED, 0))
        stats[:, 8] = np.where(finite, np.minimum(stats[:, 8], np.where(finite, clr, 0.0)), stats[:, 8])
    reset = reason != 0
    k = np.nonzero(reset)[0]
    if not reset_all:
        st[k, 3] = reason[k]
        alone = reason[k] == EP_TIMEOUT
        st[k, 5] += alone; st[k, 4] += ~alone
        stats[k, 4] = st[k, 0]
        stats[k, 5] = np.where(finite[k], fb[k, 4] - stats[k, 0], 0.0); stats[k, 6] = np.where(finite[k], fb[k, 5] - stats[k, 1], 0.0)
        stats[k, 7] = stats[k, 8]
        st[k, 1] += 1
    sp = spawn(d, ground, ground_z, table, k, st[k, 1])
    st[k, 0] = 0; st[k, 2] = 0
    fb[k] = sp["fb"]
    stats[k, 0:3] = sp["fb"][:, 4:7]; stats[k, 3] = sp["yaw"]; stats[k, 8] = d["spawn_height"]
    out = dict(fb=fb, ep_state=st, ep_stats=stats, done=(reason | flags).astype(np.int64), reset=reset, finite=finite, rzz=rzz, clearance=clr, margin=mar,
               words=sp["words"], row=sp["row"], reset_index=k)
    if prev_ori is not None:
        p = np.asarray(prev_ori, _f).astype(np.float64); p[k] = 0.0
        out["prev_ori"] = p
    if motor_cmd is not None:
        c = np.asarray(motor_cmd, _f).astype(np.float64)
        c[k, 0:12] = sp["fb"][:, 13:25]; c[k, 12:24] = d["kp"]; c[k, 24:36] = 0.0; c[k, 36:48] = d["kd"]; c[k, 48:60] = 0.0
        out["motor_cmd"] = c
    return out


# Base height at which an A1 on the joint PD hold of the default desc (stand pose, kp 100, kd 2) settles on flat ground in the float64 chain of
# body_contact_ref (1 ms ticks of 2 sub-steps, dropped from 0.30): 0.2683, still swinging by +- 0.002 between ticks 300 and 1300
# (test_episode_ref.py runs the chain).  What test_gpu_episode.py's recycled robots must come back to.
STAND_SETTLE_Z = 0.2683


# ---- shared seeded cases (test_episode_host.py checks what test_gpu_episode.py relies on)
GROUND_Z = float(np.float64(_f(-0.02)))          # (params->ground_z is a float)
TABLE = np.array([[-0.8, -0.4, 0.0, 0.4, 0.8, -0.2, 0.6], [-0.5, 0.3, 0.0, -0.3, 0.5, 0.7, -0.6], [0.0, 1.0, -2.0, 3.0, -0.5, 2.5, -3.0], [0.0] * 7], _f)
CASE_DESC = dict(status_ticks=3, tick_mask=0x4, max_ticks=50, seed=20260, align_to_slope=1, field_margin=0.15, xy_jitter=0.1, yaw_jitter=0.3, q_jitter=0.05,
                 v_jitter=0.3)
# what a robot is set up to show; the names that end an episode come first
ENDING = ("status_at", "status_beyond", "tick", "nonfinite", "tilt", "height", "off_near", "off_far", "timeout_at", "timeout_beyond", "forced", "multi",
          "zero_quat_status")
GOING = ("deb_below", "status_unmasked", "timeout_before", "zero_quat", "margin_inside", "tick_unmasked", "height_above", "tilt_below", "unnormalised") + ("none",) * 15
KINDS = ENDING + GOING


def case_ground(pkg):
    """terrain_ref.step_case's two-field stack with its pairwise field ids -> ground(n), the dict this module's functions take"""
    case = TR.step_case(pkg)
    return lambda n: dict(D=case["D"], height=case["height"], fid=((np.arange(n) // 2) % 2).astype(np.int32))


def cases(d, ground, n, seed):
    """n robots, robot i of kind KINDS[i % len(KINDS)]: -> dict fb [n, 37] float32, st [n, 6] int32, stats [n, 9] float32, pstatus, tstatus, force [n]
    int32, kind [n].  The state is healthy (inside the shrunk grid, clearance 0.2 .. 0.4, tilt under 0.5 rad, counters low) except for what
    the kind names."""
    rng = np.random.default_rng(seed)
    U = rng.uniform
    D = ground["D"]
    x1, y1 = D["x0"] + (D["nx"] - 1) * D["cell"], D["y0"] + (D["ny"] - 1) * D["cell"]
    mg = d["field_margin"]
    kind = np.array([KINDS[i % len(KINDS)] for i in range(n)])
    fb = np.zeros((n, 37))
    x, y = U(D["x0"] + mg + 0.05, x1 - mg - 0.05, n), U(D["y0"] + mg + 0.05, y1 - mg - 0.05, n)
    tilt, clr = U(0.0, 0.5, n), U(0.2, 0.4, n)
    st = np.zeros((n, 6), np.int64); st[:, 0] = rng.integers(0, 20, n); st[:, 1] = rng.integers(0, 6, n); st[:, 4] = rng.integers(0, 4, n); st[:, 5] = rng.integers(0, 3, n)
    ps, ts, fr = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    scale = np.ones(n)
    bad_row = np.full(n, -1)
    zero_q = np.zeros(n, bool)
    for i in range(n):
        k = kind[i]
        multi = k == "multi"
        pick = lambda name, p=0.5: k == name or (multi and rng.random() < p)
        if pick("status_at"): ps[i] = PL_TRUNK_CONTACT | PL_KNEE_CONTACT; st[i, 2] = d["status_ticks"] - 1
        if k == "status_beyond": ps[i] = PL_NONFINITE; st[i, 2] = d["status_ticks"] + rng.integers(0, 9)
        if k == "deb_below": ps[i] = PL_TRUNK_CONTACT; st[i, 2] = d["status_ticks"] - 2
        if k == "status_unmasked": ps[i] = PL_KNEE_CONTACT | 0x40; st[i, 2] = d["status_ticks"] - 1
        if pick("tick"): ts[i] = 0x4 | int(rng.integers(0, 4))
        if k == "tick_unmasked": ts[i] = 0x3 | 0x100
        if pick("nonfinite", 0.3): bad_row[i] = i // len(KINDS) % 37
        if pick("tilt"): tilt[i] = U(d["tilt_max"] + 0.02, 3.0)
        if k == "tilt_below": tilt[i] = U(d["tilt_max"] - 0.1, d["tilt_max"] - 0.005)
        if pick("height"): clr[i] = U(-0.05, d["min_clearance"] - 0.002)
        if k == "height_above": clr[i] = U(d["min_clearance"] + 0.001, d["min_clearance"] + 0.02)
        if pick("off_near"):
            side = rng.integers(0, 4); out = rng.random() < 0.5
            e = 1e-3 if out else U(2e-3, mg + 0.3)                     # on the margin line + 1e-3, or beyond it (past the grid's border too)
            if side == 0: x[i] = D["x0"] + mg - e
            if side == 1: x[i] = x1 - mg + e
            if side == 2: y[i] = D["y0"] + mg - e
            if side == 3: y[i] = y1 - mg + e
        if k == "margin_inside":
            side = rng.integers(0, 4)
            if side == 0: x[i] = D["x0"] + mg + 1e-3
            if side == 1: x[i] = x1 - mg - 1e-3
            if side == 2: y[i] = D["y0"] + mg + 1e-3
            if side == 3: y[i] = y1 - mg - 1e-3
        if k == "off_far": x[i], y[i] = rng.choice([-1.0, 1.0], 2) * U(5.0, 1e3, 2)
        if pick("timeout_at"): st[i, 0] = d["max_ticks"] - 1
        if k == "timeout_beyond": st[i, 0] = d["max_ticks"] + rng.integers(0, 5)
        if k == "timeout_before": st[i, 0] = d["max_ticks"] - 2
        if pick("forced"): fr[i] = rng.choice([1, -1, 77])
        if k == "zero_quat": zero_q[i] = True
        if k == "zero_quat_status": zero_q[i] = True; ps[i] = PL_QUAT_ZERO; st[i, 2] = d["status_ticks"] - 1
        if k == "unnormalised" or multi: scale[i] = U(0.3, 3.0)
    # attitude: a rotation by `tilt` about a horizontal axis, then a yaw
    az, yaw = U(-np.pi, np.pi, n), U(-np.pi, np.pi, n)
    qt = np.stack([np.cos(0.5 * tilt), np.sin(0.5 * tilt) * np.cos(az), np.sin(0.5 * tilt) * np.sin(az), np.zeros(n)], 1)
    qy = np.stack([np.cos(0.5 * yaw), np.zeros(n), np.zeros(n), np.sin(0.5 * yaw)], 1)
    q = np.stack([qy[:, 0] * qt[:, 0] - qy[:, 3] * qt[:, 3], qy[:, 0] * qt[:, 1] - qy[:, 3] * qt[:, 2], qy[:, 0] * qt[:, 2] + qy[:, 3] * qt[:, 1],
                  qy[:, 0] * qt[:, 3] + qy[:, 3] * qt[:, 0]], 1)
    fb[:, 0:4] = np.where(zero_q[:, None], 0.0, q * scale[:, None])
    fb[:, 4], fb[:, 5] = x, y
    fid, _ = _field_ids(ground, n)
    x32, y32 = fb[:, 4].astype(_f).astype(np.float64), fb[:, 5].astype(_f).astype(np.float64)
    fb[:, 6] = ground_at(ground, GROUND_Z, fid, x32, y32)[0] + clr
    fb[:, 7:13] = U(-1, 1, (n, 6)); fb[:, 13:25] = d["q_spawn"] + U(-0.3, 0.3, (n, 12)); fb[:, 25:37] = U(-3, 3, (n, 12))
    fb = fb.astype(_f)
    for i in np.nonzero(bad_row >= 0)[0]:
        fb[i, bad_row[i]] = [np.nan, np.inf, -np.inf][i % 3]
    stats = np.zeros((n, 9), _f)
    stats[:, 0:2] = U(-0.8, 0.8, (n, 2)); stats[:, 2] = 0.3; stats[:, 3] = U(-3, 3, n); stats[:, 4] = rng.integers(1, 400, n); stats[:, 5:7] = U(-1, 1, (n, 2))
    stats[:, 7] = U(0.0, 0.3, n); stats[:, 8] = U(0.05, 0.5, n)
    return dict(fb=fb, st=st.astype(np.int32), stats=stats, pstatus=ps.astype(np.int32), tstatus=ts.astype(np.int32), force=fr.astype(np.int32), kind=kind)
