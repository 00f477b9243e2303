"""TEST INFRASTRUCTURE -- the quadruped's rigid-body quantities from classical mechanics, float64 numpy, batched over a leading state axis.

No spatial algebra (no 6-vectors, no Xup): world-frame positions, rotation matrices, angular and linear velocities and accelerations of 25
rigid bodies -- the base, per leg the abad, hip and knee links, per leg three rotors -- and sums over them.  It shares no code and no
formulation with oracle/qr_oracle_fbmodel.cpp (the reference's spatial-vector recursions restated) or with qr_wbc_kernel.hip (per-leg 3-vector
algebra on lumped "effective" bodies): what the three agree on is mechanics, not a restatement.

  state37 = quat_wxyz, pos, omega_body, v_body, q[12], qd[12]      (FBModelState, QS/dynamics/floating_base_model.hpp:29-44)
  nu      = [omega_body, v_body, qd]                                (state37[7:13], state37[25:37]); the quaternion is normalised on entry

Geometry: a child frame sits at `loc` in its parent, turned by the standard rotation about the joint axis (x, y, y); legs FR, FL, RR, RL;
`loc` takes the leg signs (QS/robots/qr_robot.cpp:89-103); the foot is the point (0, +-0.004, -lower_l) of the knee link.

Body data: BuildDynamicModel, QS/robots/qr_robot_a1_sim.cpp:184-254 (qr_robot_lite3_sim.cpp:176-343 is literally identical; only hip_l,
upper_l, lower_l come from the robot's YAML).  Every literal is the float32 the reference holds, widened; products are formed in float64.
  * abad and hip links of legs 0 and 2 are mirrored in y (:284-288, :303-307): c_y, I_xy, I_yz change sign
  * the knee link is mirrored on no leg (:322, the flip is commented out)
  * a rotor is fixed in the parent of its joint's link at its rotor location, has mass float32(1e-8) (:243) and inertia
    float32(1e-2f * 1e-6) * identity (:191-198: setIdentity() overrides 33/33/63) and turns with the joint's qd (gear ratios 1, :267-271)
    about the joint axis; the hip rotor's frame is Rz(pi) of its parent (:300-302), so its axis is the parent's -y.

Jacobians by linearity: the kinematics is evaluated at the 18 unit generalised velocities.
  H = sum m Jv' Jv + Jw' (R I R') Jw          G = -sum m Jv' g,  g = (0, 0, -9.81)
  C = sum Jv' m a_c + Jw' (I_w alpha + w x I_w w),  alpha and a_c at nu_dot = 0 from the classical recursion:
      base:  alpha = 0, a = w x v;   child:  alpha_c = alpha_p + w_p x (axis qd),  a_c = a_p + alpha_p x r + w_p x (w_p x r)
  pGC, vGC, Jc (world-frame linear velocity over nu), Jcdqd: the foot point's position, velocity, velocity map and acceleration at nu_dot = 0.
"""
import numpy as np

_f = np.float32


def _w(x):
    """A float literal as the reference holds it: rounded to float32, widened to float64."""
    return np.asarray(x, _f).astype(np.float64)


# ---- BuildDynamicModel's data (QS/robots/qr_robot_a1_sim.cpp), left-hand bodies as written there
_U = _w(1e-6)                                                                              # `* 1e-6` into a Mat3<float> (:211, :221, :236, :251)
BODY = dict(m=_w(6.0), c=_w([0, 0, 0]), I=_w([[15853, 0, 0], [0, 37799, 0], [0, 0, 45654]]) * _U)                                   # :247-254
ABAD = dict(m=_w(0.696), c=_w([-0.0033, 0, 0]), I=_w([[469.2, -9.4, -0.342], [-9.4, 807.5, -0.466], [-0.342, -0.466, 552.9]]) * _U)  # :206-214
HIP = dict(m=_w(1.013), c=_w([-0.003237, -0.022327, -0.027326]),
           I=_w([[5529, 4.825, 343.9], [4.825, 5139.3, 22.4], [343.9, 22.4, 1367.8]]) * _U)                                         # :216-224
KNEE = dict(m=_w(0.166), c=_w([0.006435, 0, -0.107]), I=_w([[2998, 0, -141.2], [0, 3014, 0], [-141.2, 0, 32.4]]) * _U)               # :231-240
ROTOR_M = _w(1e-8)                                                                         # :243
ROTOR_I = _w(np.float64(_f(1e-2)) * 1e-6) * np.eye(3)                                      # :191-198 (float scale_ times a double literal, stored as float)
ABAD_LOC = _w([0.1805, 0.047, 0.0])                                                        # :185
ABAD_ROTOR_LOC = _w([0.14, 0.047, 0.0])                                                    # :184
HIP_ROTOR_LOC = _w([0.0, 0.04, 0.0])                                                       # :187
KNEE_ROTOR_LOC = _w([0.0, 0.0, 0.0])                                                       # :189
FOOT_Y = _w(0.004)                                                                         # :272
GRAVITY = np.array([0.0, 0.0, -9.81])                                                      # :342 (the oracle and the kernel hold it as double(-9.81))
LEG_SIGNS = ((1.0, -1.0), (1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0))                           # WithLegSigns, FR FL RR RL
AXES = (np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 1.0, 0]))               # abad x, hip y, knee y
HIP_ROTOR_AXIS = np.array([0.0, -1.0, 0.0])                                                # Rz(pi) rotor frame (:300-302)
MIRRORED = (True, False, True, False)                                                      # sideSign < 0 on legs 0 and 2 (:262, :339)
N_BODIES = 25


def _mirror_y(b):
    """The body seen in a y-mirrored frame: c_y, I_xy, I_yz change sign."""
    s = np.array([1.0, -1.0, 1.0])
    return dict(m=b["m"], c=b["c"] * s, I=b["I"] * np.outer(s, s))


def total_mass():
    return BODY["m"] + 4 * (ABAD["m"] + HIP["m"] + KNEE["m"]) + 12 * ROTOR_M


def _rot(axis, th):
    """Standard rotation about x (0) or y (1), batched: [...,3,3]."""
    c, s = np.cos(th), np.sin(th)
    R = np.zeros(np.shape(th) + (3, 3))
    if axis == 0:
        R[..., 0, 0] = 1; R[..., 1, 1] = c; R[..., 1, 2] = -s; R[..., 2, 1] = s; R[..., 2, 2] = c
    else:
        R[..., 1, 1] = 1; R[..., 0, 0] = c; R[..., 0, 2] = s; R[..., 2, 0] = -s; R[..., 2, 2] = c
    return R


def quat_to_rot(q):
    """Body-to-world rotation of a unit quaternion (w, x, y, z), batched."""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _mv(R, v):
    return np.einsum("...ij,...j->...i", R, v)


def bodies(model, quat, pos, q):
    """The 25 bodies placed in the world.  -> list of dicts: parent (index of the frame the body hangs on), joint (nu index of its joint or
    None), R, p (frame), r (p - parent's p), axis (joint axis, world), cw (centre of mass - p, world), m, Iw (inertia about the c.o.m., world);
    feet: list of (knee body index, foot point - knee frame origin, world)."""
    hip_l, upper_l, lower_l = (float(x) for x in np.asarray(model, _f)[:3].astype(np.float64))
    quat = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    Rb = quat_to_rot(quat)
    out, feet = [], []

    def add(parent, joint, Rp, pp, loc, Rrel, axis, body):
        r = _mv(Rp, loc) if parent is not None else np.zeros_like(pos)
        R = Rp @ Rrel if Rrel is not None else Rp
        out.append(dict(parent=parent, joint=joint, R=R, p=pp + r, r=r, axis=None if axis is None else _mv(Rp, axis), cw=_mv(R, body["c"]),
                        m=body["m"], Iw=R @ body["I"] @ np.swapaxes(R, -1, -2)))
        return len(out) - 1

    rotor = dict(m=ROTOR_M, c=np.zeros(3), I=ROTOR_I)
    base = add(None, None, Rb, pos, None, None, None, BODY)
    for leg in range(4):
        sx, sy = LEG_SIGNS[leg]
        sgn = np.array([sx, sy, 1.0])
        mir = MIRRORED[leg]
        th = [q[..., 3 * leg + k] for k in range(3)]
        j = 6 + 3 * leg
        B = out[base]
        abad = add(base, j, B["R"], B["p"], ABAD_LOC * sgn, _rot(0, th[0]), AXES[0], _mirror_y(ABAD) if mir else ABAD)
        add(base, j, B["R"], B["p"], ABAD_ROTOR_LOC * sgn, None, AXES[0], rotor)
        A = out[abad]
        hip = add(abad, j + 1, A["R"], A["p"], np.array([0.0, hip_l, 0.0]) * sgn, _rot(1, th[1]), AXES[1], _mirror_y(HIP) if mir else HIP)
        add(abad, j + 1, A["R"], A["p"], HIP_ROTOR_LOC * sgn, None, HIP_ROTOR_AXIS, rotor)
        Hh = out[hip]
        knee = add(hip, j + 2, Hh["R"], Hh["p"], np.array([0.0, 0.0, -upper_l]), _rot(1, th[2]), AXES[2], KNEE)
        add(hip, j + 2, Hh["R"], Hh["p"], KNEE_ROTOR_LOC, None, AXES[2], rotor)
        feet.append((knee, _mv(out[knee]["R"], np.array([0.0, FOOT_Y if mir else -FOOT_Y, -lower_l]))))
    assert len(out) == N_BODIES
    return out, feet


def velocities(bs, nu):
    """Angular velocity and frame-origin velocity of every body, world frame, for nu [..., 18] (leading axes broadcast against the bodies')."""
    w, v = [], []
    for b in bs:
        if b["parent"] is None:
            w.append(_mv(b["R"], nu[..., 0:3])); v.append(_mv(b["R"], nu[..., 3:6]))
        else:
            wp, vp = w[b["parent"]], v[b["parent"]]
            w.append(wp + b["axis"] * nu[..., b["joint"], None])
            v.append(vp + np.cross(wp, b["r"]))
    return w, v


def bias_accelerations(bs, nu, w, v):
    """Angular acceleration and frame-origin acceleration of every body at nu_dot = 0."""
    al, a = [], []
    for i, b in enumerate(bs):
        if b["parent"] is None:
            al.append(np.zeros_like(w[i])); a.append(np.cross(w[i], v[i]))
        else:
            k = b["parent"]
            al.append(al[k] + np.cross(w[k], b["axis"] * nu[..., b["joint"], None]))
            a.append(a[k] + np.cross(al[k], b["r"]) + np.cross(w[k], np.cross(w[k], b["r"])))
    return al, a


def _expand(bs, feet):
    """The bodies with a unit axis inserted after the state axis (to broadcast against 18 unit velocities)."""
    e = lambda x: None if x is None else x[..., None, :]
    bs2 = [dict(b, R=b["R"][..., None, :, :], r=e(b["r"]), axis=e(b["axis"]), cw=e(b["cw"])) for b in bs]
    return bs2, [(k, e(r)) for k, r in feet]


def compute(model, state37):
    """All seven quantities for state37 [n, 37] (or [37]).  -> dict of H [n,18,18], G [n,18], C [n,18], Jc [n,4,3,18], Jcdqd [n,4,3],
    pGC [n,4,3], vGC [n,4,3], plus T (kinetic energy), V (potential energy), com (centre of mass, world), mass."""
    s = np.asarray(state37, np.float64)
    single = s.ndim == 1
    s = np.atleast_2d(s)
    n = s.shape[0]
    nu = np.concatenate([s[:, 7:13], s[:, 25:37]], axis=1)
    bs, feet = bodies(model, s[:, 0:4], s[:, 4:7], s[:, 13:25])

    # velocity maps: the kinematics at the 18 unit velocities
    bs1, feet1 = _expand(bs, feet)
    wu, vu = velocities(bs1, np.broadcast_to(np.eye(18), (n, 18, 18)))
    Jw = [np.swapaxes(x, -1, -2) for x in wu]                                              # [n,3,18]
    Jv = [np.swapaxes(vu[i] + np.cross(wu[i], bs1[i]["cw"]), -1, -2) for i in range(N_BODIES)]       # c.o.m. velocity over nu

    w, v = velocities(bs, nu)
    al, a = bias_accelerations(bs, nu, w, v)
    H = np.zeros((n, 18, 18)); G = np.zeros((n, 18)); C = np.zeros((n, 18)); V = np.zeros(n); mc = np.zeros((n, 3)); mass = 0.0
    for i, b in enumerate(bs):
        m, Iw, cw = b["m"], b["Iw"], b["cw"]
        H += m * (np.swapaxes(Jv[i], -1, -2) @ Jv[i]) + np.swapaxes(Jw[i], -1, -2) @ Iw @ Jw[i]
        G -= m * _mv(np.swapaxes(Jv[i], -1, -2), GRAVITY)
        ac = a[i] + np.cross(al[i], cw) + np.cross(w[i], np.cross(w[i], cw))
        Iw_w = _mv(Iw, w[i])
        C += m * _mv(np.swapaxes(Jv[i], -1, -2), ac) + _mv(np.swapaxes(Jw[i], -1, -2), _mv(Iw, al[i]) + np.cross(w[i], Iw_w))
        V += m * 9.81 * (b["p"] + cw)[:, 2]
        mc += m * (b["p"] + cw); mass = mass + m
    Jc = np.zeros((n, 4, 3, 18)); Jcd = np.zeros((n, 4, 3)); p = np.zeros((n, 4, 3)); vf = np.zeros((n, 4, 3))
    for leg, (k, r) in enumerate(feet):
        p[:, leg] = bs[k]["p"] + r
        vf[:, leg] = v[k] + np.cross(w[k], r)
        Jcd[:, leg] = a[k] + np.cross(al[k], r) + np.cross(w[k], np.cross(w[k], r))
        Jc[:, leg] = np.swapaxes(vu[k] + np.cross(wu[k], feet1[leg][1]), -1, -2)
    T = 0.5 * np.einsum("ni,nij,nj->n", nu, H, nu)
    out = dict(H=H, G=G, C=C, Jc=Jc, Jcdqd=Jcd, pGC=p, vGC=vf, T=T, V=V, com=mc / mass, mass=mass)
    if single:
        out = {k: (x[0] if isinstance(x, np.ndarray) and x.ndim and x.shape[0] == n else x) for k, x in out.items()}
    return out


QUANTITIES = ("H", "G", "C", "Jc", "Jcdqd", "pGC", "vGC")


# ---- state families (seeded; shared by the CPU and the GPU file)
def wide_states(n, seed):
    """Far from the stand pose: attitude uniform on S^3 (w < 0 occurs), pos in +-1 with z in 0.1..0.6, omega_body in +-4, v_body in +-2,
    abad in +-1, hip in -1..2.5, knee in -2.6..-0.3, qd in +-15.  -> float64 [n, 37], unit quaternion."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 37))
    q = rng.normal(size=(n, 4))
    s[:, 0:4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    s[:, 4:6] = rng.uniform(-1, 1, (n, 2)); s[:, 6] = rng.uniform(0.1, 0.6, n)
    s[:, 7:10] = rng.uniform(-4, 4, (n, 3)); s[:, 10:13] = rng.uniform(-2, 2, (n, 3))
    s[:, 13:25:3] = rng.uniform(-1, 1, (n, 4)); s[:, 14:25:3] = rng.uniform(-1, 2.5, (n, 4)); s[:, 15:25:3] = rng.uniform(-2.6, -0.3, (n, 4))
    s[:, 25:37] = rng.uniform(-15, 15, (n, 12))
    return s


STAND_POSE = np.tile(np.array([0.0, 0.8, -1.6]), 4)
REST_EDGES = (0, 1, 2)            # edge_states() rows at rest
UNIT_EDGES = range(5, 23)         # edge_states() rows with nu = e_k, k = row - 5
NEG_PAIR = (3, 4)                 # a wide state and the same with the quaternion negated


def edge_states(seed):
    """identity attitude at rest at the stand pose; the same with straight legs; attitude (0,1,0,0) at rest at the stand pose; a wide state and
    the same with the quaternion negated; 18 states at an asymmetric pose (abad 0.3) with nu = e_k.  -> float64 [23, 37]"""
    s = np.zeros((23, 37))
    s[:, 0] = 1.0; s[:, 6] = 0.3; s[:, 13:25] = STAND_POSE
    s[1, 13:25] = 0.0
    s[2, 0:4] = (0, 1, 0, 0)
    s[3] = wide_states(1, seed)[0]
    if s[3, 0] < 0:
        s[3, 0:4] *= -1
    s[4] = s[3]; s[4, 0:4] *= -1
    rng = np.random.default_rng(seed + 1)
    pose = STAND_POSE + rng.uniform(-0.2, 0.2, 12); pose[0::3] = 0.3
    q = rng.normal(size=4)
    for k in range(18):
        s[5 + k, 0:4] = q / np.linalg.norm(q)
        s[5 + k, 13:25] = pose
        s[5 + k, 7 + k if k < 6 else 25 + k - 6] = 1.0
    return s


N_STAND, N_WIDE = 48, 48
SEEDS = dict(a1=dict(stand=7301, wide=7302, edge=7303), lite3=dict(stand=7311, wide=7312, edge=7313))


def families(pkg, robot):
    """The three state families of one robot as the float32 rows a device is given: dict stand [48,37], wide [48,37], edge [23,37]."""
    sd = SEEDS[robot]
    return dict(stand=pkg.make_batch(N_STAND, 10, robot, seed=sd["stand"])["fb_state"].copy(),
                wide=wide_states(N_WIDE, sd["wide"]).astype(_f), edge=edge_states(sd["edge"]).astype(_f))


def normalised(state32):
    """float32 rows widened, the quaternion normalised in float64."""
    s = np.asarray(state32, np.float64).copy()
    s[..., 0:4] /= np.linalg.norm(s[..., 0:4], axis=-1, keepdims=True)
    return s


# ---- WBC cases off the stand pose
FORCED = {0: (0, 0, 0, 0), 1: (0, 1, 0, 0), 2: (0, 0, 0, 0), 3: (0, 1, 0, 0)}     # row of a family -> forced contact pattern
PERTURB, AMPLIFICATION_MAX = 1e-12, 1e6


def amplification(oracle, model, s32, c32, p32, seed):
    """How much the float64 WBC tick amplifies a 1e-12 relative perturbation of state and command into tau, relative to max(1,|tau|);
    -> (rc, amplification).  The contact flags are left alone."""
    w = oracle.wbc_run(model, s32.astype(np.float64), c32.astype(np.float64), p32.astype(np.float64), dtype=np.float64)
    if w["rc"] != 0:
        return w["rc"], np.inf
    rng = np.random.default_rng(seed)
    s = s32.astype(np.float64) * (1 + PERTURB * rng.choice([-1.0, 1.0], 37))
    c = c32.astype(np.float64); c[:63] *= 1 + PERTURB * rng.choice([-1.0, 1.0], 63)
    w2 = oracle.wbc_run(model, s, c, p32.astype(np.float64), dtype=np.float64)
    if w2["rc"] != 0:
        return w2["rc"], np.inf
    return 0, float((np.abs(w2["tau"] - w["tau"]) / np.maximum(1.0, np.abs(w["tau"]))).max() / PERTURB)


_wbc_cache = {}


def wbc_cases(pkg, oracle, robot):
    """The stand and wide families with a WBC command each: wbc_cmd and prev_ori_vel are make_batch's (of the stand family's batch, row for
    row), rows 0-3 of each family get the contact patterns of FORCED with matching Fr_des.  A state on which the float64 oracle fails (rc != 0)
    or amplifies a 1e-12 perturbation by 1e6 or more is redrawn by seed (a wide state from wide_states, a stand state from make_batch) here, at
    generation; every state returned is compared.  -> dict state [96,37], cmd [96,67], prev [96,3] float32, amp [96], redrawn (count).
    Computed once per robot and shared (callers must not modify it)."""
    if robot in _wbc_cache:
        return _wbc_cache[robot]
    md = pkg.model_desc(robot)
    sd = SEEDS[robot]
    b = pkg.make_batch(N_STAND, 10, robot, seed=sd["stand"])
    fam = families(pkg, robot)
    state = np.concatenate([fam["stand"], fam["wide"]]); cmd = np.concatenate([b["wbc_cmd"], b["wbc_cmd"]]).copy()
    prev = np.concatenate([b["prev_ori_vel"], b["prev_ori_vel"]]).copy()
    for base in (0, N_STAND):
        for row, pat in FORCED.items():
            cmd[base + row, 63:67] = pat
            cmd[base + row, 51:63] = (np.array(pat, _f)[:, None] * np.array([1.0, -2.0, 30.0], _f)).reshape(12)
    amp = np.zeros(len(state)); redrawn = 0
    for i in range(len(state)):
        for attempt in range(1, 21):
            rc, amp[i] = amplification(oracle, md, state[i], cmd[i], prev[i], 100 + i)
            if rc == 0 and amp[i] < AMPLIFICATION_MAX:
                break
            redrawn += 1
            seed = sd["wide"] + 1000 * attempt + i
            state[i] = wide_states(1, seed)[0].astype(_f) if i >= N_STAND else pkg.make_batch(1, 10, robot, seed=seed)["fb_state"][0]
        else:
            raise AssertionError("no well-conditioned state found for row %d of %s" % (i, robot))
    _wbc_cache[robot] = dict(state=state, cmd=cmd, prev=prev, amp=amp, redrawn=redrawn)
    return _wbc_cache[robot]


# ---- the mixed batch of the kernel test (tests/test_gpu_rigid_body.py) and of the host build of its chains (tests/test_wbc_rigid_body_host.py)
MIXED_ROBOTS = ("a1", "lite3")       # type 0, type 1
# the project's bars, each times max(1, max|ref|)
BARS = (("H", 2e-6), ("G", 2e-5), ("C", 2e-6), ("Jc", 1e-6), ("Jcdqd", 2e-5), ("pGC", 1e-6), ("vGC", 1e-6))


def interleave(rows_a1, rows_lite3):
    """A1 rows at even places, Lite3 rows at odd ones (A1 may have one more)."""
    na, nl = len(rows_a1), len(rows_lite3)
    assert na in (nl, nl + 1)
    out = np.empty((na + nl,) + rows_a1.shape[1:], rows_a1.dtype)
    out[0::2] = rows_a1; out[1::2] = rows_lite3
    return out


_mixed_cache = {}


def mixed_batch(pkg, oracle):
    """One mixed batch, A1 = type 0 and Lite3 = type 1 interleaved through type_id, each robot with the stand (make_batch), wide and edge
    families; n = 239 is odd and above 64.  With it the float64 oracle on the same raw float32 rows and the model on the normalised ones.
    -> dict n, state [n,37] float32, tid, family[i] / row[i] (which family robot i's state is from and its row there), oracle, model.
    Computed once and shared (callers must not modify it)."""
    if _mixed_cache:
        return _mixed_cache
    states, family, row = {}, {}, {}
    for robot in MIXED_ROBOTS:
        f = families(pkg, robot)
        if robot == "a1":          # one more stand state: n odd
            f["stand"] = np.concatenate([f["stand"], pkg.make_batch(1, 10, "a1", seed=SEEDS["a1"]["stand"] + 1)["fb_state"]])
        states[robot] = np.concatenate([f["stand"], f["wide"], f["edge"]])
        family[robot] = np.array(sum(([k] * len(f[k]) for k in ("stand", "wide", "edge")), []))
        row[robot] = np.concatenate([np.arange(len(f[k])) for k in ("stand", "wide", "edge")])
    st = interleave(states["a1"], states["lite3"])
    n = len(st)
    assert n == 239 and n % 2 == 1 and n > 64
    tid = pkg.shard.interleave_types(n, 2)
    shapes = dict(H=(n, 18, 18), G=(n, 18), C=(n, 18), Jc=(n, 4, 3, 18), Jcdqd=(n, 4, 3), pGC=(n, 4, 3), vGC=(n, 4, 3))
    ora = {k: np.zeros(shapes[k]) for k, _ in BARS}
    for i in range(n):
        o = oracle.fb_compute(pkg.model_desc(MIXED_ROBOTS[tid[i]]), st[i].astype(np.float64), np.float64)
        for k, _ in BARS:
            ora[k][i] = o[k]
    model = {k: np.zeros(shapes[k]) for k in ("H", "C")}
    for t, robot in enumerate(MIXED_ROBOTS):
        r = compute(pkg.model_desc(robot), normalised(st[t::2]))
        for k in model:
            model[k][t::2] = r[k]
    _mixed_cache.update(n=n, state=st, tid=tid, oracle=ora, model=model, family=interleave(family["a1"], family["lite3"]),
                        row=interleave(row["a1"], row["lite3"]))
    return _mixed_cache


def rel(got, ref):
    """Per robot: max|got - ref| / max(1, max|ref|)."""
    n = len(ref)
    return np.abs(got - ref).reshape(n, -1).max(1) / np.maximum(1.0, np.abs(ref).reshape(n, -1).max(1))


def edge_index(mb, t, r):
    """The robot of type t that holds row r of its edge family."""
    i = np.nonzero((mb["tid"] == t) & (mb["family"] == "edge") & (mb["row"] == r))[0]
    assert len(i) == 1
    return int(i[0])
