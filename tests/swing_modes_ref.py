"""CPU restatement of the swing-leg controller of the walk and position modes and of the lift-off memory of all four modes, numpy float32
operation by operation, following the reference line by line:
  qrRaibertSwingLegController::Reset / Update / GetAction   quadruped/src/controllers/qr_swing_leg_controller.cpp:60-101, 104-229, 241-461
  qrFootholdPlanner::Reset / UpdateOnce                      quadruped/src/planner/qr_foothold_planner.cpp:49-109
  qrFootStepper                                              quadruped/src/planner/qr_foot_stepper.cpp:31-202, 483-525
  qrFootBSplinePatternGenerator, tinynurbs                   quadruped/src/controllers/qr_foot_trajectory_generator.cpp:30-163, 276-343
The unqualified abs on floats (UpdateSpline :100/:105/:123, SwingFootTrajectory :298, StepGenerator :150) is read as std::abs(float),
as in the kernels.  State rows, flags and outputs are those of include/qrgpu.h (qrgpu_swing_update_batch / qrgpu_swing_action_batch)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
MAXIMUM_STEP = f32(0.001)
MAX_PLAN = 32
STATE_FLOATS = 105 + 4 * MAX_PLAN
OUT_ROWS = 52
SS_LOCAL, SS_GLOBAL, SS_FH, SS_SRC, SS_TGT, SS_H, SS_BUILT, SS_QANG, SS_QVEL, SS_MAP = 0, 12, 24, 36, 48, 60, 64, 65, 77, 89
SS_OFF, SS_PFLAGS, SS_HEAD, SS_TAIL, SS_PLAN = 90, 102, 103, 104, 105
SW_NO_TRAJ, SW_PHASE, SW_PLAN_EXIT, SW_PLAN_EMPTY, SW_PLAN_FULL = 1, 2, 4, 8, 16
KNOTS = np.array([0, 0, 0, 0, 0.3 / 6, 1.3 / 6, 2.5 / 6, 3.0 / 6, 4.0 / 6, 1, 1, 1, 1], f32)
TX = np.array([-10, -10.3, -13, -15, 0, 11, 10.5, 10.2, 10], f32)
TZ = np.array([0, 0.2, 2, 7, 7.8, 8, 4, 1, 0], f32)
EPS_F = f32(np.finfo(np.float32).eps)


class Desc:
    """qrgpu_swing_mode_desc (and qrgpu_swing_mode_desc_default for config/a1_sim)."""
    def __init__(self, mode, terrain=None, is_sim=1, foothold_delta=0.10, gaps=None, gap_width=0.14):
        self.mode = mode
        self.terrain = terrain if terrain is not None else (1 if mode == 1 else 2 if mode == 3 else 3)
        self.is_sim = is_sim
        self.delta = f32(foothold_delta)
        if gaps is None:
            gaps = (0.51, 1.31, 1.91) if mode == 1 else ()
        self.gaps = [f32(g) for g in gaps] if self.terrain == 1 else []
        self.gap_width = f32(gap_width)


# ---- small float32 helpers (contraction off: every product and sum rounded) ------------------------------------------------------------
def quat_to_rot(w, x, y, z):
    """Eigen::Quaternion<float>::toRotationMatrix"""
    w, x, y, z = f32(w), f32(x), f32(y), f32(z)
    tx, ty, tz = f32(2) * x, f32(2) * y, f32(2) * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[f32(1) - (tyy + tzz), txy - twz, txz + twy], [txy + twz, f32(1) - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, f32(1) - (txx + tyy)]]


def base_rmat(q):
    """stateDataFlow.baseRMat = quaternionToRotationMatrix(q)^T (qr_se3.h:186-203, qr_robot.cpp:70)"""
    e0, e1, e2, e3 = (f32(v) for v in q)
    o, t = f32(1), f32(2)
    return [[o - t * (e2 * e2 + e3 * e3), t * (e1 * e2 - e0 * e3), t * (e1 * e3 + e0 * e2)],
            [t * (e1 * e2 + e0 * e3), o - t * (e1 * e1 + e3 * e3), t * (e2 * e3 - e0 * e1)],
            [t * (e1 * e3 - e0 * e2), t * (e2 * e3 + e0 * e1), o - t * (e1 * e1 + e2 * e2)]]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def world_point(q, bp, p):
    """invertRigidTransform(basePosition, q, p) (qr_se3.h:440-449)"""
    R = quat_to_rot(*q)
    return [dot3(R[r], p) + f32(bp[r]) for r in range(3)]


def rigid_transform(q, t, p):
    """RigidTransform(t, q, p) = q^-1 p + q^-1 (-t) (qr_se3.h:459-466)"""
    q = [f32(v) for v in q]
    n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])
    Ri = quat_to_rot(q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)
    mt = [-f32(v) for v in t]
    return [dot3(Ri[r], p) + dot3(Ri[r], mt) for r in range(3)]


def warp_phase(ph):
    ph = f32(ph)
    if ph <= f32(0.5):
        return f32(0.8 * math.sin(f64(ph) * math.pi))
    return f32(0.8 + (f64(ph) - 0.5) * 0.4)


def parabola_point(phase, st, tg):
    """qrFootParabolaPatternGenerator, height 0.1 (qr_foot_trajectory_generator.cpp:187-215, qr_geometry.cpp:157-190)"""
    pw = [f32(0)] * 3
    phase = f32(phase)
    if not (f64(phase) < -1e-3) and not (f64(phase) >= 1.0 + 1e-3):
        one = f32(1)
        pw[0] = (one - phase) * st[0] + phase * tg[0]
        pw[1] = (one - phase) * st[1] + phase * tg[1]
        mid = (tg[2] if tg[2] > st[2] else st[2]) + f32(0.1)
        if not (phase < 0):
            d1, d2 = mid - st[2], tg[2] - st[2]
            d3 = f32(0.25 - 0.5)
            ca = (d1 - d2 * f32(0.5)) / d3
            cb = f32((f64(d2) * 0.25 - f64(d1)) / f64(d3))
            pw[2] = f32(f64(ca) * (f64(phase) * f64(phase)) + f64(cb * phase) + f64(st[2]))
    return pw


def leg_ik(p, ho, sh, lu, ll):
    """qrRobot::FootPositionInHipFrameToJointAngle (qr_robot.cpp:106-124)"""
    x, y, z = p[0] - ho[0], p[1] - ho[1], p[2] - ho[2]
    with np.errstate(invalid="ignore"):
        tK = -f32(np.arccos(((x * x + y * y + z * z) - (sh * sh + lu * lu + ll * ll)) / (f32(2) * ll * lu)))
        l = f32(np.sqrt(lu * lu + ll * ll + f32(2) * lu * ll * f32(np.cos(tK))))
        tH = f32(np.arcsin(-x / l)) - tK / f32(2)
        c1 = sh * y - l * f32(np.cos(tH + tK / f32(2))) * z
        s1 = l * f32(np.cos(tH + tK / f32(2))) * y + sh * z
        return [f32(np.arctan2(s1, c1)), tH, tK]


def jacobian_inverse(ang, sh, lu, ll):
    """AnalyticalLegJacobian(...).inverse() (qr_robot.cpp:148-172): adjugate / determinant"""
    t0, t1, t2 = ang
    with np.errstate(invalid="ignore", divide="ignore"):
        lE = f32(np.sqrt(lu * lu + ll * ll + f32(2) * lu * ll * f32(np.cos(t2))))
        tE = t1 + t2 / f32(2)
        s0, c0, sE, cE, s2 = (f32(np.sin(t0)), f32(np.cos(t0)), f32(np.sin(tE)), f32(np.cos(tE)), f32(np.sin(t2)))
        J = [[f32(0), -lE * cE, ll * lu * s2 * sE / lE - lE * cE / f32(2)],
             [-sh * s0 + lE * c0 * cE, -lE * s0 * sE, -ll * lu * s0 * s2 * cE / lE - lE * s0 * sE / f32(2)],
             [sh * c0 + lE * s0 * cE, lE * sE * c0, ll * lu * s2 * c0 * cE / lE + lE * sE * c0 / f32(2)]]
        det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0])
        i = f32(1) / det
        return [[(J[1][1] * J[2][2] - J[1][2] * J[2][1]) * i, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * i, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * i],
                [(J[1][2] * J[2][0] - J[1][0] * J[2][2]) * i, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * i, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * i],
                [(J[1][0] * J[2][1] - J[1][1] * J[2][0]) * i, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * i, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * i]]


# ---- B-spline (SwingFootTrajectory BSpline, qrFootBSplinePatternGenerator, tinynurbs) ----------------------------------------------------
def bspline_height(src, tgt):
    """std::min(0.2f, std::max(0.1f, 0.15 + |dz|)) (:298)"""
    lo = f32(0.15) + f32(abs(f32(tgt[2]) - f32(src[2])))
    mx = lo if f32(0.1) < lo else f32(0.1)
    return mx if mx < f32(0.2) else f32(0.2)


def bspline_control_points(src, tgt, height):
    """SetParameters + UpdateSpline (:53-135): RTheta's (c, s) and the control points (x, z; y is zero) in cm."""
    src = [f32(v) for v in src]; tgt = [f32(v) for v in tgt]
    dx, dy, dz = tgt[0] - src[0], tgt[1] - src[1], tgt[2] - src[2]
    th = f32(np.arctan2(dy, dx))
    s, c = f32(np.sin(th)), f32(np.cos(th))
    h100 = f32(100)
    e0 = (c * (dx * h100) + s * (dy * h100)) + f32(0) * (dz * h100)
    e2 = (f32(0) * (dx * h100) + f32(0) * (dy * h100)) + f32(1) * (dz * h100)
    appex = f32(height) * h100
    xr = f32(abs(e0 - f32(0))) / f32(20)
    zr8 = f32(abs(appex)) / f32(8)
    xm = (e0 + f32(0)) / f32(2)
    if e2 >= 0:
        zright = appex - (e2 - f32(0))
        cx = TX * xr + xm; cz = TZ * zr8 + f32(0)
        cz[8] = e2
        for k in (7, 6, 5):
            cz[k] = cz[8] + TZ[k] / f32(8) * zright
    else:
        zleft = appex - (f32(0) - e2)
        cx = TX * xr + xm; cz = TZ * zr8 + e2
        cz[0] = f32(0)
        cz[1] = f32(f64(cz[0]) + 0.2 / 8 * f64(zleft))
        cz[2] = f32(f64(cz[0]) + 2.0 / 8 * f64(zleft))
        cz[3] = f32(f64(cz[0]) + 7.0 / 8 * f64(zleft))
    return c, s, cx.astype(f32), cz.astype(f32)


def find_span(u):
    u = f32(u)
    if u > KNOTS[9] - EPS_F:
        return 8
    if u < KNOTS[3] + EPS_F:
        return 3
    low, high = 3, 9
    mid = (low + high) // 2
    while u < KNOTS[mid] or u >= KNOTS[mid + 1]:
        if u < KNOTS[mid]:
            high = mid
        else:
            low = mid
        mid = (low + high) // 2
    return mid


def der_basis(span, u):
    """tinynurbs bsplineDerBasis (basis.h:163-240), degree 3, one derivative, float"""
    u = f32(u); deg = 3
    left = [f32(0)] * 4; right = [f32(0)] * 4
    ndu = [[f32(0)] * 4 for _ in range(4)]
    ndu[0][0] = f32(1)
    for j in range(1, deg + 1):
        left[j] = u - KNOTS[span + 1 - j]
        right[j] = KNOTS[span + j] - u
        saved = f32(0)
        for r in range(j):
            ndu[j][r] = right[r + 1] + left[j - r]
            temp = ndu[r][j - 1] / ndu[j][r]
            ndu[r][j] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        ndu[j][j] = saved
    d0 = [ndu[j][deg] for j in range(4)]
    d1 = []
    for r in range(4):
        d = f32(0)
        rk, pk = r - 1, deg - 1
        if r >= 1:
            a = f32(1) / ndu[pk + 1][rk]; d = a * ndu[rk][pk]
        if r <= pk:
            a = -f32(1) / ndu[pk + 1][r]; d = d + a * ndu[r][pk]
        d1.append(d * f32(3))
    return d0, d1


def bspline_point(src, tgt, height, u):
    """GenerateTrajectory (:138-163) at u: position and d/du, RThetaᵀ p / 100 + Tp."""
    return bspline_eval(bspline_control_points(src, tgt, height), src, u)


def bspline_eval(ctrl, src, u):
    """bspline_point with the control points of SetParameters already made: ctrl = bspline_control_points(src, tgt, height)."""
    c, s, cx, cz = ctrl
    span = find_span(u)
    d0, d1 = der_basis(span, u)
    px = pz = vx = vz = f32(0)
    for j in range(4):
        k = span - 3 + j
        px = px + d0[j] * cx[k]; pz = pz + d0[j] * cz[k]
        vx = vx + d1[j] * cx[k]; vz = vz + d1[j] * cz[k]
    h = f32(100)
    px, pz, vx, vz = px / h, pz / h, vx / h, vz / h
    z = f32(0)
    pos = [((c * px + -s * z) + z * pz) + f32(src[0]), ((s * px + c * z) + z * pz) + f32(src[1]), ((z * px + z * z) + f32(1) * pz) + f32(src[2])]
    vel = [(c * vx + -s * z) + z * vz, (s * vx + c * z) + z * vz, (z * vx + z * z) + f32(1) * vz]
    return pos, vel


# ---- qrFootStepper ----------------------------------------------------------------------------------------------------------------------
def quadprog_1d(ci, ci0):
    """QuadProg++ solve_quadprog for n = 1, G = 1, g0 = 0 and inequalities ci[k] x + ci0[k] >= 0 (ci = +-1), step for step."""
    x = -0.0
    act = -1
    for _ in range(12):
        s = []
        psi = 0.0
        for k in range(6):
            v = 0.0; v += ci[k] * x; v += ci0[k]
            s.append(v); psi += min(0.0, v)
        if abs(psi) <= 6 * np.finfo(float).eps * 1.0 * 1.0 * 100.0:
            return x, True
        ss, ip = 0.0, 0
        for k in range(6):
            if s[k] < ss and k != act:
                ss, ip = s[k], k
        if ss >= 0.0:
            return x, True
        if act >= 0:
            r = (0.0 + 1.0 * ci[ip]) / (0.0 + 1.0 * ci[act])
            if not r > 0.0:
                return x, False
            act = -1
        z = 0.0 + 1.0 * (0.0 + 1.0 * ci[ip])
        t2 = -s[ip] / (0.0 + z * ci[ip])
        if t2 < 0:
            return x, False
        x += t2 * z
        act = ip
    return x, True


def check_solution_layout(delta, cx, front, back, fg, bg, gw):
    """CheckSolution's CI and b (:85-99)"""
    delta = f32(delta)
    ci = [1.0, float(front), float(front), float(back), float(back), -1.0]
    b = [0.0] * 6
    b[0] = -f64(delta)
    b[5] = -1.0 * f64(MAXIMUM_STEP - delta)
    for i in range(1, 5):
        gd = f64(f32(fg if i <= 2 else bg))
        b[i] = -ci[i] * (f64(delta) - (gd + f64(f32(gw)) / 2.0 * ci[i]) + f64(f32(cx[i - 1])))
    return ci, b


def check_solution(delta, cx, front, back, fg, bg, gw):
    ci, b = check_solution_layout(delta, cx, front, back, fg, bg, gw)
    x, _ = quadprog_1d(ci, [-v for v in b])
    for i in range(6):
        if int(x * ci[i] * 10000) < int(b[i] * 10000):
            return f64(MAXIMUM_STEP)
    return x


def step_generator(d, cx, pf):
    """StepGenerator (:118-179) -> (flag, desiredFootholdsOffset[4], planner flags)"""
    delta = d.delta
    dn = [f32(cx[l]) + delta for l in range(4)]
    des = [delta] * 4
    ng = len(d.gaps)
    for g in range(ng):
        gd, gw = d.gaps[g], d.gap_width
        fd = bd = gd
        if g > 0: bd = d.gaps[g - 1]
        if g < ng - 1: fd = d.gaps[g + 1]
        dX = MAXIMUM_STEP
        for l in range(4):
            if f32(abs(dn[l] - gd)) <= gw / f32(2):
                if l <= 1: fd = gd
                else: bd = gd
                for i in (-1, 1):
                    for j in (-1, 1):
                        x = f32(check_solution(delta, cx, i, j, fd, bd, gw))
                        dX = x if abs(x) < abs(dX) else dX
                step = delta + dX
                des = [step] * 4
                if f64(step) < 0.001 or step >= MAXIMUM_STEP:
                    if pf & 2:
                        return -2, des, pf
                    return -1, des, pf | 2
                return 0, des, pf
    if pf & 2:
        for gd in d.gaps:
            w2 = f64(d.gap_width / f32(2))
            if abs(f64(cx[0]) + f64(delta) / 2.0 - f64(gd)) <= w2 or abs(f64(cx[3]) + f64(delta) / 2.0 - f64(gd)) <= w2:
                return 0, des, pf
        h = f32(f64(delta) / 2.0)
        des = [h, delta, delta, h]
        pf &= ~2
    return 0, des, pf


def optimal_offsets(d, st, flags):
    """GetOptimalFootholdsOffset (:483-525) on the state's plan queue -> (row 0 of the offsets, flags)"""
    off0 = [d.delta] * 4
    if not d.gaps:
        return off0, flags
    clamp = lambda v, hi: int(min(max(v, f32(0)), f32(hi))) if v == v else 0      # fminf(fmaxf(v, 0), hi): NaN -> 0
    pf = clamp(st[SS_PFLAGS], 3)
    tail = clamp(st[SS_TAIL], MAX_PLAN)
    head = clamp(st[SS_HEAD], tail)
    if not pf & 1:
        head = tail = 0
        cx = [f32(st[SS_FH + 3 * k]) for k in range(4)]
        last = d.gaps[-1]
        while f64(cx[3]) < f64(last) + f64(d.gap_width) / 2.0:
            fl, des, pf = step_generator(d, cx, pf)
            if fl == -2:
                flags |= SW_PLAN_EXIT; break
            if fl == -1:
                if tail > head:
                    for k in (0, 3):
                        st[SS_PLAN + 4 * (tail - 1) + k] = f32(f64(st[SS_PLAN + 4 * (tail - 1) + k]) + f64(d.delta) / 2.0)
                else:
                    flags |= SW_PLAN_EMPTY
                for k in (0, 3):
                    cx[k] = f32(f64(cx[k]) + f64(d.delta) / 2.0)
            else:
                if tail >= MAX_PLAN:
                    flags |= SW_PLAN_FULL; break
                for k in range(4):
                    st[SS_PLAN + 4 * tail + k] = des[k]; cx[k] = cx[k] + des[k]
                tail += 1
        pf |= 1
    if tail > head:
        off0 = [f32(st[SS_PLAN + 4 * head + k]) for k in range(4)]
        head += 1
    st[SS_PFLAGS], st[SS_HEAD], st[SS_TAIL] = pf, head, tail
    return off0, flags


# ---- the two calls, one robot ----------------------------------------------------------------------------------------------------------
def swing_update(d, reset, stop, est_in, est_out, gait_out, st, flags, swing_in=None, swing_vel_in=None, fe_in=None):
    """qrgpu_swing_update_batch for one robot: est_in[54], est_out[42], gait_out (walk [41] or open-loop [24]); st[STATE_FLOATS] float32 is
    updated in place; swing_in / swing_vel_in / fe_in (one robot's columns) likewise.  Returns the flags word."""
    q = [f32(v) for v in est_in[6:10]]
    bp = [f32(v) for v in est_out[36:39]]
    loc = [[f32(est_out[12 + 3 * l + r]) for r in range(3)] for l in range(4)]
    wld = [world_point(q, bp, loc[l]) for l in range(4)]
    side = d.mode in (0, 3)
    if reset:
        flags = 0
        for l in range(4):
            for r in range(3):
                st[SS_LOCAL + 3 * l + r] = loc[l][r]; st[SS_GLOBAL + 3 * l + r] = wld[l][r]
                if d.mode == 1:
                    st[SS_FH + 3 * l + r] = f32(f64(wld[l][r]) - 0.05) if (r == 0 and l in (0, 3)) else wld[l][r]
                elif d.mode == 2:
                    st[SS_FH + 3 * l + r] = wld[l][r]
                elif reset == 2:
                    st[SS_FH + 3 * l + r] = 0
                st[SS_OFF + 3 * l + r] = 0
                if side and swing_in is not None: swing_in[12 + 3 * l + r] = wld[l][r]
                if side and swing_vel_in is not None: swing_vel_in[8 + 3 * l + r] = loc[l][r]
        if side and fe_in is not None: fe_in[62], fe_in[63] = bp[0], bp[1]
        st[SS_MAP] = 0
        if reset == 2:
            st[SS_BUILT] = st[SS_PFLAGS] = st[SS_HEAD] = st[SS_TAIL] = 0
    Rb = base_rmat(q)
    built = int(st[SS_BUILT])
    for l in range(4):
        nst, cur = int(gait_out[8 + l]), int(gait_out[16 + l])
        if d.mode == 1: lift = nst in (0, 4) and cur == 1 and not stop
        elif d.mode == 2: lift = nst in (8, 4) and cur == 6 and not stop
        else: lift = nst == 0 and nst != cur
        if not lift:
            continue
        st[SS_LOCAL + 3 * l:SS_LOCAL + 3 * l + 3] = loc[l]
        if side:
            g = [dot3(Rb[r], loc[l]) for r in range(3)]
            st[SS_GLOBAL + 3 * l:SS_GLOBAL + 3 * l + 3] = g
            if swing_in is not None: swing_in[12 + 3 * l:15 + 3 * l] = g
            if swing_vel_in is not None: swing_vel_in[8 + 3 * l:11 + 3 * l] = loc[l]
            if d.mode == 3 and fe_in is not None: fe_in[62], fe_in[63] = bp[0], bp[1]
            continue
        st[SS_GLOBAL + 3 * l:SS_GLOBAL + 3 * l + 3] = wld[l]
        if d.mode == 2 or l == 0:
            off0 = [d.delta] * 4
            if d.terrain == 2:
                if d.mode == 2: st[SS_FH + 3 * l] = f32(st[SS_FH + 3 * l]) + f32(0.1)
            elif d.gaps:
                off0, flags = optimal_offsets(d, st, flags)
            for k in range(4):
                st[SS_OFF + 3 * k] = off0[k]; st[SS_OFF + 3 * k + 1] = 0; st[SS_OFF + 3 * k + 2] = 0
        if d.mode == 1:
            for r in range(3):
                st[SS_FH + 3 * l + r] = f32(st[SS_FH + 3 * l + r]) + f32(st[SS_OFF + 3 * l + r])
        else:
            if d.is_sim:
                src = list(wld[l]); tgt = [f32(st[SS_FH + 3 * l + r]) for r in range(3)]
                tgt[2] = src[2] + f32(st[SS_OFF + 3 * l + 2])
            else:
                src = list(loc[l])
                tgt = [f32(0.30) if l <= 1 else f32(-0.17), f32(-0.145 * (-1.0) ** l), f32(-0.32)]
            st[SS_SRC + 3 * l:SS_SRC + 3 * l + 3] = src
            st[SS_TGT + 3 * l:SS_TGT + 3 * l + 3] = tgt
            st[SS_H + l] = bspline_height(src, tgt)
            built |= 1 << l
    st[SS_BUILT] = built
    return flags


def swing_action(d, geom, stop, est_in, est_out, gait_out, gait_state, st, out, flags):
    """qrgpu_swing_action_batch for one robot; geom = workload.estimator_cfg().  out[OUT_ROWS] is written as the kernel writes it."""
    q = [f32(v) for v in est_in[6:10]]
    bp = [f32(v) for v in est_out[36:39]]
    hl, lu, ll = f32(geom[0]), f32(geom[1]), f32(geom[2])
    ho = np.asarray(geom[7:19], f32)
    mp = int(st[SS_MAP]); built = int(st[SS_BUILT])
    for l in range(4):
        if d.mode == 2:
            det, des = int(gait_out[20 + l]), int(gait_out[8 + l])
            swing = not (det == 1 or det == 2 or des != 8 or stop)
        else:
            ls = int(gait_out[12 + l])
            swing = not ((ls == 1 and gait_state[20 + l] != 0) or ls == 2)
        if not swing:
            continue
        vb = [f32(0)] * 3
        if d.mode == 1:
            stp = [f32(v) for v in st[SS_GLOBAL + 3 * l:SS_GLOBAL + 3 * l + 3]]
            tg = [f32(v) for v in st[SS_FH + 3 * l:SS_FH + 3 * l + 3]]
            pb = rigid_transform(q, bp, parabola_point(warp_phase(gait_out[4 + l]), stp, tg))
        else:
            if not (built >> l) & 1:
                flags |= SW_NO_TRAJ; continue
            u = f32(gait_out[4 + l]) - f32(0)
            if f64(u) < -1e-3 or f64(u) >= 1.0 + 1e-3:
                flags |= SW_PHASE; continue
            p, v = bspline_point(st[SS_SRC + 3 * l:SS_SRC + 3 * l + 3], st[SS_TGT + 3 * l:SS_TGT + 3 * l + 3], f32(st[SS_H + l]), u)
            if d.is_sim:
                pb = rigid_transform(q, bp, p); vb = rigid_transform(q, [0, 0, 0], v)
            else:
                pb, vb = p, v
        sh = hl * (f32(1) if l & 1 else f32(-1))
        ang = leg_ik(pb, ho[3 * l:3 * l + 3], sh, lu, ll)
        Ji = jacobian_inverse(ang, sh, lu, ll)
        for r in range(3):
            a = ang[r]
            if a != a: a = f32(est_in[17 + 3 * l + r])
            st[SS_QANG + 3 * l + r] = a
            st[SS_QVEL + 3 * l + r] = (Ji[r][0] * vb[0] + Ji[r][1] * vb[1]) + Ji[r][2] * vb[2]
            out[3 * l + r] = pb[r]; out[12 + 3 * l + r] = vb[r]
            out[24 + 3 * l + r] = a; out[36 + 3 * l + r] = st[SS_QVEL + 3 * l + r]
        mp |= 1 << l
    for l in range(4):
        cmd = False
        if (mp >> l) & 1:
            cmd = (int(gait_out[8 + l]) == 8 and int(gait_out[20 + l]) != 2) if d.mode == 2 else int(gait_out[12 + l]) == 0
        out[48 + l] = 1.0 if cmd else 0.0
        if cmd:
            out[24 + 3 * l:27 + 3 * l] = st[SS_QANG + 3 * l:SS_QANG + 3 * l + 3]
            out[36 + 3 * l:39 + 3 * l] = st[SS_QVEL + 3 * l:SS_QVEL + 3 * l + 3]
    st[SS_MAP] = mp
    return flags
