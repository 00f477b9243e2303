"""CPU restatement of the walk mode's pose planner, numpy, operation by operation:
  qrPosePlanner::Update / QpSolver / ComputeG / ComputeGradient* / ComputeHessian*   quadruped/src/planner/qr_pose_planner.cpp:72-456
  qrPosePlanner::ResetBasePose                                                      include/quadruped/planner/qr_pose_planner.h:311-320
  solve_quadprog_test                                                               quadruped/extern/QuadProgpp/src/QuadProg++.cc:52-450, 849-1149
  so3ToQuat, ConcatenationTwoQuats, quatToRPY, vectorToSkewMat                      include/quadruped/utils/qr_se3.h:95-130, 209-223, 402-418, 484-494
The scalar type T is np.float32 (the statement the kernel is held to: the reference's float assembly, the solve in double from the float
data, p narrowed back) or np.float64 (everything in double: the yardstick).  The operation order is that of
quadruped-robot_amd/csrc/qr_pose_plan_kernel.hip, whose header lists the readings of Eigen's evaluation order and why the rBCOM = 0 terms
are left out.  The QP solver is QuadProg++'s, step for step in float64, and returns the slot-ordered u and the order A[]."""
import math

import numpy as np

import stance_ref as S

f32, f64 = np.float32, np.float64
STATE_ROWS, MAX_LOOPS = 26, 20
OUT_ROWS = 7 * MAX_LOOPS + 38
FEW_CONTACTS, NOT_PD, INFEASIBLE, LAMBDA_GROWN, NONCONVEX, NAN, MAXITER = 1, 2, 4, 8, 16, 32, 64
FATAL = FEW_CONTACTS | NOT_PD | NAN
CCW = (0, 2, 3, 1)                      # slot c of the counter-clockwise order holds leg CCW[c]
SWING, STANCE = 0, 1
EPS, INF = np.finfo(f64).eps, float("inf")


class Desc:
    """qrgpu_pose_plan_desc with qrgpu_pose_plan_desc_default's values (qr_pose_planner.cpp:48-50, qr_pose_planner.h:155-160, 266-276)."""
    def __init__(self, **kw):
        self.rBH = [0.18, -0.047, 0.0, 0.18, 0.047, 0.0, -0.18, -0.047, 0.0, -0.18, 0.047, 0.0]      # 3*leg+axis
        self.l_min, self.l_max, self.omega, self.eps, self.body_height, self.loops = 0.22, 0.35, 0.5, 0.1, 0.27, 20
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


# ---- QuadProg++ ---------------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE division (python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def _distance(a, b):
    a1, b1 = abs(a), abs(b)
    if a1 > b1:
        t = b1 / a1
        return a1 * math.sqrt(1.0 + t * t)
    if b1 > a1:
        t = a1 / b1
        return b1 * math.sqrt(1.0 + t * t)
    return a1 * math.sqrt(2.0)


def _rotate(M, rows, c, cc, ss, xny):
    for k in rows:
        t1, t2 = M[k][c], M[k][c + 1]
        M[k][c] = t1 * cc + t2 * ss
        M[k][c + 1] = xny * (t1 + M[k][c]) - t2


def _add_constraint(R, J, d, iq, R_norm):
    n = len(d)
    for j in range(n - 1, iq, -1):
        cc, ss = d[j - 1], d[j]
        h = _distance(cc, ss)
        if abs(h) < EPS:
            continue
        d[j] = 0.0
        ss, cc = ss / h, cc / h
        if cc < 0.0:
            cc, ss, d[j - 1] = -cc, -ss, -h
        else:
            d[j - 1] = h
        _rotate(J, range(n), j - 1, cc, ss, ss / (1.0 + cc))
    iq += 1
    for i in range(iq):
        R[i][iq - 1] = d[i]
    if abs(d[iq - 1]) <= EPS * R_norm:
        return False, iq, R_norm
    return True, iq, max(R_norm, abs(d[iq - 1]))


def _delete_constraint(R, J, A, u, n, iq, l):
    qq = next((i for i in range(iq) if A[i] == l), None)
    if qq is None:
        return None
    for i in range(qq, iq - 1):
        A[i], u[i] = A[i + 1], u[i + 1]
        for j in range(n):
            R[j][i] = R[j][i + 1]
    A[iq - 1], u[iq - 1], A[iq], u[iq] = A[iq], u[iq], 0, 0.0
    for j in range(iq):
        R[j][iq - 1] = 0.0
    iq -= 1
    if iq == 0:
        return iq
    for j in range(qq, iq):
        cc, ss = R[j][j], R[j + 1][j]
        h = _distance(cc, ss)
        if abs(h) < EPS:
            continue
        cc, ss = cc / h, ss / h
        R[j + 1][j] = 0.0
        if cc < 0.0:
            R[j][j], cc, ss = -h, -cc, -ss
        else:
            R[j][j] = h
        xny = ss / (1.0 + cc)
        for k in range(j + 1, iq):
            t1, t2 = R[j][k], R[j + 1][k]
            R[j][k] = t1 * cc + t2 * ss
            R[j + 1][k] = xny * (t1 + R[j][k]) - t2
        _rotate(J, range(n), j, cc, ss, xny)
    return iq


def solve_quadprog(G, g0, CI, ci0, max_steps=200):
    """solve_quadprog_test without equalities.  G [n][n] (only G[i][j], j >= i, is read), g0 [n], CI [n][m], ci0 [m], python floats.
    -> x [n], u [m + 1] (slot-ordered; the reference's vector has m entries and slot m is never reached with m > n), A (the order of the
    working set, iq entries), flags (NOT_PD: the Cholesky throws; INFEASIBLE: +inf returned; MAXITER: a bound the reference does not have)"""
    n, m = len(g0), len(ci0)
    G = [[float(v) for v in row] for row in G]
    g0 = [float(v) for v in g0]
    CI = [[float(v) for v in row] for row in CI]
    ci0 = [float(v) for v in ci0]
    c1 = 0.0
    for i in range(n):
        c1 += G[i][i]
    for i in range(n):                                               # cholesky_decomposition
        for j in range(i, n):
            s = G[i][j]
            for k in range(i - 1, -1, -1):
                s -= G[i][k] * G[j][k]
            if i == j:
                if s <= 0.0:
                    return None, None, [], NOT_PD
                G[i][i] = math.sqrt(s)
            else:
                G[j][i] = s / G[i][i]
        for k in range(i + 1, n):
            G[i][k] = G[k][i]

    def forward(b):
        y = [0.0] * n
        y[0] = b[0] / G[0][0]
        for i in range(1, n):
            y[i] = b[i]
            for j in range(i):
                y[i] -= G[i][j] * y[j]
            y[i] = y[i] / G[i][i]
        return y

    R = [[0.0] * n for _ in range(n)]
    J, c2 = [], 0.0
    for i in range(n):
        z = forward([1.0 if k == i else 0.0 for k in range(n)])
        J.append(z)
        c2 += z[i]
    y = forward(g0)
    x = [0.0] * n
    x[n - 1] = y[n - 1] / G[n - 1][n - 1]
    for i in range(n - 2, -1, -1):
        x[i] = y[i]
        for j in range(i + 1, n):
            x[i] -= G[i][j] * x[j]
        x[i] = x[i] / G[i][i]
    x = [-v for v in x]
    u, A = [0.0] * (m + 1), [0] * (m + 1)
    s = [0.0] * m
    R_norm, iq, flags, steps = 1.0, 0, 0, 0
    ss, ip = 0.0, 0
    while True:                                                      # l1
        psi = 0.0
        for i in range(m):
            v = 0.0
            for j in range(n):
                v += CI[j][i] * x[j]
            v += ci0[i]
            s[i] = v
            psi += v if v < 0.0 else 0.0
        if abs(psi) <= m * EPS * c1 * c2 * 100.0:
            break
        u_old, A_old, x_old = list(u), list(A), list(x)
        ss, ip, excl = 0.0, 0, set()
        state = "l2"
        while state == "l2":
            active = set(A[:iq])
            for i in range(m):
                if s[i] < ss and i not in active and i not in excl:
                    ss, ip = s[i], i
            if ss >= 0.0:
                state = "done"
                break
            nP = [CI[i][ip] for i in range(n)]
            u[iq], A[iq] = 0.0, ip
            while True:                                              # l2a
                steps += 1
                if steps > max_steps:
                    flags |= MAXITER | INFEASIBLE
                    state = "done"
                    break
                d = [0.0] * n
                for i in range(n):
                    v = 0.0
                    for j in range(n):
                        v += J[j][i] * nP[j]
                    d[i] = v
                z = [0.0] * n
                for i in range(n):
                    v = 0.0
                    for j in range(iq, n):
                        v += J[i][j] * d[j]
                    z[i] = v
                r = [0.0] * (m + 1)
                for i in range(iq - 1, -1, -1):
                    v = 0.0
                    for j in range(i + 1, iq):
                        v += R[i][j] * r[j]
                    r[i] = _div(d[i] - v, R[i][i])
                l, t1 = 0, INF
                for k in range(iq):
                    if r[k] > 0.0 and u[k] / r[k] < t1:
                        t1, l = u[k] / r[k], A[k]
                zz = znp = 0.0
                for k in range(n):
                    zz += z[k] * z[k]
                    znp += z[k] * nP[k]
                t2 = INF
                if abs(zz) > EPS:
                    t2 = _div(-s[ip], znp)
                    if t2 < 0:
                        t2 = INF
                t = t2 if t2 < t1 else t1
                if t >= INF:
                    flags |= INFEASIBLE
                    state = "done"
                    break
                if t2 >= INF:                                        # dual step
                    for k in range(iq):
                        u[k] -= t * r[k]
                    u[iq] += t
                    iq = _delete_constraint(R, J, A, u, n, iq, l)
                    if iq is None:
                        iq, flags, state = 0, flags | MAXITER | INFEASIBLE, "done"
                        break
                    continue
                for k in range(n):
                    x[k] += t * z[k]
                for k in range(iq):
                    u[k] -= t * r[k]
                u[iq] += t
                if abs(t - t2) < EPS:                                # full step
                    if iq >= n:
                        flags |= MAXITER | INFEASIBLE
                        state = "done"
                        break
                    ok, iq, R_norm = _add_constraint(R, J, d, iq, R_norm)
                    if not ok:
                        excl.add(ip)
                        iq = _delete_constraint(R, J, A, u, n, iq, ip)
                        if iq is None:
                            iq, flags, state = 0, flags | MAXITER | INFEASIBLE, "done"
                            break
                        for i in range(iq):
                            A[i], u[i] = A_old[i], u_old[i]
                        x = list(x_old)
                        break                                        # goto l2: ss and ip keep their values
                    state = "l1"
                    break
                iq = _delete_constraint(R, J, A, u, n, iq, l)
                if iq is None:
                    iq, flags, state = 0, flags | MAXITER | INFEASIBLE, "done"
                    break
                v = 0.0
                for k in range(n):
                    v += CI[k][ip] * x[k]
                s[ip] = v + ci0[ip]
        if state == "done":
            break
    return x, u, A[:iq], flags


# ---- robotics::math additions ----------------------------------------------------------------------------------------------------------------
def skew(T, v):
    z = T(0)
    return [[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]]


def so3_to_quat(T, so3):
    so3 = [T(v) for v in so3]
    theta = T(np.sqrt((so3[0] * so3[0] + so3[1] * so3[1]) + so3[2] * so3[2]))
    if abs(f64(theta)) < 1.e-6:
        return [T(1), T(0), T(0), T(0)]
    h = f64(theta) / 2.0
    sh = math.sin(h)
    return [T(math.cos(h))] + [T(f64(so3[k] / theta) * sh) for k in range(3)]


def concatenation_two_quats(T, q, p):
    Sq = skew(T, q[1:])
    out = [q[0] * p[0] - ((q[1] * p[1] + q[2] * p[2]) + q[3] * p[3])]
    for r in range(3):
        out.append((q[0] * p[1 + r] + p[0] * q[1 + r]) + S.dot3(Sq[r], p[1:]))
    return out


def mat_add_half(T, A, B):
    return [[(A[r][c] + B[r][c]) / T(2) for c in range(3)] for r in range(3)]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------------
def new_state(T, base_pos):
    """The constructed planner (:31-69): Lambda 0.1 x 12, quat identity, rIB the estimated position, poseDest (rIB, 0)."""
    rIB = [T(v) for v in base_pos]
    return dict(lam=[T(f32(0.1))] * 12, size=12, rIB=rIB, quat=[T(1), T(0), T(0), T(0)], dest=rIB + [T(0)] * 3)


def world_feet(T, inp):
    """GetFootPositionsInWorldFrame (qr_robot.cpp:222-230), slot order"""
    q = [T(v) for v in inp["quat"]]
    bp = [T(v) for v in inp["base_pos"]]
    fb = [[T(inp["foot_base"][3 * leg + k]) for k in range(3)] for leg in CCW]
    return [S.invert_rigid_transform(T, q, bp, p) for p in fb], fb


def reset_base_pose(T, desc, inp, state):
    """-> flags, cmd rows 7-24 (source, poseDest, twist) or None.  state['dest'] is updated."""
    rIF, _ = world_feet(T, inp)
    mx = ((rIF[0][0] + rIF[1][0]) + (rIF[2][0] + rIF[3][0])) / T(4)
    my = ((rIF[0][1] + rIF[1][1]) + (rIF[2][1] + rIF[3][1])) / T(4)
    if not (np.isfinite(mx) and np.isfinite(my)):
        return NAN, None
    dest = [mx, my, T(f32(desc.body_height)), T(0), T(0), T(0)]
    state["dest"] = dest
    return 0, [T(v) for v in inp["base_pos"]] + [T(v) for v in inp["rpy"]] + dest + [T(0)] * 6


def update(T, desc, inp, state, record_qp=False):
    """qrPosePlanner::Update.  inp: quat[4], base_pos[3], foot_base[12] (3*leg+axis), ground_rpy[3], rpy[3], desired_leg_state[4].
    -> dict(flags, cmd (rows 7-18: source, poseDest; None when a fatal flag is set), p [loops][6], iq [loops], A [loops] lists, u0, lam, N,
    mask, qps).  state is updated unless a fatal flag is set."""
    with np.errstate(all="ignore"):
        return _update(T, desc, inp, state, record_qp)


def assemble(T, desc, q, rIB, rIF, rBF, rBH, valid, vert, g, lam, rSP):
    """One SQP iteration's QP data (ComputeG, ComputeGradientF / G, ComputeHessianF / G, hessGSum; :177-190, 282-443), slot order.
    -> Mf = hessF - hessGSum [6][6], gradF [6], gradG [3N][6], Gv [3N], hessF [6][6], Hn (the N leg-length Hessians)"""
    P = lambda v: T(f32(v))
    N = len(valid)
    m = 3 * N
    l_min, l_max, omega, sh = P(desc.l_min), P(desc.l_max), P(desc.omega), T(1) - P(desc.eps)
    two = T(2)
    Sn, Dn, Hn, gfh, gft = [], [], [], [], []
    gradG = [[T(0)] * 6 for _ in range(m)]
    Gv = [T(0)] * m
    for v in range(N):
        c = valid[v]
        r = S.transform_vec_by_quat(T, q, rBF[c])
        h = S.transform_vec_by_quat(T, q, rBH[c])
        dv = [rIB[k] - rIF[c][k] for k in range(3)]
        Sr, Sh, M = skew(T, r), skew(T, h), skew(T, dv)
        gfh.append([(rIB[k] + r[k]) - rIF[c][k] for k in range(3)])
        gft.append([S.dot3(Sr[k], dv) for k in range(3)])
        Sn.append(Sr)
        Dn.append(mat_add_half(T, S.mat3_mul(M, Sr), S.mat3_mul(Sr, M)))
        gv = g[v]
        g2 = (gv[0] * gv[0] + gv[1] * gv[1]) + gv[2] * gv[2]
        gn = T(np.sqrt(g2))
        gn3 = T((f64(gn) * f64(gn)) * f64(gn))
        diff = [[gv[a] * gv[b] for b in range(3)] for a in range(3)]
        h00 = [[(T(1) if a == b else T(0)) / gn - diff[a][b] / gn3 for b in range(3)] for a in range(3)]
        DS, T0 = S.mat3_mul(diff, Sh), S.mat3_mul(h00, Sh)
        DH = mat_add_half(T, S.mat3_mul(M, Sh), S.mat3_mul(Sh, M))
        dG = [(((-gv[0]) * Sh[0][j] + (-gv[1]) * Sh[1][j]) + (-gv[2]) * Sh[2][j]) / gn for j in range(3)]
        gh = [gv[j] / gn if g2 > 0 else gv[j] for j in range(3)]
        H = [[T(0)] * 6 for _ in range(6)]
        for a in range(3):
            for b in range(3):
                H[a][b] = h00[a][b]
                H[a][3 + b] = (-Sh[a][b]) / gn + DS[a][b] / gn3
                H[3 + a][b] = -T0[b][a]
                H[3 + a][3 + b] = (DH[a][b] / two - dG[a] * dG[b]) / gn
        Hn.append(H)
        for j in range(3):
            a = gh[j]
            b = ((-gh[0]) * Sh[0][j] + (-gh[1]) * Sh[1][j]) + (-gh[2]) * Sh[2][j]
            gradG[N + v][j], gradG[N + v][3 + j] = a, b
            gradG[2 * N + v][j], gradG[2 * N + v][3 + j] = -a, -b
        Gv[N + v] = gn - l_min
        Gv[2 * N + v] = l_max - gn
    if N == 3:
        O = [((vert[0][k] + vert[1][k]) + vert[2][k]) / T(3) for k in range(3)]
    else:
        O = [(((vert[0][k] + vert[1][k]) + vert[2][k]) + vert[3][k]) / T(4) for k in range(3)]
    V = [[O[k] + sh * (vert[v][k] - O[k]) for k in range(3)] for v in range(N)]
    for v in range(N):
        Pv, Q = V[v], V[(v + 1) % N]
        a0, a1, bs = Q[1] - Pv[1], Pv[0] - Q[0], Pv[0] * Q[1] - Q[0] * Pv[1]
        gradG[v][0], gradG[v][1] = a0, a1
        Gv[v] = ((a0 * rIB[0] + a1 * rIB[1]) + T(0) * rIB[2]) - bs
    Mf = [[T(0)] * 6 for _ in range(6)]
    HF = [[T(0)] * 6 for _ in range(6)]
    for r_ in range(6):
        for c_ in range(6):
            hf, hg = T(0), T(0)
            if r_ < 3 and c_ < 3:
                idn = T(1) if r_ == c_ else T(0)
                for v in range(N):
                    hf = hf + idn
                hf = hf + omega * idn
            elif r_ < 3:
                for v in range(N):
                    hf = hf - Sn[v][r_][c_ - 3]
            elif c_ < 3:
                for v in range(N):
                    hf = hf + Sn[v][r_ - 3][c_]
            else:
                for v in range(N):
                    hf = hf + Dn[v][r_ - 3][c_ - 3]
            hf = hf * two
            for v in range(N):
                hg = hg + lam[N + v] * Hn[v][r_][c_]
            for v in range(N):
                hg = hg + lam[2 * N + v] * (-Hn[v][r_][c_])
            HF[r_][c_] = hf
            Mf[r_][c_] = hf - hg
    gradF = []
    for k in range(6):
        a = T(0)
        if k < 3:
            for v in range(N):
                a = a + gfh[v][k]
            a = a + omega * (rIB[k] - rSP[k])
        else:
            for v in range(N):
                a = a + gft[v][k - 3]
        gradF.append(a * two)
    return Mf, gradF, gradG, Gv, HF, Hn


def _update(T, desc, inp, state, record_qp):
    P = lambda v: T(f32(v))                                          # a float parameter of the descriptor
    out = dict(flags=0, cmd=None, p=[], iq=[], A=[], u0=None, lam=None, N=0, mask=0, qps=[])
    q = [T(v) for v in inp["quat"]]
    rIB = [T(v) for v in inp["base_pos"]]
    src = list(rIB)
    rIF, rBF = world_feet(T, inp)
    rBH = [[P(desc.rBH[3 * leg + k]) for k in range(3)] for leg in CCW]
    contact = [int(inp["desired_leg_state"][leg]) == STANCE for leg in CCW]
    flags = 0
    if not (np.isfinite(f64(inp["ground_rpy"][1])) and all(np.isfinite(f64(v)) for v in q)
            and all(np.isfinite(f64(v)) for p in rIF + rBF for v in p)):
        flags |= NAN
    valid, vert, g = [], [], []
    sp = [T(0)] * 3
    for c in range(4):
        if contact[c]:
            t = S.transform_vec_by_quat(T, q, rBH[c])
            valid.append(c)
            vert.append(list(rIF[c]))
            sp = [sp[k] + rIF[c][k] for k in range(3)]
            g.append([(rIB[k] + t[k]) - rIF[c][k] for k in range(3)])
    cnt = len(valid)
    if cnt < 3:
        out["flags"] = flags | FEW_CONTACTS
        return out
    rSP = []
    for k in range(3):
        center = ((rIF[0][k] + rIF[1][k]) + (rIF[2][k] + rIF[3][k])) / T(4)
        mean = sp[k] / T(cnt)
        rSP.append(mean * T(2) / T(3) + center / T(3))
    rSP[2] = P(desc.body_height)
    if cnt == 4:
        invalid = -1
        for s in (1, 2):
            dst = (s + 2) % 4
            cp, cn, sr, ds = vert[s - 1], vert[s + 1], vert[s], vert[dst]
            if (ds[0] - sr[0]) * (cp[1] - sr[1]) - (ds[1] - sr[1]) * (cp[0] - sr[0]) > 0:
                invalid = s - 1
                break
            if (ds[0] - sr[0]) * (cn[1] - sr[1]) - (ds[1] - sr[1]) * (cn[0] - sr[0]) < 0:
                invalid = s + 1
                break
        if invalid >= 0:
            del valid[invalid], vert[invalid], g[invalid]
            flags |= NONCONVEX
    N = len(valid)
    m = 3 * N
    lam = [T(v) for v in state["lam"]]
    if m > state["size"]:
        flags |= LAMBDA_GROWN
        for i in range(state["size"], m):
            lam[i] = P(0.1)
    out["N"], out["mask"] = N, sum(1 << c for c in valid)
    if flags & NAN:
        out["flags"] = flags
        return out
    loops = min(max(int(desc.loops), 1), MAX_LOOPS)
    for loop in range(loops):
        Mf, gradF, gradG, Gv, _, _ = assemble(T, desc, q, rIB, rIF, rBF, rBH, valid, vert, g, lam, rSP)
        GG = [[float(Mf[j][i]) for j in range(6)] for i in range(6)]
        g0 = [float(v) for v in gradF]
        CI = [[float(gradG[i][j]) for i in range(m)] for j in range(6)]
        ci0 = [float(v) for v in Gv]
        x, u, A, qf = solve_quadprog(GG, g0, CI, ci0)
        if qf & NOT_PD:
            out["flags"] = flags | NOT_PD
            return out
        flags |= qf
        if record_qp:
            out["qps"].append(dict(G=np.array(GG), g0=np.array(g0), CI=np.array(CI), ci0=np.array(ci0), x=np.array(x), u=np.array(u[:m]), A=list(A),
                                   flags=qf))
        p = [T(v) for v in x]
        out["p"].append(p); out["iq"].append(len(A)); out["A"].append(list(A))
        if loop == 0:
            out["u0"] = [T(v) for v in u[:m]]
        rIB = [rIB[k] + p[k] for k in range(3)]
        q = concatenation_two_quats(T, so3_to_quat(T, p[3:]), q)
        lam[:m] = [T(v) for v in u[:m]]
        z3 = [T(0)] * 3
        rBF = [S.rigid_transform(T, q, z3, [rIF[c][k] - rIB[k] for k in range(3)]) for c in range(4)]
        g = []
        for c in valid:
            t = S.transform_vec_by_quat(T, q, rBH[c])
            g.append([(rIB[k] + t[k]) - rIF[c][k] for k in range(3)])
    rpy = S.quat_to_rpy(T, q)
    rpy[1] = T(f64(rpy[1] + T(inp["ground_rpy"][1])) / 2.0)
    dest = list(rIB) + list(rpy)
    out["lam"] = lam[:m]
    if not all(np.isfinite(f64(v)) for v in dest):
        out["flags"] = flags | NAN
        return out
    out["flags"] = flags
    out["cmd"] = src + [T(v) for v in inp["rpy"]] + dest
    state.update(lam=lam[:m] + list(state["lam"][m:]), size=m, rIB=list(rIB), quat=list(q), dest=dest)
    return out


# ---- batches: the device arrays of qrgpu_pose_plan_batch ---------------------------------------------------------------------------------------
def pack_inputs(cases):
    """cases: list of input dicts -> dict of [n][rows] float32 arrays in the layouts of qrgpu_stance_update_batch's inputs"""
    n = len(cases)
    est_in, est_out, ground = np.zeros((n, 29), f32), np.zeros((n, 40), f32), np.zeros((n, 31), f32)
    rpy, walk = np.zeros((n, 3), f32), np.zeros((n, 41), f32)
    for i, c in enumerate(cases):
        est_in[i, 6:10] = c["quat"]
        est_out[i, 12:24] = c["foot_base"]
        est_out[i, 36:39] = c["base_pos"]
        ground[i, 6:9] = c["ground_rpy"]
        ground[i, 9] = 1.0
        rpy[i] = c["rpy"]
        walk[i, 8:12] = c["desired_leg_state"]
        walk[i, 12:16] = c.get("leg_state", c["desired_leg_state"])
        walk[i, 16:20] = c.get("cur_leg_state", [STANCE] * 4)
    return dict(est_in=est_in, est_out=est_out, ground=ground, rpy=rpy, walk=walk)


def state_rows(T, st):
    """A state dict as the STATE_ROWS floats of d_pose_state"""
    lam = list(st["lam"]) + [T(0)] * (12 - len(st["lam"]))
    return np.array([f64(v) for v in lam + [st["size"]] + list(st["rIB"]) + list(st["quat"]) + list(st["dest"])], T)


def switch_to_swing(case):
    """the switchToSwing rule of qr_locomotion_controller.cpp:81-89 on the rows of d_walk_out"""
    ls, cur = case.get("leg_state", case["desired_leg_state"]), case.get("cur_leg_state", [STANCE] * 4)
    return any(int(ls[l]) == SWING and int(cur[l]) == STANCE for l in range(4))


# ---- test inputs -----------------------------------------------------------------------------------------------------------------------------------
NOMINAL_FEET = np.array([0.18, -0.13, -0.27, 0.18, 0.13, -0.27, -0.18, -0.13, -0.27, -0.18, 0.13, -0.27])      # A1 stance, base frame, 3*leg+axis


def rpy_to_quat(r, p, y):
    cr, sr, cp, sp_, cy, sy = math.cos(r / 2), math.sin(r / 2), math.cos(p / 2), math.sin(p / 2), math.cos(y / 2), math.sin(y / 2)
    return [cr * cp * cy + sr * sp_ * sy, sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy]


def make_case(rng, swing_leg=None, offset=(0.0, 0.0, 0.0), tilt=0.05, scatter=0.03, feet_world=None, base_xy=(0.0, 0.0)):
    """A walk-like input: A1 nominal stance with `scatter` of foot noise, the base displaced by `offset` from above the feet and tilted by up
    to `tilt` rad; swing_leg None: four stance feet.  feet_world [4][3] (leg order) fixes the feet in the world instead."""
    r, p, y = rng.uniform(-tilt, tilt, 3)
    quat = np.array(rpy_to_quat(r, p, y))
    base = np.array([base_xy[0] + offset[0], base_xy[1] + offset[1], 0.27 + offset[2]])
    R = np.array(S.quat_to_rot(f64, *quat))
    if feet_world is None:
        feet_world = NOMINAL_FEET.reshape(4, 3) + [base_xy[0], base_xy[1], 0.27] + rng.uniform(-scatter, scatter, (4, 3)) * [1, 1, 0.3]
    foot_base = (np.asarray(feet_world) - base) @ R                    # R^T (w - base)
    des = [STANCE] * 4
    ls, cur = [STANCE] * 4, [STANCE] * 4
    if swing_leg is not None:
        des[swing_leg] = SWING
        ls[swing_leg] = SWING
    return dict(quat=f32(quat), base_pos=f32(base), foot_base=f32(foot_base.reshape(-1)), ground_rpy=f32(rng.uniform(-0.05, 0.05, 3)),
                rpy=f32([r, p, y]), desired_leg_state=des, leg_state=ls, cur_leg_state=cur)


# ---- tests/golden/pose_plan_golden.npz (written by tests/golden/make_pose_plan.py) ------------------------------------------------------------
IN_KEYS = (("quat", 4), ("base_pos", 3), ("foot_base", 12), ("ground_rpy", 3), ("rpy", 3), ("desired_leg_state", 4), ("leg_state", 4),
           ("cur_leg_state", 4))
def flat_input(c):
    return np.concatenate([np.asarray(c[k], f64).reshape(-1) for k, _ in IN_KEYS]).astype(f32)


def unflat_input(row):
    c, o = {}, 0
    for k, w in IN_KEYS:
        c[k] = row[o:o + w].astype(f32) if "state" not in k else [int(v) for v in row[o:o + w]]
        o += w
    return c


def load_golden():
    """-> dict of the file's arrays plus cases (the input dicts) and cell_of (case -> cell name)"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_plan_golden.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    g["cases"] = [unflat_input(r) for r in g["inputs"]]
    g["cell_of"] = [str(g["cells"][np.searchsorted(g["cell_start"], i, side="right") - 1]) for i in range(len(g["cases"]))]
    return g
