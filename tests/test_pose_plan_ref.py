"""CPU: the walk pose planner's restatement (tests/pose_plan_ref.py) against the compiled QuadProg++ (recorded in
tests/golden/pose_plan_golden.npz, and live when oracle/_ref is there), its own derivatives, the plan's constraints, every flag, and the
new C-ABI symbols.  Reference: quadruped/src/planner/qr_pose_planner.cpp:72-456, quadruped/extern/QuadProgpp/src/QuadProg++.cc:52-450."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_plan_ref as P
import stance_ref as S

f32, f64 = np.float32, np.float64
EXCLUDE_CAP = 0.01                         # share of a cell whose float32 / float64 runs may differ in a working set or a flag (tests/test_gpu_vmc_grid.py's cap)


@functools.lru_cache(maxsize=None)
def golden():
    return P.load_golden()


@functools.lru_cache(maxsize=None)
def rerun32():
    """The float32 restatement on every golden case with its QPs, chains carried as the file carried them."""
    g = golden()
    out = []
    st = None
    for i, c in enumerate(g["cases"]):
        chained = bool(g["cell_chained"][list(g["cells"]).index(g["cell_of"][i])])
        first = i == g["cell_start"][list(g["cells"]).index(g["cell_of"][i])]
        if st is None or not chained or first:
            st = P.new_state(f32, c["base_pos"])
        assert np.array_equal(P.state_rows(f32, st), g["before32"][i], equal_nan=True), i
        out.append(P.update(f32, P.Desc(), c, st, record_qp=True))
    return out


def test_golden_is_what_the_restatement_gives():
    g, rs = golden(), rerun32()
    for i, r in enumerate(rs):
        assert r["flags"] == g["flags32"][i], i
        if r["cmd"] is not None:
            assert np.array(r["cmd"], f32).tobytes() == g["cmd32"][i].tobytes(), i
            assert np.array(r["p"], f32).tobytes() == g["p32"][i].tobytes(), i


def test_solver_x_equals_compiled_quadprog_recorded():
    """Every QP of every golden case: the restated solver's x is the compiled solve_quadprog's, bit for bit (same operations, same order)."""
    g, rs = golden(), rerun32()
    nqp = 0
    for i, r in enumerate(rs):
        for k, qp in enumerate(r["qps"]):
            assert np.array_equal(qp["x"], g["x_quadprog"][i, k]), (i, k, qp["x"] - g["x_quadprog"][i, k])
            assert np.isinf(g["f_quadprog"][i, k]) == bool(qp["flags"] & P.INFEASIBLE)
            nqp += 1
    assert nqp >= 80 * P.MAX_LOOPS


def test_solver_x_equals_compiled_quadprog_live(ref):
    """The same against oracle/_ref itself (skipped when it was not built), on the QPs with a non-empty working set and a sample of the rest."""
    rs = rerun32()
    n = 0
    for r in rs:
        for k, qp in enumerate(r["qps"]):
            if qp["A"] or k == 0:
                x, f = ref.ref_quadprog(qp["G"], qp["g0"], np.zeros((6, 0)), np.zeros(0), qp["CI"], qp["ci0"])
                assert np.array_equal(x, qp["x"]), (k, x - qp["x"])
                n += 1
    assert n > 100


def test_slot_ordered_u_against_multipliers_and_kkt(oracle):
    """u[k] is the multiplier of constraint A[k]: equal to the oracle solver's per-constraint multiplier, zero KKT residual G x + g0 - CI u,
    complementary and feasible.  G is the matrix QuadProg++ factorises: the mirror of GG's upper triangle."""
    rs = rerun32()
    n = 0
    for r in rs:
        for qp in r["qps"]:
            if not qp["A"] or qp["flags"]:
                continue
            G = np.triu(qp["G"]) + np.triu(qp["G"], 1).T
            A, u = qp["A"], qp["u"][:len(qp["A"])]
            assert len(set(A)) == len(A) and np.all(u >= 0)
            scale = np.abs(qp["g0"]).max() + 1.0
            res = G @ qp["x"] + qp["g0"] - qp["CI"][:, A] @ u
            assert np.abs(res).max() <= 1e-11 * scale, (np.abs(res).max(), scale)
            slack = qp["CI"].T @ qp["x"] + qp["ci0"]
            assert slack.min() >= -1e-10 and np.abs(slack[A]).max() <= 1e-10
            x, lam, _, rc = oracle.qp_solve(G, qp["g0"], None, None, qp["CI"], qp["ci0"])
            assert rc == 0 and np.abs(x - qp["x"]).max() <= 1e-9 * (1 + np.abs(x).max())
            assert np.abs(lam[A] - u).max() <= 1e-8 * (1 + np.abs(u).max()) and np.abs(np.delete(lam, A)).max() <= 1e-9
            n += 1
    assert n >= 20


def planner_point(c, dx=None):
    """The planner's quantities at the case's start, displaced by dx = (dr, dphi): rIB + dr, so3ToQuat(dphi) o quat, rBF held."""
    T = f64
    q = [T(v) for v in c["quat"]]
    rIB = [T(v) for v in c["base_pos"]]
    rIF, rBF = P.world_feet(T, c)
    if dx is not None:
        rIB = [rIB[k] + T(dx[k]) for k in range(3)]
        q = P.concatenation_two_quats(T, P.so3_to_quat(T, dx[3:]), q)
    rBH = [[T(f32(P.Desc().rBH[3 * leg + k])) for k in range(3)] for leg in P.CCW]
    valid = [s for s in range(4) if int(c["desired_leg_state"][P.CCW[s]]) == P.STANCE]
    vert = [rIF[s] for s in valid]
    g = [[(rIB[k] + S.transform_vec_by_quat(T, q, rBH[s])[k]) - rIF[s][k] for k in range(3)] for s in valid]
    rSP = [T(0.01), T(-0.02), T(0.27)]
    return q, rIB, rIF, rBF, rBH, valid, vert, g, rSP


def compute_F(c, dx):
    """ComputeF (:446-456) in float64"""
    q, rIB, rIF, rBF, rBH, valid, vert, g, rSP = planner_point(c, dx)
    f = 0.0
    for s in valid:
        r1 = np.array(rIB) + np.array(S.transform_vec_by_quat(f64, q, rBF[s])) - np.array(rIF[s])
        f += float(r1 @ r1)
    r2 = np.array(rSP) - np.array(rIB)
    return f + 0.5 * float(r2 @ r2)


@pytest.mark.parametrize("case", [0, 9, 17, 48, 52])
def test_gradients_against_central_differences(case):
    c = golden()["cases"][case]
    d = P.Desc()
    lam = [f64(0.1)] * 12
    Mf, gradF, gradG, Gv, HF, Hn = P.assemble(f64, d, *planner_point(c)[:8], lam, planner_point(c)[8])
    h = 1e-6
    for k in range(6):
        e = np.zeros(6); e[k] = h
        num = (compute_F(c, e) - compute_F(c, -e)) / (2 * h)
        assert abs(num - gradF[k]) <= 1e-7 * (1 + abs(gradF[k])), (k, num, gradF[k])
        Gp = P.assemble(f64, d, *planner_point(c, e)[:8], lam, planner_point(c)[8])[3]
        Gm = P.assemble(f64, d, *planner_point(c, -e)[:8], lam, planner_point(c)[8])[3]
        for i in range(len(Gv)):
            num = float(Gp[i] - Gm[i]) / (2 * h)
            assert abs(num - gradG[i][k]) <= 1e-7 * (1 + abs(gradG[i][k])), (i, k, num, gradG[i][k])
    # ComputeHessianF is symmetric term by term (blocks -S / S^T, (M S + S M) / 2): exactly so.  ComputeHessianG's blocks are symmetric as
    # formulas (hess(3,0) = -(hess(0,0) S)^T against hess(0,3) = -S / |g| + g g^T S / |g|^3) but not operation by operation.
    HF = np.array(HF, f64)
    assert np.array_equal(HF, HF.T)
    for H in Hn:
        H = np.array(H, f64)
        assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max()


def test_finished_plans_satisfy_their_constraints():
    """Wherever no INFEASIBLE bit is set the last iterate lies inside the shrunk polygon and every stance leg's length in [lMin, lMax], to
    the size of the last SQP step (the constraints are linearised: what one iteration leaves is second order in its step)."""
    g, rs = golden(), rerun32()
    d = P.Desc()
    n = 0
    for i, r in enumerate(rs):
        if r["cmd"] is None or r["flags"] & P.INFEASIBLE:
            continue
        c = g["cases"][i]
        st = dict(lam=list(g["after32"][i][:12]), size=int(g["after32"][i][12]))
        q, rIB = [f64(v) for v in g["after32"][i][16:20]], [f64(v) for v in g["after32"][i][13:16]]
        rIF, _ = P.world_feet(f64, c)
        rBH = [[f64(f32(d.rBH[3 * leg + k])) for k in range(3)] for leg in P.CCW]
        valid = [s for s in range(4) if (int(g["mask"][i]) >> s) & 1]
        vert = [rIF[s] for s in valid]
        gl = [[(rIB[k] + S.transform_vec_by_quat(f64, q, rBH[s])[k]) - rIF[s][k] for k in range(3)] for s in valid]
        Gv = P.assemble(f64, d, q, rIB, rIF, [rIF[s] for s in range(4)], rBH, valid, vert, gl, [f64(0.1)] * 12, [f64(0)] * 3)[3]
        step = np.abs(np.array(r["p"][-1], f64)).max()
        tol = 1e-5 + 4 * step
        assert min(float(v) for v in Gv) >= -tol, (i, g["cell_of"][i], min(float(v) for v in Gv), step)
        assert st["size"] == 3 * len(valid)
        n += 1
    assert n >= 80


def test_cells_are_not_decided_by_rounding():
    """The float32 and float64 restatements choose working sets of the same size in every iteration and set the same flags: per cell at most
    EXCLUDE_CAP of the cases may differ (they would be compared on flags only)."""
    g = golden()
    diff = np.any(g["iq32"] != g["iq64"], axis=1) | (g["flags32"] != g["flags64"])
    for k, name in enumerate(g["cells"]):
        a, b = g["cell_start"][k], g["cell_start"][k + 1]
        assert diff[a:b].sum() <= EXCLUDE_CAP * (b - a), (str(name), int(diff[a:b].sum()), int(b - a))
    # the cells are not trivial: constraints bind in a good share of them
    assert (g["iq32"][:, 0] > 0).sum() >= 20
    own = np.abs(g["cmd32"].astype(f64) - g["cmd64"])
    assert np.nanmax(own) < 1e-5


def not_pd_case():
    """A carried Lambda of 100 on the lower leg-length rows makes hessF - hessGSum indefinite."""
    c = golden()["cases"][0]
    st = P.new_state(f32, c["base_pos"])
    st["lam"] = [f32(0.1)] * 3 + [f32(100.0)] * 3 + [f32(0.1)] * 6
    st["size"] = 9
    return c, st


def infeasible_desc():
    return P.Desc(l_min=0.35, l_max=0.22)                          # contradictory leg-length window: every QP is infeasible


def test_every_flag_is_reached():
    g = golden()
    cell = lambda name: [i for i, c in enumerate(g["cell_of"]) if c == name]
    few = cell("flag_few")
    assert all(g["flags32"][i] & P.FEW_CONTACTS for i in few) and all(np.isnan(g["cmd32"][i]).all() for i in few)
    assert sum(int(v) == P.STANCE for v in g["cases"][few[0]]["desired_leg_state"]) == 2
    assert sum(int(v) == P.STANCE for v in g["cases"][few[1]]["desired_leg_state"]) == 0
    assert all(g["flags32"][i] & P.NAN for i in cell("flag_nan"))
    # Lambda grown: chain2 alternates N = 3 and N = 4, so every N = 4 plan after an N = 3 plan grows Lambda from 9 to 12
    ch = cell("chain2")
    assert [bool(g["flags32"][i] & P.LAMBDA_GROWN) for i in ch] == [False, True] * 4
    assert [int(g["after32"][i][12]) for i in ch] == [9, 12] * 4
    # non-convex: each invalidId path, the erased vertex is the foot pulled inside (slot of leg: 0 -> 0, 1 -> 3, 2 -> 1, 3 -> 2)
    nc = cell("four_nonconvex")
    erased = [(~int(g["mask"][i])) & 0xf for i in nc]
    assert all(g["flags32"][i] & P.NONCONVEX for i in nc) and erased == [1, 1, 8, 8, 2, 2, 4, 4] and all(g["N"][i] == 3 for i in nc)
    assert not any(g["flags32"][i] & P.NONCONVEX for i in cell("four_nominal") + cell("four_offset"))
    # not positive definite: fatal, the state stays
    c, st = not_pd_case()
    before = P.state_rows(f32, st)
    r = P.update(f32, P.Desc(), c, st)
    assert r["flags"] & P.NOT_PD and r["cmd"] is None and np.array_equal(P.state_rows(f32, st), before)
    # infeasible: the reference goes on with the iterate QuadProg++ had
    r = P.update(f32, infeasible_desc(), c, P.new_state(f32, c["base_pos"]))
    assert r["flags"] & P.INFEASIBLE and not r["flags"] & P.MAXITER and r["cmd"] is not None


def test_reset_base_pose():
    c = golden()["cases"][3]
    st = P.new_state(f32, c["base_pos"])
    fl, cmd = P.reset_base_pose(f32, P.Desc(), c, st)
    rIF, _ = P.world_feet(f64, c)
    assert fl == 0 and len(cmd) == 18 and all(v == 0 for v in cmd[12:]) and all(v == 0 for v in cmd[9:12]) and cmd[8] == f32(0.27)
    assert abs(float(cmd[6]) - np.mean([p[0] for p in rIF])) < 1e-6 and abs(float(cmd[7]) - np.mean([p[1] for p in rIF])) < 1e-6
    assert np.array_equal(np.array(cmd[:3], f32), c["base_pos"]) and np.array_equal(np.array(cmd[3:6], f32), c["rpy"])


def test_new_symbols_are_exported(pkg):
    lib = C.CDLL(pkg._build.build())
    for s in ("qrgpu_pose_plan_desc_default", "qrgpu_pose_plan_batch"):
        assert hasattr(lib, s), s
        assert s in pkg.qrgpu.EXPORTS
    d = pkg.pose_plan_desc()
    ref = P.Desc()
    assert list(d.rBH) == [f32(v) for v in ref.rBH] and d.loops == ref.loops == pkg.qrgpu.POSE_MAX_LOOPS
    assert [d.l_min, d.l_max, d.omega, d.eps, d.body_height] == [f32(v) for v in (ref.l_min, ref.l_max, ref.omega, ref.eps, ref.body_height)]
    assert (pkg.qrgpu.POSE_STATE_ROWS, pkg.qrgpu.POSE_OUT_ROWS) == (P.STATE_ROWS, P.OUT_ROWS)
    assert data_has_kernel(pkg)


def data_has_kernel(pkg):
    return b"qr_pose_plan_kernel" in open(pkg._build.build(), "rb").read()
