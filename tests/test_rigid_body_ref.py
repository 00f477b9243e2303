"""CPU: the first-principles rigid-body model (tests/rigid_body_ref.py) against mechanics, and the oracle's float64 rigid-body quantities
against the model, on three seeded state families of both robots (stand = make_batch, wide = far off the stand pose, edge list).

This is the second link of the chain  kernel -> oracle -> mechanics  (the first is tests/test_gpu_rigid_body.py).

The chain has two links because a float32 quaternion is not unit (norm defect up to 8e-8): the oracle and the kernel feed it unnormalised
into 1 - 2(y^2 + z^2), so their R is not orthogonal and G, Jc, Jcdqd, pGC, vGC sit up to about 1e-6 from what the normalised model gives
(test_unnormalised_float32_quaternion measures it).  The oracle is compared with the model on the normalised float64 state, at 1e-10.

Finite-difference bars are the truncation error of the central difference, h^2/6 * sup|f'''|, plus its rounding error, 64 eps sup|f| / h
(64: the few dozen accumulations behind an energy or a position).  sup|f'''| comes from Bernstein's inequality: along a flow the functions
differenced are sums of products of sines and cosines of the angles, i.e. of exponential type Omega = the sum of the rates of the angles
that multiply, so |f'''| <= Omega^3 sup|f|, and sup|f| is bounded over ALL configurations from the speeds and the robot's reach.
"""
import numpy as np
import pytest

import rigid_body_ref as M

ROBOTS = ("a1", "lite3")
EPS = np.finfo(np.float64).eps
REACH_BASE = 0.75      # >= |any point of the robot - base origin|: |abad_loc| 0.187 + hip_l <= 0.0985 + upper + lower 0.4 + foot_y 0.004 = 0.69
REACH_LEG = 0.55       # >= |any point of a leg - its abad axis|: 0.0985 + 0.4 + 0.004 (+ c.o.m. offsets inside the links)
SUM_TRACE_I = 0.2      # >= sum over bodies of trace(I): body 0.0993, four legs of 0.0018 + 0.0120 + 0.0060
M_LEG = 1.9            # >= mass of one leg: 0.696 + 1.013 + 0.166


@pytest.fixture(scope="module")
def fam(pkg):
    """float64 normalised states per robot and family, and the model's quantities on them (computed once, shared, read-only)."""
    out = {}
    for robot in ROBOTS:
        f = M.families(pkg, robot)
        for name, s32 in f.items():
            s = M.normalised(s32)
            out[robot, name] = dict(s32=s32, s=s, ref=M.compute(pkg.model_desc(robot), s))
    return out


def _cases(fam):
    return [(robot, name, fam[robot, name]) for robot in ROBOTS for name in ("stand", "wide", "edge")]


def _leg_rate(s):
    """max over legs of |qd_abad| + |qd_hip| + |qd_knee|, per state."""
    return np.abs(s[:, 25:37]).reshape(-1, 4, 3).sum(2).max(1)


def flow(s, nu, t):
    """The state after time t of constant generalised velocity nu [n,18] (body frame): attitude by the body-frame exponential, joints linearly,
    position to second order (p' = R v, p'' = R (w x v))."""
    s2 = s.copy()
    w, v = nu[:, 0:3], nu[:, 3:6]
    ang = np.linalg.norm(w, axis=1) * t
    wn = np.where(np.linalg.norm(w, axis=1, keepdims=True) > 0, w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300), 0.0)
    dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * wn], axis=1)
    a, b = s[:, 0:4], dq
    s2[:, 0] = a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(1)
    s2[:, 1:4] = a[:, 0:1] * b[:, 1:] + b[:, 0:1] * a[:, 1:] + np.cross(a[:, 1:], b[:, 1:])
    R = M.quat_to_rot(s[:, 0:4])
    s2[:, 4:7] = s[:, 4:7] + t * M._mv(R, v) + 0.5 * t * t * M._mv(R, np.cross(w, v))
    s2[:, 13:25] = s[:, 13:25] + t * nu[:, 6:18]
    return s2


def _nu(s):
    return np.concatenate([s[:, 7:13], s[:, 25:37]], axis=1)


# ------------------------------------------------------------------------------------------------ the model against mechanics
def test_model_power_balance(fam, pkg):
    """nu' C = dT/dt along constant nu (with no force and no gravity H nu_dot = -C and the energy is conserved, so nu' C = 1/2 nu' H_dot nu).
    T = 1/2 nu' H(q) nu depends on the joint angles only: central difference over q +- h qd, h = 1e-6 s.
    T(t) is of exponential type Omega = 2 * max over legs of sum|qd_leg| (H is quadratic in the legs' rotation matrices) and bounded by
    Tb = 1/2 m (|v| + REACH_BASE |w| + REACH_LEG S)^2 + 1/2 SUM_TRACE_I (|w| + S)^2, S = max leg rate, in every configuration, so the bar is
    h^2/6 Omega^3 Tb + 64 eps Tb / h: 1e-3 at most on the fastest wide states (where |nu' C| reaches 150; measured error 7e-8), 1e-7 on the stand family."""
    h = 1e-6
    worst = 0.0
    for robot, name, f in _cases(fam):
        s, r, md = f["s"], f["ref"], pkg.model_desc(robot)
        nu = _nu(s)
        sp, sm = s.copy(), s.copy()
        sp[:, 13:25] += h * s[:, 25:37]; sm[:, 13:25] -= h * s[:, 25:37]
        dT = (M.compute(md, sp)["T"] - M.compute(md, sm)["T"]) / (2 * h)
        S = _leg_rate(s)
        wn, vn = np.linalg.norm(s[:, 7:10], axis=1), np.linalg.norm(s[:, 10:13], axis=1)
        Tb = 0.5 * M.total_mass() * (vn + REACH_BASE * wn + REACH_LEG * S) ** 2 + 0.5 * SUM_TRACE_I * (wn + S) ** 2
        bar = h * h / 6 * (2 * S) ** 3 * Tb + 64 * EPS * Tb / h
        err = np.abs(np.einsum("ni,ni->n", nu, r["C"]) - dT)
        print("power balance %-5s %-5s worst err %.2e  worst err/bar %.2e  max|nu'C| %.2e" % (robot, name, err.max(), (err / np.maximum(bar, 1e-300)).max(),
                                                                                          np.abs(dT).max()))
        assert np.all(err <= bar), (robot, name, int(np.argmax(err - bar)), err.max())
        worst = max(worst, np.abs(dT).max())
    assert worst > 100.0           # the wide family does exercise C


def test_model_gravity_is_the_gradient_of_the_potential(fam, pkg):
    """G = grad V, V = sum m 9.81 z_c.  Joints: central difference, h = 1e-4 rad; V is sinusoidal in one joint angle with amplitude
    <= 9.81 M_LEG REACH_LEG, which bounds V''' too; |V| <= m 9.81 (|z| + REACH_BASE).  Bar h^2/6 * 9.81 M_LEG REACH_LEG + 64 eps |V|max / h = 4e-8.
    Base rows from positions, not differences: the weight at the centre of mass, force R'(0,0,mg) and moment R'((c - p) x (0,0,mg))."""
    h = 1e-4
    for robot, name, f in _cases(fam):
        s, r, md = f["s"], f["ref"], pkg.model_desc(robot)
        bar = h * h / 6 * 9.81 * M_LEG * REACH_LEG + 64 * EPS * M.total_mass() * 9.81 * (np.abs(s[:, 6]) + REACH_BASE) / h
        sp, sm = np.repeat(s, 12, axis=0), np.repeat(s, 12, axis=0)                    # row 12 i + j: state i, joint j moved
        step = np.tile(h * np.eye(12), (len(s), 1))
        sp[:, 13:25] += step; sm[:, 13:25] -= step
        g = ((M.compute(md, sp)["V"] - M.compute(md, sm)["V"]) / (2 * h)).reshape(len(s), 12)
        err = np.abs(g - r["G"][:, 6:]).max(1)
        assert np.all(err <= bar), (robot, name, err.max())
        R = M.quat_to_rot(s[:, 0:4])
        Wt = np.array([0.0, 0.0, r["mass"] * 9.81])
        force = np.einsum("nji,j->ni", R, Wt)
        moment = np.einsum("nji,nj->ni", R, np.cross(r["com"] - s[:, 4:7], Wt))
        eb = max(np.abs(r["G"][:, 3:6] - force).max(), np.abs(r["G"][:, 0:3] - moment).max())
        print("gravity %-5s %-5s joints worst err %.2e (bar %.1e)  base rows %.2e" % (robot, name, err.max(), bar.min(), eb))
        assert eb <= 1e-12 * r["mass"] * 9.81
        assert abs(r["mass"] - M.total_mass()) < 1e-14


def test_model_foot_jacobian_is_the_derivative_of_the_foot_position(fam, pkg):
    """Jc[:, :, k] = d pGC / dt along nu = e_k: central difference over the flow, h = 1e-4.  A foot turns about any axis at a radius
    <= REACH_BASE, so |p'''| <= REACH_BASE (translations: 0).  Bar h^2/6 REACH_BASE + 64 eps (|pos| + REACH_BASE) / h = 1.3e-9."""
    h = 1e-4
    for robot, name, f in _cases(fam):
        s, r, md = f["s"], f["ref"], pkg.model_desc(robot)
        bar = h * h / 6 * REACH_BASE + 64 * EPS * (np.linalg.norm(s[:, 4:7], axis=1) + REACH_BASE) / h
        s18, e = np.repeat(s, 18, axis=0), np.tile(np.eye(18), (len(s), 1))               # row 18 i + k: state i flowing along e_k
        d = ((M.compute(md, flow(s18, e, h))["pGC"] - M.compute(md, flow(s18, e, -h))["pGC"]) / (2 * h)).reshape(len(s), 18, 4, 3)
        err = np.abs(d.transpose(0, 2, 3, 1) - r["Jc"]).max((1, 2, 3))
        print("Jc %-5s %-5s worst err %.2e (bar %.1e)" % (robot, name, err.max(), bar.min()))
        assert np.all(err <= bar), (robot, name, err.max())


def test_model_foot_bias_acceleration_is_the_derivative_of_the_foot_velocity(fam, pkg):
    """Jcdqd = d vGC / dt along the constant-nu flow: central difference, h = 1e-5 s.  vGC(t) is of exponential type Omega = |w| + S (the base's
    rotation times one leg's) and bounded by Vb = |v| + REACH_BASE |w| + REACH_LEG S.  Bar h^2/6 Omega^3 Vb + 64 eps Vb / h: 1e-4 on the fastest
    wide states (|Jcdqd| in the hundreds), 1e-9 on the stand family."""
    h = 1e-5
    seen = 0.0
    for robot, name, f in _cases(fam):
        s, r, md = f["s"], f["ref"], pkg.model_desc(robot)
        nu = _nu(s)
        d = (M.compute(md, flow(s, nu, h))["vGC"] - M.compute(md, flow(s, nu, -h))["vGC"]) / (2 * h)
        S = _leg_rate(s)
        wn, vn = np.linalg.norm(s[:, 7:10], axis=1), np.linalg.norm(s[:, 10:13], axis=1)
        Vb = vn + REACH_BASE * wn + REACH_LEG * S
        bar = h * h / 6 * (wn + S) ** 3 * Vb + 64 * EPS * Vb / h
        err = np.abs(d - r["Jcdqd"]).max((1, 2))
        print("Jcdqd %-5s %-5s worst err %.2e  worst err/bar %.2e  max|Jcdqd| %.2e" % (robot, name, err.max(), (err / np.maximum(bar, 1e-300)).max(),
                                                                                      np.abs(r["Jcdqd"]).max()))
        assert np.all(err <= bar), (robot, name, err.max())
        seen = max(seen, np.abs(r["Jcdqd"]).max())
    assert seen > 100.0


def test_model_structure(fam):
    """What holds by construction of mechanics: H symmetric positive definite with the total mass on the translation block; vGC = Jc nu;
    nu = e_k states: vGC = Jc[:, :, k]; rest states: C, Jcdqd, vGC vanish; q and -q are the same attitude."""
    for robot, name, f in _cases(fam):
        s, r = f["s"], f["ref"]
        assert np.abs(r["H"] - np.swapaxes(r["H"], 1, 2)).max() < 1e-13 and np.linalg.eigvalsh(r["H"]).min() > 0
        assert np.abs(r["H"][:, 3:6, 3:6] - r["mass"] * np.eye(3)).max() < 1e-13
        assert np.abs(np.einsum("nlik,nk->nli", r["Jc"], _nu(s)) - r["vGC"]).max() <= 1e-13 * max(1.0, np.abs(r["vGC"]).max())
    for robot in ROBOTS:
        r = fam[robot, "edge"]["ref"]
        for row in M.UNIT_EDGES:
            assert np.abs(r["vGC"][row] - r["Jc"][row][:, :, row - 5]).max() <= 1e-14
        for row in M.REST_EDGES:
            assert max(np.abs(r[k][row]).max() for k in ("C", "Jcdqd", "vGC")) == 0.0
        a, b = M.NEG_PAIR
        assert fam[robot, "edge"]["s"][a, 0] > 0 > fam[robot, "edge"]["s"][b, 0]
        for k in M.QUANTITIES:
            assert np.array_equal(r[k][a], r[k][b]), k
    assert (fam["a1", "wide"]["s"][:, 0] < 0).any() and (fam["a1", "wide"]["s"][:, 0] > 0).any()


# ------------------------------------------------------------------------------------------------ the oracle against the model
def test_oracle_float64_against_the_model(fam, pkg, oracle):
    """Same float64 state, quaternion normalised, every state of every family, all seven quantities: <= 1e-10 * max(1, max|x|) -- both sides are
    float64 evaluations of the same function (the bar test_golden_wbc uses for these quantities).  Measured: 1.0e-14 (C and vGC, wide family)."""
    worst = {}
    for robot, name, f in _cases(fam):
        md, s, r = pkg.model_desc(robot), f["s"], f["ref"]
        o = [oracle.fb_compute(md, s[i], np.float64) for i in range(len(s))]
        for k in M.QUANTITIES:
            ok = np.stack([x[k] for x in o])
            gap = np.abs(ok - r[k]).reshape(len(s), -1).max(1) / np.maximum(1.0, np.abs(r[k]).reshape(len(s), -1).max(1))
            worst[robot, name, k] = gap.max()
            assert gap.max() <= 1e-10, (robot, name, k, int(gap.argmax()), gap.max())
        if name == "edge":
            for row in M.UNIT_EDGES:           # nu = e_k: the oracle's foot velocity is column k of its own Jacobian
                assert np.abs(o[row]["vGC"] - o[row]["Jc"][:, :, row - 5]).max() <= 1e-12
            for row in M.REST_EDGES:
                assert max(np.abs(o[row][k]).max() for k in ("C", "Jcdqd", "vGC")) <= 1e-12
    for name in ("stand", "wide", "edge"):
        print("oracle f64 vs model, %-5s: " % name + "  ".join("%s %.1e" % (k, max(worst[r, name, k] for r in ROBOTS)) for k in M.QUANTITIES))
    print("oracle f64 vs model, worst gap %.2e" % max(worst.values()))


def test_unnormalised_float32_quaternion(fam, pkg, oracle):
    """The oracle on the raw float32 state (widened; its quaternion is off the unit sphere by up to 8e-8) against the model, which normalises.
    H and C live in body coordinates and do not see the attitude: within 1e-10 * max(1, max|x|).  G, Jc, Jcdqd, pGC, vGC move with R's lost
    orthogonality; the worst relative gaps are printed and recorded in LAB_NOTES.md (G 1.0e-7, Jc 1.1e-7, Jcdqd 2.3e-7, pGC 4.6e-7, vGC 1.0e-6), with no bar: that gap
    is the effect that forces the two-link chain, not an error of either side."""
    worst = {k: 0.0 for k in M.QUANTITIES}
    defect = 0.0
    for robot, name, f in _cases(fam):
        md, r = pkg.model_desc(robot), f["ref"]
        raw = f["s32"].astype(np.float64)
        defect = max(defect, np.abs(np.linalg.norm(raw[:, 0:4], axis=1) - 1).max())
        for i in range(len(raw)):
            o = oracle.fb_compute(md, raw[i], np.float64)
            for k in M.QUANTITIES:
                worst[k] = max(worst[k], np.abs(o[k] - r[k][i]).max() / max(1.0, np.abs(r[k][i]).max()))
    print("float32 quaternion: norm defect %.1e; oracle(raw) vs model(normalised): " % defect + "  ".join("%s %.1e" % kv for kv in worst.items()))
    assert worst["H"] <= 1e-10 and worst["C"] <= 1e-10
    assert defect > 1e-8            # the families do carry the effect


def test_floating_base_dynamics_with_the_models_matrices(fam, pkg, oracle):
    """The oracle's float64 WBC solution obeys the equations of motion written with the MODEL's matrices, on the stand and wide families:
    (H qdd + C + G - sum Jc' f)[0:6] = 0 and [6:] = tau, to 1e-8 and 1e-9 times max(1, max|tau|) -- the bars of
    test_wbc_satisfies_floating_base_dynamics, scaled because torques reach the thousands of N m far off the stand pose."""
    worst = [0.0, 0.0]
    tau_max = 0.0
    for robot in ROBOTS:
        md = pkg.model_desc(robot)
        cs = M.wbc_cases(pkg, oracle, robot)
        s = M.normalised(cs["state"])
        r = M.compute(md, s)
        for i in range(len(s)):
            c = cs["cmd"][i].astype(np.float64)
            w = oracle.wbc_run(md, s[i], c, cs["prev"][i].astype(np.float64), dtype=np.float64)
            assert w["rc"] == 0
            gen = r["H"][i] @ w["qddot"] + r["C"][i] + r["G"][i]
            for k, leg in enumerate([l for l in range(4) if c[63 + l] != 0]):
                gen -= r["Jc"][i, leg].T @ w["fr"][3 * k:3 * k + 3]
            scale = max(1.0, np.abs(w["tau"]).max())
            worst = [max(worst[0], np.abs(gen[:6]).max() / scale), max(worst[1], np.abs(gen[6:] - w["tau"]).max() / scale)]
            tau_max = max(tau_max, np.abs(w["tau"]).max())
            assert np.abs(gen[:6]).max() <= 1e-8 * scale, (robot, i)
            assert np.abs(gen[6:] - w["tau"]).max() <= 1e-9 * scale, (robot, i)
    print("floating-base dynamics with the model's matrices: base rows %.1e, joint rows %.1e (relative), max|tau| %.0f" % (worst[0], worst[1], tau_max))


def test_wbc_cases_are_well_conditioned(pkg, oracle):
    """The condition under which the GPU file asserts 1e-6 on the torques: on every state used the float64 oracle succeeds and amplifies a
    1e-12 relative perturbation of state and command by less than 1e6 (relative to max(1,|tau|)), so the float32 rounding of the OUTPUT is
    what the 1e-6 bar has to cover, not conditioning.  Also records how far the float32 oracle is from its own float64 evaluation on the wide
    family (1.8e-3 of max(1,|tau|): why the 1e-4 float32-oracle bar is not asserted there)."""
    for robot in ROBOTS:
        md = pkg.model_desc(robot)
        cs = M.wbc_cases(pkg, oracle, robot)
        assert len(cs["state"]) == M.N_STAND + M.N_WIDE and np.all(cs["amp"] < M.AMPLIFICATION_MAX)
        gap = np.zeros(len(cs["state"]))
        for i in range(len(gap)):
            w64 = oracle.wbc_run(md, cs["state"][i].astype(np.float64), cs["cmd"][i].astype(np.float64), cs["prev"][i].astype(np.float64), dtype=np.float64)
            w32 = oracle.wbc_run(md, cs["state"][i], cs["cmd"][i], cs["prev"][i], dtype=np.float32)
            assert w64["rc"] == 0
            gap[i] = (np.abs(w32["tau"] - w64["tau"]) / np.maximum(1.0, np.abs(w64["tau"]))).max()
        print("wbc cases %-5s: worst amplification stand %.1e wide %.1e, redrawn %d; float32 oracle vs float64 oracle: stand %.1e wide %.1e"
              % (robot, cs["amp"][:M.N_STAND].max(), cs["amp"][M.N_STAND:].max(), cs["redrawn"], gap[:M.N_STAND].max(), gap[M.N_STAND:].max()))
