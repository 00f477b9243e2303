"""CPU: the float64 plant with a body of tests/body_contact_ref.py on its own -- its points' Jacobians, its equation of motion, its limit against
terrain_ref, the continuity of its laws, the robots' limits -- the conditions the seeded step case of tests/test_gpu_body_contact.py leans on, and
the two scenario chains that give that file its bands."""
import numpy as np
import pytest

import body_contact_ref as BR
import plant_ref as PR
import rigid_body_ref as M
import terrain_ref as TR


def _per_type(pkg, case):
    models, bodies = BR.models_and_bodies(pkg)
    for t in range(len(PR.ROBOTS)):
        yield t, models[t], bodies[t], np.nonzero(case["tid"] == t)[0]


def _moved(s, k, d):
    """The state s [n, 37] moved by d along the unit generalised velocity e_k for unit time: attitude quat (x) exp(d e_k) (body angular velocity), position
    + d R e_k (body linear velocity), joint + d."""
    o = s.copy()
    if k < 3:
        w = np.zeros((len(s), 3)); w[:, k] = d
        o[:, 0:4] = PR.quat_mul(s[:, 0:4], PR.quat_exp(w))
    elif k < 6:
        o[:, 4:7] += d * M.quat_to_rot(s[:, 0:4])[:, :, k - 3]
    else:
        o[:, 13 + k - 6] += d
    return o


def test_point_jacobians_are_the_derivatives_of_the_points(pkg):
    """J of all sixteen points against central differences of their positions along each of the 18 generalised velocities, step d = 1e-5.  Along a
    rotation a point at lever L moves on a circle: the difference's error is d^2 L / 6; L <= 0.75 m (trunk corner to foot, legs straight).  Along a
    translation the position is linear.  Plus the rounding of the two positions, 2 * 2.2e-16 Pmax / (2 d) per subtraction and as much again in the
    chains that place the point, Pmax <= 2 m: bar 1.25e-11 + 1.8e-10.  Measured 3.3e-11."""
    case = BR.step_case(pkg)
    d, L, pmax = 1e-5, 0.75, 2.0
    bar = d * d * L / 6 + 4 * 2.2e-16 * pmax / d
    worst = 0.0
    for t, model, body, k in _per_type(pkg, case):
        s = M.normalised(case["state"][k])
        P, _, J = BR.points(model, body, s)
        assert np.abs(P).max() <= pmax
        for g in range(18):
            hi, lo = BR.points(model, body, _moved(s, g, d))[0], BR.points(model, body, _moved(s, g, -d))[0]
            worst = max(worst, np.abs((hi - lo) / (2 * d) - J[..., g]).max())
    print("point Jacobians against central differences: %.2e (bar %.2e)" % (worst, bar))
    assert worst <= bar


def test_feet_are_rigid_body_refs_and_velocities_are_j_nu(pkg):
    """The foot rows of points() are rigid_body_ref.compute's pGC, vGC, Jc to the bit; every point's velocity is J nu to 1e-12."""
    case = BR.step_case(pkg)
    for t, model, body, k in _per_type(pkg, case):
        s = M.normalised(case["state"][k])
        P, V, J = BR.points(model, body, s)
        rb = M.compute(model, s)
        assert np.array_equal(P[:, BR.FEET], rb["pGC"]) and np.array_equal(V[:, BR.FEET], rb["vGC"]) and np.array_equal(J[:, BR.FEET], rb["Jc"])
        nu = np.concatenate([s[:, 7:13], s[:, 25:37]], 1)
        assert np.abs(np.einsum("npak,nk->npa", J, nu) - V).max() <= 1e-12 * max(1.0, np.abs(V).max())


def test_equation_of_motion_closes(pkg):
    """H nu_dot + C + G = [0; tau_motor + tau_lim] + sum over the sixteen points J^T f + [R^T moment; R^T force; 0] on the first-principles model, to
    1e-9 * max(1, |rhs|): the level the push test of test_terrain_ref.py reaches.  And each new term moves the result."""
    case = BR.step_case(pkg)
    p = PR.params(substeps=1, **TR.STEP_PARAMS)
    for t, model, body, k in _per_type(pkg, case):
        s = M.normalised(case["state"][k])
        push = case["push"][k].astype(np.float64)
        _, aux = BR.substep(model, body, p, case["D"], case["height"], case["fid"][k], push, s, case["cmd"][k], p["dt"])
        rhs = np.einsum("npak,npa->nk", aux["J"], aux["force"]) + TR.push_rhs(s, push)
        rhs[:, 6:] += aux["tau"] + aux["tlim"]
        lhs = np.einsum("nij,nj->ni", aux["H"], aux["nu_dot"]) + aux["C"] + aux["G"]
        res = np.abs(lhs - rhs) / np.maximum(1.0, np.abs(rhs))
        print("%s: equation residual %.2e" % (PR.ROBOTS[t], res.max()))
        assert res.max() <= 1e-9
        _, ter = TR.substep(model, p, case["D"], case["height"], case["fid"][k], push, s, case["cmd"][k], p["dt"])
        loaded = (aux["fn"][:, 4:] > 0).any(1) | (aux["tlim"] != 0).any(1)
        assert loaded.sum() >= 8
        assert np.abs(aux["nu_dot"] - ter["nu_dot"])[loaded].max(1).min() > 1e-3
        assert np.array_equal(aux["nu_dot"][~loaded], ter["nu_dot"][~loaded])


def test_clear_of_everything_is_terrain_ref(pkg):
    """The terrain step case's robots with every base 0.27 above the ground under it -- trunk and knees clear of the ground, joints inside their
    limits: step equals terrain_ref.step exactly, every output; body_out and the new status bits are zero.  A quarter of the feet or more are
    in contact."""
    case = BR.clear_case(pkg)
    models, bodies = BR.models_and_bodies(pkg)
    for substeps in (1, 2):
        p = PR.params(substeps=substeps, **TR.STEP_PARAMS)
        a = BR.step_mixed(models, bodies, case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
        b = TR.step_mixed(models, case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
        for key, v in b.items():
            assert np.array_equal(a[key][:, :4] if key in ("fn", "off") else a[key], v), key
        assert not a["body_out"].any() and not a["fn"][:, 4:].any()
        assert not (a["status"] & (BR.PL_TRUNK_CONTACT | BR.PL_KNEE_CONTACT | BR.PL_JOINT_LIMIT)).any()
        assert (a["fn"][:, BR.FEET] > 0).sum() >= 48


def test_laws_are_continuous_across_their_thresholds(pkg):
    """tau_lim on either side of each limit, +-1e-9 rad at joint rates of +-10 rad/s, and every point's force on either side of the surface, +-1e-9 m:
    the one-sided evaluations differ by at most k x (1 + a |qd|) resp. contact_k x (1 + contact_a |v|) (1 + mu) at x = 2e-9, and are zero on the
    inner side."""
    rng = np.random.default_rng(31)
    eps = 1e-9
    for robot in PR.ROBOTS:
        body = BR.body_of(pkg.plant_body_desc(robot))
        qd = rng.uniform(-10, 10, (64, 12))
        for lim, sign in ((np.tile(body["q_hi"], 4), 1.0), (np.tile(body["q_lo"], 4), -1.0)):
            q = np.broadcast_to(lim, (64, 12))
            inside, beyond = BR.limit_torque(body, q - sign * eps, qd), BR.limit_torque(body, q + sign * eps, qd)
            assert not inside.any() and not BR.limit_torque(body, q, qd).any()
            assert np.all(sign * beyond <= 0) and np.abs(beyond).max() <= body["limit_k"] * 2 * eps * (1 + body["limit_a"] * 10)
            assert (beyond != 0).sum() >= 300
    # the points: each of the sixteen of the step case's robots put on the surface under it, then +-eps along z
    case = BR.step_case(pkg)
    p = PR.params(substeps=1, **TR.STEP_PARAMS)
    for t, model, body, k in _per_type(pkg, case):
        s = M.normalised(case["state"][k])
        P, V, _ = BR.points(model, body, s)
        fid = np.asarray(case["fid"][k])
        z = TR.sample(case["D"], case["height"], fid[:, None], P[..., 0], P[..., 1])[0] + p["ground_z"]
        on = P.copy(); on[..., 2] = z
        up, down = on.copy(), on.copy()
        up[..., 2] += eps; down[..., 2] -= eps
        f_up, f_down = BR.point_forces(p, case["D"], case["height"], fid, up, V)[0], BR.point_forces(p, case["D"], case["height"], fid, down, V)[0]
        speed = np.linalg.norm(V, axis=-1)
        assert not f_up.any()
        assert np.all(np.linalg.norm(f_down, axis=-1) <= p["contact_k"] * 2 * eps * (1 + p["contact_a"] * speed) * (1 + p["mu"]))
        assert (f_down[..., 2] > 0).sum() >= 100


def test_stand_pose_lies_inside_the_limits(pkg):
    """Each robot's stand pose strictly inside its limits, with a tenth of a radian to spare; the trunk boxes and the limits are the robots' own."""
    for robot in PR.ROBOTS:
        body = BR.body_of(pkg.plant_body_desc(robot))
        pose = M.STAND_POSE[:3]
        assert np.all(body["q_lo"] + 0.1 < pose) and np.all(pose < body["q_hi"] - 0.1), robot
        assert np.all(body["trunk_half"] > 0) and not body["trunk_center"].any() and body["limit_k"] > 0 and body["limit_a"] > 0
    a1, l3 = (BR.body_of(pkg.plant_body_desc(r)) for r in PR.ROBOTS)
    assert np.allclose(2 * a1["trunk_half"], [0.267, 0.194, 0.114], rtol=1e-6) and np.allclose(2 * l3["trunk_half"], [0.234, 0.184, 0.08], rtol=1e-6)
    assert np.allclose(np.degrees(a1["q_lo"]), [-46, -60, -154.5], atol=1e-4) and np.allclose(np.degrees(a1["q_hi"]), [46, 240, -52.5], atol=1e-4)
    assert np.allclose(l3["q_lo"], [-0.523, -0.314, -2.792], atol=1e-6) and np.allclose(l3["q_hi"], [0.523, 2.67, -0.524], atol=1e-6)
    # the default stops at the default sub-step: omega h <= 0.2 on the smallest reflected inertia, the knee link about its axis (the rotor adds 1e-8)
    I_knee = float(M.KNEE["I"][1, 1] + M.KNEE["m"] * (M.KNEE["c"][0] ** 2 + M.KNEE["c"][2] ** 2) + M.ROTOR_I[1, 1])
    h = PR.DEFAULTS["dt"] / PR.DEFAULTS["substeps"]
    assert h == 0.001 and np.sqrt(a1["limit_k"] / I_knee) * h <= 0.2


@pytest.mark.parametrize("substeps", PR.STEP_SUBSTEPS)
def test_step_case_meets_what_the_gpu_test_leans_on(pkg, substeps):
    """On the reference alone, in the last sub-step at every sub-step count: at least 16 loaded corners, at least 4 of them top corners; at least 16
    loaded knees; at least 16 joints with tau_lim != 0, on both sides of the limits; at least 8 loaded points that are no feet off the grid; at most
    2 % of the 768 contact flags within 1e-6 of the threshold; no point within 1e-6 cell of a border line; everything finite; every family holds both
    types and both fields.  Measured at 1 / 2 / 8 sub-steps: loaded corners 67 / 67 / 67 (top 32), knees 49 / 46 / 49, joints at a stop 18 (11 high,
    7 low), off the grid 11, near the threshold 0."""
    case = BR.step_case(pkg)
    models, bodies = BR.models_and_bodies(pkg)
    p = PR.params(substeps=substeps, **TR.STEP_PARAMS)
    r = BR.step_mixed(models, bodies, case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
    fn, off, tl = r["fn"], r["off"], r["tlim"]
    loose, _ = BR.status_masks(p, fn)
    print("substeps", substeps, "corners", (fn[:, BR.CORNERS] > 0).sum(), "top", (fn[:, BR.TOP] > 0).sum(), "knees", (fn[:, BR.KNEES] > 0).sum(), "stops high",
          (tl < 0).sum(), "low", (tl > 0).sum(), "off the grid", (off[:, 4:] & (fn[:, 4:] > 0)).sum(), "near threshold", loose.sum())
    assert fn.shape == (48, 16)
    assert (fn[:, BR.CORNERS] > 0).sum() >= 16 and (fn[:, BR.TOP] > 0).sum() >= 4
    assert (fn[:, BR.KNEES] > 0).sum() >= 16
    assert (tl != 0).sum() >= 16 and (tl < 0).sum() >= 4 and (tl > 0).sum() >= 4
    assert (off[:, 4:] & (fn[:, 4:] > 0)).sum() >= 8
    assert loose.sum() <= 0.02 * fn.size
    assert np.all(np.isfinite(r["fb_state"])) and np.all(np.isfinite(r["plant_out"])) and np.all(np.isfinite(r["body_out"]))
    # the points of the last sub-step: one sub-step less from the same start
    s = M.normalised(case["state"])
    for t, model, body, k in _per_type(pkg, case):
        sk = s[k]
        for _ in range(substeps - 1):
            sk, _ = BR.substep(model, body, p, case["D"], case["height"], case["fid"][k], case["push"][k], sk, case["cmd"][k], p["dt"] / substeps)
        assert not TR.near_border(case["D"], BR.points(model, body, sk)[0]).any()
    for b in (BR.PL_TRUNK_CONTACT, BR.PL_KNEE_CONTACT, BR.PL_JOINT_LIMIT, TR.PL_OFF_FIELD):
        assert 4 <= ((r["status"] & b) != 0).sum() <= 44, hex(b)
    assert (r["status"] == 0).sum() >= 4
    for f in range(len(BR.FAMILIES)):
        k = case["family"] == f
        assert set(case["tid"][k]) == {0, 1} and set(case["fid"][k]) == {0, 1}, f
    # the wide family is what meets the stops; belly, kneeling and back are what load corners and knees
    wide = case["family"] == BR.FAMILIES.index("wide")
    assert (tl[wide] != 0).sum() >= 12
    assert (fn[case["family"] == BR.FAMILIES.index("back")][:, BR.TOP] > 0).sum() >= 4


def test_fall_chains_give_the_bands_of_the_gpu_test(pkg):
    """The two float64 chains -- limp drop from z = 0.30, and the same rolled by pi; 1400 ticks of 1 ms at 2 sub-steps, all gains and torques zero --
    end at the values and with the residual swing over their last 350 ticks that body_contact_ref.FALL_END / FALL_SWING record for the GPU test (bands:
    end +- 3 swing).  Asserted outright, because the law gives them: every state finite, the base origin above the ground at the end.  And what the
    feature is for: TRUNK_CONTACT at the end in both, JOINT_LIMIT seen in the limp drop."""
    r = BR.fall_chains(pkg)
    for name in BR.SCENARIOS:
        x = r[name]
        print("%s: end %s swing %s seen %s at the end %s" % (name, x["end"], x["swing"], hex(x["seen"]), hex(x["status"])))
        assert x["finite"]
        assert x["state"][6] > 0.0
        assert x["status"] & BR.PL_TRUNK_CONTACT
        end, swing = np.array(BR.FALL_END[name]), np.array(BR.FALL_SWING[name])
        # (a bouncing robot amplifies the last place of a solve: the recorded values are asserted to a swing, not to 1e-5 as the slope chain's)
        assert np.all(np.abs(x["end"] - end) <= swing)
        assert np.all(x["swing"] <= 2 * swing) and np.all(x["swing"] >= 0.5 * swing)
        assert np.all(swing > 0)
    assert r["limp"]["seen"] & BR.PL_JOINT_LIMIT
