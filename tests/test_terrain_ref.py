"""CPU: the float64 terrain plant of tests/terrain_ref.py on its own -- the sampler's exactness on planes, its continuity, its slopes, the flat
limit against plant_ref, the push in the equations of motion -- and the conditions the seeded cases of tests/test_gpu_terrain.py lean on."""
import numpy as np
import pytest

import plant_ref as PR
import rigid_body_ref as M
import terrain_ref as TR


def _rough(pkg):
    """The two-field stack of the GPU step test."""
    case = TR.step_case(pkg)
    return case["D"], case["height"]


def test_sampler_reproduces_a_plane(pkg):
    """A 64 x 64 plane whose nodes are exact in float32 (cell 1/8, slopes 1/4 and -1/2): height and both slopes to 1e-12 wherever the 4 x 4 stencil
    is not clamped, i.e. at least one cell away from the border.  Measured: height 1.3e-15, slopes 8.6e-15."""
    T = pkg.terrain
    g = T.Grid(64, 64, -4.0, -4.0, 0.125)
    sx, sy = 0.25, -0.5
    h = T.stack([T.plane(g, sx, sy)])
    D = TR.desc(n_fields=1, **g.desc())
    rng = np.random.default_rng(17)
    lo, hi = -4.0 + 0.125, -4.0 + 62 * 0.125
    x, y = rng.uniform(lo, hi, 4000), rng.uniform(lo, hi, 4000)
    x[:64] = -4.0 + 0.125 * np.arange(1, 65).clip(1, 62)            # on grid lines too
    z, zx, zy, off = TR.sample(D, h, 0, x, y)
    print("plane: height %.2e, slopes %.2e %.2e" % (np.abs(z - (sx * x + sy * y)).max(), np.abs(zx - sx).max(), np.abs(zy - sy).max()))
    assert not off.any()
    assert np.abs(z - (sx * x + sy * y)).max() <= 1e-12
    assert np.abs(zx - sx).max() <= 1e-12 and np.abs(zy - sy).max() <= 1e-12


def test_surface_is_continuous_across_grid_lines_and_at_the_border(pkg):
    """Height and both slopes on either side of a grid line, +-1e-9 cell, agree to 1e-7 (the surface is C1: picking the cell on either side gives
    the same height and normal); the same at the four border lines, where the outer side is the border's own value."""
    D, h = _rough(pkg)
    c = D["cell"]
    eps = 1e-9 * c
    xs, ys = D["x0"] + c * np.arange(D["nx"]), D["y0"] + c * np.arange(D["ny"])
    rng = np.random.default_rng(18)
    worst = 0.0
    for f in (0, 1):
        for line, other, along_x in ((xs, rng.uniform(ys[0] - 0.2, ys[-1] + 0.2, 50), True), (ys, rng.uniform(xs[0] - 0.2, xs[-1] + 0.2, 50), False)):
            a, b = np.meshgrid(line, other)
            lo = TR.sample(D, h, f, a - eps, b) if along_x else TR.sample(D, h, f, b, a - eps)
            hi = TR.sample(D, h, f, a + eps, b) if along_x else TR.sample(D, h, f, b, a + eps)
            for u, v in zip(lo[:3], hi[:3]):
                worst = max(worst, np.abs(u - v).max())
            # across the first and last line the flag changes, the surface does not
            assert lo[3][:, 0].all() and not hi[3][:, 0][(other >= (ys[0] if along_x else xs[0])) & (other <= (ys[-1] if along_x else xs[-1]))].any()
    print("one-sided evaluations differ by at most %.2e" % worst)
    assert worst <= 1e-7


def test_outside_the_grid_is_the_nearest_border_point(pkg):
    D, h = _rough(pkg)
    c = D["cell"]
    x1, y1 = D["x0"] + (D["nx"] - 1) * c, D["y0"] + (D["ny"] - 1) * c
    rng = np.random.default_rng(19)
    x, y = rng.uniform(D["x0"] - 1, x1 + 1, 500), rng.uniform(D["y0"] - 1, y1 + 1, 500)
    for f in (0, 1):
        a = TR.sample(D, h, f, x, y)
        b = TR.sample(D, h, f, np.clip(x, D["x0"], x1), np.clip(y, D["y0"], y1))
        for u, v in zip(a[:3], b[:3]):
            assert np.abs(u - v).max() <= 1e-12          # (x - x0) / cell at the clipped x may round to the last place of nx - 1
        assert np.array_equal(a[3], (x < D["x0"]) | (x > x1) | (y < D["y0"]) | (y > y1)) and not b[3].any()


def test_slopes_are_the_derivatives_of_the_height(pkg):
    """Central differences of the height with step d = 1e-4 cell, inside one cell (t in 0.01..0.99), where the height is a cubic in x and in y: the
    difference's error is d^2 / 6 |z'''| with z''' = 3 (-h0 + 3 h1 - 3 h2 + h3) / cell^3 of rows already blended by weights of absolute sum <= 1.25, so
    at most 1.25 * 4 d^2 Hmax / cell^3, plus the rounding of the two heights, 4 * 2.2e-16 Hmax / d.  Bar 1.7e-7; measured 1.0e-8."""
    D, h = _rough(pkg)
    c = D["cell"]
    d = 1e-4 * c
    hmax = float(np.abs(h).max())
    bar = 1.25 * 4 * d * d * hmax / c ** 3 + 4 * 2.2e-16 * hmax / d
    rng = np.random.default_rng(20)
    i, j = rng.integers(0, D["nx"] - 1, 3000), rng.integers(0, D["ny"] - 1, 3000)
    x = D["x0"] + c * (i + rng.uniform(0.01, 0.99, 3000)); y = D["y0"] + c * (j + rng.uniform(0.01, 0.99, 3000))
    worst = 0.0
    for f in (0, 1):
        _, zx, zy, _ = TR.sample(D, h, f, x, y)
        dx = (TR.sample(D, h, f, x + d, y)[0] - TR.sample(D, h, f, x - d, y)[0]) / (2 * d)
        dy = (TR.sample(D, h, f, x, y + d)[0] - TR.sample(D, h, f, x, y - d)[0]) / (2 * d)
        worst = max(worst, np.abs(zx - dx).max(), np.abs(zy - dy).max())
    print("slopes against central differences: %.2e (bar %.2e)" % (worst, bar))
    assert worst <= bar


def test_flat_field_without_push_is_plant_ref(pkg):
    """All-zero field, no push: terrain_ref.step equals plant_ref.step to 1e-12 on the 48 mixed robots, every output.  Measured: 0."""
    s, c, tid = PR.step_cases()
    models = [pkg.model_desc(r) for r in PR.ROBOTS]
    D = TR.desc(n_fields=1, **TR.STEP_GRID)
    z = np.zeros((1, D["ny"], D["nx"]), np.float32)
    for gz in (0.0, -0.02):
        p = PR.params(ground_z=gz)
        a = TR.step_mixed(models, tid, p, D, z, None, None, s, c)
        b = PR.step_mixed(models, tid, p, s, c)
        for k, v in b.items():
            assert np.abs(a[k] - v).max() <= 1e-12, k
        assert np.array_equal(a["terrain_out"][:, 4:].reshape(-1, 4, 3), np.broadcast_to([0.0, 0.0, 1.0], (len(s), 4, 3)))
        assert np.all(a["terrain_out"][:, :4] == p["ground_z"])
    assert (a["fn"] > 0).sum() >= 10


def test_push_enters_the_equations_of_motion(pkg):
    """H nu_dot + C + G = [0; tau] + sum Jc^T f + [R^T moment; R^T force; 0] on the first-principles model, and the push's power is
    force . v_origin(world) + moment . omega(world)."""
    case = TR.step_case(pkg)
    p = PR.params(substeps=1, **TR.STEP_PARAMS)
    for t, robot in enumerate(PR.ROBOTS):
        k = np.nonzero(case["tid"] == t)[0]
        model = pkg.model_desc(robot)
        s = M.normalised(case["state"][k])
        push = case["push"][k].astype(np.float64)
        _, aux = TR.substep(model, p, case["D"], case["height"], case["fid"][k], push, s, case["cmd"][k], p["dt"])
        rb = M.compute(model, s)
        R = M.quat_to_rot(s[:, 0:4])
        rhs = np.einsum("nlak,nla->nk", rb["Jc"], aux["force"])
        rhs[:, 6:] += aux["tau"]
        rhs[:, 0:3] += np.einsum("nji,nj->ni", R, push[:, 3:6]); rhs[:, 3:6] += np.einsum("nji,nj->ni", R, push[:, 0:3])
        lhs = np.einsum("nij,nj->ni", rb["H"], aux["nu_dot"]) + rb["C"] + rb["G"]
        res = np.abs(lhs - rhs) / np.maximum(1.0, np.abs(rhs))
        print("%s: equation residual %.2e" % (robot, res.max()))
        assert res.max() <= 1e-9
        nu = np.concatenate([s[:, 7:13], s[:, 25:37]], 1)
        power = np.einsum("ni,ni->n", TR.push_rhs(s, push), nu)
        direct = np.einsum("ni,ni->n", push[:, 0:3], np.einsum("nij,nj->ni", R, s[:, 10:13])) + np.einsum("ni,ni->n", push[:, 3:6], np.einsum("nij,nj->ni", R, s[:, 7:10]))
        assert np.abs(power - direct).max() <= 1e-12 * np.maximum(1.0, np.abs(direct)).max()
        # and it moves the result: the same sub-step without it
        _, aux0 = TR.substep(model, p, case["D"], case["height"], case["fid"][k], None, s, case["cmd"][k], p["dt"])
        assert np.abs(aux["nu_dot"][:, 0:6] - aux0["nu_dot"][:, 0:6]).max(1).min() > 1e-2


@pytest.mark.parametrize("substeps", PR.STEP_SUBSTEPS)
def test_step_case_meets_what_the_gpu_test_leans_on(pkg, substeps):
    """On the reference alone, at every sub-step count: at most 2 of 192 feet with f_n within 1e-6 of the contact threshold, at least a quarter of
    the feet in contact in the last sub-step and a quarter not, at least 8 feet in contact off the grid, no foot within 1e-6 cell of a border line
    (in the last sub-step or in the state written), both fields and both robot types among the robots flagged OFF_FIELD or not, everything finite.
    Measured at 1 / 2 / 8 sub-steps: in contact 110 / 84 / 101, off the grid and in contact 14 / 9 / 13, near the threshold 0, near a border 0."""
    case = TR.step_case(pkg)
    models = [pkg.model_desc(r) for r in PR.ROBOTS]
    p = PR.params(substeps=substeps, **TR.STEP_PARAMS)
    r = TR.step_mixed(models, case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
    fn = r["fn"]
    print("substeps", substeps, "in contact", (fn > 0).sum(), "off grid and in contact", (r["off"] & (fn > 0)).sum(), "near threshold", PR.near_threshold(p, fn).sum())
    assert fn.size == 192
    assert PR.near_threshold(p, fn).sum() <= 2
    assert (fn > 0).sum() >= 48 and (fn == 0).sum() >= 48
    assert (r["off"] & (fn > 0)).sum() >= 8
    assert not TR.near_border(case["D"], r["plant_out"][:, 12:24].reshape(-1, 4, 3)).any()
    # the feet of the last sub-step: one sub-step less from the same start
    if substeps > 1:
        s = M.normalised(case["state"])
        for t, model in enumerate(models):
            k = np.nonzero(case["tid"] == t)[0]
            sk = s[k]
            for _ in range(substeps - 1):
                sk, _ = TR.substep(model, p, case["D"], case["height"], case["fid"][k], case["push"][k], sk, case["cmd"][k], p["dt"] / substeps)
            assert not TR.near_border(case["D"], M.compute(model, sk)["pGC"]).any()
    else:
        for t, model in enumerate(models):
            k = np.nonzero(case["tid"] == t)[0]
            assert not TR.near_border(case["D"], M.compute(model, M.normalised(case["state"][k]))["pGC"]).any()
    assert np.all(np.isfinite(r["fb_state"])) and np.all(np.isfinite(r["plant_out"]))
    assert set(np.unique(r["status"])) == {0, TR.PL_OFF_FIELD}
    assert not np.array_equal(case["fid"], case["tid"]) and set(zip(case["fid"].tolist(), case["tid"].tolist())) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert np.abs(case["push"][:, 0:3]).max() <= 40 and np.abs(case["push"][:, 3:6]).max() <= 10 and np.abs(case["push"]).min() > 0


def test_slope_chain_gives_the_bands_of_the_gpu_test(pkg):
    """32 identical robots are one robot: the float64 chain of the slope scenario (aligned with plane(tan 0.2, 0), joint PD, 1500 ticks of 1 ms at
    4 sub-steps) ends on four feet with status 0 on every tick, at the end values and with the residual swing over its last 500 ticks that
    terrain_ref.SLOPE_END / SLOPE_SWING record for the GPU test (bands: end +- 3 swing)."""
    r = TR.slope_chain(pkg)
    print("slope chain: end", r["end"], "swing", r["swing"], "sum f_z / m g - 1 = %.4f" % (r["fz"] / (M.total_mass() * 9.81) - 1))
    assert r["status"] == 0 and np.all(r["contact"] == 1)
    assert np.all(np.abs(r["end"] - np.array(TR.SLOPE_END)) <= 1e-5)
    assert np.all(np.abs(r["swing"] - np.array(TR.SLOPE_SWING)) <= 1e-3 * np.array(TR.SLOPE_SWING) + 1e-6)
    assert np.all(np.array(TR.SLOPE_SWING) > 0)
