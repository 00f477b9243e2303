"""CPU checks of the swing-mode restatement (tests/swing_modes_ref.py): the B-spline against scipy, the trajectory's shape, CheckSolution's
one-variable QP against compiled QuadProg++, and the gap-crossing plan against hand-derived offsets.
Reference: qr_foot_trajectory_generator.cpp:30-163, 276-343; qr_foot_stepper.cpp:85-179, 483-525."""
import numpy as np
import pytest

import swing_modes_ref as R

f32 = np.float32


def walk_pairs(n, seed):
    """source / target pairs in the walk envelope (|dxy| <= 0.3 m, |dz| <= 0.15 m) with the edge cases first."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-0.5, 0.5, (n, 3)).astype(f32)
    d = np.zeros((n, 3), f32)
    ang = rng.uniform(-np.pi, np.pi, n); rad = 0.3 * np.sqrt(rng.uniform(0, 1, n))
    d[:, 0] = rad * np.cos(ang); d[:, 1] = rad * np.sin(ang); d[:, 2] = rng.uniform(-0.15, 0.15, n)
    d[0] = 0                                                  # no step
    d[1] = (0, 0, 0.12)                                       # purely vertical, up
    d[2] = (0, 0, -0.12)                                      # purely vertical, down
    d[3] = (-0.25, 0, 0)                                      # backwards
    d[4] = (0.2, 0.05, -0.15)                                 # walk-down
    d[5] = (0.1, 0, 0.15)                                     # walk-up at the height cap
    return src, (src + d).astype(f32)


def scipy_curve(ctrl):
    from scipy.interpolate import BSpline
    c, s, cx, cz = ctrl
    P = np.stack([cx.astype(np.float64), np.zeros(9), cz.astype(np.float64)], 1)
    return BSpline(R.KNOTS.astype(np.float64), P, 3, extrapolate=True)


def test_bspline_matches_scipy():
    src, tgt = walk_pairs(2000, 11)
    us = np.linspace(0, 1, 101).astype(f32)
    worst_p = worst_v = 0.0
    for k in range(len(src)):
        h = R.bspline_height(src[k], tgt[k])
        ctrl = R.bspline_control_points(src[k], tgt[k], h)
        c, s = ctrl[0], ctrl[1]
        crv = scipy_curve(ctrl)
        Rt = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)
        pe = (Rt @ (crv(us.astype(np.float64)).T / 100.0)).T + src[k].astype(np.float64)       # every pair at all 101 phases
        ve = (Rt @ (crv.derivative()(us.astype(np.float64)).T / 100.0)).T
        for j, u in enumerate(us):
            p, v = R.bspline_eval(ctrl, src[k], u)
            worst_p = max(worst_p, float(np.abs(np.array(p, np.float64) - pe[j]).max()))
            worst_v = max(worst_v, float(np.abs(np.array(v, np.float64) - ve[j]).max()))
    assert worst_p <= 1e-6, worst_p
    assert worst_v <= 1e-5, worst_v


def test_bspline_trajectory_properties():
    src, tgt = walk_pairs(300, 12)
    for k in range(len(src)):
        h = R.bspline_height(src[k], tgt[k])
        dz = abs(float(tgt[k, 2]) - float(src[k, 2]))
        assert h == f32(min(0.2, max(0.1, 0.15 + dz))) or abs(h - min(0.2, max(0.1, 0.15 + dz))) < 1e-7
        p0, _ = R.bspline_point(src[k], tgt[k], h, 0.0)
        p1, _ = R.bspline_point(src[k], tgt[k], h, 1.0)
        assert np.abs(np.array(p0) - src[k]).max() <= 1e-6, k
        assert np.abs(np.array(p1) - tgt[k]).max() <= 2e-6, k
        d = (tgt[k] - src[k]).astype(np.float64)
        nrm = np.array([-d[1], d[0], 0.0]); ln = np.linalg.norm(nrm)
        top = max(src[k, 2], tgt[k, 2])
        zmax = -1e9
        for u in np.linspace(0, 1, 41):
            p, _ = R.bspline_point(src[k], tgt[k], h, u)
            p = np.array(p, np.float64)
            if ln > 1e-3:                                     # the vertical plane through source and target
                assert abs(np.dot(p - src[k], nrm / ln)) <= 2e-6, (k, u)
            zmax = max(zmax, p[2])
        if float(tgt[k, 2]) >= float(src[k, 2]):              # walk-up: the apex clears the source by the height
            assert zmax >= float(src[k, 2]) + 0.95 * h - 1e-6, (k, zmax)
        assert zmax <= top + h + 0.02, (k, zmax)


def test_step_qp_matches_quadprog(ref):
    rng = np.random.default_rng(3)
    n = 0
    decided = {True: 0, False: 0}
    G = np.eye(1); g0 = np.zeros(1); CE = np.zeros((1, 0)); ce0 = np.zeros(0)
    for _ in range(2600):
        delta = f32(rng.choice([0.1, 0.05, 0.2, rng.uniform(0.01, 0.3)]))
        cx = rng.uniform(-0.4, 2.2, 4).astype(f32)
        fg, bg = f32(rng.uniform(0.3, 2.0)), f32(rng.uniform(0.3, 2.0))
        gw = f32(rng.choice([0.14, rng.uniform(0.02, 0.4)]))
        for i in (-1, 1):
            for j in (-1, 1):
                ci, b = R.check_solution_layout(delta, cx, i, j, fg, bg, gw)
                x, _ = R.quadprog_1d(ci, [-v for v in b])
                xr, fr = ref.ref_quadprog(G, g0, CE, ce0, np.array(ci).reshape(1, 6), -np.array(b))
                assert x == xr[0] or (x == 0 and xr[0] == 0), (ci, b, x, xr)
                acc = all(int(x * ci[k] * 10000) >= int(b[k] * 10000) for k in range(6))
                acc_r = all(int(xr[0] * ci[k] * 10000) >= int(b[k] * 10000) for k in range(6))
                assert acc == acc_r
                decided[acc] += 1
                n += 1
    assert n >= 10000
    assert decided[True] > 100 and decided[False] > 100, decided


def plan(d, fh_x):
    st = np.zeros(R.STATE_FLOATS, f32)
    for k in range(4):
        st[R.SS_FH + 3 * k] = fh_x[k]
    offs, flags = [], 0
    for _ in range(40):
        o, flags = R.optimal_offsets(d, st, flags)
        offs.append(o)
    return offs, flags, st


def test_gap_plan_cases():
    d = R.Desc(1)                                             # a1_sim: gaps 0.51, 1.31, 1.91, width 0.14, delta 0.10
    # no gaps: the default delta every time
    offs, flags, _ = plan(R.Desc(1, gaps=()), [0.2, 0.2, -0.2, -0.2])
    assert all(o == [f32(0.1)] * 4 for o in offs) and flags == 0
    # a start beyond the last gap: the plan is empty, the default delta is returned
    offs, flags, st = plan(d, [3.0, 3.0, 2.6, 2.6])
    assert all(o == [f32(0.1)] * 4 for o in offs) and flags == 0 and st[R.SS_TAIL] == 0 and st[R.SS_PFLAGS] == 1
    # a -1 cross-gait shift that recovers (gap 0.51 +- 0.07): from x = (0.335, 0, -0.3, -0.3) step 1 is free (leg 0 to 0.435); leg 0's next
    # default, 0.535, meets the gap -> -1: the planned step 1 takes +0.05 on legs 0 and 3 and leg 0 stands at 0.485; its next, 0.585, is
    # clear, but 0.485 + 0.05 still lies in the gap, so step 2 is the default; step 3 is the recovery {0.05, 0.1, 0.1, 0.05}.  Leg 1 then
    # meets the gap (-1 on step 4), and with it the plan ends in a -2, as the reference's exit(-1) does: a 0.14 m gap cannot be stepped over
    # with 0.1 m by a leg that the shift does not move.
    offs, flags, st = plan(R.Desc(1, gaps=(0.51,)), [0.335, 0.0, -0.3, -0.3])
    o = [list(map(float, v)) for v in offs]
    assert np.allclose(o[0], [0.15, 0.1, 0.1, 0.15]), o[0]
    assert np.allclose(o[1], [0.1] * 4), o[1]
    assert np.allclose(o[2], [0.05, 0.1, 0.1, 0.05]), o[2]
    assert np.allclose(o[3], [0.15, 0.1, 0.1, 0.15]), o[3]
    assert flags == R.SW_PLAN_EXIT and int(st[R.SS_TAIL]) == 4, (flags, st[R.SS_TAIL])
    assert all(np.allclose(v, [0.1] * 4) for v in o[4:])
    # a narrow gap that every leg steps over: no flag, the whole plan is the default step
    offs, flags, st = plan(R.Desc(1, gaps=(0.51,), gap_width=0.04), [0.25, 0.25, -0.15, -0.15])
    assert flags == 0 and int(st[R.SS_TAIL]) > 0 and all(np.allclose(list(map(float, v)), [0.1] * 4) for v in offs)
    # the first step meets a gap: the -1 shift finds no planned step (steps.back() on an empty queue) and is flagged
    _, flags, _ = plan(d, [0.44, 0.44, 0.04, 0.04])
    assert flags & R.SW_PLAN_EMPTY
    # a -2 (exit(-1) in the reference): both pairs meet a gap after the shift
    d2 = R.Desc(1, gaps=(0.55, 0.75), gap_width=0.3)
    _, flags, _ = plan(d2, [0.3, 0.3, 0.3, 0.3])
    assert flags & R.SW_PLAN_EXIT, flags
