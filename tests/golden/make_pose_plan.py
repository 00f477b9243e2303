"""Writes tests/golden/pose_plan_golden.npz: inputs of the walk pose planner by cell, the float32 and float64 restatements' results
(tests/pose_plan_ref.py) and, for every QP of the float32 run, the x the compiled QuadProg++ of oracle/_ref returns (recorded reference-solver
output).  Run from the repository root:  python tests/golden/make_pose_plan.py
Cells: A1 nominal stance, 3 cm foot scatter, 0.05 rad tilt; one swing leg (N = 3) x {nominal, base offset 0.10-0.15 m in x, in y, in both,
0.07 m low, 0.09 m high}; four stance feet (N = 4) nominal, offset and non-convex (one case pair per invalidId path); chains of 8 consecutive
plans that carry Lambda while the feet move (one alternates N = 3 and N = 4, so Lambda grows); the flag cases."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import pose_plan_ref as P  # noqa: E402

f32, f64 = np.float32, np.float64
OFFSETS = dict(nominal=lambda r: (0, 0, 0), x=lambda r: (r.choice([-1, 1]) * r.uniform(0.10, 0.15), 0, 0),
               y=lambda r: (0, r.choice([-1, 1]) * r.uniform(0.10, 0.15), 0),
               xy=lambda r: (r.choice([-1, 1]) * r.uniform(0.10, 0.15), r.choice([-1, 1]) * r.uniform(0.10, 0.15), 0),
               low=lambda r: (0, 0, -0.07), high=lambda r: (0, 0, 0.09))


def nonconvex_case(rng, leg):
    """Four stance feet with foot `leg` pulled inside the triangle of the other three."""
    feet = P.NOMINAL_FEET.reshape(4, 3) + [0, 0, 0.27] + rng.uniform(-0.01, 0.01, (4, 3)) * [1, 1, 0.3]
    cen = feet[[l for l in range(4) if l != leg]].mean(axis=0)
    feet[leg, :2] = cen[:2] + 0.1 * (feet[leg, :2] - cen[:2])
    return P.make_case(rng, swing_leg=None, feet_world=feet)


def chain(rng, alternate):
    """8 consecutive plans: each swing foot lands 5-10 cm ahead, the base follows the last plan's destination."""
    feet = P.NOMINAL_FEET.reshape(4, 3) + [0, 0, 0.27] + rng.uniform(-0.03, 0.03, (4, 3)) * [1, 1, 0.3]
    base_xy = np.zeros(2)
    order = [0, 3, 1, 2, 0, 3, 1, 2]
    st64 = None
    for k, leg in enumerate(order):
        four = alternate and (k % 2 == 1)
        c = P.make_case(rng, swing_leg=None if four else leg, feet_world=feet.copy(), base_xy=tuple(base_xy), offset=tuple(rng.uniform(-0.01, 0.01, 3)))
        if st64 is None:
            st64 = P.new_state(f64, c["base_pos"])
        r = P.update(f64, P.Desc(), c, st64)
        yield c
        if r["cmd"] is not None:
            base_xy = np.array([float(r["cmd"][6]), float(r["cmd"][7])])
        feet[leg, 0] += rng.uniform(0.05, 0.10)


def build_cells():
    rng = np.random.default_rng(20260)
    cells = []                                                       # (name, chained, [cases])
    for leg in range(4):
        for name, off in OFFSETS.items():
            cells.append(("swing%d_%s" % (leg, name), False, [P.make_case(rng, swing_leg=leg, offset=off(rng)) for _ in range(2)]))
    cells.append(("four_nominal", False, [P.make_case(rng, swing_leg=None) for _ in range(3)]))
    cells.append(("four_offset", False, [P.make_case(rng, swing_leg=None, offset=OFFSETS[k](rng)) for k in ("x", "y", "xy", "x", "y", "xy")]))
    cells.append(("four_nonconvex", False, [nonconvex_case(rng, leg) for leg in (0, 1, 2, 3) for _ in range(2)]))
    for k, alt in enumerate((False, False, True)):
        cells.append(("chain%d" % k, True, list(chain(rng, alt))))
    # flag cases that need nothing but inputs: two stance feet, none, a non-finite foot position (NOT_PD and INFEASIBLE need a carried Lambda /
    # another descriptor: tests/test_pose_plan_ref.py builds them)
    two = P.make_case(rng, swing_leg=0); two["desired_leg_state"] = [P.SWING, P.SWING, P.STANCE, P.STANCE]
    none = P.make_case(rng, swing_leg=0); none["desired_leg_state"] = [P.SWING] * 4
    nan = P.make_case(rng, swing_leg=1); nan["foot_base"] = nan["foot_base"].copy(); nan["foot_base"][4] = np.nan
    cells.append(("flag_few", False, [two, none]))
    cells.append(("flag_nan", False, [nan]))
    return cells


def run(T, cells, compiled=None):
    """-> per-case results in cell order; chained cells carry one planner state through their cases."""
    d = P.Desc()
    res = []
    for name, chained, cases in cells:
        st = None
        for c in cases:
            if st is None or not chained:
                st = P.new_state(T, c["base_pos"])
            before = P.state_rows(T, st)
            r = P.update(T, d, c, st, record_qp=compiled is not None)
            r["before"], r["after"] = before, P.state_rows(T, st)
            if compiled is not None:
                xq = np.full((P.MAX_LOOPS, 6), np.nan)
                fq = np.full(P.MAX_LOOPS, np.nan)
                for k, qp in enumerate(r["qps"]):
                    xq[k], fq[k] = compiled.ref_quadprog(qp["G"], qp["g0"], np.zeros((6, 0)), np.zeros(0), qp["CI"], qp["ci0"])
                r["xq"], r["fq"] = xq, fq
            res.append(r)
    return res


def pad(rows, width, fill=np.nan, dtype=f64):
    out = np.full((len(rows), width), fill, dtype)
    for i, r in enumerate(rows):
        if r is not None:
            out[i, :len(r)] = np.asarray(r, f64)
    return out


def main():
    import oracle_py
    assert oracle_py.ref() is not None, "oracle/_ref (the compiled QuadProg++) is needed"
    cells = build_cells()
    r32, r64 = run(f32, cells, compiled=oracle_py), run(f64, cells)
    names, starts, chained = [], [], []
    k = 0
    for name, ch, cases in cells:
        names.append(name); starts.append(k); chained.append(ch); k += len(cases)
    n = k
    L = P.MAX_LOOPS

    def P3(rs, dt):
        a = np.full((n, L, 6), np.nan, dt)
        for i, r in enumerate(rs):
            for k_, p in enumerate(r["p"]):
                a[i, k_] = np.asarray(p, f64)
        return a

    out = dict(cells=np.array(names), cell_start=np.array(starts + [n]), cell_chained=np.array(chained),
               inputs=np.stack([P.flat_input(c) for _, _, cases in cells for c in cases]),
               before32=np.stack([r["before"] for r in r32]).astype(f32), after32=np.stack([r["after"] for r in r32]).astype(f32),
               after64=np.stack([r["after"] for r in r64]),
               flags32=np.array([r["flags"] for r in r32]), flags64=np.array([r["flags"] for r in r64]),
               cmd32=pad([r["cmd"] for r in r32], 12, dtype=f32), cmd64=pad([r["cmd"] for r in r64], 12),
               p32=P3(r32, f32), p64=P3(r64, f64),
               iq32=pad([r["iq"] for r in r32], L, -1, np.int8), iq64=pad([r["iq"] for r in r64], L, -1, np.int8),
               u0_32=pad([r["u0"] for r in r32], 12, 0, f32), A0_32=pad([r["A"][0] if r["A"] else None for r in r32], 12, -1, np.int8),
               lam32=pad([r["lam"] for r in r32], 12, 0, f32), N=np.array([r["N"] for r in r32]), mask=np.array([r["mask"] for r in r32]),
               x_quadprog=np.stack([r["xq"] for r in r32]), f_quadprog=np.stack([r["fq"] for r in r32]))
    np.savez_compressed(os.path.join(HERE, "pose_plan_golden.npz"), **out)
    diff = [(r32[i]["iq"] != r64[i]["iq"]) or (r32[i]["flags"] != r64[i]["flags"]) for i in range(n)]
    print("cases", n, "cells", len(cells), "decided by rounding", int(np.sum(diff)), "flags", sorted(set(out["flags32"].tolist())))


if __name__ == "__main__":
    main()
