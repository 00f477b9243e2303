"""The force-balance (VMC) kernel away from the A1 defaults: the parameter grid of tests/golden/vmc_grid_golden.npz (friction 0.2 .. 0.9,
fMaxRatio 1, other weights, Lite3, both overloads -- QuadProg++'s recorded answers, no oracle in the loop), Lite3 and the world-frame
friction 0.6 live against the oracle, four types mixed in one call, the type contract, the batch sizes around the 8-block XCD mapping and
the single-robot entry points.

Bars (those of test_gpu_vmc.py): forces within 1e-5 * max(1, |f|max), torques within 1e-4 * max(1, |tau|), the +inf flag case by case.
They are asked where the reference's answer is well defined (`well_posed` of the golden file: QuadProg++'s own iterate does not move under
perturbations far below its input's rounding, make_golden.vmc_grid_scan).  On the other cases -- all of them +inf ticks, at most 0.7 % of a
cell -- only the flag, finiteness and "no other flag" are asked: this is also what guards the kernel's dependent-row question
(z.n > 1e-8 n'Mn, qr_vmc_kernel.hip): at 1e-12 the flag of some well-posed case flips, at 1e-4 forces leave the bar (LAB_NOTES "VMC grid")."""
import numpy as np
import pytest

import golden_io
import gpu_helpers as G
from gpu_helpers import tau_tol

pytestmark = pytest.mark.gpu
GRID = golden_io.make_golden().VMC_GRID
BAD_TYPE = 0x01000000


def _run(ctx, pkg, vin, q, ratio=None, type_id=None, pad=0, sentinel=None):
    """One call of qrgpu_vmc_force_batch (ratio None) or qrgpu_vmc_force_world_batch.  pad > 0: the output buffers are `pad` elements
    longer than [12][n] / [n] and pre-filled with `sentinel`; the tails come back as out['tail']."""
    n = vin.shape[0]
    S = pkg.to_soa
    bufs = [ctx.alloc((37, n)).upload(S(vin)), ctx.alloc((12, n)).upload(S(q))]
    d_in, d_q = bufs
    d_r = None
    if ratio is not None:
        d_r = ctx.alloc((8, n)).upload(S(ratio)); bufs.append(d_r)
    d_f = ctx.alloc((12 * n + pad,)); d_t = ctx.alloc((12 * n + pad,)); d_s = ctx.alloc((n + pad,), np.int32)
    bufs += [d_f, d_t, d_s]
    if pad:
        d_f.upload(np.full(12 * n + pad, sentinel, np.float32)); d_t.upload(np.full(12 * n + pad, sentinel, np.float32))
        d_s.upload(np.full(n + pad, -7, np.int32))
    tid = None
    if type_id is not None:
        tid = ctx.alloc((n,), np.int32).upload(np.asarray(type_id, np.int32)); bufs.append(tid)
    try:
        if ratio is None:
            ctx.vmc_force_batch(n, d_in, d_q, d_f, d_t, d_s, tid)
        else:
            ctx.vmc_force_world_batch(n, d_in, d_r, d_q, d_f, d_t, d_s, tid)
        ctx.sync()
        f, t, s = d_f.download(), d_t.download(), d_s.download()
    finally:
        for v in bufs:
            v.free()
    out = dict(force=f[:12 * n].reshape(12, n).T.copy(), tau=t[:12 * n].reshape(12, n).T.copy(), status=s[:n].copy())
    if pad:
        out["tail"] = (f[12 * n:], t[12 * n:], s[n:])
    return out


def _same(a, b, rows=None):
    """force, tau and status of two results bit for bit (on `rows`)."""
    rows = slice(None) if rows is None else rows
    return all(np.array_equal(a[k][rows].view(np.int32), b[k][rows].view(np.int32)) for k in ("force", "tau")) and \
        np.array_equal(a["status"][rows], b["status"][rows])


def _oracle_bars(oracle, g, i, cfg, geom, vin, q, ratio=None):
    force, tau, x, st, rc = oracle.vmc_solve(cfg, geom, vin, q, ratio)
    assert bool(G.flags(g["status"][i]) & 0x80) == (rc == 1), (i, g["status"][i], rc)
    assert np.abs(g["force"][i] - force).max() <= 1e-5 * max(1.0, np.abs(force).max()), (i, np.abs(g["force"][i] - force).max())
    assert np.all(np.abs(g["tau"][i] - tau) <= tau_tol(tau, 1e-4)), i
    return rc


@pytest.fixture(scope="module")
def grid_cells():
    return golden_io.load_vmc_grid()


@pytest.fixture(scope="module")
def ctx4(pkg):
    """A context of its own with four force-balance types: 0 A1 defaults, 1 Lite3 defaults, 2 A1 at friction 0.6, 3 A1 with
    fMaxRatio 1 and other weights."""
    W = pkg.workload
    cfgs = [W.vmc_cfg("a1"), W.vmc_cfg("lite3"), W.vmc_cfg("a1", friction=0.6),
            W.vmc_cfg("a1", fmax_ratio=1.0, acc_weight=(5, 5, 1, 1, 1, 20), reg_weight=1e-3)]
    geoms = [pkg.model_desc(r)[:3] for r in ("a1", "lite3", "a1", "a1")]
    ctx = pkg.Context(device_id=0, max_batch=512, horizon_max=16)
    for t in range(4):
        ctx.vmc_setup_packed(t, cfgs[t], geoms[t])
    yield ctx, cfgs, geoms
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_vmc_unknown_type_is_flagged(pkg):
    """qrgpu.h: a d_type_id outside the table or naming a type that was never set up -> QRGPU_ST_BAD_TYPE, computed with the first type
    that was set up (as the MPC and WBC kernels do, test_unknown_type_is_flagged); NULL d_type_id means type 0."""
    W = pkg.workload
    cfg = W.vmc_cfg("a1"); geom = pkg.model_desc("a1")[:3]
    vin, q = W.make_vmc_batch(8, sloped=0.5, seed=81)
    tid = np.array([0, 3, 0, 7, -1, 0, 2, 0], np.int32)            # 2, 3 were never set up on this context; 7, -1 do not exist
    ctx = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
    try:
        with pytest.raises(pkg.QrgpuError):                        # nothing set up yet: NOT_SETUP with or without ids
            _run(ctx, pkg, vin, q, type_id=np.zeros(8, np.int32))
        with pytest.raises(pkg.QrgpuError):
            _run(ctx, pkg, vin, q)
        ctx.vmc_setup_packed(0, cfg, geom)
        out = _run(ctx, pkg, vin, q, type_id=tid)
        ref = _run(ctx, pkg, vin, q)                               # NULL ids: all type 0
        ref0 = _run(ctx, pkg, vin, q, type_id=np.zeros(8, np.int32))
    finally:
        ctx.close()
    bad = (out["status"] & BAD_TYPE) != 0
    assert np.array_equal(bad, tid != 0), out["status"]
    assert np.all(np.isfinite(out["force"])) and np.all(np.isfinite(out["tau"]))
    assert _same(out, ref, ~bad) and _same(ref, ref0)
    assert np.all((G.flags(ref["status"]) & ~0x80) == 0)
    # flagged robots were computed with the first valid type: everything but the flag is the type-0 result
    assert np.array_equal(out["force"][bad], ref["force"][bad]) and np.array_equal(out["status"][bad] & ~BAD_TYPE, ref["status"][bad])
    # a context that set up type 1 alone: usable through d_type_id, NOT_SETUP without it; a robot naming type 0 there is flagged
    ctx = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
    try:
        ctx.vmc_setup_packed(1, cfg, geom)
        with pytest.raises(pkg.QrgpuError):
            _run(ctx, pkg, vin, q)
        one = _run(ctx, pkg, vin, q, type_id=np.array([1, 1, 1, 1, 0, 1, 1, 1], np.int32))
    finally:
        ctx.close()
    assert np.array_equal((one["status"] & BAD_TYPE) != 0, np.arange(8) == 4)
    assert np.array_equal(one["force"], ref["force"]) and np.array_equal(one["tau"], ref["tau"])     # the same constants in slot 1


@pytest.mark.parametrize("cell", GRID, ids=[c["name"] for c in GRID])
def test_vmc_grid_golden_quadprog(gpu_ctx, pkg, grid_cells, cell):
    """Every kept case of the cell through its entry point against QuadProg++'s recorded x (no oracle in the loop)."""
    g = grid_cells[cell["name"]]
    gpu_ctx.vmc_setup_packed(0, g["cfg"], g["geom"])
    out = _run(gpu_ctx, pkg, g["vin"], g["q"], g["ratio"])
    flags = G.flags(out["status"])
    assert np.all((flags & ~0x80) == 0), np.unique(flags)
    assert np.all(np.isfinite(out["force"])) and np.all(np.isfinite(out["tau"]))
    assert np.array_equal((flags & 0x80) != 0, g["quadprog_inf"]), np.flatnonzero(((flags & 0x80) != 0) != g["quadprog_inf"])
    worst = 0.0
    for k in range(g["vin"].shape[0]):
        if not g["well_posed"][k]:
            continue                                                 # a +inf tick whose iterate the reference's own rounding decides
        R = g["vin"][k, 22:31].reshape(3, 3).astype(np.float64)
        f_ref = ((-g["x_quadprog"][k].reshape(4, 3)) @ R).reshape(-1)                 # (X * Rcb)^T, force[3*leg+axis]
        err = np.abs(out["force"][k] - f_ref).max() / max(1.0, np.abs(f_ref).max())
        worst = max(worst, err)
        assert err <= 1e-5, (cell["name"], int(g["idx"][k]), err)
    print("%s: %d cases (%d not well-posed), worst force error %.2e of the bar's scale" % (cell["name"], len(g["idx"]), (~g["well_posed"]).sum(), worst))
    assert 0 < g["quadprog_inf"].sum() < len(g["idx"])


@pytest.mark.parametrize("name", ["lite3", "lite3_world_mu060", "a1_world_mu060"])
def test_vmc_grid_live_against_oracle(gpu_ctx, pkg, oracle, grid_cells, name):
    """Robots 0..255 of the cell's batch in one call, with the bars of test_vmc_parity, wherever the cell's scan found the reference well
    posed (the golden file keeps every case that is not; these three cells have none)."""
    cell = [c for c in GRID if c["name"] == name][0]
    cfg, geom, vin, q, ratio = golden_io.make_golden().vmc_grid_inputs(cell)
    g = grid_cells[name]
    assert np.array_equal(cfg, g["cfg"]) and np.array_equal(vin[g["idx"]], g["vin"])
    ill = set(g["idx"][~g["well_posed"]].tolist())
    n = 256
    gpu_ctx.vmc_setup_packed(0, cfg, geom)
    out = _run(gpu_ctx, pkg, vin[:n], q[:n], None if ratio is None else ratio[:n])
    flags = G.flags(out["status"])
    assert np.all((flags & ~0x80) == 0), np.unique(flags)
    assert np.all(np.isfinite(out["force"])) and np.all(np.isfinite(out["tau"]))
    n_inf = 0
    for i in range(n):
        if i not in ill:
            n_inf += _oracle_bars(oracle, out, i, cfg, geom, vin[i], q[i], None if ratio is None else ratio[i]) == 1
    assert 0 < n_inf < n


def _mixed_inputs(pkg, n, world):
    """Rows of an A1 batch, with Lite3's rows (id 1) from a Lite3 batch: each robot's feet fit its own type."""
    W = pkg.workload
    tid = (np.arange(n) % 4).astype(np.int32)
    if world:
        va, qa, ratio = W.make_vmc_world_batch(n, "a1", seed=62, excite=2.0)
        vl, ql, _ = W.make_vmc_world_batch(n, "lite3", seed=62, excite=2.0)
    else:
        va, qa = W.make_vmc_batch(n, "a1", seed=61, sloped=0.5, excite=2.0)
        vl, ql = W.make_vmc_batch(n, "lite3", seed=61, sloped=0.5, excite=2.0)
        ratio = None
    vin = np.where((tid == 1)[:, None], vl, va); q = np.where((tid == 1)[:, None], ql, qa)
    return tid, vin, q, ratio


@pytest.mark.parametrize("world", [False, True], ids=["control_frame", "world_frame"])
def test_vmc_mixed_types_in_one_call(ctx4, gpu_ctx, pkg, oracle, world):
    """260 robots (no multiple of 8 or 64), ids cycling 0..3: each robot's force, torque and status equal, bit for bit, the same robot in a
    call where every robot has its type -- a mixed-up type constant shows without any oracle.  Then the oracle bars on sampled robots:
    those on level ground or with four feet down (an ill-posed +inf tick needs a swing foot on a pitched normal; such ticks are the grid
    tests' business, with the reference's own mask)."""
    ctx, cfgs, geoms = ctx4
    n = 260
    tid, vin, q, ratio = _mixed_inputs(pkg, n, world)
    mixed = _run(ctx, pkg, vin, q, ratio, type_id=tid)
    assert np.all((G.flags(mixed["status"]) & ~0x80) == 0)
    differs = 0
    for t in range(4):
        single = _run(ctx, pkg, vin, q, ratio, type_id=None if t == 0 else np.full(n, t, np.int32))
        assert _same(mixed, single, tid == t), t
        gpu_ctx.vmc_setup_packed(0, cfgs[t], geoms[t])             # ... and slot t holds what slot 0 of another context holds for the same constants
        assert _same(single, _run(gpu_ctx, pkg, vin, q, ratio)), t
        differs += not np.array_equal(mixed["force"][tid != t], single["force"][tid != t])
    assert differs == 4                                   # every type's constants matter on this batch
    level = vin[:, 36] == 1.0
    sampled = [i for i in range(0, n, 3) if level[i] or np.all(vin[i, 18:22] > 0)]
    assert len(sampled) >= 40 and len({int(tid[i]) for i in sampled}) == 4
    n_inf = sum(_oracle_bars(oracle, mixed, i, cfgs[tid[i]], geoms[tid[i]], vin[i], q[i], None if ratio is None else ratio[i]) == 1 for i in sampled)
    assert 0 < n_inf < len(sampled)


def test_vmc_batch_size_edges(ctx4, pkg):
    """The grid is 8 * ceil(n / 8) blocks and a block without a robot returns: n = 1, 7, 8, 9, 63, 65 give each robot the result it has
    inside a 256-robot call, bit for bit, and nothing is written behind [12][n] / [n]."""
    ctx, cfgs, geoms = ctx4
    tid, vin, q, _ = _mixed_inputs(pkg, 256, False)
    full = _run(ctx, pkg, vin, q, type_id=tid)
    sent = np.float32(-1234.5)
    for n in (1, 7, 8, 9, 63, 65):
        part = _run(ctx, pkg, vin[:n], q[:n], type_id=tid[:n], pad=96, sentinel=sent)
        assert _same(part, dict(force=full["force"][:n], tau=full["tau"][:n], status=full["status"][:n])), n
        ft, tt, st = part["tail"]
        assert np.all(ft == sent) and np.all(tt == sent) and np.all(st == -7), n


def test_vmc_single_robot_entry_points(ctx4, pkg):
    """qrgpu_vmc_force1 / qrgpu_vmc_force_world1 with type_id = 1 (Lite3): the batch result of the same robot, bit for bit."""
    ctx, cfgs, geoms = ctx4
    W = pkg.workload
    n = 6
    vin, q = W.make_vmc_batch(n, "lite3", seed=71, sloped=0.5, excite=2.0)
    batch = _run(ctx, pkg, vin, q, type_id=np.full(n, 1, np.int32))
    vw, qw, ratio = W.make_vmc_world_batch(n, "lite3", seed=72, excite=2.0)
    wbatch = _run(ctx, pkg, vw, qw, ratio, type_id=np.full(n, 1, np.int32))
    other = _run(ctx, pkg, vin, q)                                  # as type 0 (A1): must differ, or type_id would not matter here
    assert not np.array_equal(other["force"], batch["force"])
    for i in range(n):
        f, tau, st = ctx.vmc_force1(vin[i], q[i], type_id=1)
        assert np.array_equal(f, batch["force"][i]) and np.array_equal(tau, batch["tau"][i]) and st == batch["status"][i], i
        f, tau, st = ctx.vmc_force_world1(vw[i], ratio[i], qw[i], type_id=1)
        assert np.array_equal(f, wbatch["force"][i]) and np.array_equal(tau, wbatch["tau"][i]) and st == wbatch["status"][i], i
    with pytest.raises(pkg.QrgpuError):
        ctx.vmc_force1(vin[0], q[0], type_id=7)                     # the single-robot calls return NOT_SETUP for an unknown type
