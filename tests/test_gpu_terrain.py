"""-m gpu: the plant on height fields -- qrgpu_plant_step_terrain_batch -- against the float64 restatement of tests/terrain_ref.py, at the batch
edges, across field ids, in the flat limit against qrgpu_plant_step_batch, standing on a slope, and its error returns.

Bars: the plant's 1e-6 * max(1, |ref|) per component (tests/test_gpu_plant.py)."""
import ctypes as C

import numpy as np
import pytest

import gpu_helpers as G
import plant_ref as PR
import rigid_body_ref as M
import terrain_ref as TR

pytestmark = pytest.mark.gpu

BAR = 1e-6
KEYS = (("fb_state", 37), ("plant_out", PR.PLANT_OUT_ROWS), ("terrain_out", TR.TERRAIN_OUT_ROWS), ("mpc_state", 28), ("est_in", 41))


def _setup_both(ctx, pkg):
    for t, robot in enumerate(PR.ROBOTS):
        ctx.mpc_setup_packed(t, pkg.mpc_cfg(robot), PR.HORIZON); ctx.wbc_setup_packed(t, pkg.model_desc(robot))


def _tdesc(pkg, D):
    return pkg.terrain_desc(D["nx"], D["ny"], D["n_fields"], D["x0"], D["y0"], D["cell"])


class TerrainPlant:
    """Device arrays of one batch of simulated robots on a stack of fields."""

    def __init__(self, ctx, pkg, D, height, state, cmd, tid=None, fid=None, push=None):
        self.ctx, self.pkg, self.n = ctx, pkg, len(state)
        n = self.n
        self.desc = _tdesc(pkg, D)
        self.height = ctx.alloc(height.shape).upload(height)
        self.fb = ctx.alloc((37, n)).upload(pkg.to_soa(state)); self.cmd = ctx.alloc((60, n)).upload(pkg.to_soa(cmd))
        self.out = ctx.alloc((PR.PLANT_OUT_ROWS, n)); self.tout = ctx.alloc((TR.TERRAIN_OUT_ROWS, n)); self.mpc = ctx.alloc((28, n)); self.est = ctx.alloc((54, n))
        self.status = ctx.alloc((n,), np.int32).upload(np.full(n, -1, np.int32))
        self.tid = None if tid is None else ctx.alloc((n,), np.int32).upload(tid)
        self.fid = None if fid is None else ctx.alloc((n,), np.int32).upload(fid)
        self.push = None if push is None else ctx.alloc((6, n)).upload(pkg.to_soa(push))

    def step(self, params, status=None):
        self.ctx.plant_step_terrain_batch(self.n, params, self.desc, self.height, self.fb, self.cmd, field_id=self.fid, base_push=self.push, plant_out=self.out,
                                          terrain_out=self.tout, mpc_state=self.mpc, est_in=self.est, status=self.status if status is None else status,
                                          type_id=self.tid)

    def get(self):
        self.ctx.sync()
        return dict(fb_state=self.fb.download().T.copy(), plant_out=self.out.download().T.copy(), terrain_out=self.tout.download().T.copy(),
                    mpc_state=self.mpc.download().T.copy(), est_in=self.est.download().T.copy(), status=self.status.download())

    def free(self):
        for v in (self.height, self.fb, self.cmd, self.out, self.tout, self.mpc, self.est, self.status, self.tid, self.fid, self.push):
            if v is not None:
                v.free()


def _run(ctx, pkg, case, params, sel=slice(None), fid=None, height=None, D=None):
    """One tick of the robots `sel` of the step case.  -> outputs"""
    fid = case["fid"] if fid is None else fid
    pl = TerrainPlant(ctx, pkg, case["D"] if D is None else D, case["height"] if height is None else height, case["state"][sel], case["cmd"][sel],
                      case["tid"][sel], fid[sel], case["push"][sel])
    pl.step(params)
    got = pl.get()
    pl.free()
    return got


def _bits_equal(a, b, sel_a=slice(None), sel_b=slice(None)):
    for k, rows in KEYS:                     # (rows 41-53 of est_in are not the plant's)
        if not np.array_equal(a[k][sel_a][:, :rows].view(np.uint32), b[k][sel_b][:, :rows].view(np.uint32)):
            return False
    return np.array_equal(a["status"][sel_a], b["status"][sel_b])


def _worst(got, ref):
    e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    return float(e.max()), np.unravel_index(int(e.argmax()), e.shape)


@pytest.fixture(scope="module")
def case(pkg):
    return TR.step_case(pkg)


@pytest.fixture(scope="module")
def batch48(gpu_ctx, pkg, case):
    """The step case at 2 sub-steps on the device: shared, read-only."""
    _setup_both(gpu_ctx, pkg)
    got = _run(gpu_ctx, pkg, case, pkg.plant_params(substeps=2, **TR.STEP_PARAMS))
    G.setup_a1(gpu_ctx, pkg, 10)
    return got


@pytest.mark.parametrize("substeps", PR.STEP_SUBSTEPS)
def test_step_against_terrain_ref(gpu_ctx, pkg, case, substeps):
    """One control tick of the 48 mixed robots on two stacked 20 x 24 fields (a rough plane, stairs; ids in pairs; some feet beyond the y border) with
    a push of +-40 N, +-10 N m, against the float64 restatement: fb_state, plant_out, terrain_out, mpc_state and rows 0-40 of est_in within
    1e-6 * max(1, |ref|); status equal bit for bit, OFF_FIELD included; contact flags equal except where the reference's f_n is within 1e-6 of the
    threshold (at most 2 of 192 feet: none, test_terrain_ref.py); rows 41-53 of est_in as uploaded.  Measured worst, in units of the bar, at 1 / 2 / 8
    sub-steps: fb_state 0.059 / 0.056 / 0.058, plant_out 0.058 / 0.058 / 0.057, terrain_out 0.029 / 0.030 / 0.030, mpc_state 0.097 / 0.099 / 0.113,
    est_in 0.059 / 0.058 / 0.058."""
    _setup_both(gpu_ctx, pkg)
    p = PR.params(substeps=substeps, **TR.STEP_PARAMS)
    ref = TR.step_mixed([pkg.model_desc(r) for r in PR.ROBOTS], case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
    n = len(case["state"])
    pl = TerrainPlant(gpu_ctx, pkg, case["D"], case["height"], case["state"], case["cmd"], case["tid"], case["fid"], case["push"])
    marker = np.arange(54 * n, dtype=np.float32).reshape(54, n) + 0.5
    pl.est.upload(marker)
    pl.step(pkg.plant_params(substeps=substeps, **TR.STEP_PARAMS))
    got = pl.get()
    pl.free()
    G.setup_a1(gpu_ctx, pkg, 10)
    loose = PR.near_threshold(p, ref["fn"])
    assert loose.sum() <= 2
    flag_rows = {"plant_out": slice(24, 28), "est_in": slice(13, 17)}
    fails = []
    for k, rows in KEYS:
        g, r = got[k][:, :rows].astype(np.float64), ref[k].copy()
        if k in flag_rows:
            assert np.array_equal(g[:, flag_rows[k]][~loose], r[:, flag_rows[k]][~loose]), k
            g[:, flag_rows[k]] = r[:, flag_rows[k]]
        w, at = _worst(g, r)
        print("substeps %d %-11s worst %.3e of its bar at robot %d row %d" % (substeps, k, w / BAR, at[0], at[1]))
        if not np.all(np.abs(g - r) <= BAR * np.maximum(1.0, np.abs(r))):
            fails.append(k)
    assert not fails, fails
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert (got["status"] & pkg.qrgpu.PL_OFF_FIELD).any() and not (got["status"] & ~pkg.qrgpu.PL_OFF_FIELD).any()
    assert np.array_equal(got["est_in"][:, 41:], marker.T[:, 41:])


@pytest.mark.parametrize("n", [1, 17])
def test_batch_edges(gpu_ctx, pkg, case, batch48, n):
    """The first n robots on their own give the bits they give inside the batch of 48: n = 1 and 17 leave quads of the last workgroup idle."""
    _setup_both(gpu_ctx, pkg)
    alone = _run(gpu_ctx, pkg, case, pkg.plant_params(substeps=2, **TR.STEP_PARAMS), slice(0, n))
    G.setup_a1(gpu_ctx, pkg, 10)
    assert _bits_equal(alone, batch48, slice(None), slice(0, n))


def test_field_selection(gpu_ctx, pkg, case, batch48):
    """The alternating call equals, bit for bit, two calls with one field each; an id of -1 or n_fields is flagged BAD_FIELD and gives field 0's
    bits."""
    _setup_both(gpu_ctx, pkg)
    params = pkg.plant_params(substeps=2, **TR.STEP_PARAMS)
    n = len(case["state"])
    D1 = dict(case["D"], n_fields=1)
    zeros = np.zeros(n, np.int32)
    for f in (0, 1):
        one = _run(gpu_ctx, pkg, case, params, fid=zeros, height=np.ascontiguousarray(case["height"][f:f + 1]), D=D1)
        k = np.nonzero(case["fid"] == f)[0]
        assert len(k) == n // 2
        assert _bits_equal(one, batch48, k, k), f
    on0 = _run(gpu_ctx, pkg, case, params, fid=zeros)
    bad_id = np.where(np.arange(n) % 3 == 0, -1, np.where(np.arange(n) % 3 == 1, 2, 0)).astype(np.int32)
    bad = _run(gpu_ctx, pkg, case, params, fid=bad_id)
    G.setup_a1(gpu_ctx, pkg, 10)
    for k, rows in KEYS:
        assert np.array_equal(bad[k][:, :rows].view(np.uint32), on0[k][:, :rows].view(np.uint32)), k
    assert np.array_equal(bad["status"], on0["status"] | np.where(bad_id != 0, pkg.qrgpu.PL_BAD_FIELD, 0))
    assert not (on0["status"] & pkg.qrgpu.PL_BAD_FIELD).any()
    assert not _bits_equal(on0, batch48)                               # the fields do differ


def test_flat_limit(gpu_ctx, pkg, case):
    """All-zero field, no push: within the bar of qrgpu_plant_step_batch on the same inputs, terrain_out normals exactly (0, 0, 1) and heights
    ground_z; the flat call, run here, still matches plant_ref as tests/test_gpu_plant.py asserts.  Measured: the two calls bit-equal."""
    _setup_both(gpu_ctx, pkg)
    s, c, tid = case["state"], case["cmd"], case["tid"]
    n = len(s)
    D = dict(case["D"], n_fields=1)
    fields = dict(ground_z=-0.02)
    p = PR.params(**fields)
    pl = TerrainPlant(gpu_ctx, pkg, D, np.zeros((1, D["ny"], D["nx"]), np.float32), s, c, tid)
    pl.step(pkg.plant_params(**fields))
    got = pl.get()
    pl.free()
    S = pkg.to_soa
    d = dict(fb=gpu_ctx.alloc((37, n)).upload(S(s)), cmd=gpu_ctx.alloc((60, n)).upload(S(c)), out=gpu_ctx.alloc((PR.PLANT_OUT_ROWS, n)), mpc=gpu_ctx.alloc((28, n)),
             est=gpu_ctx.alloc((54, n)), st=gpu_ctx.alloc((n,), np.int32), tid=gpu_ctx.alloc((n,), np.int32).upload(tid))
    gpu_ctx.plant_step_batch(n, pkg.plant_params(**fields), d["fb"], d["cmd"], plant_out=d["out"], mpc_state=d["mpc"], est_in=d["est"], status=d["st"], type_id=d["tid"])
    gpu_ctx.sync()
    flat = dict(fb_state=d["fb"].download().T.copy(), plant_out=d["out"].download().T.copy(), mpc_state=d["mpc"].download().T.copy(),
                est_in=d["est"].download().T.copy(), status=d["st"].download())
    for v in d.values():
        v.free()
    G.setup_a1(gpu_ctx, pkg, 10)
    ref = PR.step_mixed([pkg.model_desc(r) for r in PR.ROBOTS], tid, p, s, c)
    loose = PR.near_threshold(p, ref["fn"])
    assert loose.sum() <= 2
    # (the grid is the step case's: feet beyond its border that carry load are flagged, as the restatement flags them)
    tref = TR.step_mixed([pkg.model_desc(r) for r in PR.ROBOTS], tid, p, D, np.zeros((1, D["ny"], D["nx"]), np.float32), None, None, s, c)
    assert np.array_equal(got["status"], tref["status"]) and not (got["status"] & ~pkg.qrgpu.PL_OFF_FIELD).any() and np.all(flat["status"] == 0)
    flag_rows = {"plant_out": slice(24, 28), "est_in": slice(13, 17)}
    for k, rows in (("fb_state", 37), ("plant_out", PR.PLANT_OUT_ROWS), ("mpc_state", 28), ("est_in", 41)):
        r = ref[k].copy()
        for what, x in (("terrain", got), ("flat", flat)):
            g = x[k][:, :rows].astype(np.float64)
            if k in flag_rows:
                assert np.array_equal(g[:, flag_rows[k]][~loose], r[:, flag_rows[k]][~loose]), (what, k)
                g[:, flag_rows[k]] = r[:, flag_rows[k]]
            assert np.all(np.abs(g - r) <= BAR * np.maximum(1.0, np.abs(r))), (what, k)
        a, b = got[k][:, :rows].astype(np.float64), flat[k][:, :rows].astype(np.float64)
        if k in flag_rows:
            a[:, flag_rows[k]][loose] = b[:, flag_rows[k]][loose]
        w, at = _worst(a, b)
        print("flat limit %-9s terrain call against flat call: worst %.3e of the bar" % (k, w / BAR))
        assert np.all(np.abs(a - b) <= BAR * np.maximum(1.0, np.abs(b))), k
    assert np.array_equal(got["terrain_out"][:, 4:].reshape(n, 4, 3), np.broadcast_to(np.float32([0, 0, 1]), (n, 4, 3)))
    assert np.all(got["terrain_out"][:, :4] == np.float32(-0.02))


def test_standing_on_a_slope(gpu_ctx, pkg):
    """32 A1 robots aligned with plane(tan 0.2, 0) (attitude a rotation of -0.2 about y, position 0.30 n) on joint PD (Kp 100, Kd 2), 1500 ticks
    of 1 ms at 4 sub-steps: status 0 on every tick, four feet in contact, and |sum f - (0, 0, m g)| / (m g), the height along the normal and the
    pitch within the float64 chain's end values +- three times its residual swing over its last 500 ticks (terrain_ref.SLOPE_END, SLOPE_SWING;
    test_terrain_ref.py runs that chain).  Measured: 0.08654, 0.26507, -0.24958 on every robot, the chain's 0.08655, 0.26507, -0.24958."""
    G.setup_a1(gpu_ctx, pkg, 10)
    n, ticks = 32, TR.SLOPE_TICKS
    D, height, s, c = TR.slope_case(pkg, n)
    pl = TerrainPlant(gpu_ctx, pkg, D, height, s, c)
    status = gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32))
    params = pkg.plant_params(**TR.SLOPE_PARAMS)
    for k in range(ticks):
        pl.step(params, status=status.row(k))
    got = pl.get()
    st = status.download()
    pl.free(); status.free()
    m = TR.slope_measures(got["fb_state"], got["plant_out"])
    end, band = np.array(TR.SLOPE_END), 3 * np.array(TR.SLOPE_SWING)
    for j, what in enumerate(("|sum f - m g z| / m g", "height along the normal", "pitch")):
        print("slope: %-24s %.5f .. %.5f   (chain %.5f +- %.5f)" % (what, m[:, j].min(), m[:, j].max(), end[j], band[j]))
    assert np.all(st == 0)
    assert np.all(got["plant_out"][:, 24:28] == 1)
    assert np.all(np.abs(m - end) <= band)
    # the plane's normal: the float32 nodes' rounding (6e-8 * 0.2) through derivative weights of absolute sum <= 2 / cell = 16, and the float32 output
    assert np.allclose(got["terrain_out"][:, 4:].reshape(n, 4, 3), [-np.sin(TR.SLOPE_ANGLE), 0.0, np.cos(TR.SLOPE_ANGLE)], rtol=0, atol=1e-6)


def test_error_returns(gpu_ctx, pkg):
    """QRGPU_ERR_BAD_ARG, with d_fb_state untouched, for a NULL desc or heights, nx or ny < 2, n_fields < 1, cell <= 0 or not finite, and for the
    flat call's cases (n, NULL state or command or params, substeps, dt); QRGPU_ERR_NOT_SETUP on a fresh context."""
    G.setup_a1(gpu_ctx, pkg, 10)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    n = 5
    s, c = PR.stand_state(n), PR.stand_cmd(n)
    D = TR.desc(n_fields=1, **TR.STEP_GRID)
    pl = TerrainPlant(gpu_ctx, pkg, D, np.zeros((1, D["ny"], D["nx"]), np.float32), s, c)
    P = pkg.plant_params
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    BAD, NOT_SETUP = 2, 3

    def call(handle, lib_, n_=n, par=P(), desc=pl.desc, height=pl.height, fb=pl.fb, cmd=pl.cmd):
        return lib_.qrgpu_plant_step_terrain_batch(handle, n_, None if par is None else C.byref(par), None if desc is None else C.byref(desc), vp(height), None, None,
                                                   None, vp(fb), vp(cmd), None, None, None, None, None)

    T = lambda **kw: _tdesc(pkg, dict(D, **kw))
    assert call(h, lib, desc=None) == BAD and call(h, lib, height=None) == BAD
    assert call(h, lib, desc=T(nx=1)) == BAD and call(h, lib, desc=T(ny=1)) == BAD and call(h, lib, desc=T(n_fields=0)) == BAD
    for cell in (0.0, -0.1, float("nan"), float("inf")):
        assert call(h, lib, desc=T(cell=cell)) == BAD, cell
    assert call(h, lib, n_=0) == BAD and call(h, lib, n_=gpu_ctx.max_batch + 1) == BAD
    assert call(h, lib, par=None) == BAD and call(h, lib, fb=None) == BAD and call(h, lib, cmd=None) == BAD
    assert call(h, lib, par=P(substeps=0)) == BAD and call(h, lib, par=P(substeps=65)) == BAD and call(h, lib, par=P(dt=0.0)) == BAD
    gpu_ctx.sync()
    assert np.array_equal(pl.fb.download(), pkg.to_soa(s))                       # nothing was launched by the refused calls
    assert call(h, lib) == 0
    gpu_ctx.sync()
    assert not np.array_equal(pl.fb.download(), pkg.to_soa(s))
    fresh = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
    try:
        a = fresh.alloc((60, n)); hh = fresh.alloc((1, D["ny"], D["nx"]))
        assert call(fresh._h, fresh._lib, height=hh, fb=a, cmd=a) == NOT_SETUP
        a.free(); hh.free()
    finally:
        fresh.close()
    pl.free()
