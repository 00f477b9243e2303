"""-m gpu: the plant with a body -- qrgpu_plant_step_body_batch: knee and trunk contact, joint limits, the status bits that name a fall -- against the
float64 restatement of tests/body_contact_ref.py, at the batch edges, across field ids, clear of everything against
qrgpu_plant_step_terrain_batch, through two falls, and its error returns.

Bars: the plant's 1e-6 * max(1, |ref|) per component (tests/test_gpu_plant.py)."""
import ctypes as C

import numpy as np
import pytest

import body_contact_ref as BR
import gpu_helpers as G
import plant_ref as PR
import terrain_ref as TR

pytestmark = pytest.mark.gpu

BAR = 1e-6
KEYS = (("fb_state", 37), ("plant_out", PR.PLANT_OUT_ROWS), ("terrain_out", TR.TERRAIN_OUT_ROWS), ("body_out", BR.BODY_OUT_ROWS), ("mpc_state", 28),
        ("est_in", 41))
NEW_BITS = BR.PL_TRUNK_CONTACT | BR.PL_KNEE_CONTACT | BR.PL_JOINT_LIMIT


def _bodies(ctx, pkg):
    """Both types' bodies: the session's context may carry type 1's model from a test that ran before, and every type with a model needs one."""
    for t, robot in enumerate(PR.ROBOTS):
        ctx.plant_body_setup(t, pkg.plant_body_desc(robot))


def _setup_both(ctx, pkg):
    for t, robot in enumerate(PR.ROBOTS):
        ctx.mpc_setup_packed(t, pkg.mpc_cfg(robot), PR.HORIZON); ctx.wbc_setup_packed(t, pkg.model_desc(robot))
    _bodies(ctx, pkg)


def _setup_a1(ctx, pkg):
    G.setup_a1(ctx, pkg, 10)
    _bodies(ctx, pkg)


def _tdesc(pkg, D):
    return pkg.terrain_desc(D["nx"], D["ny"], D["n_fields"], D["x0"], D["y0"], D["cell"])


class BodyPlant:
    """Device arrays of one batch of simulated robots with a body on a stack of fields."""

    def __init__(self, ctx, pkg, D, height, state, cmd, tid=None, fid=None, push=None):
        self.ctx, self.pkg, self.n = ctx, pkg, len(state)
        n = self.n
        self.desc = _tdesc(pkg, D)
        self.height = ctx.alloc(height.shape).upload(height)
        self.fb = ctx.alloc((37, n)).upload(pkg.to_soa(state)); self.cmd = ctx.alloc((60, n)).upload(pkg.to_soa(cmd))
        self.out = ctx.alloc((PR.PLANT_OUT_ROWS, n)); self.tout = ctx.alloc((TR.TERRAIN_OUT_ROWS, n)); self.bout = ctx.alloc((BR.BODY_OUT_ROWS, n))
        self.mpc = ctx.alloc((28, n)); self.est = ctx.alloc((54, n))
        self.status = ctx.alloc((n,), np.int32).upload(np.full(n, -1, np.int32))
        self.tid = None if tid is None else ctx.alloc((n,), np.int32).upload(tid)
        self.fid = None if fid is None else ctx.alloc((n,), np.int32).upload(fid)
        self.push = None if push is None else ctx.alloc((6, n)).upload(pkg.to_soa(push))

    def step(self, params, status=None, body=True):
        kw = dict(field_id=self.fid, base_push=self.push, plant_out=self.out, terrain_out=self.tout, mpc_state=self.mpc, est_in=self.est,
                  status=self.status if status is None else status, type_id=self.tid)
        if body:
            self.ctx.plant_step_body_batch(self.n, params, self.desc, self.height, self.fb, self.cmd, body_out=self.bout, **kw)
        else:
            self.ctx.plant_step_terrain_batch(self.n, params, self.desc, self.height, self.fb, self.cmd, **kw)

    def get(self):
        self.ctx.sync()
        return dict(fb_state=self.fb.download().T.copy(), plant_out=self.out.download().T.copy(), terrain_out=self.tout.download().T.copy(),
                    body_out=self.bout.download().T.copy(), mpc_state=self.mpc.download().T.copy(), est_in=self.est.download().T.copy(),
                    status=self.status.download())

    def free(self):
        for v in (self.height, self.fb, self.cmd, self.out, self.tout, self.bout, self.mpc, self.est, self.status, self.tid, self.fid, self.push):
            if v is not None:
                v.free()


def _run(ctx, pkg, case, params, sel=slice(None), fid=None, height=None, D=None, body=True):
    """One tick of the robots `sel` of a case.  -> outputs"""
    fid = case["fid"] if fid is None else fid
    pl = BodyPlant(ctx, pkg, case["D"] if D is None else D, case["height"] if height is None else height, case["state"][sel], case["cmd"][sel],
                   case["tid"][sel], fid[sel], case["push"][sel])
    if not body:
        pl.bout.zero()
    pl.step(params, body=body)
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
    return BR.step_case(pkg)


@pytest.fixture(scope="module")
def batch48(gpu_ctx, pkg, case):
    """The step case at 2 sub-steps on the device: shared, read-only."""
    _setup_both(gpu_ctx, pkg)
    got = _run(gpu_ctx, pkg, case, pkg.plant_params(substeps=2, **TR.STEP_PARAMS))
    _setup_a1(gpu_ctx, pkg)
    return got


@pytest.mark.parametrize("substeps", PR.STEP_SUBSTEPS)
def test_step_against_body_contact_ref(gpu_ctx, pkg, case, substeps):
    """One control tick of 48 mixed robots -- standing, belly on the ground, kneeling, on their backs, joints beyond their limits -- on the terrain step
    case's two stacked fields with its pushes, against the float64 restatement: fb_state, plant_out, terrain_out, body_out, mpc_state and rows 0-40 of
    est_in within 1e-6 * max(1, |ref|); status equal bit for bit and contact flags equal, except where the reference's f_n is within 1e-6 of the
    threshold (at most 2 % of the 768 flags: none, test_body_contact_ref.py); rows 41-53 of est_in as uploaded.  The worst distance of each output is printed in
    units of the bar (not yet recorded from a device: LAB_NOTES A.16)."""
    _setup_both(gpu_ctx, pkg)
    p = PR.params(substeps=substeps, **TR.STEP_PARAMS)
    models, bodies = BR.models_and_bodies(pkg)
    ref = BR.step_mixed(models, bodies, case["tid"], p, case["D"], case["height"], case["fid"], case["push"], case["state"], case["cmd"])
    n = len(case["state"])
    pl = BodyPlant(gpu_ctx, pkg, case["D"], case["height"], case["state"], case["cmd"], case["tid"], case["fid"], case["push"])
    marker = np.arange(54 * n, dtype=np.float32).reshape(54, n) + 0.5
    pl.est.upload(marker)
    pl.step(pkg.plant_params(substeps=substeps, **TR.STEP_PARAMS))
    got = pl.get()
    pl.free()
    _setup_a1(gpu_ctx, pkg)
    loose, loose_bits = BR.status_masks(p, ref["fn"])
    assert loose.sum() <= 0.02 * loose.size
    # where each group's flags go: (output, rows, the reference's loose flags of the group)
    flag_rows = (("plant_out", slice(24, 28), loose[:, BR.FEET]), ("est_in", slice(13, 17), loose[:, BR.FEET]), ("body_out", slice(12, 16), loose[:, BR.KNEES]))
    fails = []
    for k, rows in KEYS:
        g, r = got[k][:, :rows].astype(np.float64), ref[k].copy()
        for kk, sl, lo in flag_rows:
            if kk == k:
                assert np.array_equal(g[:, sl][~lo], r[:, sl][~lo]), k
                g[:, sl] = r[:, sl]
        w, at = _worst(g, r)
        print("substeps %d %-11s worst %.3e of its bar at robot %d row %d" % (substeps, k, w / BAR, at[0], at[1]))
        if not np.all(np.abs(g - r) <= BAR * np.maximum(1.0, np.abs(r))):
            fails.append(k)
    assert not fails, fails
    assert np.array_equal(got["status"] & ~loose_bits, ref["status"] & ~loose_bits), (got["status"], ref["status"])
    for b in (BR.PL_TRUNK_CONTACT, BR.PL_KNEE_CONTACT, BR.PL_JOINT_LIMIT, TR.PL_OFF_FIELD):
        assert (got["status"] & b).any(), hex(b)
    assert not (got["status"] & ~(NEW_BITS | TR.PL_OFF_FIELD)).any()
    assert np.array_equal(got["est_in"][:, 41:], marker.T[:, 41:])


@pytest.mark.parametrize("n", [1, 17])
def test_batch_edges(gpu_ctx, pkg, case, batch48, n):
    """The first n robots on their own give the bits they give inside the batch of 48: n = 1 and 17 leave quads of the last workgroup idle."""
    _setup_both(gpu_ctx, pkg)
    alone = _run(gpu_ctx, pkg, case, pkg.plant_params(substeps=2, **TR.STEP_PARAMS), slice(0, n))
    _setup_a1(gpu_ctx, pkg)
    assert _bits_equal(alone, batch48, slice(None), slice(0, n))


def test_field_selection(gpu_ctx, pkg, case, batch48):
    """The call with field ids in pairs equals, bit for bit, two calls with one field each."""
    _setup_both(gpu_ctx, pkg)
    params = pkg.plant_params(substeps=2, **TR.STEP_PARAMS)
    n = len(case["state"])
    D1 = dict(case["D"], n_fields=1)
    zeros = np.zeros(n, np.int32)
    ones = []
    for f in (0, 1):
        one = _run(gpu_ctx, pkg, case, params, fid=zeros, height=np.ascontiguousarray(case["height"][f:f + 1]), D=D1)
        k = np.nonzero(case["fid"] == f)[0]
        assert len(k) == n // 2
        assert _bits_equal(one, batch48, k, k), f
        ones.append(one)
    _setup_a1(gpu_ctx, pkg)
    assert not _bits_equal(ones[0], ones[1])                           # the fields do differ


def test_clear_of_everything_is_the_terrain_call(gpu_ctx, pkg):
    """The terrain step case's robots 0.29 above the ground under them -- trunk and knees clear, joints inside their limits, a quarter of the feet or
    more in contact: the body call within 1e-6 * max(1, |ref|) of qrgpu_plant_step_terrain_batch on the same inputs, body_out all zero, no new status
    bit.  Whether the two are bit for bit is printed, not required: two kernels may contract multiply-adds differently (LAB_NOTES A.16)."""
    _setup_both(gpu_ctx, pkg)
    clear = BR.clear_case(pkg)
    params = pkg.plant_params(substeps=2, **TR.STEP_PARAMS)
    a = _run(gpu_ctx, pkg, clear, params)
    b = _run(gpu_ctx, pkg, clear, params, body=False)
    _setup_a1(gpu_ctx, pkg)
    assert (b["plant_out"][:, 24:28] == 1).sum() >= 48
    same = True
    for k, rows in KEYS:
        if k == "body_out":
            continue
        x, y = a[k][:, :rows].astype(np.float64), b[k][:, :rows].astype(np.float64)
        w, _ = _worst(x, y)
        bits = np.array_equal(a[k][:, :rows].view(np.uint32), b[k][:, :rows].view(np.uint32))
        same = same and bits
        print("clear of everything %-11s body call against terrain call: worst %.3e of the bar, bit for bit: %s" % (k, w / BAR, bits))
        assert np.all(np.abs(x - y) <= BAR * np.maximum(1.0, np.abs(y))), k
    print("clear of everything: all outputs bit for bit: %s" % same)
    assert not a["body_out"].any()
    assert np.array_equal(a["status"], b["status"]) and not (a["status"] & NEW_BITS).any()


def test_falls_are_physical(gpu_ctx, pkg):
    """32 A1 robots, all gains and torques zero, dropped from z = 0.30 -- the even ones level, the odd ones rolled by pi -- through 1400 ticks of 1 ms at 2
    sub-steps on the flat field: finite on every tick; base height, sum f_z over the sixteen points / (m g) and the largest excursion beyond a joint
    limit end within the float64 chains' end values +- three times their residual swing over their last 350 ticks (body_contact_ref.FALL_END,
    FALL_SWING; test_body_contact_ref.py runs the chains); TRUNK_CONTACT at the end on every robot; JOINT_LIMIT seen on the limp-drop robots.  The same
    32 robots through qrgpu_plant_step_terrain_batch end with the base origin below the ground: the contrast the feature is for."""
    _setup_a1(gpu_ctx, pkg)
    n, ticks = 32, BR.FALL_TICKS
    D, height, s, c, scen = BR.fall_case(pkg, n)
    body = BR.body_of(pkg.plant_body_desc("a1"))
    params = pkg.plant_params(**BR.FALL_PARAMS)
    pl = BodyPlant(gpu_ctx, pkg, D, height, s, c)
    status = gpu_ctx.alloc((ticks, n), np.int32).upload(np.full((ticks, n), -1, np.int32))
    for k in range(ticks):
        pl.step(params, status=status.row(k))
    got = pl.get()
    st = status.download()
    pl.free(); status.free()
    old = BodyPlant(gpu_ctx, pkg, D, height, s, c)
    for k in range(ticks):
        old.step(params, body=False)
    sunk = old.get()
    old.free()
    assert np.isfinite(got["fb_state"]).all() and not (st & pkg.qrgpu.PL_NONFINITE).any() and not (st & ~NEW_BITS).any()
    m = BR.fall_measures(body, got["fb_state"], got["plant_out"], got["body_out"])
    for i, name in enumerate(BR.SCENARIOS):
        k = scen == i
        end, band = np.array(BR.FALL_END[name]), 3 * np.array(BR.FALL_SWING[name])
        for j, what in enumerate(("base height", "sum f_z / m g", "excursion beyond a limit")):
            print("%-4s %-24s %.5f .. %.5f   (chain %.5f +- %.5f)" % (name, what, m[k, j].min(), m[k, j].max(), end[j], band[j]))
        assert np.all(np.abs(m[k] - end) <= band), name
    assert np.all(got["fb_state"][:, 6] > 0.0)
    assert np.all(st[-1] & BR.PL_TRUNK_CONTACT)
    assert np.all(np.bitwise_or.reduce(st[:, scen == 0], axis=0) & BR.PL_JOINT_LIMIT)
    # without a body the trunk goes through the ground (where the state stays finite at all)
    z_old = sunk["fb_state"][:, 6]
    print("the terrain call's base heights at the end: %s" % np.array2string(z_old, precision=3))
    assert np.all(~np.isfinite(z_old) | (z_old < 0.0))


def test_error_returns(gpu_ctx, pkg):
    """qrgpu_plant_body_setup: QRGPU_ERR_BAD_ARG for a non-finite or non-positive trunk_half, q_lo >= q_hi, a negative or non-finite limit_k or limit_a, a
    type id outside 0..3, a NULL desc.  qrgpu_plant_step_body_batch: the terrain call's QRGPU_ERR_BAD_ARG cases with d_fb_state untouched;
    QRGPU_ERR_NOT_SETUP on a fresh context, and on a context whose type 1 has a model and no body."""
    _setup_a1(gpu_ctx, pkg)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    n = 5
    s, c = PR.stand_state(n), PR.stand_cmd(n)
    D = TR.desc(n_fields=1, **TR.STEP_GRID)
    pl = BodyPlant(gpu_ctx, pkg, D, np.zeros((1, D["ny"], D["nx"]), np.float32), s, c)
    P = pkg.plant_params
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    BAD, NOT_SETUP = 2, 3

    def call(handle, lib_, n_=n, par=P(), desc=pl.desc, height=pl.height, fb=pl.fb, cmd=pl.cmd):
        return lib_.qrgpu_plant_step_body_batch(handle, n_, None if par is None else C.byref(par), None if desc is None else C.byref(desc), vp(height), None, None,
                                                None, vp(fb), vp(cmd), None, None, None, None, None, None)

    B = pkg.plant_body_desc
    setup = lambda d, t=2: lib.qrgpu_plant_body_setup(h, t, None if d is None else C.byref(d))
    nan, inf = float("nan"), float("inf")
    for half in ((0.0, 0.1, 0.1), (0.1, -0.1, 0.1), (0.1, 0.1, nan), (inf, 0.1, 0.1)):
        assert setup(B(trunk_half=half)) == BAD, half
    assert setup(B(q_lo=(0.9, -1.0, -2.6))) == BAD and setup(B(q_hi=(0.8, 4.1, -2.69653369433))) == BAD and setup(B(q_lo=(nan, -1.0, -2.6))) == BAD
    for v in (-1.0, nan, inf):
        assert setup(B(limit_k=v)) == BAD and setup(B(limit_a=v)) == BAD, v
    assert setup(B(), t=-1) == BAD and setup(B(), t=4) == BAD and setup(None) == BAD
    assert setup(B(limit_k=0.0, limit_a=0.0), t=3) == 0                    # no stops at all is a body too; a type without a model may have one

    T = lambda **kw: _tdesc(pkg, dict(D, **kw))
    assert call(h, lib, desc=None) == BAD and call(h, lib, height=None) == BAD
    assert call(h, lib, desc=T(nx=1)) == BAD and call(h, lib, desc=T(ny=1)) == BAD and call(h, lib, desc=T(n_fields=0)) == BAD
    for cell in (0.0, -0.1, nan, inf):
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
        a = fresh.alloc((60, n)); hh = fresh.alloc((1, D["ny"], D["nx"])); fb = fresh.alloc((37, n)).upload(pkg.to_soa(s))
        f = lambda: call(fresh._h, fresh._lib, height=hh, fb=fb, cmd=a)
        assert f() == NOT_SETUP                                                    # no model at all
        fresh.wbc_setup_packed(0, pkg.model_desc("a1"))
        assert f() == NOT_SETUP                                                    # a model and no body
        fresh.plant_body_setup(0, pkg.plant_body_desc("a1"))
        fresh.wbc_setup_packed(1, pkg.model_desc("lite3"))
        assert f() == NOT_SETUP                                                    # type 1 has a model and no body
        fresh.sync()
        assert np.array_equal(fb.download(), pkg.to_soa(s))
        fresh.plant_body_setup(1, pkg.plant_body_desc("lite3"))
        a.zero()
        assert f() == 0
        fresh.sync()
        assert not np.array_equal(fb.download(), pkg.to_soa(s))
        a.free(); hh.free(); fb.free()
    finally:
        fresh.close()
    pl.free()
