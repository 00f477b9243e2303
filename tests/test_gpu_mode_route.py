"""-m gpu: the mode per robot -- qrgpu_mode_route_batch, qrgpu_set_mode_route, qrgpu_mode_command_batch (include/qrgpu.h).

Every equality is bit for bit: the kernels copy, compare and skip.  Shapes: n = 130 (two workgroups and a partial one), n = 9 (the force-balance launch
rounds its grid up to 16 workgroups), n = 1.  Chain patterns (tests/mode_route_ref.py): r % 3; one whole wavefront idle; nobody on the MPC chain; nobody
on the force-balance chain; everybody on one chain.

  * the route and the merge against the numpy restatement, the flags and the counters onto poisoned arrays, the merge into each of its inputs;
  * every BAD_ARG launches nothing, names its argument, and a valid call follows;
  * qrgpu_tick_cadence_batch, qrgpu_stance_tick_batch, qrgpu_vmc_force_batch and qrgpu_vmc_force_world_batch under the binding: a robot on the call's
    chain carries what the same call gives it with nothing bound, every output column of any other robot keeps its poison, and clearing the binding
    restores the unbound result.  The cadenced contexts start every solve cold (gpu_helpers.cold_start), so a call's result is a function of its inputs;
  * qrgpu_tick_batch ignores the binding."""
import ctypes

import numpy as np
import pytest

import gpu_helpers as G
import mode_route_ref as R
import stance_ref as SR

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
POISON_F, POISON_I = f32(-12345.5), 0x7f0000ff
SHAPES = (130, 9, 1)
BAD_ARG = 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def desc_of(pkg, table=R.DEFAULT_TABLE, fallback=R.DEFAULT_FALLBACK):
    return pkg.mode_route_desc(chain_of_mode=list(table), fallback_chain=fallback)


# ----------------------------------------------------------------------------------------------------------------------------------- the route
@pytest.mark.parametrize("n", SHAPES + (4096,))
@pytest.mark.parametrize("cfg", ["default_with_plan", "custom_no_plan"])
def test_route_against_the_restatement(gpu_ctx, pkg, n, cfg):
    table, fallback, with_plan = (R.DEFAULT_TABLE, R.DEFAULT_FALLBACK, True) if cfg == "default_with_plan" else ((R.CHAIN_MPC, R.CHAIN_FORCE_BALANCE, 0, 2), 2, False)
    sel, plan = R.random_columns(n, 40 + n)
    ctx = gpu_ctx
    d_sel, d_plan = ctx.alloc((n,)).upload(sel), ctx.alloc((n,), i32).upload(plan)
    d_chain, d_flags, d_count = (ctx.alloc((n,), i32).upload(np.full(n, POISON_I, i32)), ctx.alloc((n,), i32).upload(np.full(n, POISON_I, i32)),
                                 ctx.alloc((3,), i32).upload(np.full(3, POISON_I, i32)))
    try:
        ctx.mode_route(n, desc_of(pkg, table, fallback), d_sel, d_chain, plan=d_plan if with_plan else None, route_flags=d_flags, chain_count=d_count)
        ctx.sync()
        chain, flags, count = R.route(sel, plan if with_plan else None, table, fallback)
        assert np.array_equal(d_chain.download(), chain) and np.array_equal(d_flags.download(), flags) and np.array_equal(d_count.download(), count)
        assert int(count.sum()) == n
        # the flags and the counters are written, not accumulated: a second call on other selections, on the arrays the first one left
        sel2 = np.roll(sel, 1) if n > 1 else np.array([3], f32)
        d_sel.upload(sel2)
        ctx.mode_route(n, desc_of(pkg, table, fallback), d_sel, d_chain, plan=d_plan if with_plan else None, route_flags=d_flags, chain_count=d_count)
        ctx.sync()
        chain, flags, count = R.route(sel2, plan if with_plan else None, table, fallback)
        assert np.array_equal(d_chain.download(), chain) and np.array_equal(d_flags.download(), flags) and np.array_equal(d_count.download(), count)
        # ... and the optional outputs are optional
        d_chain.upload(np.full(n, POISON_I, i32)); d_flags.upload(np.full(n, POISON_I, i32)); d_count.upload(np.full(3, POISON_I, i32))
        ctx.mode_route(n, desc_of(pkg, table, fallback), d_sel, d_chain)
        ctx.sync()
        assert np.array_equal(d_chain.download(), R.route(sel2, None, table, fallback)[0])
        assert np.all(d_flags.download() == POISON_I) and np.all(d_count.download() == POISON_I)
    finally:
        for v in (d_sel, d_plan, d_chain, d_flags, d_count):
            v.free()


def test_route_hand_table(gpu_ctx, pkg):
    """The header's table on the device, without the restatement in between: every mode, the selections that are no mode, a plan that runs nothing."""
    sel = np.array([-1, 0, 1, 2, 3, np.nan, 1.5, 4, -2, 3, 0], f32)
    plan = np.array([1, 1, 1, 2, 2, 1, 1, 1, 1, 0x10, 0x408], i32)
    n = len(sel)
    ctx = gpu_ctx
    d = [ctx.alloc((n,)).upload(sel), ctx.alloc((n,), i32).upload(plan), ctx.alloc((n,), i32), ctx.alloc((n,), i32), ctx.alloc((3,), i32)]
    try:
        ctx.mode_route(n, pkg.mode_route_desc(), d[0], d[2], plan=d[1], route_flags=d[3], chain_count=d[4])
        ctx.sync()
        assert d[2].download().tolist() == [0, 2, 1, 1, 1, 1, 1, 1, 1, 0, 0]
        assert d[3].download().tolist() == [0, 0, 2, 2, 0, 1, 1, 1, 1, 0, 0]
        assert d[4].download().tolist() == [3, 7, 1]
        q = pkg.qrgpu
        assert (q.CHAIN_NONE, q.CHAIN_MPC, q.CHAIN_FORCE_BALANCE, q.ROUTE_BAD_MODE, q.ROUTE_NO_CHAIN) == (0, 1, 2, 1, 2)
        dd = pkg.mode_route_desc()
        assert list(dd.chain_of_mode) == [2, 0, 0, 1] and dd.fallback_chain == 1
    finally:
        for v in d:
            v.free()


# ----------------------------------------------------------------------------------------------------------------------------------- the merge
def _merge_inputs(n, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((60, n)).astype(f32), rng.standard_normal((60, n)).astype(f32)
    a[:, rng.random(n) < 0.3] = np.nan
    b[:, rng.random(n) < 0.3] = np.nan
    a[7, 0] = np.array([0x7fc01234], np.uint32).view(f32)[0]                  # a NaN with a payload: passed through where it is selected
    return a, b, rng.integers(1, 1 << 30, n).astype(i32), rng.integers(1, 1 << 30, n).astype(i32)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("pattern", R.PATTERNS + ("out_of_range",))
def test_merge_against_the_restatement_and_into_each_input(gpu_ctx, pkg, n, pattern):
    chain = (np.arange(n) % 7 - 2).astype(i32) if pattern == "out_of_range" else R.pattern(pattern, n)
    a, b, sa, sb = _merge_inputs(n, 7 * n)
    want, want_st = R.command(chain, a, b, sa, sb)
    ctx = gpu_ctx
    d = dict(chain=ctx.alloc((n,), i32).upload(chain), a=ctx.alloc((60, n)).upload(a), b=ctx.alloc((60, n)).upload(b), sa=ctx.alloc((n,), i32).upload(sa),
             sb=ctx.alloc((n,), i32).upload(sb), out=ctx.alloc((60, n)).upload(np.full((60, n), POISON_F, f32)), st=ctx.alloc((n,), i32).upload(np.full(n, POISON_I, i32)))
    try:
        ctx.mode_command(n, d["chain"], d["a"], d["b"], d["out"], status_mpc=d["sa"], status_fb=d["sb"], status=d["st"])
        ctx.sync()
        assert same(d["out"].download(), want) and np.array_equal(d["st"].download(), want_st)
        assert same(d["a"].download(), a) and same(d["b"].download(), b)
        idle = (chain != 1) & (chain != 2)
        assert not bits(want[:, idle]).any() and not want_st[idle].any()
        # without the status arrays: the command alone, and status 0 where an input is missing
        d["out"].upload(np.full((60, n), POISON_F, f32)); d["st"].upload(np.full(n, POISON_I, i32))
        ctx.mode_command(n, d["chain"], d["a"], d["b"], d["out"], status_fb=d["sb"], status=d["st"])
        ctx.sync()
        assert same(d["out"].download(), want) and np.array_equal(d["st"].download(), R.command(chain, a, b, None, sb)[1])
        ctx.mode_command(n, d["chain"], d["a"], d["b"], d["out"])
        # into the MPC chain's array, then into the force-balance chain's; the status into its own input too
        ctx.mode_command(n, d["chain"], d["a"], d["b"], d["a"], status_mpc=d["sa"], status_fb=d["sb"], status=d["sa"])
        ctx.sync()
        assert same(d["a"].download(), want) and same(d["b"].download(), b) and np.array_equal(d["sa"].download(), want_st)
        d["a"].upload(a); d["sa"].upload(sa)
        ctx.mode_command(n, d["chain"], d["a"], d["b"], d["b"], status_mpc=d["sa"], status_fb=d["sb"], status=d["sb"])
        ctx.sync()
        assert same(d["b"].download(), want) and same(d["a"].download(), a) and np.array_equal(d["sb"].download(), want_st)
    finally:
        for v in d.values():
            v.free()


# ----------------------------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_launch_nothing_and_a_valid_call_follows(pkg):
    n = 9
    ctx = pkg.Context(0, n, 16)
    sel, plan = R.random_columns(n, 3)
    a, b, sa, sb = _merge_inputs(n, 4)
    d = dict(sel=ctx.alloc((n,)).upload(sel), plan=ctx.alloc((n,), i32).upload(plan), chain=ctx.alloc((n,), i32), flags=ctx.alloc((n,), i32), count=ctx.alloc((3,), i32),
             a=ctx.alloc((60, n)).upload(a), b=ctx.alloc((60, n)).upload(b), sa=ctx.alloc((n,), i32).upload(sa), sb=ctx.alloc((n,), i32).upload(sb),
             out=ctx.alloc((60, n)), st=ctx.alloc((n,), i32))
    lib, h = ctx._lib, ctx._h
    P = lambda k: None if k is None else d[k].ptr

    def poison():
        for k in ("chain", "flags", "st"):
            d[k].upload(np.full(n, POISON_I, i32))
        d["count"].upload(np.full(3, POISON_I, i32)); d["out"].upload(np.full((60, n), POISON_F, f32))

    def untouched():
        ctx.sync()
        return (all(np.all(d[k].download() == POISON_I) for k in ("chain", "flags", "count", "st")) and np.all(d["out"].download() == POISON_F))

    def route(n_=n, desc=None, no_desc=False, sel_="sel", chain_="chain"):
        dd = pkg.mode_route_desc() if desc is None else desc
        return lib.qrgpu_mode_route_batch(h, n_, None if no_desc else ctypes.byref(dd), P(sel_), P("plan"), P(chain_), P("flags"), P("count"))

    def merge(n_=n, chain_="chain", a_="a", b_="b", out_="out"):
        return lib.qrgpu_mode_command_batch(h, n_, P(chain_), P(a_), P(b_), P("sa"), P("sb"), P(out_), P("st"))

    try:
        assert pkg.qrgpu.ERRORS[BAD_ARG] == "BAD_ARG"
        poison()
        refused = [(route(no_desc=True), "desc"), (route(sel_=None), "d_mode_sel"), (route(chain_=None), "d_chain"), (route(0), "n"), (route(n + 1), "n"),
                   (route(desc=pkg.mode_route_desc(chain_of_mode=[2, 0, 3, 1])), "chain_of_mode"), (route(desc=pkg.mode_route_desc(chain_of_mode=[-1, 0, 0, 1])), "chain_of_mode"),
                   (route(desc=pkg.mode_route_desc(fallback_chain=3)), "fallback_chain"), (route(desc=pkg.mode_route_desc(fallback_chain=-1)), "fallback_chain")]
        for rc, _ in refused:
            assert rc == BAD_ARG
        # (the message of the last refusal of each kind names its argument)
        for call, word in ((lambda: route(no_desc=True), "desc"), (lambda: route(sel_=None), "d_mode_sel"), (lambda: route(chain_=None), "d_chain"),
                           (lambda: route(0), ": n"), (lambda: route(desc=pkg.mode_route_desc(fallback_chain=3)), "fallback_chain"),
                           (lambda: merge(chain_=None), "d_chain"), (lambda: merge(a_=None), "d_cmd_mpc"), (lambda: merge(b_=None), "d_cmd_fb"),
                           (lambda: merge(out_=None), "d_motor_cmd"), (lambda: merge(0), ": n"), (lambda: merge(n + 1), ": n")):
            assert call() == BAD_ARG
            assert word in ctx.last_error(), (word, ctx.last_error())
        assert untouched()
        assert route() == 0 and merge() == 0
        ctx.sync()
        chain, flags, count = R.route(sel, plan)
        assert np.array_equal(d["chain"].download(), chain) and np.array_equal(d["flags"].download(), flags) and np.array_equal(d["count"].download(), count)
        want, want_st = R.command(chain, a, b, sa, sb)
        assert same(d["out"].download(), want) and np.array_equal(d["st"].download(), want_st)
    finally:
        for v in d.values():
            v.free()
        ctx.close()


# ----------------------------------------------------------------------------------------------------------------------------------- the cadenced tick
CAD_OUT = ("force", "hold", "tau", "qdes", "prev", "status")


class _Cadence:
    """One cold context and one set of arrays per n; the inputs every call starts from; the unbound result per `updated` mask, made once."""

    def __init__(self, pkg, n, h=10):
        self.pkg, self.n = pkg, n
        self.ctx = ctx = pkg.Context(0, max(n, 64), 16)
        G.setup_a1(ctx, pkg, h)
        ctx.set_torque_epilogue(hip_comp=True, clip=True)
        ctx.set_warm_start(False); ctx.set_planned_list(False)
        b = pkg.make_batch(n, h, "a1", seed=0x40DE + n)
        S = pkg.to_soa
        self.d = dict(state=ctx.alloc((28, n)).upload(S(b["mpc_state"])), traj=ctx.alloc((12 * h, n)).upload(S(b["traj"])), gait=ctx.alloc((4 * h, n)).upload(S(b["gait"])),
                      fb=ctx.alloc((37, n)).upload(S(b["fb_state"])), cmd=ctx.alloc((67, n)).upload(S(b["wbc_cmd"])), prev=ctx.alloc((3, n)), force=ctx.alloc((12, n)),
                      hold=ctx.alloc((12, n)), tau=ctx.alloc((12, n)), qdes=ctx.alloc((24, n)), status=ctx.alloc((n,), i32), due=ctx.alloc((n,), i32),
                      chain=ctx.alloc((n,), i32))
        rng = np.random.default_rng(n)
        self.inputs = dict(force=np.zeros((12, n), f32), hold=np.zeros((12, n), f32), prev=rng.uniform(-0.2, 0.2, (3, n)).astype(f32))
        # the memory every case starts from: the forces and the kept forces of one tick in which everybody was solved
        first = self.call(np.ones(n, i32))
        self.inputs.update(force=first["force"], hold=first["hold"])
        assert np.isfinite(first["force"]).all() and np.abs(first["force"]).max() > 1.0
        self.refs = {}

    def call(self, updated, keep=None):
        """One cadenced tick from the inputs; keep [n] bool: the robots whose memory columns are the inputs (the others start at the poison)."""
        n, d = self.n, self.d
        keep = np.ones(n, bool) if keep is None else keep
        for k in ("force", "hold", "prev"):
            d[k].upload(np.where(keep[None, :], self.inputs[k], POISON_F).astype(f32))
        d["tau"].upload(np.full((12, n), POISON_F, f32)); d["qdes"].upload(np.full((24, n), POISON_F, f32)); d["status"].upload(np.full(n, POISON_I, i32))
        d["due"].upload(np.asarray(updated, i32))
        self.ctx.tick_cadence_batch(n, d["due"], d["state"], d["traj"], d["gait"], d["fb"], d["cmd"], d["prev"], d["force"], d["hold"], d["tau"],
                                    status=d["status"], qdes=d["qdes"])
        self.ctx.sync()
        return {k: d[k].download() for k in CAD_OUT}

    def ref(self, which):
        if which not in self.refs:
            self.refs[which] = self.call(self.updated(which))
        return self.refs[which]

    def updated(self, which):
        return ((np.arange(self.n) % 2 == (0 if which == "even" else 1)) * 5).astype(i32)        # (any non-zero word counts)

    def close(self):
        for v in self.d.values():
            v.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def cadence(pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = _Cadence(pkg, n)
        return made[n]
    yield get
    for c in made.values():
        c.close()


def _columns_equal(got, ref, cols, names, tag):
    for k in names:
        g, r = got[k], ref[k]
        assert same(g[..., cols], r[..., cols]), (tag, k)


def _columns_poison(got, cols, names, tag):
    for k in names:
        assert np.all(got[k][..., cols] == (POISON_I if got[k].dtype == np.int32 else POISON_F)), (tag, k)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_cadenced_tick_under_the_binding(cadence, n, pattern):
    C = cadence(n)
    chain = R.pattern(pattern, n)
    on = chain == R.CHAIN_MPC
    for which in ("even", "odd"):
        ref, up = C.ref(which), C.updated(which)
        assert np.isfinite(ref["tau"]).all() and not np.any(ref["status"] == POISON_I)
        C.d["chain"].upload(chain)
        C.ctx.set_mode_route(C.d["chain"])
        try:
            got = C.call(up, keep=on)
        finally:
            C.ctx.clear_mode_route()
        tag = (n, pattern, which)
        _columns_equal(got, ref, on, CAD_OUT, tag)                     # on the chain: exactly the unbound call, due or held
        _columns_poison(got, ~on, CAD_OUT, tag)                        # idle: nothing of the robot was written
        again = C.call(up)                                             # cleared: today's result
        _columns_equal(again, ref, np.ones(n, bool), CAD_OUT, tag + ("cleared",))
    if n > 1 and pattern in ("mod3", "no_fb", "all_mpc"):              # not vacuous: robots on the chain, each solved under one mask and held under the other
        assert on.any() and np.all((C.updated("even") != 0) ^ (C.updated("odd") != 0))


def test_tick_batch_ignores_the_binding(pkg):
    n = 9
    ctx = pkg.Context(0, 64, 16)
    G.setup_a1(ctx, pkg, 10)
    b = pkg.make_batch(n, 10, "a1", seed=77)
    d_chain = ctx.alloc((n,), i32).upload(R.pattern("mod3", n))
    try:
        with G.cold_start(ctx):
            ref = G.run_tick(ctx, pkg, b, want_qdes=True)
            ctx.set_mode_route(d_chain)
            got = G.run_tick(ctx, pkg, b, want_qdes=True)
            ctx.clear_mode_route()
        for k in ref:
            assert same(got[k], ref[k]), k
        assert np.isfinite(ref["tau"]).all()
    finally:
        d_chain.free(); ctx.close()


# ----------------------------------------------------------------------------------------------------------------------------------- the force-balance QP
def _vmc_setup(ctx, pkg):
    ctx.vmc_setup_packed(0, pkg.workload.vmc_cfg("a1"), pkg.model_desc("a1")[:3])


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("world", [False, True], ids=["base", "world"])
def test_force_balance_qp_under_the_binding(gpu_ctx, pkg, n, world):
    ctx, W, S = gpu_ctx, pkg.workload, pkg.to_soa
    _vmc_setup(ctx, pkg)
    if world:
        vin, q, ratio = W.make_vmc_world_batch(n, seed=50 + n)
    else:
        (vin, q), ratio = W.make_vmc_batch(n, seed=50 + n), None
    d = dict(vin=ctx.alloc((37, n)).upload(S(vin)), q=ctx.alloc((12, n)).upload(S(q)), force=ctx.alloc((12, n)), tau=ctx.alloc((12, n)), status=ctx.alloc((n,), i32),
             chain=ctx.alloc((n,), i32))
    if world:
        d["ratio"] = ctx.alloc((8, n)).upload(S(ratio))

    def call():
        d["force"].upload(np.full((12, n), POISON_F, f32)); d["tau"].upload(np.full((12, n), POISON_F, f32)); d["status"].upload(np.full(n, POISON_I, i32))
        if world:
            ctx.vmc_force_world_batch(n, d["vin"], d["ratio"], d["q"], d["force"], d["tau"], d["status"])
        else:
            ctx.vmc_force_batch(n, d["vin"], d["q"], d["force"], d["tau"], d["status"])
        ctx.sync()
        return {k: d[k].download() for k in ("force", "tau", "status")}

    try:
        ref = call()
        assert np.isfinite(ref["force"]).all() and not np.any(ref["status"] == POISON_I)
        for pattern in R.PATTERNS:
            chain = R.pattern(pattern, n)
            on = chain == R.CHAIN_FORCE_BALANCE
            d["chain"].upload(chain)
            ctx.set_mode_route(d["chain"])
            try:
                got = call()
            finally:
                ctx.clear_mode_route()
            _columns_equal(got, ref, on, ("force", "tau", "status"), (n, pattern))
            _columns_poison(got, ~on, ("force", "tau", "status"), (n, pattern))
            _columns_equal(call(), ref, np.ones(n, bool), ("force", "tau", "status"), (n, pattern, "cleared"))
    finally:
        ctx.clear_mode_route()
        for v in d.values():
            v.free()


@pytest.mark.parametrize("n", SHAPES)
def test_stance_tick_under_the_binding(gpu_ctx, pkg, n):
    """The update and command kernels run for everybody (vmc_in, ratio, stance_out and the stage's memory are the unbound call's on every robot); the QP's
    force, torque and status, and with them the motor command, are the unbound call's on the force-balance chain and untouched (the command: made from
    the untouched torque) anywhere else."""
    ctx, q = gpu_ctx, pkg.qrgpu
    _vmc_setup(ctx, pkg)
    inp = SR.make_inputs(n, SR.VELOCITY, 0x57A1)
    desc = pkg.stance_desc(q.MODE_VELOCITY, terrain=3)
    T = lambda a: np.ascontiguousarray(a.T)
    ins = {k: ctx.alloc(T(v).shape).upload(T(v)) for k, v in inp.items()}
    rng = np.random.default_rng(n)
    sq, fl = rng.normal(0, 1, (24, n)).astype(f32), (rng.random((4, n)) < 0.3).astype(f32)
    d = dict(st=ctx.alloc((q.STANCE_STATE_FLOATS, n)), vmc=ctx.alloc((37, n)), ratio=ctx.alloc((8, n)), out=ctx.alloc((33, n)), force=ctx.alloc((12, n)),
             tau=ctx.alloc((12, n)), status=ctx.alloc((n,), i32), cmd=ctx.alloc((60, n)), sq=ctx.alloc((24, n)).upload(sq), fl=ctx.alloc((4, n)).upload(fl),
             chain=ctx.alloc((n,), i32))
    outs = ("st", "vmc", "ratio", "out", "force", "tau", "status", "cmd")

    def call():
        d["st"].upload(np.full((q.STANCE_STATE_FLOATS, n), 0.3, f32))
        for k in ("vmc", "ratio", "out", "force", "tau", "cmd"):
            d[k].upload(np.full(d[k].shape, POISON_F, f32))
        d["status"].upload(np.full(n, POISON_I, i32))
        ctx.stance_tick_batch(n, desc, ins["est_in"], ins["est_out"], ins["ground"], ins["rpy"], ins["gait_out"], ins["cmd"], d["st"], d["vmc"], d["force"], d["tau"],
                              d["cmd"], gait_state=ins["gait_state"], ratio=d["ratio"], stance_out=d["out"], status=d["status"], swing_q=d["sq"], swing_flag=d["fl"],
                              current_time=0.1)
        ctx.sync()
        return {k: d[k].download() for k in outs}

    try:
        ref = call()
        assert not np.any(ref["force"] == POISON_F) and not np.any(ref["cmd"] == POISON_F) and not np.any(ref["status"] == POISON_I)
        everybody = np.ones(n, bool)
        for pattern in R.PATTERNS:
            chain = R.pattern(pattern, n)
            on = chain == R.CHAIN_FORCE_BALANCE
            d["chain"].upload(chain)
            ctx.set_mode_route(d["chain"])
            try:
                got = call()
            finally:
                ctx.clear_mode_route()
            tag = (n, pattern)
            _columns_equal(got, ref, everybody, ("st", "vmc", "ratio", "out"), tag)
            _columns_equal(got, ref, on, ("force", "tau", "status", "cmd"), tag)
            _columns_poison(got, ~on, ("force", "tau", "status"), tag)
            _columns_equal(call(), ref, everybody, outs, tag + ("cleared",))
    finally:
        ctx.clear_mode_route()
        for v in (*ins.values(), *d.values()):
            v.free()
