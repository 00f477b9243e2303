"""GPU: qrgpu_gait_select_update_batch and qrgpu_stage_clock_batch -- the open-loop gait generator on the table entry each robot latched at its last
reset, and the stage clock that restarts where a mask says.  n = 65 throughout (one full wavefront and one lane).  Bar: bit for bit.
  1 a uniform selection is qrgpu_gait_update_batch with that entry (a kernel pinned to the oracle)      2 the mixed schedules of tests/gait_select_ref.py,
  resets from a device mask under qrgpu_set_stage_reset, the clock from qrgpu_stage_clock_batch, against the restatement      3 what is not owned is not
  written      4 bad selections      5 every QRGPU_ERR_BAD_ARG      6 the clock against numpy      7 with the state machine, on the set-up of
  tests/test_gpu_fsm_loop.py."""
import numpy as np
import pytest

import fsm_ref as F
import gait_ref as G
import gait_select_ref as R

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
N, T = R.N_ROBOTS, R.TICKS
POISON = f32(-12345.5)
IPOISON = 0x7ABCDEF0


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def first_bad(a, b):
    a, b = np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32)
    return tuple(int(v[0]) for v in np.nonzero(a != b)) if (a != b).any() else None


def free(d):
    for v in d.values():
        v.free()


# ----------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["default", "reset"])
@pytest.mark.parametrize("entry", range(5))
def test_uniform_selection_is_the_existing_kernel(gpu_ctx, pkg, entry, name):
    ctx, q = gpu_ctx, pkg.qrgpu
    table = pkg.workload.gait_table()
    c = G.configuration(pkg, name)
    nan = np.full((52, N), np.nan, f32)
    d = dict(sel=ctx.alloc((N,)).upload(np.full(N, entry, f32)), c=ctx.alloc((T, 4, N)).upload(np.ascontiguousarray(c["contact"].transpose(0, 2, 1))),
             st=ctx.alloc((52, N)).upload(nan), st0=ctx.alloc((52, N)).upload(nan), out=ctx.alloc((T, 24, N)).upload(np.full((T, 24, N), np.nan, f32)),
             out0=ctx.alloc((T, 24, N)).upload(np.full((T, 24, N), np.nan, f32)), fe=ctx.alloc((T, 64, N)).upload(np.full((T, 64, N), POISON, f32)),
             fe0=ctx.alloc((T, 64, N)).upload(np.full((T, 64, N), POISON, f32)))
    try:
        for k in range(T):
            reset = q.GAIT_RESET_CONSTRUCT if k == 0 else (q.GAIT_RESET_LIVE if c["reset"][k] else 0)
            ct = d["c"].row(k)
            ctx.gait_select_update_batch(N, table, d["sel"], float(c["time"][k]), ct, d["st"], d["out"].row(k), d["fe"].row(k), stop=bool(c["stop"][k]), reset=reset)
            ctx.gait_update_batch(N, table[entry], float(c["time"][k]), ct, d["st0"], d["out0"].row(k), d["fe0"].row(k), stop=bool(c["stop"][k]), reset=reset)
            st, st0 = d["st"].download(), d["st0"].download()
            assert bits_equal(st[:48], st0[:48]), (entry, name, k, first_bad(st[:48], st0[:48]))
            assert np.all(st[48] == entry)
        out, out0, fe, fe0 = d["out"].download(), d["out0"].download(), d["fe"].download(), d["fe0"].download()
        assert bits_equal(out, out0), (entry, name, "gait_out [tick, row, robot]", first_bad(out, out0))
        assert bits_equal(fe, fe0), (entry, name, "fe_in", first_bad(fe, fe0))
        assert np.isfinite(out).all() and np.all(fe[:, 46:50] == table[entry][4])
    finally:
        free(d)


# ----------------------------------------------------------------------------- 2, 3
def ticks_of(n, ticks):
    """A tick count per robot that never restarts: the clock under test restarts it."""
    return (np.arange(ticks)[:, None] + 11 * np.arange(n)[None, :]).astype(i32)


def run_schedule(ctx, pkg, table, S, level, sel=None):
    """The schedule through the C ABI: per tick the mask word 0x40 for the robots with a reset (a word outside the bits for the others), the clock from
    stage_clock, the binding (bits 0xff, `level`), the gait call; the scalar reset only at tick 0.  Every array starts at poison.
    -> dict(state [T][52][n], out, fe, sw, flags, origin, local, sel_after, contact_after)."""
    q = pkg.qrgpu
    n = S["level"].shape[1]
    mask = np.where(S["level"] != 0, 0x40, 0x01000000).astype(i32)
    sel = S["sel"] if sel is None else sel
    contact = np.ascontiguousarray(S["contact"].transpose(0, 2, 1))
    d = dict(sel=ctx.alloc((T, n)).upload(sel), mask=ctx.alloc((T, n), i32).upload(mask), ticks=ctx.alloc((T, n), i32).upload(ticks_of(n, T)),
             c=ctx.alloc((T, 4, n)).upload(contact), st=ctx.alloc((52, n)).upload(np.full((52, n), POISON, f32)),
             out=ctx.alloc((T, 24, n)).upload(np.full((T, 24, n), POISON, f32)), fe=ctx.alloc((T, 64, n)).upload(np.full((T, 64, n), POISON, f32)),
             sw=ctx.alloc((T, 24, n)).upload(np.full((T, 24, n), POISON, f32)), flags=ctx.alloc((T, n), i32).upload(np.full((T, n), IPOISON, i32)),
             origin=ctx.alloc((n,), i32).upload(np.full(n, IPOISON, i32)), local=ctx.alloc((T, n), i32).upload(np.full((T, n), IPOISON, i32)))
    got = dict(state=np.empty((T, 52, n), f32), origin=np.empty((T, n), i32))
    try:
        for k in range(T):
            ctx.stage_clock(n, d["mask"].row(k), 0xff, d["ticks"].row(k), d["origin"], d["local"].row(k))
            ctx.set_stage_reset(mask=d["mask"].row(k), bits=0xff, level=level, ticks=d["local"].row(k), tick_dt=R.DT)
            ctx.gait_select_update_batch(n, table, d["sel"].row(k), 123.0, d["c"].row(k), d["st"], d["out"].row(k), d["fe"].row(k), d["sw"].row(k),
                                         d["flags"].row(k), stop=bool(S["stop"][k]), reset=q.GAIT_RESET_CONSTRUCT if k == 0 else 0)
            got["state"][k] = d["st"].download(); got["origin"][k] = d["origin"].download()
        for key in ("out", "fe", "sw", "flags", "local"):
            got[key] = d[key].download()
        got["sel_after"], got["contact_after"] = d["sel"].download(), d["c"].download()
        assert bits_equal(got["sel_after"], sel) and bits_equal(got["contact_after"], contact)           # inputs are not written
        return got
    finally:
        ctx.clear_stage_reset()
        free(d)


@pytest.fixture(scope="module")
def mixed(gpu_ctx, pkg):
    """The two runs of test 2 and their restatements, computed once: schedule 0 under a CONSTRUCT binding, schedule 2 (robot_stop from tick 300) under
    a LIVE one."""
    table = pkg.workload.gait_table()
    runs = {}
    for name, run_id, level in (("construct", 0, R.CONSTRUCT), ("live", 2, R.LIVE)):
        S = R.schedule(table, run_id, level=level)
        runs[name] = dict(S=S, got=run_schedule(gpu_ctx, pkg, table, S, level), ref=R.reference(table, S))
    return runs


@pytest.mark.parametrize("name", ["construct", "live"])
def test_mixed_schedule_against_the_restatement(mixed, name):
    S, got, ref = mixed[name]["S"], mixed[name]["got"], mixed[name]["ref"]
    for key, a, b in (("gait_state 0-48", got["state"][:, :49], ref["state"]), ("gait_out", got["out"], ref["out"]), ("fe_in 42-61", got["fe"][:, 42:62], ref["fe"]),
                      ("swing_in 8-11", got["sw"][:, 8:12], ref["swing"])):
        assert bits_equal(a, b), (name, key, "[tick, row, robot]", first_bad(a, b))
    assert np.array_equal(got["flags"], ref["flags"]) and not got["flags"].any()
    assert np.array_equal(got["local"], S["local"])
    # the schedule is not vacuous: every entry in force somewhere, a selection array that differs from the index in force wherever there is no reset
    assert set(np.unique(ref["state"][:, 48])) == set(range(5))
    assert np.all((S["sel"] != ref["state"][:, 48]) == (S["level"] == 0))
    assert (ref["out"][:, 12:16] == 2).any() and (ref["state"][:, 20:24] == 0).any() and bool(S["stop"].any()) == (name == "live")


@pytest.mark.parametrize("name", ["construct", "live"])
def test_what_is_not_owned_is_not_written(mixed, name):
    got = mixed[name]["got"]
    assert np.all(got["state"][:, 49:52] == POISON)
    assert np.all(got["fe"][:, :42] == POISON) and np.all(got["fe"][:, 62:] == POISON)
    assert np.all(got["sw"][:, :8] == POISON) and np.all(got["sw"][:, 12:] == POISON)
    # d_gait_sel and d_contact: compared with what was uploaded inside run_schedule, after the last tick


# ----------------------------------------------------------------------------- 4
def test_bad_selections_run_entry_zero_and_raise_the_flag(gpu_ctx, pkg, mixed):
    """NaN, 2.5, -1, n_gaits and 1e9 in single lanes at the robots' reset ticks: entry 0 there, the flag in exactly those lanes at exactly those ticks,
    every other lane bit-identical to the run without them."""
    table = pkg.workload.gait_table()
    S, clean = mixed["live"]["S"], mixed["live"]["got"]
    bad = {3: np.nan, 17: 2.5, 40: -1.0, 63: float(len(table)), 64: 1e9}
    sel = S["sel"].copy()
    for r, v in bad.items():
        sel[:, r] = np.where(S["level"][:, r] != 0, f32(v), sel[:, r])
    got = run_schedule(gpu_ctx, pkg, table, S, R.LIVE, sel=sel)
    want_flags = np.zeros((T, N), i32)
    for r in bad:
        want_flags[:, r] = np.where(S["level"][:, r] != 0, pkg.qrgpu.GAIT_BAD_SEL, 0)
        assert np.all(got["state"][:, 48, r] == 0)
    assert np.array_equal(got["flags"], want_flags)
    others = [r for r in range(N) if r not in bad]
    for key in ("state", "out", "fe", "sw"):
        assert bits_equal(got[key][:, :, others], clean[key][:, :, others]), key
    # the lanes themselves: the restatement on the same words
    ref = R.reference(table, dict(S, sel=sel), robots=list(bad))
    rb = list(bad)
    assert bits_equal(got["state"][:, :49, rb], ref["state"][:, :, rb]) and bits_equal(got["out"][:, :, rb], ref["out"][:, :, rb])
    assert np.array_equal(ref["flags"][:, rb], want_flags[:, rb])


# ----------------------------------------------------------------------------- 5
def test_every_bad_argument(gpu_ctx, pkg):
    ctx, q = gpu_ctx, pkg.qrgpu
    table = pkg.workload.gait_table()
    n = N
    d = dict(sel=ctx.alloc((n,)).zero(), c=ctx.alloc((4, n)).zero(), st=ctx.alloc((52, n)).upload(np.full((52, n), POISON, f32)),
             out=ctx.alloc((24, n)).upload(np.full((24, n), POISON, f32)), fe=ctx.alloc((64, n)).upload(np.full((64, n), POISON, f32)),
             sw=ctx.alloc((24, n)).upload(np.full((24, n), POISON, f32)), flags=ctx.alloc((n,), i32).upload(np.full(n, IPOISON, i32)),
             mask=ctx.alloc((n,), i32).zero(), ticks=ctx.alloc((n,), i32).zero(), origin=ctx.alloc((n,), i32).upload(np.full(n, IPOISON, i32)),
             local=ctx.alloc((n,), i32).upload(np.full(n, IPOISON, i32)))

    def gait(n_=n, table_=table, sel="sel", contact="c", st="st", reset=q.GAIT_RESET_CONSTRUCT):
        g = lambda k: None if k is None else d[k]
        ctx.gait_select_update_batch(n_, table_, g(sel), 0.0, g(contact), g(st), d["out"], d["fe"], d["sw"], d["flags"], reset=reset)

    def row(e, **kw):
        t = table.copy(); t[e] = pkg.workload.gait_cfg(**kw); return t
    duty0 = table.copy(); duty0[3, 6] = 0.0                              # one leg of one entry: a USERDEFINED_SWING leg
    stance0 = table.copy(); stance0[1, 1] = 0.0
    nine = np.concatenate([table, table[:4]])
    cases = [("n", dict(n_=0)), ("n", dict(n_=4097)), ("n_gaits", dict(table_=[])), ("n_gaits", dict(table_=nine)), ("d_gait_sel", dict(sel=None)),
             ("d_contact", dict(contact=None)), ("d_gait_state", dict(st=None)), ("reset", dict(reset=3)), ("reset", dict(reset=-1)),
             ("duty_factor", dict(table_=duty0)), ("duty_factor", dict(table_=row(4, duty_factor=0.001))), ("duty_factor", dict(table_=row(0, duty_factor=np.nan))),
             ("stance_duration", dict(table_=stance0)), ("stance_duration", dict(table_=row(2, stance_duration=-0.5)))]
    clock_cases = [("n", dict(n_=0)), ("n", dict(n_=4097)), ("d_mask", dict(mask=None)), ("bits", dict(bits=0)), ("d_ticks", dict(ticks=None)),
                   ("d_origin", dict(origin=None)), ("d_local", dict(local=None))]

    def clock(n_=n, mask="mask", bits=0xff, ticks="ticks", origin="origin", local="local"):
        g = lambda k: None if k is None else d[k]
        ctx.stage_clock(n_, g(mask), bits, g(ticks), g(origin), g(local))
    try:
        lib = pkg.load_library()
        # a NULL table: the Python mirror always passes an array, so this one case goes to the library as it is
        rc = lib.qrgpu_gait_select_update_batch(ctx._h, n, None, 5, q._dp(d["sel"]), 0.0, 0, 1, q._dp(d["c"]), q._dp(d["st"]), None, None, None, None)
        assert rc == 2, rc                                              # QRGPU_ERR_BAD_ARG
        assert "table" in ctx.last_error()
        for what, kw in cases:
            with pytest.raises(pkg.QrgpuError, match="BAD_ARG") as e:
                gait(**kw)
            assert "qrgpu_gait_select_update_batch" in str(e.value) and what in str(e.value), (what, str(e.value))
            assert ctx.last_error()
        for what, kw in clock_cases:
            with pytest.raises(pkg.QrgpuError, match="BAD_ARG") as e:
                clock(**kw)
            assert "qrgpu_stage_clock_batch" in str(e.value) and what in str(e.value), (what, str(e.value))
        ctx.sync()
        for k in ("st", "out", "fe", "sw"):
            assert np.all(d[k].download() == POISON), k
        for k in ("flags", "origin", "local"):
            assert np.all(d[k].download() == IPOISON), k
        # and the same arrays with good arguments are written: the poison check above is not vacuous
        d["mask"].upload(np.full(n, 0x40, i32))                          # (every robot masked: the first call on this origin)
        gait(); clock()
        ctx.sync()
        assert np.all(d["st"].download()[:49] != POISON) and np.all(d["flags"].download() == 0) and np.all(d["local"].download() == 0)
    finally:
        free(d)


# ----------------------------------------------------------------------------- 6
def test_clock_against_numpy(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(0xC10C)
    calls, bits = 50, 0x000100ff
    inside = np.array([0x1, 0x40, 0x80, 0x10000, 0x10040], np.uint32)
    outside = np.array([0x0, 0x100, 0x01000000, 0x20000, 0x7ffe0f00], np.uint32)
    for respawn_at_zero in (False, True):
        # ticks count up per robot and jump back to 0 as after a respawn; there the mask has a bit inside `bits` (always when respawn_at_zero, where
        # no other call is masked: the local clock is then the tick count itself)
        ticks = np.zeros((calls, N), i32); mask = np.zeros((calls, N), np.uint32)
        run = rng.integers(0, 30, N)
        for k in range(calls):
            jump = (rng.uniform(0, 1, N) < 0.06) | (k == 0)
            run = np.where(jump, 0, run + 1)
            ticks[k] = run
            hit = rng.uniform(0, 1, N) < 0.15
            word = np.where(hit, rng.choice(inside, N), rng.choice(outside, N)) | rng.choice(outside, N)
            if respawn_at_zero:
                word = np.where(jump, rng.choice(inside, N), rng.choice(outside, N))
            elif k == 0:
                word = word | 0x40                                       # the first call on a new origin: every robot masked
            mask[k] = word
        d = dict(mask=ctx.alloc((calls, N), i32).upload(mask.view(i32)), ticks=ctx.alloc((calls, N), i32).upload(ticks),
                 origin=ctx.alloc((calls + 1, N), i32).upload(np.full((calls + 1, N), IPOISON, i32)), local=ctx.alloc((calls, N), i32).upload(np.full((calls, N), IPOISON, i32)),
                 work=ctx.alloc((N,), i32).upload(np.full(N, IPOISON, i32)))
        try:
            origins = np.empty((calls, N), i32)
            for k in range(calls):
                ctx.stage_clock(N, d["mask"].row(k), bits, d["ticks"].row(k), d["work"], d["local"].row(k))
                origins[k] = d["work"].download()
            local = d["local"].download()
            origin = np.full(N, IPOISON, i32)
            for k in range(calls):
                origin, want = R.stage_clock(mask[k], bits, ticks[k], origin)
                assert np.array_equal(origins[k], origin) and np.array_equal(local[k], want), (respawn_at_zero, k)
            if respawn_at_zero:
                assert np.array_equal(local, ticks)
            else:
                assert (local != ticks).any() and (local == 0).any()
        finally:
            free(d)


# ----------------------------------------------------------------------------- 7
def test_with_the_state_machine(gpu_ctx, pkg):
    """The set-up of tests/test_gpu_fsm_loop.py -- 16 robots, 150 ticks, time_step 0.1, transition_ticks 8, X at ticks 36 and 52 of the episode, robot 3
    respawned at tick 70 -- with stage_clock, the binding (LIVE; the scalar CONSTRUCT at the first tick) and the gait-select call on row 44 of fsm_state
    after fsm_update; contacts: rows 13-16 of the plant's est_in.  Fed the downloaded inputs, fsm_ref and gait_select_ref reproduce row 48, the clock
    and the gait's state and output."""
    ctx, q = gpu_ctx, pkg.qrgpu
    n, ticks_, forced, forced_at = 16, 150, 3, 70
    script = np.array([[36, F.BTN_X, 0.0, 0.0, 0.0], [52, F.BTN_X, 0.0, 0.0, 1.0]], f32).T.copy()
    D = dict(F.A1, time_step=0.1, transition_ticks=8)
    table = pkg.workload.gait_table()
    ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
    ctx.plant_body_setup(0, pkg.plant_body_desc("a1"))
    grid, field = pkg.terrain.make("flat", None)
    tdesc = pkg.terrain_desc(n_fields=1, **grid.desc())
    fdesc = pkg.fsm_desc(**D)
    sit = np.asarray(D["sit_down_angles"], f32)
    edesc = pkg.episode_desc(status_mask=0, tilt_max=4.0, min_clearance=0.0, spawn_height=0.14, q_spawn=list(sit), seed=3, q_jitter=0.02)
    params = pkg.plant_params(dt=0.002, substeps=2)
    cx, cy = grid.x0 + 0.5 * (grid.nx - 1) * grid.cell, grid.y0 + 0.5 * (grid.ny - 1) * grid.cell
    spawn = np.zeros((4, 1), f32); spawn[0] = cx; spawn[1] = cy
    bits = q.EP_REASONS | q.FSM_ENTERED
    d = dict(fb=ctx.alloc((37, n)).zero(), cmd=ctx.alloc((60, n)).zero(), est_in=ctx.alloc((54, n)).zero(), height=ctx.alloc((1, grid.ny, grid.nx)).upload(pkg.terrain.stack([field])),
             table=ctx.alloc((4, 1)).upload(spawn), ep_state=ctx.alloc((q.EPISODE_STATE_ROWS, n), i32).zero(), ep_stats=ctx.alloc((q.EPISODE_STATS_ROWS, n)).zero(),
             done=ctx.alloc((n,), i32), force=ctx.alloc((n,), i32).zero(), prev=ctx.alloc((3, n)).zero(), status=ctx.alloc((n,), i32),
             state=ctx.alloc((q.FSM_STATE_ROWS, n)).upload(np.full((q.FSM_STATE_ROWS, n), F.POISON, f32)), joy=ctx.alloc((q.JOY_ROWS, n)), plan=ctx.alloc((n,), i32),
             mask=ctx.alloc((n,), i32), out=ctx.alloc((q.FSM_OUT_ROWS, n)), script=ctx.alloc(script.shape).upload(script),
             origin=ctx.alloc((n,), i32).zero(), local=ctx.alloc((n,), i32), gst=ctx.alloc((52, n)).upload(np.full((52, n), np.nan, f32)), gout=ctx.alloc((24, n)),
             gflags=ctx.alloc((n,), i32))
    fsm = [None] * n
    gait = [R.Robot(table) for _ in range(n)]
    origin = np.zeros(n, i32)
    row48 = np.zeros((ticks_, n), f32); entered_at = [[] for _ in range(n)]
    try:
        for t in range(ticks_):
            force = np.zeros(n, i32); force[forced] = int(t == forced_at)
            d["force"].upload(force)
            ctx.episode_step_batch(n, edesc, d["fb"], d["table"], 1, d["ep_state"], d["ep_stats"], d["done"], reset_all=(t == 0), params=params, terrain=tdesc,
                                   height=d["height"], force_reset=d["force"], prev_ori=d["prev"], motor_cmd=d["cmd"])
            ctx.plant_step_body_batch(n, params, tdesc, d["height"], d["fb"], d["cmd"], est_in=d["est_in"], status=d["status"])
            loco = d["cmd"].download()
            ctx.fsm_update(n, fdesc, d["state"], d["joy"], d["plan"], stage_mask=d["mask"], script=d["script"], n_script=script.shape[1], ticks=d["ep_state"],
                           done=d["done"], bits=q.EP_REASONS)
            ctx.stage_clock(n, d["mask"], bits, d["ep_state"], d["origin"], d["local"])
            ctx.set_stage_reset(mask=d["mask"], bits=bits, level=q.STAGE_RESET_LIVE, ticks=d["local"], tick_dt=D["time_step"])
            sel = d["state"].download()[44]
            ctx.gait_select_update_batch(n, table, d["state"].row(44), 0.0, d["est_in"].row(13), d["gst"], d["gout"], flags=d["gflags"],
                                         reset=q.GAIT_RESET_CONSTRUCT if t == 0 else 0)
            ctx.fsm_command(n, fdesc, d["plan"], d["est_in"], d["cmd"], d["state"], d["cmd"], fsm_out=d["out"])
            est, done, eticks, mask = d["est_in"].download(), d["done"].download(), d["ep_state"].download()[0], d["mask"].download()
            local, gst, gout = d["local"].download(), d["gst"].download(), d["gout"].download()
            assert not d["gflags"].download().any()
            origin, want_local = R.stage_clock(mask, bits, eticks, origin)
            assert np.array_equal(local, want_local), t
            for r in range(n):
                rst = (done[r] & q.EP_REASONS) != 0
                if rst:
                    fsm[r] = F.Robot(D)
                want_sel = 0.0 if rst else fsm[r].state_rows()[44]                  # row 44 as fsm_update leaves it: the gait of the last OnEnter
                o = fsm[r].tick(F.script_message(script, eticks[r]), False, est[13:17, r], est[17:29, r], loco[:, r])
                want_mask = (done[r] & q.EP_REASONS) | (F.ENTERED if o["entered"] else 0)
                assert mask[r] == want_mask and sel[r] == want_sel, (t, r)
                level = R.CONSTRUCT if t == 0 else (R.LIVE if want_mask & bits else 0)
                g = gait[r].tick(R.clock_time(want_local[r], D["time_step"]), est[13:17, r], want_sel, level)
                assert bits_equal(gst[:49, r], g["state"]) and bits_equal(gout[:, r], g["out"]), (t, r, first_bad(gst[:49, r], g["state"]))
                if o["entered"]:
                    entered_at[r].append((t, int(want_sel)))
                    assert local[r] == 0
                if rst:
                    assert local[r] == 0 and gst[48, r] == 0
                if gst[48, r] == q.FSM_GAIT_STAND:
                    assert np.all(gout[8:12, r] == G.STANCE)
            row48[t] = gst[48]
        # row 48: 0 before a robot's first OnEnter, 4 (stand) from the tick the stage mask carries it -- the mask of tick t carries the OnEnter that ran at
        # the end of tick t - 1; OnEnter runs again, still on stand, when the stand loop ends -- and 2 (advanced_trot) from the first OnEnter after the
        # second press; 0 again for the respawned robot, which then goes the same way
        def pattern(r, events, lo, hi):
            gaits = [g for _, g in events]
            assert gaits and gaits[0] == q.FSM_GAIT_STAND and gaits == sorted(gaits, reverse=True) and set(gaits) <= {q.FSM_GAIT_STAND, q.FSM_GAIT_ADVANCED_TROT}, (r, events)
            first = events[0][0]
            second = min([t for t, g in events if g == q.FSM_GAIT_ADVANCED_TROT] + [hi])
            assert np.all(row48[lo:first, r] == 0) and np.all(row48[first:second, r] == q.FSM_GAIT_STAND), (r, events)
            assert np.all(row48[second:hi, r] == q.FSM_GAIT_ADVANCED_TROT), (r, events)
            return second < hi
        for r in range(n):
            if r != forced:
                assert pattern(r, entered_at[r], 0, ticks_), (r, entered_at[r])
        assert pattern(forced, [e for e in entered_at[forced] if e[0] < forced_at], 0, forced_at)
        later = [e for e in entered_at[forced] if e[0] > forced_at]
        assert row48[forced_at, forced] == 0 and row48[forced_at - 1, forced] == q.FSM_GAIT_ADVANCED_TROT
        if later:
            pattern(forced, later, forced_at, ticks_)
        else:
            assert np.all(row48[forced_at:, forced] == 0)
    finally:
        ctx.clear_stage_reset()
        free(d)
