"""GPU parity of the walk pose planner (qrgpu_pose_plan_batch) against the CPU restatement tests/pose_plan_ref.py on the cells of
tests/golden/pose_plan_golden.npz.  Reference: quadruped/src/planner/qr_pose_planner.cpp:72-456, include/quadruped/planner/qr_pose_planner.h:311-320.
Bars: everything up to the first so3ToQuat uses no math-library call, so the first SQP iteration's step p, its working set A[] and its
slot-ordered u are bit-equal to the float32 restatement, as are the flags, N, the kept vertices, the segment source and ResetBasePose's rows.
The finished rows (poseDest, rIB, quat, Lambda) satisfy tests/test_gpu_stance.py's rule: |gpu - ref64| <= 8 max(|ref32 - ref64| over the cell,
4 ulp of the row's magnitude).  The committed cells hold no case whose float32 and float64 restatements differ in a working-set size or a
flag (tests/test_pose_plan_ref.py checks the 1 % cap), so every case is compared in full.
One wavefront (one 64-thread block) per robot: the batch sizes are those at which the XCD chunking of the robot index changes shape."""
import functools

import numpy as np
import pytest

import pose_plan_ref as P
import stance_ref as SR

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
PAD = 64
SENT = f32(-777.0)
FLAG_SENT = -12345
ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def golden():
    g = P.load_golden()
    chained = np.array([bool(g["cell_chained"][list(g["cells"]).index(c)]) for c in g["cell_of"]])
    g["single"] = np.nonzero(~chained)[0]
    # per cell and row: the float32 restatement's own distance from the float64 one, floored at 4 ulp of the row's magnitude in the cell
    fin32 = np.concatenate([g["cmd32"][:, 6:], g["after32"][:, 16:20], g["after32"][:, :12]], axis=1).astype(f64)        # dest[6], quat[4], Lambda[12]
    fin64 = np.concatenate([g["cmd64"][:, 6:], g["after64"][:, 16:20], g["after64"][:, :12]], axis=1)
    scale = np.zeros_like(fin64)
    for k in range(len(g["cells"])):
        a, b = g["cell_start"][k], g["cell_start"][k + 1]
        ok = ~np.isnan(fin64[a:b, 0])
        if ok.any():
            own = np.abs(fin32[a:b][ok] - fin64[a:b][ok]).max(axis=0)
            scale[a:b] = np.maximum(own, 4 * ULP * np.abs(fin64[a:b][ok]).max(axis=0))
    g["fin64"], g["scale"] = fin64, scale
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


class Run:
    """One call's device arrays for the robots `idx` (golden case numbers); outputs carry sentinels in every row and PAD behind."""
    def __init__(self, ctx, cases, states):
        n = self.n = len(cases)
        self.ctx = ctx
        inp = P.pack_inputs(cases)
        up = lambda a: ctx.alloc(a.T.shape).upload(np.ascontiguousarray(a.T))
        self.ins = {k: up(v) for k, v in inp.items()}
        self.state = ctx.alloc((P.STATE_ROWS * n + PAD,)).upload(np.concatenate([np.ascontiguousarray(np.asarray(states, f32).T).reshape(-1), np.full(PAD, SENT)]))
        self.cmd = ctx.alloc((28 * n + PAD,)).upload(np.full(28 * n + PAD, SENT, f32))
        self.out = ctx.alloc((P.OUT_ROWS * n + PAD,)).upload(np.full(P.OUT_ROWS * n + PAD, SENT, f32))
        self.flags = ctx.alloc((n + PAD,), np.int32).upload(np.full(n + PAD, FLAG_SENT, np.int32))

    def plan(self, desc, **kw):
        i = self.ins
        ew = kw.pop("event_words", None)
        d_ew = self.ctx.alloc((self.n,), np.int32).upload(np.asarray(ew, np.int32)) if ew is not None else None
        self.ctx.pose_plan_batch(self.n, desc, i["est_in"], i["est_out"], i["ground"], i["rpy"], i["walk"], self.state, self.cmd, self.flags,
                                 event_words=d_ew, pose_out=kw.pop("pose_out", self.out), **kw)
        self.ctx.sync()
        if d_ew is not None:
            d_ew.free()

    def get(self):
        n = self.n
        res = {}
        for key, arr, rows in (("state", self.state, P.STATE_ROWS), ("cmd", self.cmd, 28), ("out", self.out, P.OUT_ROWS)):
            flat = arr.download()
            assert np.all(flat[rows * n:] == SENT), key
            res[key] = flat[:rows * n].reshape(rows, n).T.copy()
        fl = self.flags.download()
        assert np.all(fl[n:] == FLAG_SENT)
        res["flags"] = fl[:n].copy()
        return res

    def free(self):
        for v in (*self.ins.values(), self.state, self.cmd, self.out, self.flags):
            v.free()


def bits(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


def check_update(g, idx, res, states_before, first_iteration_exact=True, ratios=None):
    """Robot r of the call ran Update on golden case idx[r] from states_before[r]."""
    for r, i in enumerate(idx):
        tag = (r, int(i), g["cell_of"][i])
        assert res["flags"][r] == g["flags32"][i], (tag, hex(res["flags"][r]), hex(g["flags32"][i]))
        cmd, st, out = res["cmd"][r], res["state"][r], res["out"][r]
        assert np.all(cmd[:7] == SENT) and np.all(cmd[19:] == SENT), tag
        if g["flags32"][i] & P.FATAL:
            assert np.all(cmd == SENT) and bits(st, states_before[r]), tag
            continue
        m = 3 * int(g["N"][i])
        assert out[152] == g["N"][i] and out[153] == g["mask"][i] and st[12] == m, tag
        assert bits(cmd[7:13], g["cmd32"][i][:6]), tag                                   # the segment's source: copies
        assert bits(st[13:16], cmd[13:16]) and bits(st[20:26], cmd[13:19]) and bits(st[m:12], states_before[r][m:12]), tag
        assert bits(out[140:140 + m], st[:m]) and np.all(out[140 + m:152] == 0), tag
        iq = out[6:140:7]
        if first_iteration_exact:
            assert bits(out[0:6], g["p32"][i][0]) and iq[0] == g["iq32"][i][0], (tag, out[0:6], g["p32"][i][0])
            assert bits(out[154:166], g["u0_32"][i]) and np.array_equal(out[166:178], g["A0_32"][i].astype(f32)), tag
        assert np.array_equal(iq, g["iq32"][i].astype(f32)), (tag, iq, g["iq32"][i])
        got = np.concatenate([cmd[13:19], st[16:20], st[:12]]).astype(f64)
        want, scale = g["fin64"][i].copy(), g["scale"][i]
        got[10 + m:] = want[10 + m:] = 0                                                 # Lambda beyond 3N is not this plan's
        err = np.abs(got - want)
        ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))
        if ratios is not None:
            ratios.append(ratio.max())
        assert np.all(err <= 8 * scale), (tag, int(np.argmax(ratio)), ratio.max(), err[np.argmax(ratio)], scale[np.argmax(ratio)])


# ---- 1. the golden cells at every batch-size edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 7, 8, 9, 64, 65, 130])
def test_golden_cells(gpu_ctx, pkg, n):
    """n robots cycle through the unchained cases (8 and 9: the XCD chunk grows from one robot to two)."""
    g = golden()
    idx = [g["single"][(r * 5 + n) % len(g["single"])] for r in range(n)] if n < len(g["single"]) else [g["single"][r % len(g["single"])] for r in range(n)]
    before = g["before32"][idx]
    run = Run(gpu_ctx, [g["cases"][i] for i in idx], before)
    run.plan(pkg.pose_plan_desc(), event=1)
    res = run.get()
    run.free()
    ratios = []
    check_update(g, idx, res, before, ratios=ratios)
    print("n = %d: largest |gpu - ref64| / max(|ref32 - ref64|, 4 ulp) over the finished rows: %.3f" % (n, max(ratios) if ratios else 0.0))


# ---- 2. mixed events, untouched rows and robots, event 3 ---------------------------------------------------------------------------------------------
def test_mixed_events_and_switch_rule(gpu_ctx, pkg):
    g = golden()
    n = 65
    idx = [g["single"][r % len(g["single"])] for r in range(n)]
    cases = [g["cases"][i] for i in idx]
    before = g["before32"][idx]
    words = np.array([r % 3 for r in range(n)], np.int32)
    run = Run(gpu_ctx, cases, before)
    run.plan(pkg.pose_plan_desc(), event=1, event_words=words)                          # the words win over `event`
    res = run.get()
    run.free()
    for r in np.nonzero(words == 0)[0]:
        assert np.all(res["cmd"][r] == SENT) and np.all(res["out"][r] == SENT) and res["flags"][r] == FLAG_SENT and bits(res["state"][r], before[r])
    upd = np.nonzero(words == 1)[0]
    check_update(g, [idx[r] for r in upd], {k: v[upd] for k, v in res.items()}, before[upd])
    for r in np.nonzero(words == 2)[0]:                                                  # ResetBasePose: no math-library call at all
        st = P.new_state(f32, cases[r]["base_pos"])
        fl, cmd = P.reset_base_pose(f32, P.Desc(), cases[r], st)
        assert res["flags"][r] == fl
        if fl == 0:
            assert bits(res["cmd"][r][7:25], cmd) and np.all(res["cmd"][r][:7] == SENT) and np.all(res["cmd"][r][25:] == SENT)
            assert bits(res["state"][r][20:26], cmd[6:12]) and bits(res["state"][r][:20], before[r][:20]) and np.all(res["out"][r] == SENT)
        else:
            assert np.all(res["cmd"][r] == SENT) and bits(res["state"][r], before[r])
    # event 3 = explicit words from the switchToSwing rule; legs vary: swinging from STANCE, still swinging, in stance
    cs = []
    for r, c in enumerate(cases):
        c = dict(c)
        if r % 4 == 1:
            c["cur_leg_state"] = list(c["leg_state"])                                      # the swing began earlier: no switch
        if r % 4 == 2:
            c["leg_state"] = [P.STANCE] * 4
        cs.append(c)
    sw = np.array([P.switch_to_swing(c) for c in cs])
    assert 0 < sw.sum() < n
    a, b = Run(gpu_ctx, cs, before), Run(gpu_ctx, cs, before)
    a.plan(pkg.pose_plan_desc(), event=3)
    b.plan(pkg.pose_plan_desc(), event=0, event_words=sw.astype(np.int32))
    ra, rb = a.get(), b.get()
    a.free(); b.free()
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert np.all((ra["flags"] != FLAG_SENT) == sw)


# ---- 3. chains: Lambda carried on the device ------------------------------------------------------------------------------------------------------
def test_chains(gpu_ctx, pkg):
    g = golden()
    chains = [k for k, ch in enumerate(g["cell_chained"]) if ch]
    starts = [int(g["cell_start"][k]) for k in chains]
    run = Run(gpu_ctx, [g["cases"][s] for s in starts], g["before32"][starts])
    desc = pkg.pose_plan_desc()
    prev = g["before32"][starts].copy()
    for step in range(8):
        idx = [s + step for s in starts]
        inp = P.pack_inputs([g["cases"][i] for i in idx])
        for k, v in inp.items():
            run.ins[k].upload(np.ascontiguousarray(v.T))
        run.cmd.upload(np.full(28 * run.n + PAD, SENT, f32))
        run.plan(desc, event=1)
        res = run.get()
        check_update(g, idx, res, prev, first_iteration_exact=(step == 0))
        prev = res["state"]
    run.free()
    grown = [bool(f & P.LAMBDA_GROWN) for f in g["flags32"][starts[-1]:starts[-1] + 8]]
    assert grown == [False, True] * 4                                                    # the last chain alternates N = 3 and N = 4


# ---- 4. flags the inputs alone do not reach: a carried Lambda that makes the QP matrix indefinite, a contradictory leg window ---------------------------
def test_not_pd_and_infeasible(gpu_ctx, pkg):
    g = golden()
    c = g["cases"][0]
    st = P.new_state(f32, c["base_pos"])
    st["lam"] = [f32(0.1)] * 3 + [f32(100.0)] * 3 + [f32(0.1)] * 6
    st["size"] = 9
    rows = P.state_rows(f32, st)
    run = Run(gpu_ctx, [c, c], [rows, g["before32"][0]])
    run.plan(pkg.pose_plan_desc(), event=1)
    res = run.get()
    run.free()
    assert res["flags"][0] == P.NOT_PD and np.all(res["cmd"][0] == SENT) and bits(res["state"][0], rows)
    assert res["flags"][1] == 0 and bits(res["out"][1][:6], g["p32"][0][0])
    bad = P.Desc(l_min=0.35, l_max=0.22)
    want = P.update(f32, bad, c, P.new_state(f32, c["base_pos"]))
    assert want["flags"] & P.INFEASIBLE
    run = Run(gpu_ctx, [c], [g["before32"][0]])
    run.plan(pkg.pose_plan_desc(l_min=0.35, l_max=0.22), event=1)
    res = run.get()
    run.free()
    assert res["flags"][0] == want["flags"] and bits(res["out"][0][:6], want["p"][0]) and res["out"][0][6] == want["iq"][0]
    assert bits(res["out"][0][154:154 + len(want["u0"])], want["u0"])
    assert np.isfinite(res["cmd"][0][7:19]).all() and np.abs(res["cmd"][0][13:19].astype(f64) - np.array(want["cmd"][6:], f64)).max() < 1e-4


# ---- 5. reset, event 0 -------------------------------------------------------------------------------------------------------------------------------------
def test_reset_and_event_zero(gpu_ctx, pkg):
    g = golden()
    idx = list(g["single"][:9])
    cases = [g["cases"][i] for i in idx]
    junk = np.full((len(idx), P.STATE_ROWS), 3.0, f32)
    desc = pkg.pose_plan_desc()
    run = Run(gpu_ctx, cases, junk)
    run.plan(desc, event=0)                                                              # nothing to do: nothing is launched, nothing changes
    res = run.get()
    assert np.all(res["cmd"] == SENT) and np.all(res["out"] == SENT) and np.all(res["flags"] == FLAG_SENT) and bits(res["state"], junk)
    run.plan(desc, event=0, reset=True)                                                  # the constructed state, no plan
    res = run.get()
    fresh = np.stack([P.state_rows(f32, P.new_state(f32, c["base_pos"])) for c in cases])
    assert bits(res["state"], fresh) and np.all(res["cmd"] == SENT) and np.all(res["flags"] == FLAG_SENT)
    run.state.upload(np.concatenate([np.ascontiguousarray(junk.T).reshape(-1), np.full(PAD, SENT)]))
    run.plan(desc, event=1, reset=True)                                                  # reset, then Update: as from a fresh planner
    res = run.get()
    run.free()
    check_update(g, idx, res, fresh)


# ---- 6. composition with the stance front-end, bad arguments --------------------------------------------------------------------------------------------------
def test_plan_then_stance_update_equals_the_host_path(gpu_ctx, pkg):
    """plan -> qrgpu_stance_update_batch (WALK) on the device gives bit for bit what the same plan copied through the host gives."""
    g = golden()
    n = 65
    idx = [g["single"][r % len(g["single"])] for r in range(n)]
    cases = [g["cases"][i] for i in idx]
    inp = SR.make_inputs(n, SR.WALK, 11)
    mine = P.pack_inputs(cases)
    inp["est_in"][:, 6:10] = mine["est_in"][:, 6:10]
    inp["est_out"][:, 12:24] = mine["est_out"][:, 12:24]; inp["est_out"][:, 36:39] = mine["est_out"][:, 36:39]
    inp["ground"][:, 6:9] = mine["ground"][:, 6:9]
    inp["rpy"][:] = mine["rpy"]
    inp["gait_out"][:, 8:20] = mine["walk"][:, 8:20]
    ctx = gpu_ctx
    up = lambda a: ctx.alloc(a.T.shape).upload(np.ascontiguousarray(a.T))
    d = {k: up(v) for k, v in inp.items()}
    cmd0 = np.ascontiguousarray(inp["cmd"].T)
    state = ctx.alloc((P.STATE_ROWS, n)).upload(np.ascontiguousarray(g["before32"][idx].T))
    flags = ctx.alloc((n,), np.int32)
    sdesc = pkg.stance_desc(SR.WALK)
    outs = []
    for path in ("device", "host"):
        d["cmd"].upload(cmd0)
        state.upload(np.ascontiguousarray(g["before32"][idx].T))
        st = ctx.alloc((n,)).upload(np.full(n, 0.3, f32))
        vmc, ratio, sout = ctx.alloc((37, n)), ctx.alloc((8, n)), ctx.alloc((33, n))
        ctx.pose_plan_batch(n, pkg.pose_plan_desc(), d["est_in"], d["est_out"], d["ground"], d["rpy"], d["gait_out"], state, d["cmd"], flags, event=1)
        if path == "host":
            ctx.sync()
            planned = d["cmd"].download()
            assert not np.array_equal(planned, cmd0)
            d["cmd"].upload(cmd0)                                                        # the plan's rows come back through the host
            h = cmd0.copy(); h[7:25] = planned[7:25]
            d["cmd"].upload(h)
        ctx.stance_update_batch(n, sdesc, d["est_in"], d["est_out"], d["ground"], d["rpy"], d["gait_out"], d["cmd"], st, vmc_in=vmc, ratio=ratio,
                                stance_out=sout)
        ctx.sync()
        outs.append([a.download() for a in (vmc, ratio, sout, st)])
        for a in (vmc, ratio, sout, st):
            a.free()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert np.isfinite(outs[0][2][12:18]).all()
    for v in (*d.values(), state, flags):
        v.free()


def test_bad_arguments(gpu_ctx, pkg):
    g = golden()
    run = Run(gpu_ctx, [g["cases"][0]] * 4, g["before32"][[0] * 4])
    i = run.ins
    desc = pkg.pose_plan_desc()
    args = dict(est_in=i["est_in"], est_out=i["est_out"], ground_out=i["ground"], rpy=i["rpy"], walk_out=i["walk"], pose_state=run.state,
                stance_cmd=run.cmd, pose_flags=run.flags)
    for bad in list(args) + ["n0", "nbig", "event"]:
        a = dict(args)
        kw = dict(event=1)
        n = 4
        if bad in a:
            a[bad] = None
        elif bad == "n0":
            n = 0
        elif bad == "nbig":
            n = 4097
        else:
            kw["event"] = 4
        with pytest.raises(pkg.QrgpuError):
            gpu_ctx.pose_plan_batch(n, desc, **a, **kw)
    gpu_ctx.sync()
    res = run.get()
    run.free()
    assert np.all(res["cmd"] == SENT) and np.all(res["flags"] == FLAG_SENT) and bits(res["state"], g["before32"][[0] * 4])
