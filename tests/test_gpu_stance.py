"""GPU parity of the stance front-end and motor commands of the force-balance modes (qrgpu_stance_update_batch / _command_batch /
_tick_batch) against the CPU restatement tests/stance_ref.py, and the chained force-balance tick queued without host copies.
Reference: qr_torque_stance_leg_controller.cpp:89-172, 174-477, 503-541; qr_locomotion_controller.cpp:128-147.
Bars: rows that involve no math-library call are bit-equal to the float32 restatement; every other row satisfies
|gpu - ref64| <= 8 max_batch |ref32 - ref64| of that row (a device sinf / atan2f / asinf / erf may carry a few ulp where numpy's carries at
most one), over the robots the float64 restatement does not place within 1e-4 of a branch threshold (stance_ref.excluded)."""
import functools

import numpy as np
import pytest

import gpu_helpers as G
import stance_ref as R
from gpu_helpers import tau_tol

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
N = 257                                   # four blocks and one robot more
PAD = 64                                  # sentinel floats behind row n of every output
SENT = f32(-777.0)
DESC_KW = dict(desired_speed=[0.3, -0.1, 0.0], desired_twisting_speed=0.2, pose_reset_time=0.5)
OUT_ROWS = dict(vmc=37, ratio=8, out=R.OUT_ROWS)


def ref_desc(case):
    mode, terrain, fiw, seed = R.CASES[case]
    return R.Desc(mode, terrain=terrain, force_in_world=fiw, **DESC_KW), seed


def lib_desc(pkg, rd):
    return pkg.stance_desc(rd.mode, terrain=rd.terrain, force_in_world=rd.force_in_world, kp=rd.kp, kd=rd.kd, max_ddq=rd.max_ddq, min_ddq=rd.min_ddq,
                           desired_height=rd.desired_height, desired_speed=rd.desired_speed, desired_twisting_speed=rd.desired_twisting_speed,
                           body_height=rd.body_height, pose_reset_time=rd.pose_reset_time, motor_kp=rd.motor_kp, motor_kd=rd.motor_kd)


@functools.lru_cache(maxsize=None)
def reference(case, stop=False, current_time=0.0):
    """The case's inputs and both restatements, computed once and shared (read-only)."""
    rd, seed = ref_desc(case)
    inp = R.make_inputs(N, rd.mode, seed)
    st0 = np.full((N, 1), 0.3, f32)
    st32, st64 = st0.copy(), st0.copy()
    r32 = R.run_batch(f32, rd, inp, st32, current_time=current_time, stop=stop, reset=False)
    r64 = R.run_batch(f64, rd, inp, st64, current_time=current_time, stop=stop, reset=False)
    for a in (*inp.values(), *r32, *r64, st0, st32):
        a.setflags(write=False)
    return rd, inp, st0, st32, r32, r64, R.excluded(rd, inp, stop)


class Arrays:
    """The device arrays of one qrgpu_stance_update_batch call on the first n robots of `inp`; outputs carry PAD sentinels behind row n."""
    def __init__(self, ctx, inp, n, st0):
        S = lambda a: np.ascontiguousarray(a[:n].T)
        self.ctx, self.n = ctx, n
        self.ins = {k: ctx.alloc(S(v).shape).upload(S(v)) for k, v in inp.items()}
        self.st = ctx.alloc((1 * n + PAD,)).upload(np.concatenate([S(st0).reshape(-1), np.full(PAD, SENT)]))
        self.outs = {k: ctx.alloc((r * n + PAD,)).upload(np.full(r * n + PAD, SENT, f32)) for k, r in OUT_ROWS.items()}

    def update(self, desc, skip=(), **kw):
        i, o = self.ins, {k: (None if k in skip else v) for k, v in self.outs.items()}
        self.ctx.stance_update_batch(self.n, desc, i["est_in"], i["est_out"], i["ground"], i["rpy"], i["gait_out"], i["cmd"], self.st,
                                     gait_state=i["gait_state"], vmc_in=o["vmc"], ratio=o["ratio"], stance_out=o["out"], **kw)

    def get(self, key):
        """-> ([n][rows] of the output, its sentinel tail)"""
        arr = self.st if key == "st" else self.outs[key]
        rows = 1 if key == "st" else OUT_ROWS[key]
        flat = arr.download()
        return flat[:rows * self.n].reshape(rows, self.n).T.copy(), flat[rows * self.n:]

    def free(self):
        for v in (*self.ins.values(), *self.outs.values(), self.st):
            v.free()


def same_bits(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


def check_parity(case, got, r32, r64, ex, rd):
    """got / r32 / r64: (vmc_in, ratio, out) [n][rows].  Exact rows bit-equal on every robot, the others within 8 x the float32 restatement's own
    distance from the float64 one, on the robots that are not excluded."""
    n = got[0].shape[0]
    exact_out, exact_vin = R.exact_rows(rd)
    keep = ~ex[:n]
    assert same_bits(got[1], r32[1][:n].astype(f32)), (case, "ratio")
    for name, g, a32, a64, exact in (("vmc_in", got[0], r32[0], r64[0], exact_vin), ("stance_out", got[2], r32[2], r64[2], exact_out)):
        a32, a64 = a32[:n], a64[:n]
        assert same_bits(g[:, exact], a32[:, exact]), (case, name, [k for k in exact if not same_bits(g[:, k], a32[:, k])])
        for k in sorted(set(range(g.shape[1])) - set(exact)):
            # the yardstick is the whole 257-robot batch's float32 error in this row (a smaller n compares against the same bound)
            own = np.abs(r32[0 if name == "vmc_in" else 2][:, k].astype(f64) - r64[0 if name == "vmc_in" else 2][:, k])[~ex].max()
            err = np.abs(g[:, k].astype(f64) - a64[:, k])[keep].max()
            ratio = err / own if own > 0 else (0.0 if err == 0 else np.inf)
            line = "%s %s row %d: |gpu - ref64| %.3e, |ref32 - ref64| %.3e, ratio %.2f" % (case, name, k, err, own, ratio)
            print(line)
            assert err <= 8 * own, line


# ---- 1. parity, every mode / terrain / frame --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_update_parity(gpu_ctx, pkg, case):
    rd, inp, st0, st32, r32, r64, ex = reference(case)
    a = Arrays(gpu_ctx, inp, N, st0)
    a.update(lib_desc(pkg, rd))
    gpu_ctx.sync()
    got = [a.get(k) for k in ("vmc", "ratio", "out")]
    st, st_tail = a.get("st")
    a.free()
    assert all(np.all(t == SENT) for _, t in got) and np.all(st_tail == SENT)
    assert same_bits(st, st32)
    assert np.isnan(inp["est_out"][:, 39]).any() and np.all(st[np.isnan(inp["est_out"][:, 39])] == f32(0.3))
    check_parity(case, [g for g, _ in got], r32, r64, ex, rd)
    assert ex.sum() <= R.EXCLUDE_CAP * N


# ---- 2. batch edges, NULL-able outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("case", ["walk_slope", "position_piles"])
def test_batch_edges_and_null_outputs(gpu_ctx, pkg, case, n):
    rd, inp, st0, st32, r32, r64, ex = reference(case)
    desc = lib_desc(pkg, rd)
    a = Arrays(gpu_ctx, inp, n, st0)
    a.update(desc)
    gpu_ctx.sync()
    full = {k: a.get(k) for k in ("vmc", "ratio", "out", "st")}
    for k, (g, tail) in full.items():
        assert np.all(tail == SENT), (k, n)
    check_parity(case, [full[k][0] for k in ("vmc", "ratio", "out")], r32, r64, ex, rd)
    assert same_bits(full["st"][0], st32[:n])
    a.free()
    for skip in (("vmc",), ("ratio",), ("out",), ("vmc", "ratio", "out")):     # every output may be NULL; the others do not change
        b = Arrays(gpu_ctx, inp, n, st0)
        b.update(desc, skip=skip)
        gpu_ctx.sync()
        for k in ("vmc", "ratio", "out"):
            g, tail = b.get(k)
            assert np.all(tail == SENT)
            assert np.all(g == SENT) if k in skip else same_bits(g, full[k][0]), (k, skip)
        assert same_bits(b.get("st")[0], full["st"][0])
        b.free()


# ---- 3. robot_stop in every mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["velocity_slope", "position_piles", "walk_slope", "trot_world_slope", "trot_control_slope"])
def test_stop(gpu_ctx, pkg, case):
    rd, inp, st0, st32, r32, r64, ex = reference(case, True, 2.25)
    a = Arrays(gpu_ctx, inp, N, st0)
    a.update(lib_desc(pkg, rd), stop=True, current_time=2.25)
    gpu_ctx.sync()
    got = [a.get(k)[0] for k in ("vmc", "ratio", "out")]
    a.free()
    assert np.all(got[0][:, 18:22] == 1) and np.all(got[2][:, 30] == 4) and np.all(got[2][:, 31] == 1)
    assert np.all(got[1][:, :4] == f32(0.01)) and np.all(got[1][:, 4:] == 10)
    check_parity(case + "/stop", got, r32, r64, ex, rd)
    if rd.mode == R.WALK:                                                      # the pose runs on wall time: (2.25 - 0.5) / 5 of the way from source to dest
        ph = f32(f32(2.25) - f32(0.5)) / f32(5.0)
        want = ph * inp["cmd"][:, 13:16] + f32(1.0 - f64(ph)) * inp["cmd"][:, 7:10]
        assert same_bits(got[2][:, 12:15], want)


# ---- 4 / 5. the height memory over ticks, reset ---------------------------------------------------------------------------------------------
def test_height_memory_and_reset(gpu_ctx, pkg):
    case = "trot_control_slope"                                                 # the branch that reads heightInControlFrame (:285)
    rd, inp, st0, *_ = reference(case)
    desc = lib_desc(pkg, rd)
    nan = np.isnan(inp["est_out"][:, 39])
    a = Arrays(gpu_ctx, inp, N, st0)
    a.update(desc, reset=True)
    gpu_ctx.sync()
    st, _ = a.get("st"); out, _ = a.get("out")
    assert np.all(st[nan] == f32(rd.body_height)) and same_bits(st[~nan, 0], inp["est_out"][~nan, 39])
    assert same_bits(out[:, 2], st[:, 0])
    eo = inp["est_out"].copy(); eo[:, 39] = np.nan                              # two ticks with no foot in stance anywhere: every robot keeps its height
    a.ins["est_out"].upload(np.ascontiguousarray(eo.T))
    for _ in range(2):
        a.update(desc)
        gpu_ctx.sync()
        st2, _ = a.get("st"); out2, _ = a.get("out")
        assert same_bits(st2, st) and same_bits(out2[:, 2], st[:, 0]) and np.isfinite(out2).all()
    a.update(desc, reset=True)                                                  # reset restores bodyHeight
    gpu_ctx.sync()
    st3, _ = a.get("st")
    assert np.all(st3 == f32(rd.body_height))
    a.free()


# ---- 6. bad arguments leave the outputs untouched -------------------------------------------------------------------------------------------
def test_bad_arguments(gpu_ctx, pkg):
    rd, inp, st0, *_ = reference("position_piles")
    n = 8
    a = Arrays(gpu_ctx, inp, n, st0)
    i, o = a.ins, a.outs
    ok = lib_desc(pkg, rd)
    d_tau = gpu_ctx.alloc((12, n)).upload(np.ones((12, n), f32)); d_f = gpu_ctx.alloc((12, n)).upload(np.full((12, n), SENT))
    d_mc = gpu_ctx.alloc((60, n)).upload(np.full((60, n), SENT))

    def upd(desc=ok, n_=n, **over):
        arg = dict(est_in=i["est_in"], est_out=i["est_out"], ground=i["ground"], rpy=i["rpy"], gait_out=i["gait_out"], cmd=i["cmd"], st=a.st,
                   gait_state=i["gait_state"])
        arg.update(over)
        gpu_ctx.stance_update_batch(n_, desc, arg["est_in"], arg["est_out"], arg["ground"], arg["rpy"], arg["gait_out"], arg["cmd"], arg["st"],
                                    gait_state=arg["gait_state"], vmc_in=o["vmc"], ratio=o["ratio"], stance_out=o["out"])

    bad_mode = lib_desc(pkg, rd); bad_mode.mode = 4
    neg_mode = lib_desc(pkg, rd); neg_mode.mode = -1
    bad_terrain = lib_desc(pkg, rd); bad_terrain.terrain = 5
    trot = pkg.stance_desc(3)
    calls = [lambda: upd(bad_mode), lambda: upd(neg_mode), lambda: upd(bad_terrain), lambda: upd(n_=0), lambda: upd(n_=5000),
             lambda: upd(gait_state=None), lambda: upd(trot, gait_state=None)]             # POSITION / ADVANCED_TROT need allowSwitchLegState
    calls += [functools.partial(upd, **{k: None}) for k in ("est_in", "est_out", "ground", "rpy", "gait_out", "cmd", "st")]
    walk = pkg.stance_desc(2)
    calls += [lambda: gpu_ctx.stance_command_batch(n, walk, d_tau, d_mc),                    # WALK without contacts / N / moveBasePhase
              lambda: gpu_ctx.stance_command_batch(n, ok, None, d_mc), lambda: gpu_ctx.stance_command_batch(n, ok, d_tau, None),
              lambda: gpu_ctx.stance_command_batch(n, ok, d_tau, d_mc, swing_q=i["est_in"]),  # swing targets without flags
              lambda: gpu_ctx.stance_command_batch(n, bad_mode, d_tau, d_mc), lambda: gpu_ctx.stance_command_batch(5000, ok, d_tau, d_mc)]
    gpu_ctx.vmc_setup_packed(0, pkg.workload.vmc_cfg("a1"), pkg.model_desc("a1")[:3])

    def tick(desc=ok, **over):
        arg = dict(vmc_in=o["vmc"], force=d_f, tau=d_tau, motor_cmd=d_mc, gait_state=i["gait_state"], ratio=o["ratio"], stance_out=o["out"])
        arg.update(over)
        gpu_ctx.stance_tick_batch(n, desc, i["est_in"], i["est_out"], i["ground"], i["rpy"], i["gait_out"], i["cmd"], a.st, arg["vmc_in"], arg["force"],
                                  arg["tau"], arg["motor_cmd"], gait_state=arg["gait_state"], ratio=arg["ratio"], stance_out=arg["stance_out"])
    walk_tick = pkg.stance_desc(2)
    calls += [lambda: tick(bad_mode), lambda: tick(vmc_in=None), lambda: tick(force=None), lambda: tick(motor_cmd=None), lambda: tick(gait_state=None),
              lambda: tick(walk_tick, ratio=None), lambda: tick(walk_tick, stance_out=None)]
    for k, call in enumerate(calls):
        with pytest.raises(pkg.QrgpuError):
            call()
    gpu_ctx.sync()
    for k in ("vmc", "ratio", "out"):
        assert np.all(o[k].download() == SENT), k
    assert same_bits(a.get("st")[0], st0[:n]) and np.all(d_mc.download() == SENT) and np.all(d_f.download() == SENT) and np.all(d_tau.download() == 1)
    upd()                                                                       # and the good call is accepted
    gpu_ctx.sync()
    assert not np.any(a.get("out")[0] == SENT)
    for v in (d_tau, d_f, d_mc):
        v.free()
    a.free()


# ---- 7. the command kernel ------------------------------------------------------------------------------------------------------------------
def test_command_kernel(gpu_ctx, pkg):
    n = N
    rng = np.random.default_rng(70)
    tau = rng.normal(0, 5, (n, 12)).astype(f32)
    sq = rng.normal(0, 1, (n, 24)).astype(f32)
    flags = np.zeros((n, 4), f32)                                              # the swing merge with 0, 1 and 4 legs flagged
    flags[n // 3:2 * n // 3, :] = np.eye(4, dtype=f32)[rng.integers(0, 4, 2 * n // 3 - n // 3)]
    flags[2 * n // 3:] = 1
    vin = np.zeros((n, 37), f32); so = np.zeros((n, 33), f32)
    vin[:, 18:22] = rng.integers(0, 2, (n, 4))
    so[:, 30] = vin[:, 18:22].sum(1); so[:, 31] = rng.uniform(0.4, 1.0, n)    # both sides of moveBasePhase = 0.7; N = 4 and N < 4
    S = lambda a: np.ascontiguousarray(a.T)
    d_tau, d_sq, d_fl = gpu_ctx.alloc((12, n)).upload(S(tau)), gpu_ctx.alloc((24, n)).upload(S(sq)), gpu_ctx.alloc((4, n)).upload(S(flags))
    d_vin, d_so = gpu_ctx.alloc((37, n)).upload(S(vin)), gpu_ctx.alloc((33, n)).upload(S(so))
    d_mc = gpu_ctx.alloc((60 * n + PAD,))
    kinds = set()
    for mode in range(4):
        rd = R.Desc(mode, motor_kp=[100.0 + j for j in range(12)], motor_kd=[1.0 + 0.25 * j for j in range(12)])
        desc = lib_desc(pkg, rd)
        for stop in (False, True):
            for swing in (True, False):                                        # NULL swing arrays: the stance command alone
                d_mc.upload(np.full(60 * n + PAD, SENT, f32))
                gpu_ctx.stance_command_batch(n, desc, d_tau, d_mc, vmc_in=d_vin if mode == 2 else None, stance_out=d_so if mode == 2 else None,
                                             swing_q=d_sq if swing else None, swing_flag=d_fl if swing else None, stop=stop)
                gpu_ctx.sync()
                flat = d_mc.download()
                got = flat[:60 * n].reshape(60, n).T
                want = np.stack([R.stance_command(rd, stop, vin[i], so[i], tau[i], sq[i] if swing else None, flags[i] if swing else None) for i in range(n)])
                assert same_bits(got, want), (mode, stop, swing)
                assert np.all(flat[60 * n:] == SENT)
                if mode != 2 and not swing:                                    # the default form: {0, 0, 0, 0, tau}
                    assert np.all(got[:, :48] == 0) and same_bits(got[:, 48:], tau)
                if mode == 2 and not swing and not stop:
                    c = vin[:, 18:22] != 0
                    moving = (so[:, 30] < 4) & (so[:, 31].astype(f64) < 0.7)
                    k1, k2, k3 = c, ~c & moving[:, None], ~c & ~moving[:, None]
                    kinds |= {1} if k1.any() else set(); kinds |= {2} if k2.any() else set(); kinds |= {3} if k3.any() else set()
                    kd = np.array(rd.motor_kd, f32).reshape(4, 3)
                    assert np.all(got[:, 36:48].reshape(n, 4, 3)[k1] == f32(0.5) * kd[np.nonzero(k1)[1]])
                    assert np.all(got[:, 48:60].reshape(n, 4, 3)[k3] == 0) and np.all(got[:, 36:48].reshape(n, 4, 3)[~k1] == 0)
                    assert same_bits(got[:, 48:60].reshape(n, 4, 3)[k2], tau.reshape(n, 4, 3)[k2])
    assert kinds == {1, 2, 3}
    for v in (d_tau, d_sq, d_fl, d_vin, d_so, d_mc):
        v.free()


# ---- 8. the tick is its three calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["velocity_slope", "walk_slope"])
def test_tick_equals_three_calls(gpu_ctx, pkg, case):
    W = pkg.workload
    rd, inp, st0, *_ = reference(case)
    desc = lib_desc(pkg, rd)
    n = N
    geom = pkg.model_desc("a1")[:3]
    gpu_ctx.vmc_setup_packed(0, W.vmc_cfg("a1"), geom)
    gpu_ctx.vmc_setup_packed(1, W.vmc_cfg("a1", friction=0.6, acc_weight=(2., 1., 1., 10., 5., 1.)), geom)
    tid = (np.arange(n) % 2).astype(np.int32)
    rng = np.random.default_rng(80)
    sq = rng.normal(0, 1, (24, n)).astype(f32); fl = (rng.random((4, n)) < 0.3).astype(f32)
    d_tid = gpu_ctx.alloc((n,), np.int32).upload(tid); d_sq = gpu_ctx.alloc((24, n)).upload(sq); d_fl = gpu_ctx.alloc((4, n)).upload(fl)
    world = rd.mode == R.WALK

    def run(fused):
        a = Arrays(gpu_ctx, inp, n, st0)
        i, o = a.ins, a.outs
        d_f, d_t, d_s, d_mc = gpu_ctx.alloc((12, n)), gpu_ctx.alloc((12, n)), gpu_ctx.alloc((n,), np.int32), gpu_ctx.alloc((60, n))
        for v in (d_f, d_t, d_mc):
            v.upload(np.full(v.shape, SENT, f32))
        if fused:
            gpu_ctx.stance_tick_batch(n, desc, i["est_in"], i["est_out"], i["ground"], i["rpy"], i["gait_out"], i["cmd"], a.st, o["vmc"], d_f, d_t, d_mc,
                                      gait_state=i["gait_state"], ratio=o["ratio"], stance_out=o["out"], status=d_s, swing_q=d_sq, swing_flag=d_fl,
                                      type_id=d_tid, current_time=0.1)
        else:
            a.update(desc, current_time=0.1)
            gpu_ctx.sync()
            d_q = i["est_in"].ptr + 17 * n * 4
            if world:
                gpu_ctx.vmc_force_world_batch(n, o["vmc"], o["ratio"], d_q, d_f, d_t, d_s, d_tid)
            else:
                gpu_ctx.vmc_force_batch(n, o["vmc"], d_q, d_f, d_t, d_s, d_tid)
            gpu_ctx.sync()
            gpu_ctx.stance_command_batch(n, desc, d_t, d_mc, vmc_in=o["vmc"], stance_out=o["out"], swing_q=d_sq, swing_flag=d_fl)
        gpu_ctx.sync()
        res = {k: a.get(k)[0] for k in ("vmc", "ratio", "out", "st")}
        res.update(force=d_f.download(), tau=d_t.download(), status=d_s.download(), cmd=d_mc.download())
        for v in (d_f, d_t, d_s, d_mc):
            v.free()
        a.free()
        return res

    x, y = run(True), run(False)
    for k in x:
        assert x[k].tobytes() == y[k].tobytes(), k
    assert np.all(x["out"][:, 32] == (1 if world else 0))
    assert np.isfinite(x["force"]).all() and not np.any(x["cmd"] == SENT)
    assert np.all((G.flags(x["status"]) & ~0x80) == 0)
    for v in (d_tid, d_sq, d_fl):
        v.free()


# ---- 9. the chained tick: ground -> estimator -> gait -> swing update -> stance tick -> swing action ---------------------------------------------
@pytest.mark.parametrize("mode", [R.WALK, R.VELOCITY])
def test_chained_tick_on_device(gpu_ctx, pkg, oracle, mode):
    """50 ticks queued with no host copy in between (every tick's sensor rows and contacts sit on the device beforehand) against the same
    calls with a sync and a download after every call, bit for bit; on the last tick the forces, torques and flags against the oracle's QP on
    the downloaded vmc_in / ratio (the bounds of test_gpu_vmc.py / test_gpu_swing_modes.py).  The swing command merged by a tick's command
    kernel is the one the previous tick's swing action left, as the order of the calls has it.  VELOCITY's swing action is
    qrgpu_swing_velocity_batch on a synthetic swing_vel_in whose lift-off rows the swing update maintains."""
    import test_gpu_ground as TG
    W = pkg.workload
    S = pkg.to_soa
    n, T, DT = 128, 50, 0.002
    walk = mode == R.WALK
    ecfg = W.estimator_cfg("a1", window=16)
    x, stamp = W.make_estimator_sequence(n, T, seed=91)
    gin = TG.make_sequences(n, T, seed=92)
    gin[:, :, 0:4] = x[:, :, 13:17]; gin[:, :, 19:23] = x[:, :, 6:10]
    if walk:
        gcfg = W.walk_cfg(stance_duration=0.06)                                # an 80 ms walk cycle: every sub-state inside 50 ticks
    else:
        gcfg = W.gait_cfg(stance_duration=0.03, duty_factor=0.6)
    vcfg, geom = W.vmc_cfg("a1", friction=0.6 if walk else 0.5), pkg.model_desc("a1")[:3]
    gpu_ctx.vmc_setup_packed(0, vcfg, geom)
    rd = R.Desc(mode, terrain=3, **DESC_KW)
    desc, sdesc = lib_desc(pkg, rd), pkg.swing_mode_desc(mode)
    inp = R.make_inputs(n, mode, 93)
    sv = None if walk else W.make_swing_velocity_batch(n, seed=94)
    svcfg = None if walk else W.swing_velocity_cfg("a1")
    nd = gpu_ctx.estimator_state_doubles(16)
    d_x = gpu_ctx.alloc((T, 54, n)).upload(np.ascontiguousarray(x.transpose(0, 2, 1)))
    d_gin = gpu_ctx.alloc((T, 23, n)).upload(np.ascontiguousarray(gin.transpose(0, 2, 1)))
    d_stamp = gpu_ctx.alloc((T, n), np.uint32).upload(stamp)
    d_rpy = gpu_ctx.alloc((3, n)).upload(S(inp["rpy"])); d_cmd = gpu_ctx.alloc((28, n)).upload(S(inp["cmd"]))
    go_rows, gs_rows = (41, 33) if walk else (24, 52)

    def run(synced):
        d = dict(gst=gpu_ctx.alloc((13, n), f64).upload(np.full((13, n), np.nan)), gout=gpu_ctx.alloc((32, n)), est=gpu_ctx.alloc((nd, n), f64).upload(np.zeros((nd, n))),
                 eo=gpu_ctx.alloc((42, n)), gs=gpu_ctx.alloc((gs_rows, n)).upload(np.zeros((gs_rows, n), f32)), go=gpu_ctx.alloc((go_rows, n)),
                 sst=gpu_ctx.alloc((pkg.qrgpu.SWING_STATE_FLOATS, n)).upload(np.full((pkg.qrgpu.SWING_STATE_FLOATS, n), np.nan, f32)), sfl=gpu_ctx.alloc((n,), np.int32),
                 sout=gpu_ctx.alloc((52, n)).upload(np.zeros((52, n), f32)), st=gpu_ctx.alloc((1, n)).upload(np.zeros((1, n), f32)), vmc=gpu_ctx.alloc((37, n)),
                 ratio=gpu_ctx.alloc((8, n)), out=gpu_ctx.alloc((33, n)), force=gpu_ctx.alloc((12, n)), tau=gpu_ctx.alloc((12, n)), status=gpu_ctx.alloc((n,), np.int32),
                 mc=gpu_ctx.alloc((60, n)))
        if not walk:
            d["sv"] = gpu_ctx.alloc((53, n)).upload(S(sv))
        seen = []

        def step(name=None):
            if synced:
                gpu_ctx.sync()
                if name:
                    seen.append(d[name].download())

        for k in range(T):
            ei = d_x.ptr + k * 54 * n * 4
            ct = ei + 13 * n * 4                                                # footContact: rows 13-16 of est_in
            gpu_ctx.ground_update_batch(n, d_gin.ptr + k * 23 * n * 4, d["gst"], d["gout"], ei, reset=(k == 0)); step("gout")
            gpu_ctx.estimator_update_batch(n, ecfg, ei, d_stamp.ptr + k * n * 4, d["est"], d["eo"]); step("eo")
            if walk:
                gpu_ctx.walk_gait_update_batch(n, gcfg, k * DT, ct, d["gs"], d["go"], reset=2 if k == 0 else 0)
            else:
                gpu_ctx.gait_update_batch(n, gcfg, k * DT, ct, d["gs"], d["go"], reset=(k == 0))
            step("go")
            gpu_ctx.swing_update_batch(n, sdesc, ei, d["eo"], d["go"], d["sst"], d["sfl"], swing_vel_in=None if walk else d["sv"], reset=2 if k == 0 else 0); step("sst")
            sq, sf = (d["sout"].ptr + 24 * n * 4, d["sout"].ptr + 48 * n * 4) if walk else (d["sout"].ptr + 24 * n * 4, d["sv"].ptr)
            gpu_ctx.stance_tick_batch(n, desc, ei, d["eo"], d["gout"], d_rpy, d["go"], d_cmd, d["st"], d["vmc"], d["force"], d["tau"], d["mc"],
                                      gait_state=None if walk else d["gs"], ratio=d["ratio"], stance_out=d["out"], status=d["status"], swing_q=sq, swing_flag=sf,
                                      current_time=k * DT, reset=(k == 0))
            step("mc")
            if walk:
                gpu_ctx.swing_action_batch(n, sdesc, ecfg, ei, d["eo"], d["go"], d["sst"], d["sout"], d["sfl"])
            else:
                gpu_ctx.swing_velocity_batch(n, ecfg, svcfg, d["sv"], d["sout"])
            step("sout")
        gpu_ctx.sync()
        res = {k: v.download() for k, v in d.items()}
        for v in d.values():
            v.free()
        return res, seen

    a, _ = run(False)
    b, seen = run(True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                            # bit for bit
    gos = np.stack(seen[2::6])                                                 # the gait outputs of every tick
    if walk:
        assert set(np.unique(gos[:, 8:12])) >= {1, 5, 6, 7, 8}                  # every walk sub-state was met
    else:
        assert set(np.unique(gos[:, 8:12])) == {0, 1}
    assert np.isfinite(b["out"]).all() and np.isfinite(b["force"]).all()
    assert np.all(b["out"][32] == (1 if walk else 0))
    vin_f, ratio_f, force, tau = b["vmc"].T, b["ratio"].T, b["force"].T, b["tau"].T
    q_last = x[T - 1, :, 17:29]
    flags = G.flags(b["status"])
    assert np.all((flags & ~0x80) == 0), np.unique(flags)
    for i in range(0, n, 4):
        f, t, _, _, rc = oracle.vmc_solve(vcfg, geom, vin_f[i], q_last[i], ratio_f[i] if walk else None)
        assert bool(flags[i] & 0x80) == (rc == 1), (i, flags[i], rc)
        assert np.abs(force[i] - f).max() <= 1e-5 * max(1.0, np.abs(f).max()), i
        assert np.all(np.abs(tau[i] - t) <= tau_tol(t, 1e-4)), i
    # the motor command of the last tick from the downloaded pieces, through the restatement
    sw = seen[6 * (T - 2) + 5]                                                  # the swing output the last tick's command kernel read: tick T - 2's
    for i in range(0, n, 4):
        if walk:
            want = R.stance_command(rd, False, vin_f[i], b["out"][:, i], tau[i], sw[24:48, i], sw[48:52, i])
            assert same_bits(b["mc"][:, i], want), i
    for v in (d_x, d_gin, d_stamp, d_rpy, d_cmd):
        v.free()


# ---- 10. the kernels are in the gfx950 code object ----------------------------------------------------------------------------------------------
def test_kernels_present(gpu_ctx, pkg):
    data = open(pkg._build.build(), "rb").read()
    assert b"gfx950" in data and b"qr_stance_update_kernel" in data and b"qr_stance_command_kernel" in data
