"""GPU parity of the swing-leg controller of the walk and position modes and of the lift-off memory of all four modes
(qrgpu_swing_update_batch / qrgpu_swing_action_batch) against the CPU restatement tests/swing_modes_ref.py, with the gait inputs from the
real gait kernels, and the two chains the controller feeds: walk gait -> swing -> world-frame force distribution queued without host copies,
and ADVANCED_TROT lift-off rows -> qrgpu_swing_targets_batch.
Reference: qr_swing_leg_controller.cpp:60-461, qr_foothold_planner.cpp:49-109, qr_foot_stepper.cpp:31-202, 483-525.
Bars: copies and flags bit-exact; rotated / translated points 1e-6 m (Eigen-order float sums, sinf / cosf / atan2f may differ from libm
by an ulp); trajectory points 2e-6 m, velocities 2e-5, joint targets 2e-5 rad."""
import numpy as np
import pytest

import gpu_helpers as G
import swing_modes_ref as R
from gpu_helpers import tau_tol

pytestmark = pytest.mark.gpu

N = 1024
SPREAD = 48            # robots spread over the batch ...
TOP = 16               # ... and the ones with the most lift-offs: the replayed sample
DT = 0.002
WALK_SHORT = dict(stance_duration=0.75)        # a 1 s walk cycle next to the 10 s one of the yaml


def est_arrays(n, k, seed, drift=0.4):
    """est_in [54][n] and est_out [42][n] of tick k: a slowly tilting, yawing base drifting forward at `drift` m/s, feet near the nominal
    stance.  The walk mode steps in place (its footholds move only on STAIRS), so its runs keep the base where it is: a base drifting away from
    world-frame footholds stretches the legs towards the singular, straight knee, where J^-1 multiplies the last-ulp differences of sinf /
    cosf between the device and numpy by ~80."""
    rng = np.random.default_rng(seed + 7919 * k)
    r = np.random.default_rng(seed)
    ph = r.uniform(0, 2 * np.pi, n)
    t = k * DT
    yaw = 0.3 * np.sin(0.7 * t + ph); pitch = 0.05 * np.sin(1.3 * t + 2 * ph); roll = 0.04 * np.cos(1.1 * t + ph)
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    q = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])
    est_in = np.zeros((54, n), np.float32)
    est_in[6:10] = q
    est_in[17:29] = np.tile(np.array([0.0, 0.9, -1.8], np.float32), 4)[:, None] + rng.normal(0, 0.05, (12, n))
    nominal = np.array([0.18, -0.13, -0.28, 0.18, 0.13, -0.28, -0.18, -0.13, -0.28, -0.18, 0.13, -0.28], np.float32)
    est_out = np.zeros((42, n), np.float32)
    est_out[12:24] = nominal[:, None] + rng.normal(0, 0.02, (12, n))
    est_out[36] = drift * t + r.uniform(-0.3, 0.3, n); est_out[37] = r.uniform(-0.2, 0.2, n); est_out[38] = 0.28 + 0.01 * np.sin(3 * t + ph)
    return est_in, est_out


def lift_mask(mode, go, stop):
    """Update's lift-off triggers of every robot and leg from a gait output [rows][n] (qr_swing_leg_controller.cpp:124-196)."""
    nst, cur = go[8:12], go[16:20]
    if mode == 1:
        return np.isin(nst, (0, 4)) & (cur == 1) & (not stop)
    if mode == 2:
        return np.isin(nst, (8, 4)) & (cur == 6) & (not stop)
    return (nst == 0) & (nst != cur)


def gait_pass(gpu_ctx, pkg, mode, ticks, walk_kw=None, stop_at=None, seed=5):
    """The gait generator alone over `ticks`: its config, the contacts [ticks][n][4] it is driven with and the lift-offs per robot.  The walk
    gait's contacts follow its schedule: a foot is down unless the previous tick had it in TRUE_SWING, and about one swing in eight touches
    down early, in the last fifth of its true swing (EARLY_CONTACT).  The open-loop gait gets make_gait_contacts' late / early touch-downs."""
    W = pkg.workload
    n = N
    walk = mode == 2
    if walk:
        gcfg = W.walk_cfg(**(walk_kw or {}))
        d_gs = gpu_ctx.alloc((33, n)); d_go = gpu_ctx.alloc((41, n)); rows = 41
        contacts = np.ones((ticks, n, 4), np.float32)
        early = np.random.default_rng(seed).uniform(0, 1, (4, n)) < 0.125
    else:
        gcfg = W.gait_cfg()
        d_gs = gpu_ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32)); d_go = gpu_ctx.alloc((24, n)); rows = 24
        contacts = W.make_gait_contacts(n, ticks, gcfg, seed=seed)
    d_ct = gpu_ctx.alloc((4, n))
    lifts = np.zeros(n, int)
    prev = None
    for k in range(ticks):
        if walk and prev is not None:
            sw = prev[8:12] == 8
            c = (~sw).astype(np.float32)
            c[sw & early & (prev[4:8] > 0.8)] = 1.0
            contacts[k] = c.T
        d_ct.upload(pkg.to_soa(contacts[k]))
        stop = stop_at is not None and stop_at[0] <= k < stop_at[1]
        if walk:
            gpu_ctx.walk_gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, stop=stop, reset=2 if k == 0 else 0)
        else:
            gpu_ctx.gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, stop=stop, reset=(k == 0))
        prev = d_go.download().reshape(rows, n)
        lifts += lift_mask(mode, prev, stop).sum(0)
    for v in (d_gs, d_go, d_ct):
        v.free()
    return gcfg, contacts, lifts


def run_modes(gpu_ctx, pkg, mode, desc_kw, ticks, act=True, walk_kw=None, stop_at=None):
    """gait -> swing update (-> swing action) over the whole batch on the device; records what the restatement needs for the sample (spread
    over the batch plus the robots with the most lift-offs) every tick, and the sample's outputs of every tick."""
    W = pkg.workload
    S = pkg.to_soa
    n = N
    gcfg, contacts, lifts = gait_pass(gpu_ctx, pkg, mode, ticks, walk_kw, stop_at)
    sample = np.unique(np.concatenate([np.linspace(0, n - 1, SPREAD).astype(int), np.argsort(-lifts, kind="stable")[:TOP]]))
    assert lifts[sample].max() == lifts.max()
    desc = pkg.swing_mode_desc(mode, **desc_kw)
    rdesc = R.Desc(mode, terrain=desc.terrain, is_sim=desc.is_sim, foothold_delta=desc.foothold_delta,
                   gaps=[desc.gap_distance[k] for k in range(desc.n_gaps)], gap_width=desc.gap_width)
    walk = mode == 2
    if walk:
        d_gs = gpu_ctx.alloc((33, n)); d_go = gpu_ctx.alloc((41, n)); rows_go = 41
    else:
        d_gs = gpu_ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32)); d_go = gpu_ctx.alloc((24, n)); rows_go = 24
    d_ct = gpu_ctx.alloc((4, n))
    d_ei = gpu_ctx.alloc((54, n)); d_eo = gpu_ctx.alloc((42, n))
    d_st = gpu_ctx.alloc((R.STATE_FLOATS, n)).upload(np.full((R.STATE_FLOATS, n), np.nan, np.float32))
    d_fl = gpu_ctx.alloc((n,))                                              # one int32 word per robot
    sentinel = np.float32(-777.0)
    d_sw = gpu_ctx.alloc((58, n)).upload(np.full((58, n), sentinel, np.float32))
    d_sv = gpu_ctx.alloc((53, n)).upload(np.full((53, n), sentinel, np.float32))
    d_fe = gpu_ctx.alloc((64, n)).upload(np.full((64, n), sentinel, np.float32))
    d_out = gpu_ctx.alloc((R.OUT_ROWS, n)).upload(np.full((R.OUT_ROWS, n), sentinel, np.float32))
    ecfg = W.estimator_cfg("a1")
    rec, outs = [], []
    for k in range(ticks):
        d_ct.upload(S(contacts[k]))
        stop = stop_at is not None and stop_at[0] <= k < stop_at[1]
        if walk:
            gpu_ctx.walk_gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, stop=stop, reset=2 if k == 0 else 0)
        else:
            gpu_ctx.gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, stop=stop, reset=(k == 0))
        ei, eo = est_arrays(n, k, 17, drift=0.0 if walk else 0.4)
        d_ei.upload(ei); d_eo.upload(eo)
        gpu_ctx.swing_update_batch(n, desc, d_ei, d_eo, d_go, d_st, d_fl, gait_state=d_gs, swing_in=d_sw, swing_vel_in=d_sv, fe_in=d_fe,
                                   reset=2 if k == 0 else 0, stop=stop)
        if act:
            gpu_ctx.swing_action_batch(n, desc, ecfg, d_ei, d_eo, d_go, d_st, d_out, d_fl, gait_state=d_gs, stop=stop)
        gpu_ctx.sync()
        go = d_go.download().reshape(rows_go, n)
        gs = d_gs.download().reshape(-1, n) if not walk else None
        rec.append((ei[:, sample].T.copy(), eo[:, sample].T.copy(), go[:, sample].T.copy(), None if gs is None else gs[:, sample].T.copy(), stop))
        if act:
            outs.append(d_out.download().reshape(R.OUT_ROWS, n)[:, sample].T.copy())
    res = dict(state=d_st.download().reshape(R.STATE_FLOATS, n)[:, sample].T, flags=np.asarray(d_fl.download()).view(np.int32).reshape(-1)[sample],
               swing_in=d_sw.download().reshape(58, n)[:, sample].T, swing_vel_in=d_sv.download().reshape(53, n)[:, sample].T,
               fe_in=d_fe.download().reshape(64, n)[:, sample].T, outs=outs)
    for v in (d_gs, d_go, d_ct, d_ei, d_eo, d_st, d_fl, d_sw, d_sv, d_fe, d_out):
        v.free()
    return rdesc, ecfg, rec, res, sentinel


def replay(rdesc, ecfg, rec, sentinel, act=True):
    m = len(rec[0][0])
    st = np.full((m, R.STATE_FLOATS), np.nan, np.float32)
    fl = np.zeros(m, np.int64)
    sw = np.full((m, 58), sentinel, np.float32); sv = np.full((m, 53), sentinel, np.float32); fe = np.full((m, 64), sentinel, np.float32)
    out = np.full((m, R.OUT_ROWS), sentinel, np.float32)
    lifts = np.zeros(m, int)
    outs = []
    for k, (ei, eo, go, gs, stop) in enumerate(rec):
        for j in range(m):
            before = st[j, R.SS_LOCAL:R.SS_LOCAL + 12].copy()
            fl[j] = R.swing_update(rdesc, 2 if k == 0 else 0, stop, ei[j], eo[j], go[j], st[j], int(fl[j]), sw[j], sv[j], fe[j])
            lifts[j] += int(not np.array_equal(before, st[j, R.SS_LOCAL:R.SS_LOCAL + 12], equal_nan=True))
            if act:
                fl[j] = R.swing_action(rdesc, ecfg, stop, ei[j], eo[j], go[j], None if gs is None else gs[j], st[j], out[j], int(fl[j]))
        outs.append(out.copy())
    return st, fl, sw, sv, fe, outs, lifts


def close(a, b, tol):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and (np.nan_to_num(np.abs(a - b), nan=0.0).max(initial=0.0) <= tol)


def walk_coverage(us):
    """commanded walk legs reached the end of the trajectory and every knot span of the B-spline was evaluated"""
    us = np.asarray(us, np.float32)
    assert us.size and us.max() > 0.9, us.max(initial=0)
    spans = {R.find_span(u) for u in us}
    assert spans == set(range(3, 9)), spans


EXACT_ROWS = [R.SS_BUILT, R.SS_MAP] + list(range(R.SS_OFF, R.STATE_FLOATS))
LIFTOFF_CASES = {"velocity": (0, {}), "position": (1, {}), "walk": (2, {}), "advanced_trot": (3, {}),
                 "position_stairs": (1, dict(terrain=2)), "walk_stairs": (2, dict(terrain=2)),
                 "walk_plum_piles": (2, dict(terrain=1, gaps=(0.51, 1.31, 1.91)))}


@pytest.mark.parametrize("case", list(LIFTOFF_CASES))
def test_liftoff_parity(gpu_ctx, pkg, case):
    mode, kw = LIFTOFF_CASES[case]
    walk_kw = WALK_SHORT if mode == 2 else None
    rdesc, ecfg, rec, res, sentinel = run_modes(gpu_ctx, pkg, mode, kw, 600, act=False, walk_kw=walk_kw)
    st, fl, sw, sv, fe, _, lifts = replay(rdesc, ecfg, rec, sentinel, act=False)
    g = res["state"]
    assert np.array_equal(res["flags"], fl.astype(np.int32))
    assert lifts.sum() > 2 * len(lifts), lifts.sum()                     # the reset and at least one lift-off per robot on average
    assert np.array_equal(g[:, R.SS_LOCAL:R.SS_LOCAL + 12], st[:, R.SS_LOCAL:R.SS_LOCAL + 12], equal_nan=True)   # copies
    assert close(g[:, R.SS_GLOBAL:R.SS_GLOBAL + 12], st[:, R.SS_GLOBAL:R.SS_GLOBAL + 12], 1e-6)
    if mode in (1, 2):
        assert close(g[:, R.SS_FH:R.SS_H + 4], st[:, R.SS_FH:R.SS_H + 4], 1e-6)
        assert np.array_equal(g[:, EXACT_ROWS], st[:, EXACT_ROWS], equal_nan=True)
    if case == "walk_plum_piles":
        assert (g[:, R.SS_PFLAGS].astype(int) & 1).any()                  # the stepper planned on the walk mode's footholds
    if case.endswith("stairs"):
        assert np.all(g[:, R.SS_OFF:R.SS_OFF + 12:3] == np.float32(0.1))   # nextFootholdsOffset row 0 on STAIRS
    # rows written into the existing kernels' inputs: identical, sentinel rows untouched
    for a, b, rows in ((res["swing_in"], sw, range(12, 24)), (res["swing_vel_in"], sv, range(8, 20)), (res["fe_in"], fe, range(62, 64))):
        rows = list(rows)
        other = [r for r in range(a.shape[1]) if r not in rows]
        assert np.all(a[:, other] == sentinel)
        if mode in (0, 3):
            assert close(a[:, rows], b[:, rows], 1e-6)
        else:
            assert np.all(a[:, rows] == sentinel)


def check_action(res, st, fl, outs):
    """every tick's outputs of the sample (rows a call does not write keep what earlier ticks left, on both sides)"""
    assert np.array_equal(res["flags"], fl.astype(np.int32))
    commanded = 0
    for k, (g, out) in enumerate(zip(res["outs"], outs)):
        assert np.array_equal(g[:, 48:52], out[:, 48:52]), k                   # command flags
        assert close(g[:, 0:12], out[:, 0:12], 2e-6), k
        assert close(g[:, 12:24], out[:, 12:24], 2e-5), k
        assert close(g[:, 24:48], out[:, 24:48], 2e-5), k
        commanded += int((g[:, 48:52] == 1).sum())
    assert np.array_equal(res["state"][:, EXACT_ROWS], st[:, EXACT_ROWS], equal_nan=True)
    assert commanded > 0


@pytest.mark.parametrize("variant", ["sim", "real"])
def test_walk_action_parity(gpu_ctx, pkg, variant):
    rdesc, ecfg, rec, res, sentinel = run_modes(gpu_ctx, pkg, 2, dict(is_sim=(variant == "sim")), 600, walk_kw=WALK_SHORT, stop_at=(450, 470))
    st, fl, sw, sv, fe, outs, lifts = replay(rdesc, ecfg, rec, sentinel)
    check_action(res, st, fl, outs)
    assert int(res["state"][:, R.SS_BUILT].max()) == 15
    us = [rec[k][2][:, 4:8][res["outs"][k][:, 48:52] == 1] for k in range(len(rec))]
    walk_coverage(np.concatenate(us))
    assert any((r[2][:, 20:24] == 2).any() for r in rec)                    # early touch-downs dropped legs from the swing set


@pytest.mark.parametrize("variant", ["no_gaps", "a1_sim_gaps"])
def test_position_action_parity(gpu_ctx, pkg, variant):
    kw = dict(gaps=()) if variant == "no_gaps" else {}
    rdesc, ecfg, rec, res, sentinel = run_modes(gpu_ctx, pkg, 1, kw, 600)
    st, fl, sw, sv, fe, outs, lifts = replay(rdesc, ecfg, rec, sentinel)
    check_action(res, st, fl, outs)
    if variant == "a1_sim_gaps":
        assert (res["state"][:, R.SS_PFLAGS].astype(int) & 1).all()       # every robot planned its crossing


def test_walk_mode_tick_on_device(gpu_ctx, pkg, oracle):
    """walk gait -> swing update -> swing action -> qrgpu_vmc_force_world_batch for one full walk cycle, every call queued with no host copy
    between ticks (the contacts of all ticks sit on the device), against the same calls with a sync and a download after every tick; the
    forces and torques of sampled robots against the oracle on the final tick's inputs (the bounds of test_vmc_world_frame_parity)."""
    W = pkg.workload
    S = pkg.to_soa
    n, T = N, 500                                                          # 1 s = one cycle of the shortened walk
    gcfg, contacts, _ = gait_pass(gpu_ctx, pkg, 2, T, WALK_SHORT, seed=9)
    desc = pkg.swing_mode_desc(2)
    ecfg = W.estimator_cfg("a1")
    vcfg = W.vmc_cfg("a1"); geom = pkg.model_desc("a1")[:3]
    gpu_ctx.vmc_setup_packed(0, vcfg, geom)
    vin, q, ratio0 = W.make_vmc_world_batch(n, seed=23)
    ei, eo = est_arrays(n, 0, 17)
    d_ct = gpu_ctx.alloc((T, 4, n)).upload(np.ascontiguousarray(contacts.transpose(0, 2, 1)))
    d_ei = gpu_ctx.alloc((54, n)).upload(ei); d_eo = gpu_ctx.alloc((42, n)).upload(eo); d_q = gpu_ctx.alloc((12, n)).upload(S(q))

    def run(synced):
        d_ws = gpu_ctx.alloc((33, n)); d_wo = gpu_ctx.alloc((41, n))
        d_ratio = gpu_ctx.alloc((8, n)).upload(S(ratio0)); d_vmc = gpu_ctx.alloc((37, n)).upload(S(vin))
        d_st = gpu_ctx.alloc((R.STATE_FLOATS, n)).upload(np.full((R.STATE_FLOATS, n), np.nan, np.float32))
        d_fl = gpu_ctx.alloc((n,), np.int32); d_out = gpu_ctx.alloc((R.OUT_ROWS, n)).upload(np.zeros((R.OUT_ROWS, n), np.float32))
        d_f = gpu_ctx.alloc((12, n)); d_t = gpu_ctx.alloc((12, n)); d_s = gpu_ctx.alloc((n,), np.int32)
        seen = []
        for k in range(T):
            gpu_ctx.walk_gait_update_batch(n, gcfg, k * DT, d_ct.ptr + k * 4 * n * 4, d_ws, d_wo, d_ratio, d_vmc, reset=2 if k == 0 else 0)
            gpu_ctx.swing_update_batch(n, desc, d_ei, d_eo, d_wo, d_st, d_fl, reset=2 if k == 0 else 0)
            gpu_ctx.swing_action_batch(n, desc, ecfg, d_ei, d_eo, d_wo, d_st, d_out, d_fl)
            gpu_ctx.vmc_force_world_batch(n, d_vmc, d_ratio, d_q, d_f, d_t, d_s)
            if synced:
                gpu_ctx.sync()
                o, wo = d_out.download(), d_wo.download()
                seen.append(wo[4:8][o[48:52] == 1])
        gpu_ctx.sync()
        res = dict(out=d_out.download(), st=d_st.download(), fl=d_fl.download(), force=d_f.download(), tau=d_t.download(), status=d_s.download(),
                   vmc=d_vmc.download(), ratio=d_ratio.download())
        for v in (d_ws, d_wo, d_ratio, d_vmc, d_st, d_fl, d_out, d_f, d_t, d_s):
            v.free()
        return res, seen

    a, _ = run(False)
    b, seen = run(True)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key                    # bit for bit
    walk_coverage(np.concatenate(seen))
    assert (b["fl"] == 0).all()
    vin_f, ratio_f, force, tau = b["vmc"].T, b["ratio"].T, b["force"].T, b["tau"].T
    flags = G.flags(b["status"])
    assert np.all((flags & ~0x80) == 0), np.unique(flags)
    for i in range(0, n, 16):
        f, t, x, st, rc = oracle.vmc_solve(vcfg, geom, vin_f[i], q[i], ratio_f[i])
        assert bool(flags[i] & 0x80) == (rc == 1), (i, flags[i], rc)
        assert np.abs(force[i] - f).max() <= 1e-5 * max(1.0, np.abs(f).max()), i
        assert np.all(np.abs(tau[i] - t) <= tau_tol(t, 1e-4)), i
    for v in (d_ct, d_ei, d_eo, d_q):
        v.free()


def test_advanced_trot_liftoff_feeds_swing_targets(gpu_ctx, pkg):
    """gait -> swing update (writing swing_in rows 12-23 and fe_in rows 62-63) -> footholds -> qrgpu_swing_targets_batch, against the same
    chain with those rows computed by the restatement and uploaded."""
    W = pkg.workload
    S = pkg.to_soa
    n, ticks = 256, 130
    gcfg, fcfg, ecfg = W.gait_cfg(), W.foothold_cfg("a1"), W.estimator_cfg("a1")
    contacts = W.make_gait_contacts(n, ticks, gcfg, seed=5)
    fh = W.make_foothold_batch(n, "a1", seed=6)
    sw0 = W.make_swing_batch(n, seed=7)
    desc = pkg.swing_mode_desc(3)
    rdesc = R.Desc(3)
    sentinel = np.float32(-777.0)

    def chain(on_device):
        d_gs = gpu_ctx.alloc((52, n)).upload(np.zeros((52, n), np.float32)); d_go = gpu_ctx.alloc((24, n)); d_ct = gpu_ctx.alloc((4, n))
        d_fh = gpu_ctx.alloc((46, n)).upload(S(fh)); d_sw = gpu_ctx.alloc((58, n)).upload(S(sw0))
        d_cmd = gpu_ctx.alloc((67, n)).upload(np.zeros((67, n), np.float32))
        d_ei = gpu_ctx.alloc((54, n)); d_eo = gpu_ctx.alloc((42, n))
        d_st = gpu_ctx.alloc((R.STATE_FLOATS, n)).upload(np.full((R.STATE_FLOATS, n), np.nan, np.float32)); d_fl = gpu_ctx.alloc((n,), np.int32)
        d_fe = gpu_ctx.alloc((64, n)).upload(np.full((64, n), sentinel, np.float32))
        st = np.full((n, R.STATE_FLOATS), np.nan, np.float32); fl = np.zeros(n, np.int64)
        sw = S(sw0).T.copy(); fe = np.full((n, 64), sentinel, np.float32)
        for k in range(ticks):
            d_ct.upload(S(contacts[k]))
            ei, eo = est_arrays(n, k, 29)
            gpu_ctx.gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, reset=(k == 0))
            if on_device:
                d_ei.upload(ei); d_eo.upload(eo)
                gpu_ctx.swing_update_batch(n, desc, d_ei, d_eo, d_go, d_st, d_fl, swing_in=d_sw, fe_in=d_fe, reset=2 if k == 0 else 0)
            else:
                gpu_ctx.sync()
                go = d_go.download()
                for i in range(n):
                    fl[i] = R.swing_update(rdesc, 2 if k == 0 else 0, False, ei[:, i], eo[:, i], go[:, i], st[i], int(fl[i]), sw[i], None, fe[i])
            gpu_ctx.footholds_batch(n, fcfg, d_fh, d_sw, gait_state=d_gs, gait_out=d_go)
        if not on_device:                                                  # the lift-off rows from the host, uploaded
            gpu_ctx.sync()
            g = d_sw.download(); g[12:24] = sw.T[12:24]; d_sw.upload(g)
        gpu_ctx.swing_targets_batch(n, ecfg, d_sw, d_cmd)
        gpu_ctx.sync()
        out = dict(cmd=d_cmd.download().T.copy(), sw=d_sw.download().T.copy(), fe=d_fe.download().T.copy() if on_device else fe)
        for v in (d_gs, d_go, d_ct, d_fh, d_sw, d_cmd, d_ei, d_eo, d_st, d_fl, d_fe):
            v.free()
        return out

    dev, host = chain(True), chain(False)
    lifted = dev["sw"][:, 12:24] != S(sw0).T[:, 12:24]
    assert lifted.any(axis=1).mean() > 0.9                                 # nearly every robot's lift-off rows came from the update
    assert close(dev["sw"][:, 12:24], host["sw"][:, 12:24], 1e-6)
    assert np.array_equal(dev["sw"][:, :12], host["sw"][:, :12]) and np.array_equal(dev["sw"][:, 24:], host["sw"][:, 24:])
    assert close(dev["fe"][:, 62:64], host["fe"][:, 62:64], 0.0)
    assert np.all(dev["fe"][:, :62] == sentinel)
    assert int(dev["sw"][:, :4].sum()) > 0
    assert np.abs(dev["cmd"][:, 15:51] - host["cmd"][:, 15:51]).max() <= 1e-6


def test_swing_modes_bad_arguments(gpu_ctx, pkg):
    n = 8
    a = [gpu_ctx.alloc((R.STATE_FLOATS, n)) for _ in range(4)]
    d_fl = gpu_ctx.alloc((n,))
    ecfg = pkg.workload.estimator_cfg("a1")
    ok = pkg.swing_mode_desc(2)
    gpu_ctx.swing_update_batch(n, ok, a[0], a[1], a[2], a[3], d_fl, reset=2)          # accepted
    gpu_ctx.sync()
    bad_mode = pkg.swing_mode_desc(2); bad_mode.mode = 4
    many = pkg.swing_mode_desc(1); many.n_gaps = 9
    for desc in (bad_mode, many):
        with pytest.raises(pkg.QrgpuError):
            gpu_ctx.swing_update_batch(n, desc, a[0], a[1], a[2], a[3], d_fl)
    for mode in (0, 3):                                                                  # their actions have kernels of their own
        with pytest.raises(pkg.QrgpuError):
            gpu_ctx.swing_action_batch(n, pkg.swing_mode_desc(mode), ecfg, a[0], a[1], a[2], a[3], a[0], d_fl, gait_state=a[1])
    with pytest.raises(pkg.QrgpuError):
        gpu_ctx.swing_update_batch(5000, ok, a[0], a[1], a[2], a[3], d_fl)              # n > max_batch
    with pytest.raises(pkg.QrgpuError):
        gpu_ctx.swing_update_batch(n, ok, a[0], a[1], None, a[3], d_fl)                 # NULL gait output
    with pytest.raises(pkg.QrgpuError):
        gpu_ctx.swing_update_batch(n, ok, a[0], a[1], a[2], a[3], d_fl, reset=3)
    with pytest.raises(pkg.QrgpuError):
        gpu_ctx.swing_action_batch(n, pkg.swing_mode_desc(1), ecfg, a[0], a[1], a[2], a[3], a[0], d_fl)   # position without gait state
    for v in a + [d_fl]:
        v.free()


def test_swing_stages_read_only_the_geometry(gpu_ctx, pkg):
    """qrgpu_swing_targets_batch, qrgpu_swing_velocity_batch and qrgpu_swing_action_batch (WALK) hand the caller's qrgpu_estimator_desc to their
    kernels as it is: the members that are not leg geometry may hold anything.  n = 65: two workgroups, the second with one robot.  Each stage
    runs on the same inputs with a clean geometry-only block and with window = -7, time_step = NaN, variances 1e30, body_height = -1: bit-equal."""
    W = pkg.workload
    S = pkg.to_soa
    n = 65
    sentinel = np.float32(-777.0)
    clean = pkg.qrgpu._estimator_desc(W.estimator_cfg("a1"), geometry_only=True)
    junk = pkg.qrgpu._estimator_desc(W.estimator_cfg("a1", time_step=np.nan, accelerometer_variance=1e30, sensor_variance=1e30, window=-7, body_height=-1.0))
    assert (clean.window, clean.time_step, clean.body_height) == (0, 0.0, 0.0)
    assert junk.window == -7 and np.isnan(junk.time_step) and junk.sensor_variance == np.float32(1e30) and junk.body_height == -1.0
    assert list(junk.hip_offset) == list(clean.hip_offset) and (junk.hip_l, junk.upper_l, junk.lower_l) == (clean.hip_l, clean.upper_l, clean.lower_l)

    def fresh(rows):
        return gpu_ctx.alloc((rows, n)).upload(np.full((rows, n), sentinel, np.float32))

    def same(a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

    # swing targets
    d_in = gpu_ctx.alloc((58, n)).upload(S(W.make_swing_batch(n, seed=31)))
    res = []
    for desc in (clean, junk):
        outs = [fresh(67), fresh(12), fresh(24)]
        gpu_ctx.swing_targets_batch(n, desc, d_in, *outs)
        gpu_ctx.sync()
        res.append([v.download() for v in outs])
        for v in outs:
            v.free()
    d_in.free()
    assert all(same(a, b) for a, b in zip(*res))
    assert (res[0][0][15:51] != sentinel).any() and (res[0][2] != sentinel).any()                 # ... and something was written

    # velocity-mode swing action
    d_in = gpu_ctx.alloc((53, n)).upload(S(W.make_swing_velocity_batch(n, seed=32)))
    res = []
    for desc in (clean, junk):
        d_out = fresh(48)
        gpu_ctx.swing_velocity_batch(n, desc, W.swing_velocity_cfg("a1"), d_in, d_out)
        gpu_ctx.sync()
        res.append(d_out.download()); d_out.free()
    d_in.free()
    assert same(*res) and (res[0] != sentinel).any()

    # walk-mode swing action: one 1 s walk cycle of gait, swing update and action (as run_modes drives them, contacts following the schedule as in
    # gait_pass: a foot is down unless the previous tick had it in TRUE_SWING); every 25th tick -- a leg's true swing lasts 37 -- the action runs
    # twice from the same state, with either block
    gcfg = W.walk_cfg(**WALK_SHORT)
    sdesc = pkg.swing_mode_desc(pkg.qrgpu.MODE_WALK)
    d_gs = gpu_ctx.alloc((33, n)); d_go = gpu_ctx.alloc((41, n)); d_ct = gpu_ctx.alloc((4, n))
    d_ei = gpu_ctx.alloc((54, n)); d_eo = gpu_ctx.alloc((42, n))
    d_st = gpu_ctx.alloc((R.STATE_FLOATS, n)).upload(np.full((R.STATE_FLOATS, n), np.nan, np.float32)); d_fl = gpu_ctx.alloc((n,))
    d_out = fresh(R.OUT_ROWS)
    compared = commanded = 0
    contact = np.ones((4, n), np.float32)
    for k in range(500):
        d_ct.upload(contact)
        gpu_ctx.walk_gait_update_batch(n, gcfg, k * DT, d_ct, d_gs, d_go, reset=2 if k == 0 else 0)
        ei, eo = est_arrays(n, k, 33, drift=0.0)
        d_ei.upload(ei); d_eo.upload(eo)
        gpu_ctx.swing_update_batch(n, sdesc, d_ei, d_eo, d_go, d_st, d_fl, gait_state=d_gs, reset=2 if k == 0 else 0)
        gpu_ctx.sync()
        contact = (d_go.download().reshape(41, n)[8:12] != 8).astype(np.float32)
        if k % 25 != 24:
            gpu_ctx.swing_action_batch(n, sdesc, clean, d_ei, d_eo, d_go, d_st, d_out, d_fl)
            continue
        before = [v.download() for v in (d_out, d_st, d_fl)]
        res = []
        for desc in (clean, junk):
            for v, h in zip((d_out, d_st, d_fl), before):
                v.upload(h)
            gpu_ctx.swing_action_batch(n, sdesc, desc, d_ei, d_eo, d_go, d_st, d_out, d_fl)
            gpu_ctx.sync()
            res.append([v.download() for v in (d_out, d_st, d_fl)])
        assert all(same(a, b) for a, b in zip(*res)), k
        compared += 1
        commanded += int((res[0][0][48:52] == 1).sum())
    for v in (d_gs, d_go, d_ct, d_ei, d_eo, d_st, d_fl, d_out):
        v.free()
    assert compared == 20 and commanded > 0                                                       # ... on ticks with legs in true swing
