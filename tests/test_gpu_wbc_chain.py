"""-m gpu: the WBC kernel's chain -- the kept rows of the null-space projector, its three SPD inverses with their guards and fallback, the
relaxation QP's fixed part and per-change loop -- against the float64 oracle, at the bars of tests/test_gpu_wbc.py:
torque 1e-6 * max(1, |tau|), q_des 1e-5, qd_des 1e-4, status 0 on every robot.  No robot is left out of any comparison.

  * all 16 contact patterns on A1 and Lite3: every contact_part<D> case and the flight default, 2..6 tasks with the swing legs in every
    position (= every set of projector rows that is kept), with and without the K12 outputs (the torques must not notice);
  * Fr_des on / outside the friction pyramid with 1, 2, 3 and 4 stance feet: the active-set QP behind S_e^-1 and the constraint normals, with working
    sets that grow and shrink;
  * a straight knee on each of the four legs as a swing leg: the eigen-decomposition fallback behind the full-rank guard;
  * one pipelined tick of 96 mixed robots with the 16 patterns in the gait table against the serial tick, bit for bit.
"""
import numpy as np
import pytest

import gpu_helpers as G

pytestmark = pytest.mark.gpu

ROBOTS = ("a1", "lite3")


def pattern(p):
    """Contact flags of pattern p = 0..15: leg l stands when bit l is set."""
    return np.array([(p >> l) & 1 for l in range(4)], np.float32)


def pattern_batch(pkg, per_type=32, h=16):
    """A1 and Lite3 interleaved (type_id = index % 2), pattern = (index within the type) % 16, Fr_des = (1, -2, 30) N on the stance feet."""
    n = 2 * per_type
    parts = [pkg.make_batch(per_type, h, r, seed=601 + k) for k, r in enumerate(ROBOTS)]
    b = dict(parts[0])
    for k in ("mpc_state", "traj", "gait", "fb_state", "wbc_cmd", "prev_ori_vel"):
        b[k] = np.empty((n,) + parts[0][k].shape[1:], parts[0][k].dtype)
        b[k][0::2] = parts[0][k]; b[k][1::2] = parts[1][k]
    b["n"] = n
    for i in range(n):
        pat = pattern((i // 2) % 16)
        b["wbc_cmd"][i, 63:67] = pat
        b["wbc_cmd"][i, 51:63] = (pat[:, None] * np.array([1.0, -2.0, 30.0], np.float32)).reshape(12)
        b["gait"][i] = np.tile(pat, h)
    return b, pkg.shard.interleave_types(n, 2)


def oracle_wbc(oracle, pkg, b, tid=None):
    n = b["n"]
    tau = np.zeros((n, 12)); qdes = np.zeros((n, 12)); qddes = np.zeros((n, 12)); nact = np.zeros(n, int)
    for i in range(n):
        md = pkg.model_desc(ROBOTS[0 if tid is None else int(tid[i])])
        r = oracle.wbc_run(md, b["fb_state"][i].astype(np.float64), b["wbc_cmd"][i].astype(np.float64), b["prev_ori_vel"][i].astype(np.float64), dtype=np.float64)
        assert r["rc"] == 0
        tau[i], qdes[i], qddes[i], nact[i] = r["tau"], r["qdes"], r["qddes"], r["qp"]["n_active"]
    return tau, qdes, qddes, nact


def setup_mixed(ctx, pkg, h):
    for t, r in enumerate(ROBOTS):
        ctx.mpc_setup_packed(t, pkg.mpc_cfg(r), h); ctx.wbc_setup_packed(t, pkg.model_desc(r))


def test_all_contact_patterns_a1_and_lite3(gpu_ctx, pkg, oracle):
    setup_mixed(gpu_ctx, pkg, 16)
    try:
        b, tid = pattern_batch(pkg)
        out = G.run_wbc(gpu_ctx, pkg, b, type_id=tid)
        tau_only = G.run_wbc(gpu_ctx, pkg, b, type_id=tid, want_qdes=False)
    finally:
        G.setup_a1(gpu_ctx, pkg, 10)
    tau64, qd64, qdd64, _ = oracle_wbc(oracle, pkg, b, tid)
    e_tau = np.abs(out["tau"] - tau64) / np.maximum(1.0, np.abs(tau64))
    print("patterns: max torque error / max(1, |tau|) %.3e, q_des %.3e, qd_des %.3e" % (e_tau.max(), np.abs(out["qdes"] - qd64).max(), np.abs(out["qddes"] - qdd64).max()))
    assert np.all(out["status"] == 0), np.unique(out["status"])
    assert np.all(tau_only["status"] == 0), np.unique(tau_only["status"])
    assert np.all(e_tau <= 1e-6), (int(e_tau.max(1).argmax()), e_tau.max())
    assert np.abs(out["qdes"] - qd64).max() <= 1e-5
    assert np.abs(out["qddes"] - qdd64).max() <= 1e-4
    assert np.array_equal(out["tau"], tau_only["tau"])                  # the torque chain does not notice whether K12 runs beside it


def friction_batch(pkg):
    """The friction-active batch of test_wbc_friction_active_and_stateful with 1, 2, 3 and 4 stance feet (robot i: i % 4 + 1 of them, the
    patterns of that count in turn); every stance foot carries a load, so its Fr_des lies on / outside the WBC's pyramid."""
    b = pkg.make_batch(64, 10, "a1", seed=61)
    rng = np.random.default_rng(5)
    cmd = b["wbc_cmd"].copy()
    fr = cmd[:, 51:63].reshape(-1, 4, 3).copy()
    fr[:, :, 2] = np.where(fr[:, :, 2] == 0, np.float32(30.0), fr[:, :, 2])
    fr[:, :, 0] = 0.45 * fr[:, :, 2] * rng.choice([-1, 1], size=fr[:, :, 0].shape)
    fr[:, :, 1] = 0.3 * fr[:, :, 2]
    fr[::4, :, 2] *= 3.0                      # above maxFz for every 4th robot
    by_count = {k: [p for p in range(16) if bin(p).count("1") == k] for k in (1, 2, 3, 4)}
    group = np.zeros(64, int)
    for i in range(64):
        k = i % 4 + 1
        pat = pattern(by_count[k][(i // 4) % len(by_count[k])])
        group[i] = k
        cmd[i, 63:67] = pat
        fr[i] *= pat[:, None]
    cmd[:, 51:63] = fr.reshape(-1, 12)
    b["wbc_cmd"] = cmd
    b["prev_ori_vel"] = rng.uniform(-0.5, 0.5, (64, 3)).astype(np.float32)
    return b, group


def test_friction_active_with_one_to_four_stance_feet(gpu_ctx, pkg, oracle):
    G.setup_a1(gpu_ctx, pkg, 10)
    b, group = friction_batch(pkg)
    out = G.run_wbc(gpu_ctx, pkg, b)
    tau64, qd64, qdd64, nact = oracle_wbc(oracle, pkg, b)
    for k in (1, 2, 3, 4):
        assert nact[group == k].max() > 0, "no active inequality with %d stance feet" % k
    e_tau = np.abs(out["tau"] - tau64) / np.maximum(1.0, np.abs(tau64))
    print("friction: active inequalities per group %s, max torque error %.3e, q_des %.3e, qd_des %.3e"
          % ([int(nact[group == k].max()) for k in (1, 2, 3, 4)], e_tau.max(), np.abs(out["qdes"] - qd64).max(), np.abs(out["qddes"] - qdd64).max()))
    assert np.all(out["status"] == 0), np.unique(out["status"])
    assert np.all(e_tau <= 1e-6), (int(e_tau.max(1).argmax()), e_tau.max())
    assert np.abs(out["qdes"] - qd64).max() <= 1e-5
    assert np.abs(out["qddes"] - qdd64).max() <= 1e-4


def straight_knee_batch(pkg):
    """test_wbc_straight_knee_rank_cut's case on each leg in turn, 8 robots each: the leg and its diagonal partner swing, its knee is straight /
    almost straight, so its foot task is rank deficient."""
    b = pkg.make_batch(32, 10, "a1", seed=81)
    fb = b["fb_state"].copy(); cmd = b["wbc_cmd"].copy()
    for i in range(32):
        leg = i // 8
        fb[i, 13 + 3 * leg + 2] = 0.0 if i % 2 == 0 else 1e-5
        fb[i, 13 + 3 * leg + 1] = 0.3
        pat = np.ones(4, np.float32); pat[leg] = 0; pat[3 - leg] = 0
        cmd[i, 63:67] = pat
        cmd[i, 51:63] = (pat[:, None] * np.array([0.0, 0.0, 60.0], np.float32)).reshape(12)
    b["fb_state"] = fb; b["wbc_cmd"] = cmd
    return b


def test_straight_knee_on_each_leg(gpu_ctx, pkg, oracle):
    G.setup_a1(gpu_ctx, pkg, 10)
    b = straight_knee_batch(pkg)
    out = G.run_wbc(gpu_ctx, pkg, b)
    tau64, qd64, _, _ = oracle_wbc(oracle, pkg, b)
    e_tau = np.abs(out["tau"] - tau64) / np.maximum(1.0, np.abs(tau64))
    print("straight knee: max torque error %.3e, q_des %.3e" % (e_tau.max(), np.abs(out["qdes"] - qd64).max()))
    assert np.all(out["status"] == 0), np.unique(out["status"])
    assert np.all(e_tau <= 1e-5), (int(e_tau.max(1).argmax()), e_tau.max())
    assert np.abs(out["qdes"] - qd64).max() <= 1e-4


def test_pipelined_tick_of_the_patterns_is_the_serial_tick(pkg):
    """One tick of 96 mixed robots, the 16 patterns in the gait table and in the WBC's contact flags, K12 and the K14 tail on: the pipelined
    tick (the relaxation QP waits for its robot's forces behind wbc_qp_setup) gives the serial tick's bits in every output array."""
    h, n = 10, 96
    b, tid = pattern_batch(pkg, per_type=n // 2, h=h)
    S = pkg.to_soa
    outs = {}
    for piped in (False, True):
        ctx = pkg.Context(0, 1024, 16)            # contexts of their own: the same (empty) history on both sides
        try:
            setup_mixed(ctx, pkg, h)
            ctx.set_tick_pipeline(piped)
            ctx.set_torque_epilogue(hip_comp=True, clip=True)
            d = dict(state=ctx.alloc((28, n)).upload(S(b["mpc_state"])), traj=ctx.alloc((12 * h, n)).upload(S(b["traj"])),
                     gait=ctx.alloc((4 * h, n)).upload(S(b["gait"])), fb=ctx.alloc((37, n)).upload(S(b["fb_state"])),
                     cmd=ctx.alloc((67, n)).upload(S(b["wbc_cmd"])), prev=ctx.alloc((3, n)).upload(S(b["prev_ori_vel"])),
                     force=ctx.alloc((12, n)).upload(np.full((12, n), np.nan, np.float32)), tau=ctx.alloc((12, n)).upload(np.full((12, n), np.nan, np.float32)),
                     qdes=ctx.alloc((24, n)).upload(np.full((24, n), np.nan, np.float32)), status=ctx.alloc((n,), np.int32).upload(np.full((n,), 0x7f0000ff, np.int32)),
                     tid=ctx.alloc((n,), np.int32).upload(tid))
            ctx.tick_batch(n, d["state"], d["traj"], d["gait"], d["fb"], d["cmd"], d["prev"], d["force"], d["tau"], d["status"], d["tid"], qdes=d["qdes"])
            ctx.sync()
            outs[piped] = {k: d[k].download().copy() for k in ("force", "tau", "status", "qdes", "prev")}
            for v in d.values():
                v.free()
        finally:
            ctx.close()
    for k in ("force", "tau", "status", "qdes", "prev"):
        assert outs[False][k].tobytes() == outs[True][k].tobytes(), k
    assert np.all(G.flags(outs[True]["status"]) & 0x02000000 == 0)              # nobody timed out waiting for its forces
    assert np.all(np.isfinite(outs[True]["tau"])) and np.all(np.isfinite(outs[True]["qdes"]))
