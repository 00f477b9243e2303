"""GPU parity of the swing-leg target kernel (qrgpu_swing_targets_batch) against the oracle.
Reference: qrRaibertSwingLegController::GetAction, ADVANCED_TROT case (qr_swing_leg_controller.cpp:362-424).
Bar: trajectory points and world-frame images within 2e-6 m (same fp32 operations); joint targets within 2e-5 rad (acosf / asinf / atan2f
of the device library against libm); legs not flagged as swinging are left untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_swing_targets_parity(gpu_ctx, pkg, oracle):
    W = pkg.workload
    n = 777
    cfg = W.estimator_cfg("a1"); geom, ho = cfg[:3], cfg[7:19]
    x = W.make_swing_batch(n, seed=8)
    S = pkg.to_soa
    sentinel = np.float32(-777.0)
    d_in = gpu_ctx.alloc((58, n)).upload(S(x))
    d_cmd = gpu_ctx.alloc((67, n)).upload(np.full((67, n), sentinel, np.float32))
    d_tgt = gpu_ctx.alloc((12, n)).upload(np.full((12, n), sentinel, np.float32))
    d_q = gpu_ctx.alloc((24, n)).upload(np.full((24, n), sentinel, np.float32))
    gpu_ctx.swing_targets_batch(n, cfg, d_in, d_cmd, d_tgt, d_q)
    gpu_ctx.sync()
    cmd = d_cmd.download().T; tgt = d_tgt.download().T; qd = d_q.download().T
    assert np.all(cmd[:, :15] == sentinel) and np.all(cmd[:, 51:] == sentinel)          # only the foot-task rows are the kernel's
    for i in range(n):
        o = oracle.swing_targets(geom, ho, x[i], np.full(72, sentinel, np.float32))
        g = np.concatenate([cmd[i, 15:51], tgt[i], qd[i]])
        assert np.array_equal(g == sentinel, o == sentinel), i                            # same legs written
        m = o != sentinel
        assert np.abs(g[:48][m[:48]] - o[:48][m[:48]]).max(initial=0) <= 2e-6, i
        # (an unreachable foothold gives NaN angles -> replaced by the current ones, and NaN joint velocities, as in the reference)
        assert np.allclose(g[48:][m[48:]], o[48:][m[48:]], rtol=0, atol=2e-5, equal_nan=True), (i, g[48:60], o[48:60])
    for v in (d_in, d_cmd, d_tgt, d_q):
        v.free()


def test_swing_velocity_mode_parity(gpu_ctx, pkg, oracle):
    """qrgpu_swing_velocity_batch (VELOCITY_LOCOMOTION case, qr_swing_leg_controller.cpp:285-309, 408-424) against the oracle: targets and
    trajectory points within 2e-6 m, joint targets within 2e-5 rad, legs that are not flagged untouched."""
    W = pkg.workload
    n = 700
    cfg = W.estimator_cfg("a1"); geom, ho = cfg[:3], cfg[7:19]
    vd = W.swing_velocity_cfg("a1")
    x = W.make_swing_velocity_batch(n, seed=9)
    sentinel = np.float32(-777.0)
    d_in = gpu_ctx.alloc((53, n)).upload(pkg.to_soa(x))
    d_out = gpu_ctx.alloc((48, n)).upload(np.full((48, n), sentinel, np.float32))
    gpu_ctx.swing_velocity_batch(n, cfg, vd, d_in, d_out)
    gpu_ctx.sync()
    g = d_out.download().T
    written = 0
    for i in range(n):
        o = oracle.swing_velocity(geom, ho, vd, x[i], np.full(48, sentinel, np.float32))
        assert np.array_equal(g[i] == sentinel, o == sentinel), i
        m = o != sentinel
        written += int(m.sum())
        assert np.abs(g[i, :24][m[:24]] - o[:24][m[:24]]).max(initial=0) <= 2e-6, (i, np.abs(g[i, :24] - o[:24]).max())
        assert np.allclose(g[i, 24:][m[24:]], o[24:][m[24:]], rtol=0, atol=2e-5, equal_nan=True), (i, g[i, 24:36], o[24:36])
    assert written > 20 * n
    d_in.free(); d_out.free()


@pytest.mark.parametrize("robot", ["a1", "lite3"])
def test_joint_targets_against_the_model_on_the_ik_domain(gpu_ctx, pkg, robot):
    """d_qdes of qrgpu_swing_targets_batch against tests/stage_ref.py: the model's forward kinematics (float64 chain) of the kernel's joint
    targets lands on the target, |FK64(angles) - p| <= 5e-6 m, for every leg over the wide joint family restricted to |t1 + t2/2| <= 1.4
    (derivation of the bar: stage_ref.check_ik); two unreachable targets give the current angles where the reference's angle is NaN."""
    import stage_ref as SR
    cfg = pkg.workload.estimator_cfg(robot)
    geom, ho = cfg[:3], cfg[7:19]
    q = SR.ik_joints(300, 51)
    xu, cur = SR.unreachable_swing_in(cfg)
    x = np.concatenate([SR.ik_swing_in(cfg, q), xu])
    n = x.shape[0]
    d_in = gpu_ctx.alloc((58, n)).upload(pkg.to_soa(x))
    d_q = gpu_ctx.alloc((24, n)).upload(np.full((24, n), np.nan, np.float32))
    gpu_ctx.swing_targets_batch(n, cfg, d_in, None, None, d_q)
    gpu_ctx.sync()
    ang = d_q.download().T[:, :12]
    assert np.all(np.isfinite(ang))
    SR.check_ik(cfg, x[:-2], ang[:-2])
    print("gpu against stage_ref  %s IK residual %.3e, angle %.3e" % (robot, np.abs(SR.foot_positions(geom, ho, ang[:-2]).reshape(-1, 12) - x[:-2, 12:24]).max(),
                                                                       np.abs(ang[:-2] - q).max()))
    a0, a1 = ang[-2], ang[-1]
    assert np.array_equal(a0[3:6], cur[3:6])                                            # beyond the leg's reach: all three angles fall back
    want = SR.leg_ik(geom, ho, xu[1, 15:18], 1)
    assert np.isnan(want[0]) and np.isnan(want[1])
    assert np.array_equal(a1[3:5], cur[3:5]) and abs(a1[5] - want[2]) <= 2e-6           # inside the hip cylinder: abad and hip fall back, the knee is solved
    for a in (a0, a1):
        assert np.abs(np.delete(a, [3, 4, 5]) - np.delete(np.tile(SR.STAND, 4), [3, 4, 5])).max() <= 2e-5
    d_in.free(); d_q.free()


@pytest.mark.parametrize("robot", ["a1", "lite3"])
def test_velocity_action_against_the_model(gpu_ctx, pkg, robot):
    """qr_swing_velocity_kernel against tests/foothold_ref.py: the Raibert target through baseRInControlFrame 1e-6 m, the trajectory point at the
    warped phase 2e-6 m, joint targets through the model's forward kinematics at 5e-6 m, legs that are not flagged untouched."""
    import foothold_ref as R
    W = pkg.workload
    cfg, vd = W.estimator_cfg(robot), W.swing_velocity_cfg(robot)
    x = R.velocity_family(pkg, robot)
    n = x.shape[0]
    d_in = gpu_ctx.alloc((53, n)).upload(pkg.to_soa(x))
    d_out = gpu_ctx.alloc((48, n)).upload(np.full((48, n), R.SENTINEL, np.float32))
    gpu_ctx.swing_velocity_batch(n, cfg, vd, d_in, d_out)
    gpu_ctx.sync()
    worst = {}
    share = R.check_velocity(cfg, vd, x, d_out.download().T, robot + " kernel", worst)
    print("%s kernel against foothold_ref: tie share %.4f, worst %s" % (robot, share, worst))
    d_in.free(); d_out.free()


@pytest.mark.parametrize("robot", ["a1", "lite3"])
def test_swing_target_trajectory_against_the_model(gpu_ctx, pkg, robot):
    """The trajectory part of qrgpu_swing_targets_batch against the model's generator at phaseModule = false: pFoot_des and the world-frame
    foot targets 2e-6 (relative beyond 1 m), legs that are not flagged untouched.  (Its IK is pinned above.)"""
    import foothold_ref as R
    cfg = pkg.workload.estimator_cfg(robot)
    x = R.targets_family(pkg, robot)
    n = x.shape[0]
    d_in = gpu_ctx.alloc((58, n)).upload(pkg.to_soa(x))
    d_cmd = gpu_ctx.alloc((67, n)).upload(np.full((67, n), R.SENTINEL, np.float32))
    d_tgt = gpu_ctx.alloc((12, n)).upload(np.full((12, n), R.SENTINEL, np.float32))
    gpu_ctx.swing_targets_batch(n, cfg, d_in, d_cmd, d_tgt, None)
    gpu_ctx.sync()
    worst = {}
    R.check_targets(x, np.concatenate([d_cmd.download().T[:, 15:51], d_tgt.download().T], axis=1), robot + " kernel", worst)
    print("%s kernel against foothold_ref: worst %s" % (robot, worst))
    for v in (d_in, d_cmd, d_tgt):
        v.free()
