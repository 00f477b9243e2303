"""CPU: tests/foothold_ref.py (swing-leg selection, foothold heuristic, velocity-mode action and the swing trajectories in float64 with vectors
and matrices) against closed forms, its threshold-tie shares, and oracle/qr_oracle_swing.cpp against it on the families of foothold_ref, A1 and
Lite3, at the bars of the existing tests: flags and phases exact, footholds 1e-6 m, trajectory points 2e-6 m, joint targets through the forward
kinematics at 5e-6 m."""
import numpy as np
import pytest

import foothold_ref as R
import stage_ref as SR


def test_trajectory_closed_form():
    rng = np.random.default_rng(1)
    for _ in range(200):
        p0, p1 = rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.3, 0.3, 3)
        apex = max(p0[2], p1[2]) + 0.1
        assert np.allclose(R.trajectory(p0, p1, 0.0), p0, atol=1e-15) and np.allclose(R.trajectory(p0, p1, 1.0), p1, atol=1e-15)
        assert abs(R.trajectory(p0, p1, 0.5)[2] - apex) < 1e-15 and np.allclose(R.trajectory(p0, p1, 0.5)[:2], (p0[:2] + p1[:2]) / 2)
        s = rng.uniform(0, 1, 3)
        z = [R.trajectory(p0, p1, v)[2] for v in s]
        c = np.polyfit([0, 0.5, 1], [p0[2], apex, p1[2]], 2)
        assert np.allclose(z, np.polyval(c, s), atol=1e-12)                       # one parabola
    assert R.warp(0.0) == 0 and abs(R.warp(0.5) - 0.8) < 1e-15 and R.warp(1.0) == 1.0 and abs(R.warp(0.75) - 0.9) < 1e-15
    assert abs(R.warp(0.25) - 0.8 * np.sqrt(0.5)) < 1e-15
    assert abs((R.warp(0.9) - R.warp(0.6)) / 0.3 - 0.4) < 1e-12                    # the second half's slope


def test_raibert_closed_form_level_and_at_rest(pkg):
    """Level base, no rotation rate: the foothold is the hip offset plus the abad link plus command * swingRemainTime - kp (command - v), at the
    height stateDes(2) - clearance below the base; a held leg keeps its foot but for the trim and the 0.02 drop."""
    W = pkg.workload
    desc = W.foothold_cfg("a1"); d = SR.widen(desc)
    x = np.zeros(46, np.float32)
    x[0:4] = R.SWING; x[4:8] = 1; x[8:12] = 0.2; x[12:16] = 0.3; x[16:19] = (0.5, 0.1, 0); x[20] = 0.28; x[33] = 1; x[40:43] = (0.3, 0.0, 0.0)
    flag, phase, ftp, tie = R.footholds(desc, x)
    assert np.all(flag == 1) and np.allclose(phase, 0.3) and not tie.any()
    for leg in range(4):
        want = d[3 * leg:3 * leg + 3] * (1, 1, 0) + (0, d[24] * R.SIDE[leg], 0) + (0.5 * 0.2 - 0.16 * 0.2, 0.1 * 0.2 - 0.16 * 0.1, -(0.28 - 0.01))
        assert np.abs(ftp[leg] - want).max() < 1e-7, (leg, ftp[leg], want)
    x[16] = 5.0                                                                     # 1.0 - 0.16 * 4.7 = 0.248: beyond the clip
    assert np.allclose(R.footholds(desc, x)[2][:, 0], d[0:12:3] + 0.2, atol=1e-7)
    x[4:8] = 0; x[21:33] = d[12:24] + np.tile(np.float32([0.02, 0.03, -0.25]), 4)
    flag, phase, ftp, _ = R.footholds(desc, x)
    assert np.all(phase == 1.0) and np.abs(ftp - (d[12:24].reshape(4, 3) + (0.02, 0.025, -0.27))).max() < 1e-7
    x[0:4] = (R.STANCE, R.EARLY_CONTACT, R.LOSE_CONTACT, R.SWING); x[4:8] = (1, 1, 1, 0)
    assert list(R.footholds(desc, x)[0]) == [0, 0, 1, 1]


@pytest.mark.parametrize("robot", R.ROBOTS)
def test_oracle_is_the_model(pkg, oracle, robot):
    W = pkg.workload
    worst = {}
    desc = W.foothold_cfg(robot)
    x = R.foothold_family(pkg, robot)
    got = np.stack([oracle.footholds(desc, x[i], np.full(58, R.SENTINEL, np.float32)) for i in range(x.shape[0])])
    R.footholds.clipped = 0
    s1 = R.check_footholds(desc, x, got, robot, worst)
    held = (x[:, 4:8] == 0) & (got[:, 0:4] == 1)
    free = int((got[:, 0:4] == 1).sum() - held.sum())
    assert held.sum() > 60 and 0.1 * free < R.footholds.clipped < 0.9 * free        # both branches; the clip active on a share, and not on all
    print("%s: %d planned legs held, %d free, of these %d at the clip" % (robot, held.sum(), free, R.footholds.clipped))
    cfg, vd = W.estimator_cfg(robot), W.swing_velocity_cfg(robot)
    xv = R.velocity_family(pkg, robot)
    gv = np.stack([oracle.swing_velocity(cfg[:3], cfg[7:19], vd, xv[i], np.full(48, R.SENTINEL, np.float32)) for i in range(xv.shape[0])])
    s2 = R.check_velocity(cfg, vd, xv, gv, robot + " velocity", worst)
    xt = R.targets_family(pkg, robot)
    gt = np.stack([oracle.swing_targets(cfg[:3], cfg[7:19], xt[i], np.full(72, R.SENTINEL, np.float32)) for i in range(xt.shape[0])])
    R.check_targets(xt, gt[:, :48], robot + " targets", worst)
    print("%s tie shares: footholds %.4f, velocity %.4f (cap %.3f); worst %s" % (robot, s1, s2, R.TIE_CAP, {k: "%.2e" % v for k, v in worst.items()}))
