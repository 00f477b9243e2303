"""The tick on the reference's cadence, restated from the reference's text in numpy -- float64 by default, any dtype on request (the float32
evaluation of the same text gives the tolerance of the comparisons, DESIGN 4.6: 8 x the restatement's own float32-to-float64 gap, never under 2e-6,
relative to max(1, |tau|)).  Nothing here reads the project's kernels or headers.

  MPCStanceLegController::SolveDenseMPC   qr_mpc_stance_leg_controller.cpp:402-409   f_ff.col(leg) = -baseRMat^T f.col(leg); Fr_des[leg] = f.col(leg)
  MPCStanceLegController::UpdateMPC       :337-382                                  re-plan when counter % (iterationsInaMPC / 2) == 0 or counter < 50
  MPCStanceLegController::Run             :305-333                                  allowAfterMPC = !mpcUpdated; ++iterationCounter after the test
  MPCStanceLegController::GetAction       :129-156                                  every tick: MapContactForceToJointTorques(leg, f_ff.col(leg))
  qrRobot::AnalyticalLegJacobian          qr_robot.cpp:148-172                      signedHipLength = hipLength * (-1)^(leg + 1)
  qrRobot::MapContactForceToJointTorques  qr_robot.cpp:241-251                      J^T f
  qrFSMStateLocomotion::Run               qr_fsm_state_locomotion.cpp:130-158       +-0.9 N m on the abads of every leg, WBC when allowAfterMPC, clip
  baseRMat = quaternionToRotationMatrix(q)^T (base -> world) = Eigen's Quaternion(w, x, y, z).toRotationMatrix()

Arrays are robot-major here: quat [n][4] (w, x, y, z), force / hold / tau / q [n][12] (3 * leg + axis or joint)."""
import numpy as np

EPILOGUE_HIP_COMP, EPILOGUE_CLIP = 1, 2
A1_LEGS = (0.08505, 0.2, 0.2)                    # hip, upper, lower link (a1_sim.yaml)
N_POSES, SEED = 384, 0x0CADE


def rotation(quat, dtype=np.float64):
    """base -> world, [n][3][3]"""
    q = np.asarray(quat, dtype)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two = dtype(2)
    R = np.empty((q.shape[0], 3, 3), dtype)
    R[:, 0, 0] = 1 - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - w * z); R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z); R[:, 1, 1] = 1 - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y); R[:, 2, 1] = two * (y * z + w * x); R[:, 2, 2] = 1 - two * (x * x + y * y)
    return R


def hold_from_force(quat, force, dtype=np.float64):
    """f_ff = -baseRMat^T f per leg: [n][12]"""
    R = rotation(quat, dtype)
    f = np.asarray(force, dtype).reshape(-1, 4, 3)
    return (-np.einsum("nki,nlk->nli", R, f)).astype(dtype).reshape(-1, 12)


def leg_jacobian(angles, leg, legs=A1_LEGS, dtype=np.float64):
    """AnalyticalLegJacobian: angles [n][3] -> [n][3][3]"""
    t = np.asarray(angles, dtype)
    hip, lu, ll = (dtype(v) for v in legs)
    sh = hip * dtype((-1) ** (leg + 1))
    t0, t1, t2 = t[:, 0], t[:, 1], t[:, 2]
    lEff = np.sqrt(lu * lu + ll * ll + 2 * lu * ll * np.cos(t2))
    tEff = t1 + t2 / 2
    s0, c0, s2, sE, cE = np.sin(t0), np.cos(t0), np.sin(t2), np.sin(tEff), np.cos(tEff)
    J = np.zeros((t.shape[0], 3, 3), dtype)
    J[:, 0, 1] = -lEff * cE
    J[:, 0, 2] = ll * lu * s2 * sE / lEff - lEff * cE / 2
    J[:, 1, 0] = -sh * s0 + lEff * c0 * cE
    J[:, 1, 1] = -lEff * s0 * sE
    J[:, 1, 2] = -ll * lu * s0 * s2 * cE / lEff - lEff * s0 * sE / 2
    J[:, 2, 0] = sh * c0 + lEff * s0 * cE
    J[:, 2, 1] = lEff * sE * c0
    J[:, 2, 2] = ll * lu * s2 * c0 * cE / lEff + lEff * sE * c0 / 2
    return J.astype(dtype)


def torque(q, hold, legs=A1_LEGS, dtype=np.float64):
    """MapContactForceToJointTorques on all four legs: tau [n][12] = J(q)^T f_ff.  legs: one triple, or [n][3] per robot."""
    q = np.asarray(q, dtype).reshape(-1, 4, 3)
    f = np.asarray(hold, dtype).reshape(-1, 4, 3)
    legs = np.asarray(legs, np.float64)
    tau = np.empty((q.shape[0], 4, 3), dtype)
    for leg in range(4):
        if legs.ndim == 1:
            J = leg_jacobian(q[:, leg], leg, legs, dtype)
        else:
            J = np.concatenate([leg_jacobian(q[r:r + 1, leg], leg, legs[r], dtype) for r in range(q.shape[0])])
        tau[:, leg] = np.einsum("nij,ni->nj", J, f[:, leg])
    return tau.reshape(-1, 12)


def epilogue(tau, comp_legs, flags, dtype=np.float64):
    """The motor-command tail: +-0.9 on the abads of the legs in comp_legs [n][4] (bool; every leg on a tick that re-plans, the legs outside
    contact_state on the others: UpdateLegCMD overwrites the rest), then the +-23 clip."""
    t = np.asarray(tau, dtype).reshape(-1, 4, 3).copy()
    if flags & EPILOGUE_HIP_COMP:
        sign = np.array([-1.0, 1.0, -1.0, 1.0], dtype) * dtype(np.float32(0.9))     # tua_ * pow(-1, (leg + 1) % 2)
        t[:, :, 0] += np.where(np.asarray(comp_legs, bool), sign[None, :], dtype(0))
    if flags & EPILOGUE_CLIP:
        t = np.clip(t, dtype(-23), dtype(23))
    return t.reshape(-1, 12).astype(dtype)


def due(counter, period):
    """UpdateMPC's test on iterationCounter, before Run increments it."""
    counter = np.asarray(counter, np.int64)
    return (counter % period == 0) | (counter < 50)


def period_of(dt_ctrl, dt_mpc):
    """iterationsInaMPC / 2 by integer division, iterationsInaMPC = round(dtMPC / dt)"""
    return int(round(float(np.float32(dt_mpc) / np.float32(dt_ctrl)))) // 2


def due_schedule(counter0, period, ticks):
    """[ticks][n] bool: who re-plans on each of `ticks` consecutive ticks from the counters counter0 [n]."""
    c = np.asarray(counter0, np.int64)
    return np.stack([due(c + t, period) for t in range(ticks)])


class Cadence:
    """The per-tick rule as a state machine over n robots.  A tick takes who is due, what a solve of everybody WOULD return (f [n][12], world frame,
    with the quaternion it read), and the joint angles of now; it returns the MPC-side command of every motor before the WBC's overwrite and says who
    runs the WBC.  Memory: force (Fr_des) and hold (f_ff) of each robot's last solve."""

    def __init__(self, force, hold, legs=A1_LEGS, dtype=np.float64):
        self.dtype, self.legs = dtype, legs
        self.force, self.hold = np.array(force, dtype), np.array(hold, dtype)

    def tick(self, is_due, solved_force, quat, q):
        is_due = np.asarray(is_due, bool)
        self.force[is_due] = np.asarray(solved_force, self.dtype)[is_due]
        self.hold[is_due] = hold_from_force(np.asarray(quat)[is_due], self.force[is_due], self.dtype)
        return torque(q, self.hold, self.legs, self.dtype), ~is_due          # (tau of every motor, allowAfterMPC)


def poses(n=N_POSES, seed=SEED):
    """Random poses for the host check: a tilted, yawed base (quaternion normalised in float64, stored float32), joints over the whole range with a
    share of them within 1e-3 rad of the A1's stops, forces of a trotting robot's size."""
    rng = np.random.default_rng(seed)
    rpy = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), rng.uniform(-np.pi, np.pi, n)], 1)
    cr, sr, cp, sp, cy, sy = (f(rpy[:, k] / 2) for k in range(3) for f in (np.cos, np.sin))
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], 1)
    lo = np.tile([-0.802851, -1.047198, -2.696534], 4); hi = np.tile([0.802851, 4.188790, -0.916298], 4)       # a1_description's joint limits
    q = rng.uniform(lo, hi, (n, 12))
    at_stop = rng.random((n, 12)) < 0.2
    q = np.where(at_stop, np.where(rng.random((n, 12)) < 0.5, lo + rng.uniform(0, 1e-3, (n, 12)), hi - rng.uniform(0, 1e-3, (n, 12))), q)
    force = np.stack([rng.uniform(-25, 25, (n, 4)), rng.uniform(-25, 25, (n, 4)), rng.uniform(0, 120, (n, 4))], 2).reshape(n, 12)
    force[rng.random((n, 4)).repeat(3, 1) < 0.3] = 0.0                                                         # swing legs carry no force
    return dict(quat=quat.astype(np.float32), q=q.astype(np.float32), force=force.astype(np.float32))


def bar(value32, value64, floor=2e-6):
    """8 x the restatement's float32-to-float64 gap on these inputs, relative to max(1, |value|); never under `floor`.  -> (gap, bar)"""
    gap = float((np.abs(np.asarray(value32, np.float64) - value64) / np.maximum(1.0, np.abs(value64))).max())
    return gap, max(8.0 * gap, floor)


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))
