"""TEST INFRASTRUCTURE -- the ground fit and the control frame in float64, in another formulation than oracle/qr_oracle_ground.cpp and
qr_ground_kernel (qrGroundSurfaceEstimator::Update / GetNormalVector / ComputeControlFrame, quadruped/src/estimators/
qr_ground_surface_estimator.cpp:40-70, 151-206):

  * the plane z = a0 + a1 x + a2 y through the four feet by numpy.linalg.lstsq on [1 x y] (an SVD solve: no normal equations, no cofactor inverse);
  * the normal from the plane's gradient, (-a1, -a2, 1) / |.|;
  * the control frame under the reference's flat-world assignment (nInWorldFrame := (0, 0, 1)): its cross products reduce to the heading of the
    base x-axis' horizontal projection, psi = atan2(R10, R00) of the raw float32 quaternion's rotation (stage_ref.quat_to_rot_raw).  The
    reference normalises that projection, so a projection of exactly (0, 0) is 0 / 0 there: the model returns NaN for it, where atan2 would say 0;
  * a first-order filter 0.2 / 0.8 on the raw angles -- no unwrapping: across +-pi the filtered yaw swings through 0 -- with roll forced to 0;
    a NaN that enters stays (0.2 * NaN);
  * groundRMat = Rz(yaw) Ry(pitch) of the filtered angles, the quaternion of the same, baseRInControlFrame = groundRMat^T baseRMat;
  * gating: the fit fires on a tick with all four feet down and at least one of them newly so; lastContactState advances on every tick.
"""
import numpy as np

import gpu_helpers as G
import stage_ref as SR

N_ROBOTS, TICKS = 65, 60
FAMILIES = ("sequences", "seam", "tilt", "coplanar", "collinear", "vertical")
BAR = 1e-6
# nearly-collinear feet: forward-error bound of the normal equations the reference solves, c * kappa2(W)^2 * 2^-53 * |a|, plus the float32 output
# rounding (one spacing of the coefficient).  c = 4 x the worst measured ratio of (|a_oracle - a_model| less half a float32 spacing) to
# kappa2^2 2^-53 |a| on the CPU over the family.  That measurement is 0 (LAB_NOTES A.19): down to a lateral spread of 1 mm (kappa2 2 173, the unit
# at most 2.7e-8 beside a float32 spacing of 3.8e-6 at |a| = 58) the oracle's float32 outputs are the model's correctly rounded, so the bar is
# the output rounding alone.  The family stops where the bound would pass 1e-4; down to 1 mm it never does.
COLLINEAR_C = 4 * 0.0
COLLINEAR_CUT = 1e-4


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])


def heading(Rb):
    x0, x1 = Rb[0, 0], Rb[1, 0]
    return np.nan if (x0 == 0 and x1 == 0) else np.arctan2(x1, x0)


class GroundEstimator:
    def __init__(self):
        self.a = np.zeros(3); self.n = np.array([0.0, 0.0, 1.0]); self.rpy = np.zeros(3)
        self.lastContactState = np.zeros(4, bool)
        self.kappa = 0.0

    def Update(self, in23):
        """-> out [32] float64: a[3], n[3], controlFrameRPY[3], controlFrameOrientation[4] (wxyz), groundRMat[9], baseRInControlFrame[9], fired"""
        x = np.asarray(in23, np.float32).astype(np.float64)
        contact = x[0:4] != 0
        fire = bool(contact.all() and (contact & ~self.lastContactState).any())
        self.lastContactState = contact.copy()
        Rb = SR.quat_to_rot_raw(x[19:23])
        if fire:
            feet = x[4:16].reshape(4, 3)
            W = np.column_stack([np.ones(4), feet[:, 0], feet[:, 1]])
            self.a, _, _, sv = np.linalg.lstsq(W, feet[:, 2], rcond=None)
            self.kappa = sv[0] / sv[-1]
            g = np.array([-self.a[1], -self.a[2], 1.0])
            self.n = g / np.linalg.norm(g)
            psi = heading(Rb)
            # flat world: raw roll and pitch of the frame are zero -- unless the frame itself is 0 / 0, which makes all of it NaN (roll is
            # then forced back to 0, pitch and yaw are not)
            new = np.array([0.0, 0.0 * psi, psi])
            self.rpy = 0.2 * self.rpy + 0.8 * new
            self.rpy[0] = 0.0
        Rg = rot_z(self.rpy[2]) @ rot_y(self.rpy[1])
        if np.isnan(self.rpy).any():
            Rg = np.full((3, 3), np.nan)          # the reference multiplies three full matrices: 0 * NaN reaches the entries a closed form keeps
        hy, hp = self.rpy[2] / 2, self.rpy[1] / 2
        q = np.array([np.cos(hy) * np.cos(hp), -np.sin(hy) * np.sin(hp), np.cos(hy) * np.sin(hp), np.sin(hy) * np.cos(hp)])
        # q and -q are one rotation; the reference's matrix-to-quaternion picks w > 0 for a positive trace, else the component of the largest
        # diagonal entry positive
        lead = 0 if np.trace(Rg) > 0 else 1 + int(np.argmax(np.diag(Rg)))
        if q[lead] < 0:
            q = -q
        return np.concatenate([self.a, self.n, self.rpy, q, Rg.reshape(9), (Rg.T @ Rb).reshape(9), [float(fire)]])


def run(in_seq):
    """One robot from Reset(): in_seq [T][23] -> out [T][32], kappa2(W) of the last fit before each tick's output [T]"""
    g = GroundEstimator()
    out = np.zeros((len(in_seq), 32)); kap = np.zeros(len(in_seq))
    for k, x in enumerate(in_seq):
        out[k] = g.Update(x); kap[k] = g.kappa
    return out, kap


def _quat(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], -1)


def family(name, n=N_ROBOTS, T=TICKS):
    """-> in [T][n][23] float32"""
    seed = 0x6D00 + FAMILIES.index(name)
    rng = np.random.default_rng(seed)
    x = G.ground_sequences(n, T, seed)
    feet = x[:, :, 4:16].reshape(T, n, 4, 3).copy()
    if name == "seam":
        # headings that cross +pi upwards and -pi downwards, slowly
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        yaw = sign * (np.pi - 0.15) + sign * np.cumsum(rng.uniform(0.0, 0.02, (T, n)), 0)
        x[:, :, 19:23] = _quat(rng.uniform(-0.1, 0.1, (T, n)), rng.uniform(-0.1, 0.1, (T, n)), yaw)
    elif name == "tilt":
        q = _quat(rng.uniform(-1.2, 1.2, (T, n)), rng.uniform(-1.2, 1.2, (T, n)), rng.uniform(-3.1, 3.1, (T, n)))
        x[:, :, 19:23] = q * rng.uniform(0.98, 1.02, (T, n, 1))            # raw, not normalised
    elif name == "coplanar":
        # robot i % 3: 0 = four feet exactly on a plane (as float32 allows), 1 = three on it and one 3 cm off, 2 = as generated
        plane = np.stack([rng.uniform(-0.35, -0.2, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
        z = plane[:, 0, None] + plane[:, 1, None] * feet[..., 0] + plane[:, 2, None] * feet[..., 1]
        for r in range(n):
            if r % 3 != 2:
                feet[:, r, :, 2] = z[:, r]
            if r % 3 == 1:
                feet[:, r, 3, 2] += 0.03
    elif name == "collinear":
        # lateral spread from 0.26 m down: the feet close in on the line y = 0
        spread = np.geomspace(0.26, 1e-3, n)
        side = np.array([-1, 1, -1, 1.0])
        feet[..., 1] = 0.5 * spread[None, :, None] * side + rng.uniform(-0.05, 0.05, (T, n, 4)) * spread[None, :, None]
        x[:, :, 0:4] = 1; x[::2, :, 0] = 0                                  # fires every other tick
    elif name == "vertical":
        # base x-axis within 1e-3 of vertical, up and down; robot 0 at exactly vertical from tick 30 on (quaternion (1, -1, 1, 1) / 2)
        d = np.geomspace(1e-6, 1e-3, n)[None, :] * rng.uniform(0.5, 1.0, (T, n))
        pitch = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (np.pi / 2 - d)
        x[:, :, 19:23] = _quat(rng.uniform(-0.2, 0.2, (T, n)), pitch, rng.uniform(-3, 3, (T, n)))
        x[30:, 0, 19:23] = (0.5, -0.5, 0.5, 0.5)
        x[:, 0, 0:4] = 1; x[::2, 0, 1] = 0
    elif name != "sequences":
        raise KeyError(name)
    x[:, :, 4:16] = feet.reshape(T, n, 12)
    return x


_cache = {}


def expected(name):
    """-> (in [T][n][23], out [n][T][32], kappa [n][T]); computed once and shared, nobody writes into it"""
    if name not in _cache:
        x = family(name)
        runs = [run(x[:, r]) for r in range(x.shape[1])]
        _cache[name] = (x, np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]))
    return _cache[name]


def check(name, got, where=""):
    """got [n][T][32] (oracle or kernel) against the model: the same ticks fire, the same entries are NaN, 1e-6 on every output -- except the
    plane coefficients of the collinear family, which get the normal-equation bound, and only where that bound is below COLLINEAR_CUT.
    -> worst |got - model| over what was compared at 1e-6; on the collinear coefficients the worst ratio of the error beyond half a float32 spacing
    to kappa2^2 2^-53 |a| (the measurement COLLINEAR_C comes from)"""
    x, want, kap = expected(name)
    got = np.asarray(got, np.float64)
    assert np.array_equal(got[:, :, 31], want[:, :, 31]), (name, where)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, where)
    err = np.abs(got[:, :, :31] - want[:, :, :31])
    err[np.isnan(err)] = 0
    ratio = 0.0
    if name == "collinear":
        norm_a = np.linalg.norm(want[:, :, 0:3], axis=2)
        bound = COLLINEAR_C * kap ** 2 * 2.0 ** -53 * norm_a
        bar = bound + np.spacing(np.abs(want[:, :, 0:3]).astype(np.float32)).max(axis=2)
        keep = (bound < COLLINEAR_CUT) & (kap > 0)
        assert keep.any(axis=1).sum() > N_ROBOTS // 2, (name, where)          # the cut leaves most of the family
        ea = err[:, :, 0:3].max(axis=2)
        assert np.all(ea[keep] <= np.maximum(bar, BAR)[keep]), (name, where, (ea / np.maximum(bar, BAR))[keep].max())
        half = 0.5 * np.spacing(np.abs(want[:, :, 0:3]).astype(np.float32)).astype(np.float64)
        excess = np.maximum(err[:, :, 0:3] - half, 0).max(axis=2)
        ratio = float((excess[keep] / (kap ** 2 * 2.0 ** -53 * norm_a)[keep]).max())
        err[:, :, 0:3] = 0                                                     # judged above; everything else at the project's bar
    assert err.max() < BAR, (name, where, np.unravel_index(err.argmax(), err.shape), err.max())
    return float(err.max()), ratio
