"""CPU: tests/ground_ref.py (plane by an SVD least-squares solve, control frame from the heading, in float64) against the properties the ground fit
must have, and oracle/qr_oracle_ground.cpp against ground_ref on every tick of every robot of ground_ref.FAMILIES at the project's 1e-6."""
import numpy as np
import pytest

import ground_ref as R
import stage_ref as SR


@pytest.mark.parametrize("name", R.FAMILIES)
def test_oracle_is_the_model_on_every_tick(oracle, name):
    x, want, _ = R.expected(name)
    got = np.stack([oracle.ground_run(x[:, r]) for r in range(R.N_ROBOTS)])
    worst, ratio = R.check(name, got, "oracle")
    print("%-10s oracle against model: worst %.3e, fired %d robot-ticks, collinear excess ratio %.3e" % (name, worst, int(want[:, :, 31].sum()), ratio))
    assert want[:, :, 31].sum() > 5 * R.N_ROBOTS


def test_gating_and_contact_memory():
    """The fit fires with all four feet down and at least one newly so; the memory advances on ticks that do not fire."""
    x = R.family("sequences")[:6, 0].copy()
    pattern = [(1, 1, 1, 0), (0, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 1, 1)]
    x[:, 0:4] = pattern
    out, _ = R.run(x)
    assert list(out[:, 31]) == [0, 0, 1, 0, 0, 1]
    assert np.all(out[:2, 0:3] == 0) and np.all(out[:2, 3:6] == (0, 0, 1)) and np.all(out[:2, 6:9] == 0)        # as Reset() left them
    assert np.array_equal(out[3, :22], out[2, :22]) and not np.array_equal(out[5, 0:3], out[2, 0:3])          # held between fits
    # had the memory stood still on tick 1, leg 3 would still be "new" on tick 3 and it would fire
    x[:, 0:4] = [(1, 1, 1, 0), (1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1)]
    assert list(R.run(x)[0][:, 31]) == [0, 0, 1, 0, 0, 0]


def test_plane_and_normal():
    x, want, _ = R.expected("coplanar")
    for r in range(R.N_ROBOTS):
        for k in np.nonzero(want[r, :, 31])[0]:
            feet = x[k, r, 4:16].astype(np.float64).reshape(4, 3)
            W = np.column_stack([np.ones(4), feet[:, :2]])
            a, n = want[r, k, 0:3], want[r, k, 3:6]
            res = W @ a - feet[:, 2]
            assert np.abs(W.T @ res).max() < 1e-12                                   # the least-squares condition, whatever the feet
            if r % 3 == 0:
                assert np.abs(res).max() < 1e-7                                      # four coplanar feet: their plane (float32 inputs)
            if r % 3 == 1:
                assert 0.005 < np.abs(res).max() < 0.03                              # one foot 3 cm off: no plane holds all four
            assert abs(np.linalg.norm(n) - 1) < 1e-12 and n[2] > 0
            assert abs(n @ (1, 0, a[1])) < 1e-12 and abs(n @ (0, 1, a[2])) < 1e-12   # normal to both tangents of the plane


def test_control_frame():
    for name in ("sequences", "tilt"):
        x, want, _ = R.expected(name)
        o = want.reshape(-1, 32)
        Rg = o[:, 13:22].reshape(-1, 3, 3)
        assert np.all(o[:, 6] == 0) and np.all(o[:, 7] == 0)                         # roll forced to 0; flat world: no pitch either
        assert np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.all(Rg[:, 2, 2] == 1)
        assert np.abs(SR.quat_to_rot_raw(o[:, 9:13]) - Rg).max() < 1e-12             # the quaternion is the matrix's
        Rb = SR.quat_to_rot_raw(x.transpose(1, 0, 2).reshape(-1, 23)[:, 19:23].astype(np.float64))
        assert np.abs(Rg @ o[:, 22:31].reshape(-1, 3, 3) - Rb).max() < 1e-12         # baseRInControlFrame = groundRMat^T baseRMat
    # a fit from rest: yaw = 0.8 x heading of the base x-axis' horizontal projection
    x, want, _ = R.expected("tilt")
    for r in range(R.N_ROBOTS):
        k = int(np.argmax(want[r, :, 31]))
        Rb = SR.quat_to_rot_raw(x[k, r, 19:23].astype(np.float64))
        assert want[r, k, 8] == 0.8 * np.arctan2(Rb[1, 0], Rb[0, 0])


def test_filtered_heading_swings_through_zero_across_the_seam():
    """The reference filters the raw angles: when the heading jumps from +pi to -pi the filtered yaw passes through small values on its way,
    and the frame turns through the robot's back.  The model does the same."""
    x, want, _ = R.expected("seam")
    swung = 0
    for r in range(R.N_ROBOTS):
        fired = np.nonzero(want[r, :, 31])[0]
        raw = np.array([R.heading(SR.quat_to_rot_raw(x[k, r, 19:23].astype(np.float64))) for k in fired])
        yaw = want[r, fired, 8]
        jump = np.nonzero(np.abs(np.diff(raw)) > 6)[0]
        if jump.size != 1:                                                             # (a robot whose fits all fell on one side of the crossing)
            continue
        j = jump[0] + 1
        assert np.all(np.abs(raw) > 2.4) and abs(yaw[j]) < 0.7 * np.pi                 # the heading never left the seam; the filtered yaw did
        assert yaw[j] == 0.2 * yaw[j - 1] + 0.8 * raw[j]
        swung += 1
    assert swung > 0.8 * R.N_ROBOTS


def test_a_vertical_x_axis_puts_a_nan_into_the_frame_for_good(oracle):
    """ComputeControlFrame normalises the horizontal projection of the base x-axis.  Within 1e-3 of vertical that is still a heading; at exactly
    vertical (quaternion (1, -1, 1, 1) / 2, exact in float32) it is 0 / 0: pitch and yaw of controlFrameRPY become NaN and stay NaN through the
    0.2 / 0.8 filter on every later tick, roll is forced back to 0, the plane and the normal are untouched."""
    x, want, _ = R.expected("vertical")
    got = np.stack([oracle.ground_run(x[:, r]) for r in range(R.N_ROBOTS)]).astype(np.float64)
    for o in (want, got):
        assert not np.isnan(o[1:]).any()                                             # 1e-6 .. 1e-3 from vertical: a heading
        first = int(np.argmax(o[0, 30:, 31])) + 30
        assert not np.isnan(o[0, :first]).any()
        assert np.isnan(o[0, first:, 7:9]).all() and np.isnan(o[0, first:, 9:31]).all()
        assert not np.isnan(o[0, first:, 0:7]).any() and np.all(o[0, first:, 6] == 0)
    x2 = x[:, 0].copy(); x2[45:, 19:23] = (1, 0, 0, 0)                              # the robot rights itself: the frame does not come back
    assert np.isnan(R.run(x2)[0][45:, 8]).all() and np.isnan(oracle.ground_run(x2)[45:, 8]).all()
