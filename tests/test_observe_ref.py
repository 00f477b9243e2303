"""CPU: the numpy restatement of the sensor stage (tests/observe_ref.py) against itself -- that its streams show what the other tests rely on, that no
discontinuous comparison of any robot at any tick lies near its threshold, the filter's closed forms, the noise's contract, and the distance between
its float32 and its float64 run, which is the yardstick of the rows behind a transcendental function in test_observe_host.py and
test_gpu_observe.py (bar = max(8 x gap, 2e-6))."""
import numpy as np

import observe_ref as OR

f32, f64 = np.float32, np.float64


def test_the_streams_cover_what_they_claim():
    raw, kind = OR.streams(OR.N_REF)
    T, n = raw.shape[:2]
    assert T >= 45 and n == OR.N_REF and T - 20 >= 2                         # the window of 20 evicts more than once, the windows of 5 many times
    assert all((kind == k).sum() >= n // 4 for k in OR.YAW_KINDS)
    ref = {c: OR.reference(c) for c in OR.CASES}
    # the raw yaw of the ramps wraps once, of the robots that swing across +-pi several times in both directions
    yaw = OR.quat_to_rpy(raw.reshape(T * n, 41)[:, 6:10], f32)[:, 2].reshape(T, n).astype(f64)
    wraps_down, wraps_up = (np.diff(yaw, axis=0) < -np.pi), (np.diff(yaw, axis=0) > np.pi)
    assert np.all(wraps_down[:, kind == "up"].sum(0) == 1) and not wraps_up[:, kind == "up"].any()
    assert np.all(wraps_up[:, kind == "down"].sum(0) == 1) and not wraps_down[:, kind == "down"].any()
    assert np.all(wraps_down[:, kind == "across"].sum(0) >= 2) and np.all(wraps_up[:, kind == "across"].sum(0) >= 2)
    assert not (wraps_up | wraps_down)[:, kind == "level"].any()
    # the rpy filter's Reset fires on every sim case, for every robot that wraps, and never for a level one at a small offset
    for c in ("sim", "sim_far_neg", "sim_far_pos"):
        cleared = ref[c]["cleared"][1:]
        assert np.all(cleared[:, kind != "level"].sum(0) >= 1), c
        assert ref[c]["neumaier_taken"]["rpy"].min() > 100, c
    assert not ref["sim"]["cleared"][1:, kind == "level"].any() and not ref["hardware"]["cleared"].any()
    # both branches of both folds: the calibrated yaw's over the cases, the averaged yaw's under the offsets beyond 2 pi
    f1 = np.concatenate([ref[c]["fold1"].ravel() for c in OR.CASES]); f2 = np.concatenate([ref[c]["fold2"].ravel() for c in OR.CASES])
    assert (f1 > 0).sum() > 100 and (f1 < 0).sum() > 100 and (f1 == 0).sum() > 100
    assert (f2 > 0).sum() > 100 and (f2 < 0).sum() > 100
    assert (ref["sim_far_neg"]["fold2"] > 0).any() and (ref["sim_far_pos"]["fold2"] < 0).any() and not ref["sim"]["fold2"].any()
    # rpyToQuat leaves through more than one branch of rotationMatrixToQuaternion
    assert all((np.bincount(ref[c]["quat_branch"].ravel(), minlength=4) > 0).sum() >= 2 for c in OR.CASES)
    # both branches of NeumaierSum on every filter that runs
    for c, names in (("sim", ("acc", "gyro", "rpy")), ("hardware", ("acc", "gyro", "qd"))):
        for k in names:
            assert ref[c]["neumaier_taken"][k].min() > 1000, (c, k, ref[c]["neumaier_taken"][k])
    assert ref["hardware"]["neumaier_taken"]["rpy"].sum() == 0 and ref["sim"]["neumaier_taken"]["qd"].sum() == 0
    # sign-alternating samples over seven decades; contacts toggle on every leg of nearly every robot, robot 0 stands; the wide joints' edge rows
    acc = raw[:, :, 0:3].astype(f64)
    assert np.all(np.sign(acc[1:]) == -np.sign(acc[:-1])) and np.abs(acc).max() / np.abs(acc).min() > 1e6
    ct = raw[:, :, 13:17]
    assert set(np.unique(ct)) == {0.0, 1.0} and (np.abs(np.diff(ct, axis=0)).sum(0) >= 2).mean() > 0.95 and np.all(ct[:, 0] == 1.0)
    assert np.all(raw[0, 0, 29:41] == 0) and np.all(raw[0, 2, 17:29:3] == 0) and np.allclose(raw[0, 3, 19:29:3], -np.pi / 2)
    assert raw[:, :, 17:29].min() < -2.5 and raw[:, :, 17:29].max() > 2.4 and np.abs(raw[:, :, 29:41]).max() > 14.0


def test_no_comparison_lies_near_its_threshold():
    """The two folds and the pi jump test, every tick of every robot of every case: at least 1e-4 rad from the threshold, so that an ulp of atan2f
    cannot flip a branch (another seed of observe_ref.streams otherwise)."""
    for c, d in OR.CASES.items():
        o = OR.reference(c)
        m = dict(calibrated=np.abs(np.abs(o["cy_pre"]) - OR.M_PI).min())
        if d["filter_rpy"]:
            m.update(jump=np.abs(o["jump"][1:] - OR.M_PI).min(), averaged=np.abs(np.abs(o["avg_pre"]) - OR.M_PI).min())
        print("%-12s nearest to a threshold: %s" % (c, {k: "%.2e" % v for k, v in m.items()}))
        assert min(m.values()) >= 1e-4, (c, m)
        # ... and the float64 run takes the same branches
        o64 = OR.reference(c, f64)
        for k in ("cleared", "fold1", "fold2", "quat_branch"):
            assert np.array_equal(o[k], o64[k]), (c, k)


def test_a_constant_input_gives_itself():
    rng = np.random.default_rng(5)
    for dt, eps in ((f32, 2.0 ** -23), (f64, 2.0 ** -52)):
        for D, W in ((3, 5), (12, 20)):
            c = rng.uniform(-50, 50, (7, D)).astype(dt); c[0] = 0.375; c[1] = -1024.0
            f = OR.MovingWindowFilter(7, D, W, dt)
            for k in range(3 * W):
                out = f.CalculateAverage(c)
                assert out.dtype == dt and np.all(np.abs(out - c) <= eps * np.abs(c)), (dt, W, k)
                assert np.array_equal(out[:2], c[:2])                        # dyadic constants: exactly
    # through run(): a robot at rest reads its own accelerometer, gyro and attitude back
    raw = np.zeros((12, 2, 41), f32); raw[:, :, 0:3] = (0.5, -0.25, 9.8125); raw[:, :, 6] = 1.0; raw[:, :, 10:13] = (0.125, 0.0, -2.0)
    o = OR.run(raw, OR.desc("sim"))
    assert np.array_equal(o["est"][:, :, 3:6], raw[:, :, 0:3]) and np.array_equal(o["est"][:, :, 10:13], raw[:, :, 10:13])
    assert np.array_equal(o["est"][:, :, 6:10], raw[:, :, 6:10]) and not o["rpy"].any()
    assert np.array_equal(o["tick"][:, 0], 2 * np.arange(1, 13))


def test_a_full_window_is_the_plain_mean():
    rng = np.random.default_rng(6)
    x = rng.uniform(-20, 20, (40, 9, 3)).astype(f32)
    f = OR.MovingWindowFilter(9, 3, 5, f32)
    for k in range(40):
        out = f.CalculateAverage(x[k])
        w = x[max(0, k - 4):k + 1].astype(f64)
        assert np.array_equal(f.length, np.full(9, min(k + 1, 5)))
        # float rounding: the compensated sum is good to an ulp of the sum, the quotient to an ulp of itself
        assert np.all(np.abs(out - w.mean(0)) <= 2.0 ** -22 * np.abs(w).sum(0) / len(w)), k


def test_a_filter_after_reset_is_a_fresh_one():
    rng = np.random.default_rng(7)
    a, b = rng.normal(0, 30, (13, 4, 3)).astype(f32), rng.normal(0, 30, (17, 4, 3)).astype(f32)
    used, fresh = OR.MovingWindowFilter(4, 3, 5, f32), OR.MovingWindowFilter(4, 3, 5, f32)
    for v in a:
        used.CalculateAverage(v)
    used.Reset(np.ones(4, bool))
    for v in b:
        assert np.array_equal(used.CalculateAverage(v).view(np.uint32), fresh.CalculateAverage(v).view(np.uint32))
    # a robot reset in the middle of a run is, from there on, the robot of a run started there (same inputs, same loop counts)
    raw, _ = OR.streams(OR.N_REF)
    d = dict(OR.CASES["hardware"], **OR.NOISE)
    k = 23
    resets = np.zeros(raw.shape[:2], bool); resets[k, 1::2] = True
    whole, tail = OR.run(raw, d, resets=resets), OR.run(raw[k:], d, steps=np.arange(k, raw.shape[0]))
    for key in ("est", "rpy", "gin", "tick", "state", "count"):
        assert np.array_equal(whole[key][k:, 1::2], tail[key][:, 1::2]), key
    assert not np.array_equal(whole["est"][k:, 0::2], tail["est"][:, 0::2])


def test_the_noise_depends_on_seed_robot_and_step_alone():
    raw, _ = OR.streams(OR.N_REF)
    d = dict(OR.CASES["sim"], **OR.NOISE)
    full = OR.reference("sim", f32, True)
    clean = OR.reference("sim", f32, False)
    # not on n: the first 7 robots alone; not on the history: the same loop counts in a run started later
    few = OR.run(raw[:, :7], d)
    late = OR.run(raw[9:], d, steps=np.arange(9, raw.shape[0]))
    for rows in (slice(0, 3), slice(17, 29)):
        assert np.array_equal(few["est"][:, :, rows], full["est"][:, :7, rows]) and np.array_equal(late["est"][:, :, rows], full["est"][9:, :, rows])
    # the drawn values: amplitude * s with s a multiple of 2^-23 in [-1, 1), exact in float32; the sum is one float32 addition
    for t in (0, 31):
        s = OR.noise_of(d, OR.N_REF, t)
        assert s.shape == (OR.N_REF, 8, 4) and np.array_equal(s.astype(f32).astype(f64), s) and s.min() >= -1 and s.max() < 1 and np.all(s * 2 ** 23 == np.round(s * 2 ** 23))
        assert np.array_equal(full["est"][t, :, 0:3], clean["est"][t, :, 0:3] + f32(d["acc_noise"]) * s[:, 0, 0:3].astype(f32))
        assert np.array_equal(full["est"][t, :, 17:29], clean["est"][t, :, 17:29] + f32(d["q_noise"]) * s[:, 2:5].reshape(-1, 12).astype(f32))
        assert np.array_equal(OR.noise_of(d, 5, t, robots=[3, 64, 129, 0, 7]), s[[3, 64, 129, 0, 7]])
    assert abs(np.mean([OR.noise_of(d, OR.N_REF, t).mean() for t in range(8)])) < 0.02
    # another seed, another robot, another step: other words
    w = OR.noise_words(20266, 5, 9)
    assert all(not np.array_equal(w, v) for v in (OR.noise_words(20267, 5, 9), OR.noise_words(20266, 6, 9), OR.noise_words(20266, 5, 10)))
    # an amplitude of 0 leaves the row's bits alone; the attitude carries no noise
    assert np.array_equal(OR.run(raw[:3], dict(d, gyro_noise=0.0))["est"][:, :, 10:13].view(np.uint32), clean["est"][:3, :, 10:13].view(np.uint32))
    assert np.array_equal(full["rpy"], clean["rpy"]) and np.array_equal(full["est"][:, :, 6:10], clean["est"][:, :, 6:10])


def test_the_float32_float64_gap_of_the_reference():
    """Printed per case and output group: the yardstick.  Measured (numpy 2, glibc): rpy 4.0e-7 .. 8.9e-7, quaternion 2.0e-7 .. 4.4e-7, foot
    positions 1.0e-7, the rpy filter's state 4.7e-6 .. 5.0e-6 (0 on the hardware class, which does not run it), the previous yaw as rpy."""
    for c in OR.CASES:
        g, b = OR.gaps(c), OR.bars(c)
        print("%-12s " % c + "  ".join("%s gap %.2e bar %.2e" % (k, g[k], b[k]) for k in g))
        assert all(np.isfinite(v) and v < 1e-4 for v in g.values()), (c, g)
        assert all(b[k] >= OR.FLOOR and b[k] >= 8 * g[k] for k in g)
        assert g["foot"] > 0 and g["rpy"] > 0 and g["quat"] > 0
