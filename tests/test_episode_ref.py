"""CPU: tests/episode_ref.py, the float64 restatement of the episode step that the host build of csrc/qr_episode.h and the GPU kernel are compared
against, pinned on its own: Philox-4x32-10 against the published known-answer vectors of Random123 (kat_vectors: counter 0 key 0; all ones), the
uniforms, the spawn row, the spawned attitude and position on a slope and on flat ground, and the bookkeeping of one call."""
import numpy as np
import pytest

import episode_ref as ER
import terrain_ref as TR


def test_philox_known_answers():
    assert ER.philox((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    ones = 0xffffffff
    assert ER.philox((ones,) * 4, (ones,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # the digits of pi (the third published vector)
    assert ER.philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_uniforms_lie_in_the_half_open_interval():
    w = np.array([0, 1, 255, 256, 0xffffff00, 0xffffffff, 0x80000000], np.uint32)
    u = ER.uniform(w)
    assert u[0] == 0.0 and u[2] == 0.0 and u[3] == 2.0 ** -24 and u[5] == 1.0 - 2.0 ** -24 and u[6] == 0.5
    assert np.all((u >= 0) & (u < 1))
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))            # exact in float
    W = np.stack([ER.words(3, r, e) for r in range(40) for e in range(5)])
    u = ER.uniform(W)
    assert np.all((u >= 0) & (u < 1)) and 0.4 < u.mean() < 0.6
    assert len(np.unique(W)) == W.size                                           # no word repeats across robots, episodes and blocks


def test_the_spawn_row_never_reaches_n_spawn():
    for ns in (1, 2, 7, 1000):
        u = np.array([0.0, 0.5, 1.0 - 2.0 ** -24])
        row = np.minimum(np.floor(u * ns).astype(int), ns - 1)
        assert row.max() == ns - 1 and row.min() == 0
    d = ER.desc(seed=11)
    table = np.zeros((4, 7), np.float32); table[0] = np.arange(7)
    sp = ER.spawn(d, None, 0.0, table, np.arange(300), np.zeros(300, int))
    assert set(sp["row"]) == set(range(7))
    assert np.array_equal(sp["fb"][:, 4], sp["row"].astype(float))


def _plane(pkg, slope):
    g = pkg.terrain.Grid.centred(1.0, 0.125)
    return dict(D=TR.desc(n_fields=1, **g.desc()), height=pkg.terrain.stack([pkg.terrain.plane(g, slope, 0.0)]), fid=None)


def test_spawn_on_a_slope_is_aligned_with_it(pkg):
    th = 0.2
    ground = _plane(pkg, np.tan(th))
    d = ER.desc(align_to_slope=1, xy_jitter=0.2, yaw_jitter=3.0, seed=5)
    table = np.zeros((4, 3), np.float32); table[0] = [-0.3, 0.0, 0.3]; table[1] = [0.1, -0.2, 0.0]; table[2] = [0.0, 1.0, -2.0]
    m = 64
    sp = ER.spawn(d, ground, -0.01, table, np.arange(m), np.arange(m) % 4)
    nrm = np.array([-np.sin(th), 0.0, np.cos(th)])
    assert np.abs(sp["normal"] - nrm).max() < 1e-6                               # (the float32 heights of the plane)
    u = ER.uniform(sp["words"])
    for i in range(m):
        q = sp["fb"][i, 0:4]
        assert abs((q * q).sum() - 1.0) < 1e-14 and q[0] >= 0
        R = ER.quat_to_rot(q)
        assert np.abs(R[:, 2] - sp["normal"][i]).max() < 1e-14                   # the base z axis is the normal
        x0 = table[0, sp["row"][i]] + d["xy_jitter"] * (2 * u[i, 0, 1] - 1); y0 = table[1, sp["row"][i]] + d["xy_jitter"] * (2 * u[i, 0, 2] - 1)
        foot = np.array([x0, y0, sp["ground"][i]])
        assert np.abs(sp["fb"][i, 4:7] - foot - d["spawn_height"] * sp["normal"][i]).max() < 1e-15
        assert abs(foot[2] - (np.tan(th) * x0 - 0.01)) < 1e-6                    # on the plane
        # the heading: the base x axis projected on the ground plane is the yaw direction tilted with the plane
        Rt = ER.quat_to_rot(ER.attitude(sp["normal"][i], 0.0, 1))
        assert np.abs(R[:, 0] - Rt @ [np.cos(sp["yaw"][i]), np.sin(sp["yaw"][i]), 0.0]).max() < 1e-14
    assert np.all(sp["fb"][:, 7:13] == 0) and np.all(sp["fb"][:, 25:37] == 0) and np.all(sp["fb"][:, 13:25] == d["q_spawn"])
    # yaw 0, no jitter: what tools/closed_loop.py sets by hand on a plane, a rotation of -theta about y
    sp0 = ER.spawn(ER.desc(align_to_slope=1), ground, 0.0, np.zeros((4, 1), np.float32), [0], [0])
    assert np.abs(sp0["fb"][0, 0:4] - [np.cos(-0.5 * th), 0.0, np.sin(-0.5 * th), 0.0]).max() < 1e-7
    assert np.abs(sp0["fb"][0, 4:7] - [-0.30 * np.sin(th), 0.0, 0.30 * np.cos(th)]).max() < 1e-7


def test_spawn_on_flat_ground_is_level(pkg):
    d = ER.desc(yaw_jitter=1.0, xy_jitter=0.5, v_jitter=0.3, q_jitter=0.1, align_to_slope=1)
    table = np.zeros((4, 2), np.float32); table[2] = [0.5, -0.5]
    g = pkg.terrain.Grid.centred(1.0, 0.125)
    flat = dict(D=TR.desc(n_fields=1, **g.desc()), height=np.full((1, g.ny, g.nx), 0.07, np.float32), fid=None)
    for ground, z in ((None, -0.02 + d["spawn_height"]), (flat, float(np.float32(0.07)) - 0.02 + d["spawn_height"])):      # (0.30 as float32)
        sp = ER.spawn(d, ground, -0.02, table, np.arange(50), np.arange(50))
        q = sp["fb"][:, 0:4]
        assert np.abs(q[:, 1:3]).max() < 1e-15 and np.all(q[:, 0] >= 0)      # (a constant field: the derivative weights sum to 0 to rounding)
        assert np.abs(2 * np.arctan2(q[:, 3], q[:, 0]) - sp["yaw"]).max() < 1e-14
        assert np.abs(sp["fb"][:, 6] - z).max() < 1e-14
        assert np.all(np.abs(sp["fb"][:, 10:12]) <= 0.3) and np.abs(sp["fb"][:, 10:12]).max() > 0.2 and np.all(sp["fb"][:, 12] == 0)
        assert np.all(np.abs(sp["fb"][:, 13:25] - d["q_spawn"]) <= 0.1 + 1e-9) and len(np.unique(sp["fb"][:, 13:25])) == 600


def test_a_spawn_depends_on_seed_robot_and_episode_alone():
    d = ER.desc(xy_jitter=0.2, q_jitter=0.1)
    table = np.zeros((4, 5), np.float32); table[0] = np.arange(5)
    a = ER.spawn(d, None, 0.0, table, np.arange(20), np.full(20, 3))
    b = ER.spawn(d, None, 0.0, table, [7, 3], [3, 3])
    assert np.array_equal(b["fb"], a["fb"][[7, 3]])
    c = ER.spawn(ER.desc(xy_jitter=0.2, q_jitter=0.1, seed=2), None, 0.0, table, [7], [3])
    assert not np.array_equal(c["fb"][0], a["fb"][7])
    assert not np.array_equal(ER.spawn(d, None, 0.0, table, [7], [4])["fb"][0], a["fb"][7])


def test_bookkeeping_of_a_call():
    """Four robots on flat ground: one goes on, one falls (status), one times out, one is forced while tilted."""
    d = ER.desc(max_ticks=10, status_ticks=2)
    table = np.zeros((4, 1), np.float32)
    fb = np.zeros((4, 37), np.float32); fb[:, 0] = 1.0; fb[:, 6] = 0.27; fb[:, 4] = [0.1, 0.2, 0.3, 0.4]
    fb[3, 0:4] = [np.cos(0.6), np.sin(0.6), 0.0, 0.0]                            # roll 1.2 rad
    r0 = ER.step(d, None, 0.0, table, fb, np.zeros((4, 6)), np.zeros((4, 9)), reset_all=True)
    assert np.all(r0["done"] == ER.EP_FORCED) and np.all(r0["ep_state"] == 0) and np.all(r0["ep_stats"][:, 8] == d["spawn_height"])
    st = r0["ep_state"].copy(); st[1, 2] = 1; st[2, 0] = 9; st[0, 0] = 8
    stats = r0["ep_stats"].copy(); stats[:, 0] = 0.05
    r = ER.step(d, None, 0.0, table, fb, st, stats, plant_status=[0x10, 0x10, 0, 0], force_reset=[0, 0, 0, 1])
    assert list(r["done"]) == [0, ER.EP_STATUS, ER.EP_TIMEOUT, ER.EP_TILT | ER.EP_FORCED]
    assert list(r["ep_state"][0]) == [9, 0, 1, 0, 0, 0]
    assert list(r["ep_state"][1]) == [0, 1, 0, ER.EP_STATUS, 1, 0] and list(r["ep_state"][2]) == [0, 1, 0, ER.EP_TIMEOUT, 0, 1]
    assert list(r["ep_state"][3]) == [0, 1, 0, ER.EP_TILT | ER.EP_FORCED, 1, 0]
    assert np.allclose(r["ep_stats"][1:, 4], [1, 10, 1]) and np.allclose(r["ep_stats"][1:, 5], np.float32([0.2, 0.3, 0.4]).astype(float) - np.float64(np.float32(0.05)))
    assert np.allclose(r["ep_stats"][:, 7], [0, 0.27, 0.27, 0.27], atol=1e-7) and np.allclose(r["ep_stats"][:, 8], [0.27, 0.30, 0.30, 0.30], atol=1e-7)
    assert np.array_equal(r["fb"][0], fb[0].astype(np.float64)) and np.all(r["fb"][1:, 6] == d["spawn_height"])


def test_the_pd_stand_settles_where_the_gpu_test_expects_it(pkg):
    """episode_ref.STAND_SETTLE_Z: the float64 chain of body_contact_ref for one A1 dropped from 0.30 onto the default desc's PD hold, 400 ticks of
    1 ms at 2 sub-steps.  Measured: 0.2664 .. 0.2695 from tick 300 to 1300, 0.26865 at tick 400, no trunk or knee contact on the way."""
    import body_contact_ref as BR
    import plant_ref as PR
    import rigid_body_ref as M
    D, height, _, _, _ = BR.fall_case(pkg, 1)
    d = ER.desc()
    cmd = PR.stand_cmd(1, kp=d["kp"], kd=d["kd"], pose=d["q_spawn"])
    model, body = pkg.model_desc("a1"), BR.body_of(pkg.plant_body_desc("a1"))
    p = PR.params(**BR.FALL_PARAMS)
    s = M.normalised(PR.stand_state(1, z=d["spawn_height"]))
    seen = 0
    for k in range(400):
        for _ in range(p["substeps"]):
            s, aux = BR.substep(model, body, p, D, height, np.zeros(1, np.int64), None, s, cmd, p["dt"] / p["substeps"])
        seen |= int(BR.status_of(p, aux)[0])
        if k >= 300:
            assert abs(s[0, 6] - ER.STAND_SETTLE_Z) <= 0.002, (k, s[0, 6])
    assert not seen & (BR.PL_TRUNK_CONTACT | BR.PL_KNEE_CONTACT | ER.PL_NONFINITE)


def test_a_tilt_bound_of_pi_judges_nothing():
    """cos(tilt_max) cannot reach -1 for a float tilt_max, and a robot on its back has R_zz = -1: from pi on the bound is off."""
    fb = np.zeros((2, 37), np.float32); fb[:, 1] = 1.0; fb[:, 6] = 0.3            # upside down
    z6, z9 = np.zeros((2, 6)), np.zeros((2, 9))
    table = np.zeros((4, 1), np.float32)
    assert list(ER.step(ER.desc(tilt_max=np.pi), None, 0.0, table, fb, z6, z9)["done"]) == [0, 0]
    assert list(ER.step(ER.desc(tilt_max=4.0), None, 0.0, table, fb, z6, z9)["done"]) == [0, 0]
    assert list(ER.step(ER.desc(tilt_max=3.1415), None, 0.0, table, fb, z6, z9)["done"]) == [ER.EP_TILT] * 2
