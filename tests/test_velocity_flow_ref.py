"""CPU: tests/velocity_flow_ref.py pinned by hand-written tables -- each branch of the swingFootIds test, an entry that outlives its swing with flag 0, a
reset that clears it, the identity rows on terrain 0 -- and what its streams reach."""
import numpy as np

import velocity_flow_ref as R

F = np.float32


def _tick(leg_state, allow, desired, mem, reset=False, terrain=0, n=1):
    """One robot's tick from small tables; every other input row is its own row number, so a copied row names its source"""
    est_in = np.tile(np.arange(100, 154, dtype=F)[:, None], (1, n))
    est_out = np.tile(np.arange(200, 242, dtype=F)[:, None], (1, n))
    ground_out = np.tile(np.arange(300, 332, dtype=F)[:, None], (1, n))
    gait_out = np.tile(np.arange(400, 424, dtype=F)[:, None], (1, n))
    gait_state = np.tile(np.arange(500, 552, dtype=F)[:, None], (1, n))
    state_des = np.tile(np.arange(600, 612, dtype=F)[:, None], (1, n))
    gait_out[8:12, 0] = desired; gait_out[12:16, 0] = leg_state; gait_state[20:24, 0] = allow
    return R.velocity_inputs(terrain, est_in, est_out, ground_out, gait_out, gait_state, state_des, np.full(n, mem, np.int32), np.full(n, reset))


def test_each_branch_of_the_swing_foot_ids_test():
    # legState, allowSwitchLegState -> in swingFootIds?   (qr_swing_leg_controller.cpp:222-227)
    table = [(R.STANCE, 1, False),             # a stance leg that may switch stays out
             (R.STANCE, 0, True),              # a stance leg held by the schedule is in
             (R.EARLY_CONTACT, 1, False), (R.EARLY_CONTACT, 0, False),
             (R.SWING, 1, True), (R.SWING, 0, True),
             (R.LOSE_CONTACT, 1, True), (R.LOSE_CONTACT, 0, True),
             (R.USERDEFINED_SWING, 1, True), (R.USERDEFINED_SWING, 0, True)]
    for state, allow, inside in table:
        assert (2 in R.swing_foot_ids([R.STANCE, R.STANCE, state, R.STANCE], [1, 1, allow, 1])) == inside, (state, allow)
        o = _tick([R.STANCE, R.STANCE, state, R.STANCE], [1, 1, allow, 1], [R.STANCE] * 4, mem=0)
        assert [float(o["sv"][l][0]) for l in range(4)] == [0, 0, float(inside), 0]
        assert int(o["mem"][0]) == (4 if inside else 0)


def test_an_entry_outlives_its_swing_and_a_reset_clears_it():
    # tick 1: leg 0 swings (desired SWING): entry and command
    o = _tick([R.SWING, R.STANCE, R.STANCE, R.STANCE], [1] * 4, [R.SWING, R.STANCE, R.STANCE, R.STANCE], mem=0)
    assert int(o["mem"][0]) == 0b0001 and o["flag"][:, 0].tolist() == [1, 0, 0, 0]
    # tick 2: it has landed and may switch: out of swingFootIds, the entry stays, the command's flag is 0
    o = _tick([R.STANCE] * 4, [1] * 4, [R.STANCE] * 4, mem=int(o["mem"][0]))
    assert int(o["mem"][0]) == 0b0001 and o["flag"][:, 0].tolist() == [0, 0, 0, 0] and float(o["sv"][0][0]) == 0
    # tick 3: the schedule asks for a swing again before the leg is in swingFootIds (EARLY_CONTACT): the old entry is commanded
    o = _tick([R.EARLY_CONTACT, R.STANCE, R.STANCE, R.STANCE], [1] * 4, [R.SWING, R.STANCE, R.STANCE, R.STANCE], mem=int(o["mem"][0]))
    assert int(o["mem"][0]) == 0b0001 and o["flag"][:, 0].tolist() == [1, 0, 0, 0] and float(o["sv"][0][0]) == 0
    # the same tick after a reset: the map was cleared, nothing is commanded
    o = _tick([R.EARLY_CONTACT, R.STANCE, R.STANCE, R.STANCE], [1] * 4, [R.SWING, R.STANCE, R.STANCE, R.STANCE], mem=0b0001, reset=True)
    assert int(o["mem"][0]) == 0 and o["flag"][:, 0].tolist() == [0, 0, 0, 0]
    # a reset clears before this tick's legs are added; bits above the four legs are dropped
    o = _tick([R.STANCE, R.SWING, R.STANCE, R.STANCE], [1] * 4, [R.STANCE, R.SWING, R.STANCE, R.STANCE], mem=0x7fffffff, reset=True)
    assert int(o["mem"][0]) == 0b0010 and o["flag"][:, 0].tolist() == [0, 1, 0, 0]
    o = _tick([R.STANCE] * 4, [1] * 4, [R.SWING] * 4, mem=0x7ffffff5)
    assert int(o["mem"][0]) == 0b0101 and o["flag"][:, 0].tolist() == [1, 0, 1, 0]
    # an entry in swingFootIds whose desired state is STANCE (a held stance leg): entry, no command
    o = _tick([R.STANCE] * 4, [0, 1, 1, 1], [R.STANCE] * 4, mem=0)
    assert int(o["mem"][0]) == 0b0001 and o["flag"][:, 0].tolist() == [0, 0, 0, 0] and float(o["sv"][0][0]) == 1


def test_rows_and_the_identity_on_horizontal_terrain():
    src = {4: 404, 5: 405, 6: 406, 7: 407, 20: 206, 21: 207, 22: 208, 23: 112, 24: 606, 25: 607, 26: 608, 27: 611}
    src.update({41 + k: 117 + k for k in range(12)})
    for terrain in range(5):
        o = _tick([R.STANCE] * 4, [1] * 4, [R.STANCE] * 4, mem=0, terrain=terrain)
        assert sorted(o["sv"]) == list(range(0, 8)) + list(range(20, 53))                  # rows 8-19 are not the stage's
        for row, want in src.items():
            assert float(o["sv"][row][0]) == want, (terrain, row)
        rot, quat = [float(o["sv"][28 + k][0]) for k in range(9)], [float(o["sv"][37 + a][0]) for a in range(4)]
        if terrain < 2:
            assert rot == [1, 0, 0, 0, 1, 0, 0, 0, 1] and quat == [1, 0, 0, 0]
        else:
            assert rot == [322 + k for k in range(9)] and quat == [106, 107, 108, 109]
        assert [float(o["ei"][41 + a][0]) for a in range(4)] == [R.STANCE] * 4 and sorted(o["ei"]) == [41, 42, 43, 44]


def test_the_streams_reach_every_case():
    S, ref0, ref3 = R.streams(), R.reference(R.PLANE), R.reference(R.SLOPE)
    assert S["est_in"].shape == (48, 54, 130)
    assert set(np.unique(S["gait_out"][:, 12:16])) == set(map(F, range(5)))
    allow = S["gait_state"][:, 20:24] != 0
    assert 0.1 < allow.mean() < 0.9
    assert S["scalar_reset"][0] and S["scalar_reset"][1:-1].sum() == 1 and S["mask_reset"][1:].sum() > 100
    assert not (S["mask_reset"] & S["scalar_reset"][:, None]).any()
    ids = ref0["sv"][:, 0:4] != 0
    entry = ((ref0["mem"][:, None, :] >> np.arange(4)[None, :, None]) & 1) != 0
    assert (entry & ~ids).sum() > 100 and (entry & ~ids & (ref0["flag"] != 0)).sum() > 100          # entries that outlive swingFootIds, some commanded
    assert (ids & (ref0["flag"] == 0)).sum() > 100 and (~entry).sum() > 100
    assert np.all(ref0["mem"] >> 4 == 0)
    assert np.all(ref0["sv"][:, 8:20] == R.POISON) and np.all(ref3["sv"][:, 8:20] == R.POISON)
    assert np.all(ref0["sv"][:, 28] == 1) and np.all(ref0["sv"][:, 29] == 0) and np.all(ref0["sv"][:, 37] == 1)
    assert ref3["sv"][:, 28:37].tobytes() == np.ascontiguousarray(S["ground_out"][:, 22:31]).tobytes()
    assert ref3["sv"][:, 37:41].tobytes() == np.ascontiguousarray(S["est_in"][:, 6:10]).tobytes()
    for k in ("mem", "flag", "est_in"):                                                              # the terrain changes rows 28-40 alone
        assert ref0[k].tobytes() == ref3[k].tobytes()
    assert np.delete(ref0["sv"], np.r_[28:41], axis=1).tobytes() == np.delete(ref3["sv"], np.r_[28:41], axis=1).tobytes()
