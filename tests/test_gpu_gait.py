"""GPU parity of the open-loop gait generator kernel (qrgpu_gait_update_batch) against the oracle over a tick sequence.
Reference: qrOpenLoopGaitGenerator::Update / Schedule (qr_openloop_gait_generator.cpp:126-249).  Bar: bit-exact (plain float arithmetic)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_gait_sequence_bit_exact(gpu_ctx, pkg, oracle):
    W = pkg.workload
    n, ticks, dt = 500, 900, 0.002
    cfg = W.gait_cfg(wait_time=0.06)
    contacts = W.make_gait_contacts(n, ticks, cfg, seed=4)
    t = (np.arange(ticks) * dt).astype(np.float32)
    d_state = gpu_ctx.alloc((52, n)).upload(np.full((52, n), np.nan, np.float32))      # reset must not depend on what was there
    d_c = gpu_ctx.alloc((4, n)); d_out = gpu_ctx.alloc((24, n))
    d_fe = gpu_ctx.alloc((64, n)).upload(np.full((64, n), -7.0, np.float32))
    snaps = {}
    for k in range(ticks):
        d_c.upload(pkg.to_soa(contacts[k]))
        gpu_ctx.gait_update_batch(n, cfg, float(t[k]), d_c, d_state, d_out, d_fe, reset=(k == 0))
        if k % 50 == 49 or k < 3:
            snaps[k] = d_out.download().T.copy()
    fe = d_fe.download().T
    for r in range(0, n, 5):
        o = oracle.gait_run(cfg, t, contacts[:, r])
        for k, g in snaps.items():
            assert np.array_equal(g[r], o[k]), (r, k, g[r], o[k])
        # rows 42-61 of the front-end input after the last tick
        assert np.array_equal(fe[r, 42:46], o[-1, 0:4]) and np.array_equal(fe[r, 50:54], o[-1, 4:8])
        assert np.array_equal(fe[r, 54:58], o[-1, 8:12]) and np.array_equal(fe[r, 58:62], o[-1, 12:16]) and np.all(fe[r, 46:50] == cfg[4])
        assert np.all(fe[r, :42] == -7.0) and np.all(fe[r, 62:] == -7.0)
    # the batch exercised the hold and the early contact
    allout = np.stack([oracle.gait_run(cfg, t, contacts[:, r]) for r in range(0, n, 5)])
    assert (allout[:, :, 12:16] == 2).any()
    for v in (d_state, d_c, d_out, d_fe):
        v.free()


@pytest.mark.parametrize("name", ["default", "plain_trot", "robot_stop", "swing_start", "reset", "irregular_clock"])
def test_gait_against_the_reference_state_machine(gpu_ctx, pkg, name):
    """The kernel against tests/gait_ref.py (the reference's Update / Schedule / Reset written out line by line in numpy float32), bit for bit,
    on every tick of every robot: the generator's memory (rows 0-47 of gait_state), gait_out, rows 42-61 of fe_in with the rest of that buffer
    untouched; a second run with both optional outputs NULL evolves the same memory.  Every tick writes its gait_out and fe_in into a slice of
    its own of one device array, downloaded once; the memory is copied per tick into a host buffer; the comparisons are whole-array."""
    import gait_ref as GR
    c = GR.configuration(pkg, name)
    cfg, t, n, T = c["cfg"], c["time"], GR.N_ROBOTS, GR.TICKS
    d_state = gpu_ctx.alloc((52, n)).upload(np.full((52, n), np.nan, np.float32))
    d_bare = gpu_ctx.alloc((52, n)).upload(np.full((52, n), np.nan, np.float32))
    d_c = gpu_ctx.alloc((T, 4, n)).upload(np.ascontiguousarray(c["contact"].transpose(0, 2, 1)))
    d_out = gpu_ctx.alloc((T, 24, n)).upload(np.full((T, 24, n), np.nan, np.float32))
    d_fe = gpu_ctx.alloc((T, 64, n)).upload(np.full((T, 64, n), -7.0, np.float32))
    st = np.empty((T, 52, n), np.float32); bare = np.empty((T, 52, n), np.float32)
    for k in range(T):
        reset = pkg.qrgpu.GAIT_RESET_CONSTRUCT if k == 0 else (pkg.qrgpu.GAIT_RESET_LIVE if c["reset"][k] else 0)
        ct = d_c.ptr + k * 4 * n * 4
        gpu_ctx.gait_update_batch(n, cfg, float(t[k]), ct, d_state, d_out.ptr + k * 24 * n * 4, d_fe.ptr + k * 64 * n * 4, stop=bool(c["stop"][k]), reset=reset)
        gpu_ctx.gait_update_batch(n, cfg, float(t[k]), ct, d_bare, None, None, stop=bool(c["stop"][k]), reset=reset)
        st[k] = d_state.download(); bare[k] = d_bare.download()
    out = d_out.download(); fe = d_fe.download()
    ref = [GR.run(cfg, t, c["contact"][:, r], c["stop"], c["reset"], want_state=True) for r in range(n)]
    want = np.stack([w for w, _ in ref], axis=2)                  # [T, 24, n]
    wst = np.stack([s_ for _, s_ in ref], axis=2)                 # [T, 48, n]

    def first_bad(a, b):
        return tuple(int(v[0]) for v in np.nonzero(a != b)) if (a != b).any() else None

    assert np.array_equal(out, want), (name, "gait_out [tick, row, robot]", first_bad(out, want))
    assert np.array_equal(st[:, :48], wst), (name, "gait_state", first_bad(st[:, :48], wst))
    assert np.array_equal(bare[:, :48], wst), (name, "gait_state without the optional outputs", first_bad(bare[:, :48], wst))
    assert np.isnan(st[-1, 48:]).all() and np.isnan(bare[-1, 48:]).all(), (name, "rows 48-51 of gait_state are the per-robot gait's: not written here")
    assert np.array_equal(fe[:, 42:46], want[:, 0:4]) and np.array_equal(fe[:, 50:54], want[:, 4:8]) and np.array_equal(fe[:, 54:58], want[:, 8:12])
    assert np.array_equal(fe[:, 58:62], want[:, 12:16]) and np.all(fe[:, 46:50] == cfg[4:8][None, :, None])
    assert np.all(fe[:, :42] == -7.0) and np.all(fe[:, 62:] == -7.0)
    for v in (d_state, d_bare, d_c, d_out, d_fe):
        v.free()
