"""Where does |v_est - v_true| = 0.1 m/s of tools/closed_loop.py --estimator come from?  The tool's flat standing loop, the estimator chain always running;
the tick fed with the truth (open-loop estimate) or with the estimate; distances printed at a few ticks, one JSON line each
(profiles/estimator_loop_diag.jsonl; DESIGN.md 4.6, the sensor stage).    python scratch/diag_estimate.py"""
import importlib.util, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("cl", os.path.join(ROOT, "tools", "closed_loop.py")); cl = importlib.util.module_from_spec(spec); spec.loader.exec_module(cl)
pkg = cl._load_pkg(); pkg._build.build()
n, h = 1024, 10
for feed in ("truth", "estimate"):
    ctx = pkg.Context(device_id=0, max_batch=n, horizon_max=16)
    ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), h); ctx.wbc_setup_packed(0, pkg.model_desc("a1"))
    fb0 = np.zeros((37, n), np.float32); fb0[0] = 1.0; fb0[6] = 0.30; fb0[13:25] = cl.STAND_POSE[:, None]
    cmd0 = np.zeros((60, n), np.float32); cmd0[0:12] = cl.STAND_POSE[:, None]; cmd0[12:24] = 100.0; cmd0[36:48] = 2.0
    traj = np.zeros((h, 12, n), np.float32); traj[:, 5] = cl.HEIGHT
    wcmd = np.zeros((67, n), np.float32); wcmd[2] = cl.HEIGHT; wcmd[63:67] = 1.0
    A = ctx.alloc
    d = dict(fb=A((37, n)).upload(fb0), cmd=A((60, n)).upload(cmd0), mpc=A((28, n)), traj=A((12 * h, n)).upload(traj.reshape(12 * h, n)),
             gait=A((4 * h, n)).upload(np.ones((4 * h, n), np.float32)), wcmd=A((67, n)).upload(wcmd), prev=A((3, n)).zero(), force=A((12, n)), st=A((n,), np.int32))
    odesc = pkg.observe_desc("sim"); ecfg = pkg.workload.estimator_cfg("a1"); com = np.asarray(pkg.workload.ROBOTS["a1"]["com_offset"], np.float32)
    est0 = np.zeros((54, n), np.float32); est0[41:45] = 1.0
    nd = ctx.estimator_state_doubles(120)
    d.update(est_in=A((54, n)).upload(est0), obs=A((71, n)), rpy=A((3, n)), gin=A((23, n)), stamp=A((n,), np.uint32), gst=A((13, n), np.float64),
             est_state=A((nd, n), np.float64).zero(), est_out=A((42, n)).zero(), mpc_est=A((28, n)), fb_est=A((37, n)))
    settle = pkg.plant_params(dt=0.001, substeps=1)
    for _ in range(400):
        ctx.plant_step_batch(n, settle, d["fb"], d["cmd"], mpc_state=d["mpc"])
    fb = d["fb"].download(); fb[10:12] += np.random.default_rng(1).uniform(-0.3, 0.3, (2, n)).astype(np.float32)
    d["fb"].upload(fb); d["cmd"].zero(); ctx.set_warm_start(True)
    params = pkg.plant_params(dt=0.002, substeps=2); tau = d["cmd"].row(48)
    for k in range(520):
        ctx.plant_step_batch(n, params, d["fb"], d["cmd"], mpc_state=d["mpc"], est_in=d["est_in"])
        ctx.observe_batch(n, odesc, d["est_in"], d["obs"], d["est_in"], d["rpy"], ground_in=d["gin"], tick=d["stamp"], est_out_prev=d["est_out"], reset=k == 0, step=k)
        ctx.ground_update_batch(n, d["gin"], d["gst"], None, d["est_in"], reset=k == 0)
        ctx.estimator_update_batch(n, ecfg, d["est_in"], d["stamp"], d["est_state"], d["est_out"])
        ctx.pack_state_batch(n, com, d["est_in"], d["est_out"], d["rpy"], d["mpc_est"], d["fb_est"])
        if feed == "truth":
            ctx.tick_batch(n, d["mpc"], d["traj"], d["gait"], d["fb"], d["wcmd"], d["prev"], d["force"], tau, d["st"])
        else:
            ctx.tick_batch(n, d["mpc_est"], d["traj"], d["gait"], d["fb_est"], d["wcmd"], d["prev"], d["force"], tau, d["st"])
        if k in (20, 60, 120, 250, 519):
            e, t = d["mpc_est"].download().astype(np.float64), d["mpc"].download().astype(np.float64)
            print(json.dumps(dict(feed=feed, tick=k, v_true=float(np.abs(t[3:6]).max(0).mean()), v_err=float(np.abs(e[3:6] - t[3:6]).max(0).mean()),
                                  xy_true=float(np.abs(t[0:2]).max(0).mean()), xy_err=float(np.abs(e[0:2] - t[0:2]).max(0).mean()),
                                  verr_axes=[float(np.abs(e[3 + a] - t[3 + a]).mean()) for a in range(3)], vtrue_axes=[float(np.abs(t[3 + a]).mean()) for a in range(3)])), flush=True)
    ctx.close()
