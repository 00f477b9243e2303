"""Reader for tests/golden/*.npz (written by tests/golden/make_golden.py)."""
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(HERE, name), allow_pickle=False)
    n = int(z["count"][0])
    rows = [dict() for _ in range(n)]
    for k in z.files:
        if k == "count":
            continue
        i, key = int(k[:3]), k[4:]
        v = z[k]
        rows[i][key] = v.item() if v.dtype.kind in "US" and v.shape == () else v
    return rows


def make_golden():
    """tests/golden/make_golden.py as a module (its generators need oracle/_ref; its cell tables and input builders do not)."""
    import importlib.util
    import sys
    if "qr_make_golden" not in sys.modules:
        spec = importlib.util.spec_from_file_location("qr_make_golden", os.path.join(HERE, "make_golden.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["qr_make_golden"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["qr_make_golden"]


def load_vmc_grid(path=None):
    """vmc_grid_golden.npz -> {cell name: dict(cfg, geom, idx, scanned, vin, q, ratio or None, x_quadprog, quadprog_inf, well_posed)}."""
    z = np.load(path or os.path.join(HERE, "vmc_grid_golden.npz"), allow_pickle=False)
    out = {}
    for name in z["cells"]:
        name = str(name)
        c = {k: z[name + "_" + k] for k in ("cfg", "geom", "idx", "scanned", "vin", "q", "x_quadprog", "quadprog_inf", "well_posed")}
        c["ratio"] = z[name + "_ratio"] if name + "_ratio" in z.files else None
        out[name] = c
    return out
