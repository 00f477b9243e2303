"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/qrgpu.h declares.
No compute call is made here (there is no GPU); creating a context must fail loudly, not fall back."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

import pytest


def _declared_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "qrgpu.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(qrgpu_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_header(pkg):
    so = pkg._build.build()
    assert os.path.exists(so)
    lib = C.CDLL(so)
    syms = _declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), "libqrgpu.so does not export %s" % s
    for s in pkg.qrgpu.EXPORTS:
        assert s in syms


def test_kernels_are_gfx950_code_objects(pkg):
    so = pkg._build.build()
    data = open(so, "rb").read()
    assert b"gfx950" in data and b"qr_mpc_kernel" in data and b"qr_wbc_kernel" in data


def test_no_cpu_fallback(pkg, monkeypatch):
    """Without the library the package raises; without a gfx950 device qrgpu_create reports NO_DEVICE."""
    monkeypatch.setattr(pkg.qrgpu, "_LIB", None)
    monkeypatch.setattr(pkg.qrgpu, "lib_path", lambda: "/nonexistent/libqrgpu.so")
    with pytest.raises(pkg.MissingExtension):
        pkg.qrgpu.load_library()
    monkeypatch.undo()
    # torch is asked in a child process: it brings a HIP runtime of its own, and once that is up in this process the library's runtime
    # cannot open the device -- every GPU test after this one in the same session would fail with NO_DEVICE
    r = subprocess.run([sys.executable, "-c", "import torch; print(int(torch.cuda.is_available()))"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    if r.stdout.split()[-1] == b"0":
        with pytest.raises(pkg.QrgpuError):
            pkg.Context(device_id=0, max_batch=4)


def test_model_desc_defaults(pkg):
    lib = pkg.load_library()
    d = pkg.model_desc_struct()
    lib.qrgpu_model_desc_default(C.byref(d))
    assert abs(d.hip_l - 0.08505) < 1e-7 and d.kp_foot == 500.0 and abs(d.mu - 0.4) < 1e-7 and abs(d.weight_fb - 0.1) < 1e-7


def test_all_kernels_present(pkg):
    """Every kernel of the path and of the SURVEY 8f rows is in the gfx950 code object."""
    data = open(pkg._build.build(), "rb").read()
    for k in (b"qr_mpc_kernel", b"qr_wbc_kernel", b"qr_vmc_kernel", b"qr_frontend_kernel", b"qr_estimator_kernel", b"qr_pack_state_kernel",
              b"qr_swing_kernel", b"qr_gait_kernel", b"qr_foothold_kernel", b"qr_lpt_order_kernel", b"qr_ground_kernel", b"qr_walk_gait_kernel", b"qr_swing_velocity_kernel"):
        assert k in data, k


def test_desc_defaults(pkg):
    lib = pkg.load_library()
    v = pkg.qrgpu.vmc_desc_struct(); lib.qrgpu_vmc_desc_default(C.byref(v))
    assert v.mass == 13.0 and abs(v.reg_weight - 1e-4) < 1e-10 and v.fmax_ratio == 10.0 and list(v.acc_weight) == [1, 1, 1, 10, 10, 1]
    e = pkg.qrgpu.estimator_desc_struct(); lib.qrgpu_estimator_desc_default(C.byref(e))
    assert e.window == 120 and abs(e.time_step - 0.002) < 1e-9 and abs(e.hip_offset[0] - 0.1805) < 1e-7
    assert lib.qrgpu_estimator_state_doubles(120) == 96 + 360 and lib.qrgpu_estimator_state_doubles(0) == 0
    f = pkg.qrgpu.foothold_desc_struct(); lib.qrgpu_foothold_desc_default(C.byref(f))
    assert abs(f.swing_kp[1] - 0.16) < 1e-7 and abs(f.foot_clearance - 0.01) < 1e-9 and abs(f.default_hip_position[1] + 0.135) < 1e-7
    assert np.allclose(np.array(f.hip_offset[:] + f.default_hip_position[:] + [f.hip_l] + f.swing_kp[:] + [f.foot_clearance], np.float32), pkg.workload.foothold_cfg("a1"))
    w = pkg.qrgpu.walk_gait_desc_struct(); lib.qrgpu_walk_gait_desc_default(C.byref(w))
    assert np.allclose(np.array(w.stance_duration[:] + w.duty_factor[:] + w.initial_leg_phase[:] + [float(x) for x in w.initial_leg_state[:]]
                                + [w.contact_detection_phase_threshold, float(w.n_states)] + [float(x) for x in w.state_switch[:]] + w.state_ratio[:], np.float32),
                       pkg.workload.walk_cfg())


def _header_structs():
    """The `typedef struct { ... } qrgpu_*_desc;` blocks of include/qrgpu.h as {name: [(member, "float" | "int", array length or 0)]};
    array lengths given by a macro are resolved from the header's own #define.  A member the parser does not understand raises."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "qrgpu.h")).read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(QRGPU_\w+)\s+(\d+|0x[0-9a-fA-F]+)\b", txt, re.M)}
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(qrgpu_\w+_desc)\s*;", code, re.S):
        members = []
        for stmt in (x.strip() for x in body.split(";")):
            if not stmt:
                continue
            m = re.fullmatch(r"(float|int)\s+(.+)", stmt, re.S)
            assert m, "%s: unparsed member %r" % (name, stmt)
            for decl in (x.strip() for x in m.group(2).split(",")):
                d = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", decl)
                assert d, "%s: unparsed declarator %r" % (name, decl)
                dim = d.group(2)
                members.append((d.group(1), m.group(1), 0 if dim is None else int(dim) if dim.isdigit() else defines[dim]))
        out[name] = members
    return out


def test_ctypes_structs_mirror_the_header(pkg):
    """Every parameter block of include/qrgpu.h against its ctypes class in qrgpu.py: member names, their order, float / int, array lengths."""
    structs = _header_structs()
    assert len(structs) >= 10, sorted(structs)
    q = pkg.qrgpu
    mirror = {"qrgpu_model_desc": q.model_desc_struct, "qrgpu_vmc_desc": q.vmc_desc_struct, "qrgpu_estimator_desc": q.estimator_desc_struct,
              "qrgpu_gait_desc": q.gait_desc_struct, "qrgpu_walk_gait_desc": q.walk_gait_desc_struct,
              "qrgpu_swing_velocity_desc": q.swing_velocity_desc_struct, "qrgpu_foothold_desc": q.foothold_desc_struct,
              "qrgpu_swing_mode_desc": q.swing_mode_desc_struct, "qrgpu_stance_desc": q.stance_desc_struct, "qrgpu_pose_plan_desc": q.pose_plan_desc_struct}
    assert set(structs) == set(mirror), set(structs) ^ set(mirror)
    base = {C.c_float: "float", C.c_int: "int"}
    for name, cls in mirror.items():
        got = []
        for field, t in cls._fields_:
            if issubclass(t, C.Array):
                got.append((field, base[t._type_], t._length_))
            else:
                got.append((field, base[t], 0))
        assert got == structs[name], name
        assert C.sizeof(cls) == 4 * sum(max(1, dim) for _, _, dim in structs[name]), name
    gaps = dict((f, dim) for f, _, dim in structs["qrgpu_swing_mode_desc"])["gap_distance"]
    assert gaps == 8 == q.MAX_GAPS


@pytest.mark.gpu
def test_error_returns(gpu_ctx, pkg):
    """The reference has no error channel on this path; the C ABI returns a code from every call (error behaviour)."""
    import numpy as np
    ctx = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
    try:
        a = ctx.alloc((28, 8)); t = ctx.alloc((120, 8)); g = ctx.alloc((40, 8)); f = ctx.alloc((12, 8))
        with pytest.raises(pkg.QrgpuError, match="NOT_SETUP"):
            ctx.mpc_solve_batch(8, a, t, g, None, f, None, None)
        ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), 10)
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            ctx.mpc_solve_batch(9, a, t, g, None, f, None, None)              # n > max_batch
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            ctx.mpc_solve_batch(8, a, t, g, None, None, None, None)           # no output array
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            ctx.mpc_solve_batch(8, a, t, g, None, f, f, None)                 # torques requested without joint angles
        with pytest.raises(pkg.QrgpuError, match="NOT_SETUP"):
            ctx.vmc_force_batch(8, a, None, f)
        with pytest.raises(pkg.QrgpuError, match="BAD_ARG"):
            ctx.mpc_setup_packed(0, pkg.mpc_cfg("a1"), 17)                    # horizon beyond K_MAX_GAIT_SEGMENTS
        # the compute stream: a non-blocking stream of the context's own, a different one per context; set_stream(None) = the default stream
        other = pkg.Context(device_id=0, max_batch=8, horizon_max=16)
        try:
            assert ctx.get_stream() != 0 and other.get_stream() != 0 and ctx.get_stream() != other.get_stream()
            own = other.get_stream()
            other.set_stream(None); assert other.get_stream() == 0
            other.set_stream(own); assert other.get_stream() == own
        finally:
            other.close()
        for v in (a, t, g, f):
            v.free()
    finally:
        ctx.close()


def test_supported_environment_switches_are_listed_in_the_header():
    """include/qrgpu.h carries the table of supported environment switches; csrc/qrgpu_ctx.h the list the library checks the environment against
    (anything else named QRGPU_* is reported once by qrgpu_create).  Every getenv of the host code -- every qrgpu_*.hip and qrgpu_*.h -- names a
    supported switch, laboratory switches go through lab_env and answer only under QRGPU_LAB=1, and every supported switch is in the header's table."""
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ctxh = open(os.path.join(root, "quadruped-robot_amd", "csrc", "qrgpu_ctx.h")).read()
    header = open(os.path.join(root, "include", "qrgpu.h")).read()
    sup = re.search(r"#define QRGPU_SUPPORTED_ENV (.*?)\n#define QRGPU_LAB_ENV (.*?)\n", ctxh, re.S)
    supported = set(re.findall(r'"(QRGPU_\w+)"', sup.group(1)))
    lab = set(re.findall(r'"(QRGPU_\w+)"', sup.group(2)))
    assert supported and lab and not (supported & lab)
    for name in supported:
        assert re.search(r"^ \*   %s\b" % name, header, re.M), name
    import glob
    csrc = os.path.join(root, "quadruped-robot_amd", "csrc")
    host = sorted(glob.glob(os.path.join(csrc, "qrgpu_*.hip")) + glob.glob(os.path.join(csrc, "qrgpu_*.h")))
    assert len(host) >= 5, host                  # (api, stages, debug, mpc, tick, comm and the context header)
    read, read_lab = set(), set()
    for f in host:
        src = open(f).read()
        got = set(re.findall(r'[^_]getenv\("(QRGPU_\w+)"\)', src))
        got_lab = set(re.findall(r'lab_env\("(QRGPU_\w+)"\)', src))
        assert got <= supported, f
        assert got_lab <= lab | {"QRGPU_LAB"}, f
        # no call site reads the environment with a name the scan cannot see: every getenv / lab_env of the host code takes a literal
        # (lab_env's own forwarding getenv(name) in the context header is the one exception)
        stray = re.findall(r'\b(?:getenv|lab_env)\((?!"QRGPU_\w+"\))[^)]*\)', src)
        assert stray in ([], ["lab_env(const char *name)", "getenv(name)"]), (f, stray)
        read |= got; read_lab |= got_lab
    # ... and the scan is not vacuous: the library does read its switches, laboratory ones included
    assert read >= {"QRGPU_LAB", "QRGPU_TICK_PIPELINE", "QRGPU_OV_PLAN_HOLD", "QRGPU_H16_TWO_HOLD", "QRGPU_COMM_EVENTS"}, read
    assert read_lab - {"QRGPU_LAB"} == lab, (read_lab, lab)
