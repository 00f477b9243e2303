"""CPU: the C ABI of the stage kernels' per-robot reset and clock (qrgpu_set_stage_reset) -- the header declares it, the library exports it, qrgpu.py
mirrors it, and the ctypes struct has the size and the member offsets the C compiler gives the header's struct."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "qrgpu.h")
FIELDS = ("d_mask", "bits", "level", "d_ticks", "tick_dt")

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "qrgpu.h"
int main(void)
{
    qrgpu_stage_reset r;
    int (*set)(qrgpu_ctx *, const qrgpu_stage_reset *) = qrgpu_set_stage_reset;      /* the declared signature */
    (void)set; (void)r;
    printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(qrgpu_stage_reset), offsetof(qrgpu_stage_reset, d_mask), offsetof(qrgpu_stage_reset, bits),
           offsetof(qrgpu_stage_reset, level), offsetof(qrgpu_stage_reset, d_ticks), offsetof(qrgpu_stage_reset, tick_dt),
           QRGPU_STAGE_RESET_CONSTRUCT, QRGPU_STAGE_RESET_LIVE);
    return 0;
}
"""


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_binding():
    code = _code()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*qrgpu_stage_reset\s*;", code)
    assert m, "include/qrgpu.h has no qrgpu_stage_reset"
    members = [re.sub(r"\s+", " ", s.strip()) for s in m.group(1).split(";") if s.strip()]
    assert members == ["const int *d_mask", "unsigned bits", "int level", "const int *d_ticks", "float tick_dt"], members
    assert re.search(r"#define\s+QRGPU_STAGE_RESET_CONSTRUCT\s+1\b", code) and re.search(r"#define\s+QRGPU_STAGE_RESET_LIVE\s+2\b", code)
    assert re.search(r"\bint\s+qrgpu_set_stage_reset\s*\(\s*qrgpu_ctx\s*\*\s*\w+\s*,\s*const\s+qrgpu_stage_reset\s*\*\s*\w+\s*\)\s*;", code)
    txt = open(HEADER).read()
    assert "Out of scope: the stage kernels" not in txt                         # the episode contract points to the binding instead ...
    assert "episode step, plant step, ground, estimator, gait, swing, front-end or stance, tick" in txt      # ... and states the loop order
    assert re.search(r"pose_reset_time\s+stays", txt)                           # the stance stage's one scalar that stays scalar


def test_library_exports_the_entry_point(pkg):
    lib = C.CDLL(pkg._build.build())
    assert hasattr(lib, "qrgpu_set_stage_reset")
    assert "qrgpu_set_stage_reset" in pkg.qrgpu.EXPORTS
    data = open(pkg._build.build(), "rb").read()
    # one kernel per stage, bound or not: the eight stage kernels are there, and none of them has a per-robot twin (suffix _pr) beside it
    for k in (b"qr_ground_kernel", b"qr_estimator_kernel", b"qr_gait_kernel", b"qr_walk_gait_kernel", b"qr_swing_update_kernel",
              b"qr_stance_update_kernel", b"qr_pose_plan_kernel", b"qr_frontend_kernel"):
        assert k in data, k
        assert k + b"_pr" not in data, k
    # a NULL context is refused before anything is read
    f = pkg.load_library().qrgpu_set_stage_reset
    assert f(None, None) == 2 and f(None, C.byref(pkg.qrgpu.stage_reset(mask=8, level=1))) == 2


def test_python_mirror(pkg):
    q = pkg.qrgpu
    assert (q.STAGE_RESET_CONSTRUCT, q.STAGE_RESET_LIVE) == (1, 2)
    assert callable(q.Context.set_stage_reset) and callable(q.Context.clear_stage_reset) and pkg.stage_reset is q.stage_reset
    assert tuple(n for n, _ in q.stage_reset_struct._fields_) == FIELDS
    b = q.stage_reset(mask=0x1000, bits=0x0f, level=q.STAGE_RESET_LIVE, ticks=0x2000, tick_dt=0.004)
    assert (b.d_mask, b.bits, b.level, b.d_ticks) == (0x1000, 0x0f, 2, 0x2000) and abs(b.tick_dt - 0.004) < 1e-9
    d = q.stage_reset(ticks=0x2000)
    assert d.d_mask is None and d.bits == q.EP_REASONS and d.level == q.STAGE_RESET_CONSTRUCT and abs(d.tick_dt - 0.002) < 1e-9


def test_ctypes_struct_has_the_compilers_layout(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    # compiled and run, not linked against the library: the entry point's address is taken in an expression the compiler drops
    subprocess.check_call([cc, "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-Wl,--unresolved-symbols=ignore-all"])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, timeout=60).stdout.split()
    size, *offsets = [int(v) for v in out[:6]]
    s = pkg.qrgpu.stage_reset_struct
    assert C.sizeof(s) == size
    assert [getattr(s, n).offset for n in FIELDS] == offsets
    assert [int(v) for v in out[6:]] == [1, 2]
