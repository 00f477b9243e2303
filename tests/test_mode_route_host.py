"""CPU: csrc/qr_mode_route.h compiled for the host (tests/stubs/mode_route_host.hip) and run over a few thousand random columns -- every mode, the
selections that are no mode, every plan kind with and without its flag bits -- against the numpy restatement of tests/mode_route_ref.py, bit for bit:
chains, flags, counts, the masks of the cadenced tick, and the merge of two motor-command arrays that carry NaNs, into an array of its own and into
each input.  Three configurations: the default table with the plan, a custom table without one, the merge without status inputs.  The same
stand-alone program is built once more with the address and undefined-behaviour sanitizers and run on the same input files: it must run clean and
write the same bytes."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mode_route_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "stubs", "mode_route_host")
N = 4099
CONFIGS = {"default_with_plan": dict(table=R.DEFAULT_TABLE, fallback=R.DEFAULT_FALLBACK, plan=True, status=True, seed=11),
           "custom_no_plan": dict(table=(R.CHAIN_MPC, R.CHAIN_FORCE_BALANCE, R.CHAIN_NONE, R.CHAIN_FORCE_BALANCE), fallback=R.CHAIN_FORCE_BALANCE, plan=False,
                                  status=True, seed=12),
           "fallback_none_no_status": dict(table=R.DEFAULT_TABLE, fallback=R.CHAIN_NONE, plan=True, status=False, seed=13)}


def _compile(exe, extra=()):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "--offload-host-only", "-w", *extra, "-I", os.path.join(ROOT, "quadruped-robot_amd", "csrc"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "stubs", "mode_route_host.hip"), "-o", exe])


def inputs(cfg):
    sel, plan = R.random_columns(N, cfg["seed"])
    rng = np.random.default_rng(cfg["seed"] + 100)
    a = rng.standard_normal((R.CMD_ROWS, N)).astype(np.float32)
    b = rng.standard_normal((R.CMD_ROWS, N)).astype(np.float32)
    a[:, rng.random(N) < 0.2] = np.nan
    b[:, rng.random(N) < 0.2] = np.nan
    return dict(sel=sel, plan=plan, updated=(rng.random(N) < 0.3).astype(np.int32) * 5, a=a, b=b,
                sa=rng.integers(1, 1 << 30, N).astype(np.int32), sb=rng.integers(1, 1 << 30, N).astype(np.int32))


def _run(exe, fin, fout):
    subprocess.check_call([exe, fin, fout], timeout=300)
    raw = open(fout, "rb").read()
    w = np.frombuffer(raw, "<u4")
    got, at = {}, 0
    for k, size, dt in (("chain", N, "<i4"), ("flags", N, "<i4"), ("count", 3, "<i4"), ("due", N, "<i4"), ("skip", N, "<i4"), ("out", 60 * N, "<f4"),
                        ("st", N, "<i4"), ("in_a", 60 * N, "<f4"), ("in_b", 60 * N, "<f4")):
        got[k] = w[at:at + size].view(dt)
        at += size
    assert at == w.size
    for k in ("out", "in_a", "in_b"):
        got[k] = got[k].reshape(60, N)
    return raw, got


@pytest.fixture(scope="module")
def host(pkg, tmp_path_factory):
    _compile(EXE)
    tmp = tmp_path_factory.mktemp("mode_route_host")
    runs = {}
    for name, cfg in CONFIGS.items():
        x = inputs(cfg)
        d = pkg.qrgpu.mode_route_desc_struct((ctypes.c_int * 4)(*cfg["table"]), cfg["fallback"])
        blob = struct.pack("<4i", N, int(cfg["plan"]), ctypes.sizeof(d), int(cfg["status"])) + bytes(d)
        blob += b"".join(np.ascontiguousarray(x[k]).tobytes() for k in ("sel", "plan", "updated", "a", "b", "sa", "sb"))
        fin, fout = str(tmp / (name + ".in")), str(tmp / (name + ".out"))
        open(fin, "wb").write(blob)
        raw, got = _run(EXE, fin, fout)
        runs[name] = dict(x=x, fin=fin, raw=raw, got=got)
    return dict(tmp=tmp, runs=runs)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_route_masks_and_merge_against_the_restatement(host, name):
    cfg, run = CONFIGS[name], host["runs"][name]
    x, got = run["x"], run["got"]
    chain, flags, count = R.route(x["sel"], x["plan"] if cfg["plan"] else None, cfg["table"], cfg["fallback"])
    assert np.array_equal(got["chain"], chain) and np.array_equal(got["flags"], flags) and np.array_equal(got["count"], count)
    due, skip = R.masks(x["updated"], chain)
    assert np.array_equal(got["due"], due) and np.array_equal(got["skip"], skip)
    out, st = R.command(chain, x["a"], x["b"], x["sa"] if cfg["status"] else None, x["sb"] if cfg["status"] else None)
    assert same_bits(got["out"], out) and np.array_equal(got["st"], st)
    assert same_bits(got["in_a"], out) and same_bits(got["in_b"], out)
    # not vacuous: every chain, both flags, NaNs on both sides that were and were not selected
    assert set(np.unique(flags)) == {0, R.ROUTE_BAD_MODE, R.ROUTE_NO_CHAIN} and count[0] > 0 and count[1] + count[2] > 0
    on_a, on_b = chain == R.CHAIN_MPC, chain == R.CHAIN_FORCE_BALANCE
    for on, mine, other in ((on_a, x["a"], x["b"]), (on_b, x["b"], x["a"])):
        if on.any():
            assert np.isnan(other[0, on]).any() and np.isnan(mine[0, on]).any() and not np.isnan(out[:, on & ~np.isnan(mine[0])]).any()
    assert not np.isnan(out[:, chain == R.CHAIN_NONE]).any()


def test_sanitized_build_runs_clean(host):
    """The same stand-alone program under the address and undefined-behaviour sanitizers, on the same files: no report, the same bytes."""
    exe = EXE + "_san"
    _compile(exe, ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-fno-omit-frame-pointer"))
    for name, run in host["runs"].items():
        fout = str(host["tmp"] / (name + ".san.out"))
        p = subprocess.run([exe, run["fin"], fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0 and not p.stderr, p.stderr.decode()[-2000:]
        assert open(fout, "rb").read() == run["raw"]
