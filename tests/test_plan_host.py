"""Host planning of libfks.so (fks_layout.cpp, fks_phx.cpp), without a device.

* tools/plan/plan_selftest.cpp, built with AddressSanitizer and UBSan from the two planning
  files and fks_gf2.cpp alone (no HIP runtime), checks the invariants the design promises:
  shards tile the stream, every live element is written exactly once, chunk tables, the
  header image, the torch_rocm pieces and shard boundaries, the window-set bookkeeping.
* the host results of libfks.so equal those recorded from the commit before the host code
  was split (tests/golden/host_plan_parent.json, written by tests/golden/make_host_plan.py;
  without a device the CU count falls back to 256).
"""
import ctypes
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fate-llm_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_plan_parent.json")
FROZEN, STREAM_ROCM = 2, 4

# ---- the tensor lists: (numel, dtype, flags, address) per tensor ----
# those of tests/test_capi_host.py ...
HAND = ([[(n, 1, 0, 16) for n in s] for s in ([16, 32, 624], [37, 5, 3, 16], [5, 3, 1, 7, 100], [1, 1, 1, 15, 17])] +
        [[(n, d, 0, 16) for n, d in s] for s in (
            [(3, 0), (20, 0)], [(5, 1), (7, 2), (1000, 1), (1, 0)], [(4096, 0), (5, 0)], [(16, 1)],
            [(100000, 0), (3, 1), (17, 2)], [(0, 0)], [(624 * 3, 1)], [(3 * 10**7 + 5, 0), (2, 1)])] +
        [[(n, d, 0, 4096) for n, d in s] for s in (
            [(600_000_000, 0)], [(1_100_000_003, 0), (5, 1)], [(2**30 + 4099, 2), (2**29, 0)])])
N_LCG = 200


def lcg_lists(count=N_LCG):
    """... and `count` lists from a fixed 64-bit LCG (plan_selftest.cpp draws the same)."""
    state = [0x9E3779B97F4A7C15]

    def rnd(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % 2**64
        return (state[0] >> 33) % n

    out = []
    for _ in range(count):
        ts = []
        for _ in range(1 + rnd(12)):
            c = rnd(8)
            if c == 0:
                n = 0
            elif c == 1:
                n = 1 + rnd(15)
            elif c == 2:
                n = 16
            elif c == 3:
                n = 17 + rnd(24)
            elif c == 4:
                n = 624 * (1 + rnd(6))
            elif c == 5:
                n = 624 * (1 + rnd(6))
                n += 3 if rnd(2) else -3
            else:
                n = 4096 if c == 6 else 100003
            d = rnd(3)
            flags = FROZEN if rnd(6) == 0 else 0
            addr = 4096 + (4 if d == 0 else 2) * rnd(64)  # 2-byte types: half are not 4-byte aligned
            ts.append((n, d, flags, addr))
        out.append(ts)
    return out


def lists_crc(lists):
    c = 0
    for ts in lists:
        for t in ts:
            c = zlib.crc32(struct.pack("<qiIQ", *t), c)
    return c


def _arr(N, ts, extra_flags=0):
    arr = (N.FksTensor * max(len(ts), 1))()
    for i, (n, d, flags, addr) in enumerate(ts):
        arr[i].data = addr if n else None
        arr[i].numel = n
        arr[i].dtype = d
        arr[i].flags = flags | extra_flags
    return arr


def record(N, L, ts):
    """Every host result of one list that needs no device, as one JSON-able dict."""
    def ok(rc):
        assert rc == 0, L.fks_last_error()

    nt = len(ts)
    mt, rocm = _arr(N, ts), _arr(N, ts, STREAM_ROCM)
    out = {}
    w = ctypes.c_int64(0)
    ok(L.fks_stream_length(ctypes.addressof(mt), nt, ctypes.byref(w)))
    out["stream_length"] = w.value
    b = ctypes.c_size_t(0)
    out["workspace"] = []
    for k in (1, 4, 5, 19, 20, 64, 65):
        ok(L.fks_workspace_size(ctypes.addressof(mt), nt, k, ctypes.byref(b)))
        out["workspace"].append(b.value)
    out["delta_workspace"] = []
    for k in (1, 20, 65):
        ok(L.fks_delta_workspace_size(ctypes.addressof(mt), nt, k, ctypes.byref(b)))
        out["delta_workspace"].append(b.value)
    ok(L.fks_project_workspace_size(ctypes.addressof(rocm), nt, 65, ctypes.byref(b)))
    out["project_workspace"] = b.value
    out["project_multi_workspace"] = []
    for nvec in (1, 4, 5):
        ok(L.fks_project_multi_workspace_size(ctypes.addressof(rocm), nt, 65, nvec, ctypes.byref(b)))
        out["project_multi_workspace"].append(b.value)
    # fks_shard_census: per stream and shard count, the CRC-32 of (range, written[]) of every shard
    for name, arr in (("census_mt", mt), ("census_rocm", rocm)):
        out[name] = []
        for nshards in (1, 3, 8):
            c = 0
            for r in range(nshards):
                rng = (ctypes.c_int64 * 2)()
                wr = (ctypes.c_int64 * max(nt, 1))()
                ok(L.fks_shard_census(ctypes.addressof(arr), nt, r, nshards, rng, wr))
                c = zlib.crc32(bytes(rng) + bytes(wr)[:8 * nt], c)
            out[name].append(c)
    st = np.zeros(624, np.uint32)
    left, nxt, valid, normal = ctypes.c_int32(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_double(0.0)
    ok(L.fks_cpu_generator_end(ctypes.addressof(mt), nt, 12345, st.ctypes.data, ctypes.byref(left), ctypes.byref(nxt),
                               ctypes.byref(valid), ctypes.byref(normal)))
    out["generator_end"] = [zlib.crc32(st.tobytes()), left.value, nxt.value, valid.value, normal.value.hex()]
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_planning_invariants_standalone_sanitized(tmp_path):
    exe = tmp_path / "plan_selftest"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-mpclmul", "-msse4.1", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tools", "plan", "plan_selftest.cpp"), os.path.join(CSRC, "fks_layout.cpp"),
                    os.path.join(CSRC, "fks_phx.cpp"), os.path.join(CSRC, "fks_gf2.cpp"), "-o", str(exe)], check=True)
    assert b"amdhip64" not in exe.read_bytes()  # no HIP runtime among its libraries (nor anywhere else)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plan_selftest ok" in r.stdout
    # the program drew the lists this module (and the recorded results) use
    assert f"lcg lists crc {lists_crc(lcg_lists()):08x}" in r.stdout, r.stdout


def test_host_results_equal_the_recorded_parent():
    from fate_llm.algo.fedkseed import _native as N
    L = N.load()
    with open(GOLDEN) as f:
        gold = json.load(f)
    lcg = lcg_lists()
    assert gold["lcg_lists_crc"] == lists_crc(lcg)
    assert len(gold["hand"]) == len(HAND)
    assert 50 <= len(gold["lcg"]) <= len(lcg)
    for name, lists in (("hand", HAND), ("lcg", lcg)):
        for i, want in enumerate(gold[name]):
            assert record(N, L, lists[i]) == want, (name, i, lists[i])
