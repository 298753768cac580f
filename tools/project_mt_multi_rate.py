"""A/B timing of fks_project_mt_multi against fks_project_mt OF ANOTHER BUILD (the parent commit's
libfks.so) on the 7B bf16 layout of the bench, 19 seeds (one fks_project_mt pass), one MI355X:

  python tools/project_mt_multi_rate.py BASE.so [intree | VARIANT.so ...]

Each build runs in a process of its own (the C ABI through ctypes, no Python layer in the timed
region), the builds alternated AB_ROUNDS times (default 3) on the one box; HIP events around each
call on the current stream, AB_WARMUP warm-ups (2), then AB_CALLS timed calls (10); every line
carries median, min and max, and the build's ids.  BASE is timed on
  project_mt     one fks_project_mt call on the f32 concatenation (27 GB), and
  project_mt_x4  four consecutive ones;
every other build on project_mt (the kernel must not have moved) and on fks_project_mt_multi with
  m1_f32      one vector, f32 views of that buffer                  (against project_mt)
  m1_bf16     one vector, bf16, 13.5 GB                             (against project_mt)
  m2 m3 m4    two, three, four bf16 vectors, each 13.5 GB           (against M baseline calls)
-- a variant built with another FKS_PMT_MAX_VEC / FKS_PMT_SEEDSn (make variant_project_mt) takes
the same calls: the library batches what its cap does not hold in one pass -- and the last round
adds, on the first non-BASE build, zo_utils.seed_projections_in_place against
zo_utils.seed_projections on bf16 parameters with bf16 .grads on torch_cpu, end to end, with the
peak of torch's allocator above the parameters and gradients.  The summary lines at the end hold
the ratios of the medians over the rounds.  No threshold here: the figures go to DESIGN.md."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = 19

CHILD = r'''
import ctypes, json, os, statistics, sys
ROOT = os.environ["ROOT"]
sys.path.insert(0, os.path.join(ROOT, "fate-llm_amd", "python"))
sys.path.insert(0, ROOT)
import torch
import bench
LIB = os.environ["AB_LIB"]
WHAT = os.environ["AB_WHAT"].split(",")
CALLS, WARMUP, K = int(os.environ["AB_CALLS"]), int(os.environ["AB_WARMUP"]), int(os.environ["AB_SEEDS"])
dev = torch.device("cuda", 0)
numels = [int(torch.Size(s).numel()) for s in bench.llama7b_shapes()]
total, nt = sum(numels), len(numels)
g = torch.Generator().manual_seed(1)
seeds = torch.randint(0, 2**32, (K,), generator=g).numpy().astype("uint64")

def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}

def emit(what, **kw):
    print(json.dumps(dict({"lib": os.path.basename(LIB), "what": what}, **kw)), flush=True)

if WHAT == ["e2e"]:
    from fate_llm.algo.fedkseed import _native, zo_utils
    store = torch.empty(total, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    grads = torch.empty(total, dtype=torch.bfloat16, device=dev).normal_()
    params, at = [], 0
    for n in numels:
        p = torch.nn.Parameter(store[at:at + n])
        p.grad = grads[at:at + n]
        params.append(p)
        at += n
    groups = [{"params": params}]
    for name, fn in (("seed_projections", lambda: zo_utils.seed_projections(groups, seeds.tolist(), stream_mode="torch_cpu")),
                     ("seed_projections_in_place", lambda: zo_utils.seed_projections_in_place(groups, seeds.tolist(), stream_mode="torch_cpu"))):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        t = timed(fn)
        out = fn().reshape(-1).cpu()
        emit("e2e_" + name, peak_bytes_above_model_and_grads=torch.cuda.max_memory_allocated(dev) - before,
             seed0=float(out[0]), **t)
    emit("ids", build_id=_native.build_id(), source_id=_native.source_id())
    sys.exit(0)

L = ctypes.CDLL(LIB)
P, I, Z = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
from fate_llm.algo.fedkseed._native import FksTensor, FksVec, BF16, F32
for f in ("fks_build_id", "fks_source_id", "fks_last_error"):
    getattr(L, f).restype = ctypes.c_char_p
L.fks_project_mt_workspace_size.argtypes = [P, I, I, ctypes.POINTER(Z)]
L.fks_project_mt.argtypes = [P, I, P, I, P, I, I, P, P, Z, P]
if hasattr(L, "fks_project_mt_multi"):
    L.fks_project_mt_multi_workspace_size.argtypes = [P, I, I, I, ctypes.POINTER(Z)]
    L.fks_project_mt_multi.argtypes = [P, I, P, I, P, I, I, I, P, P, Z, P]

def check(rc):
    if rc:
        raise SystemExit("libfks error %d: %s" % (rc, L.fks_last_error().decode()))

# the parameters are never read (their addresses key the plan): one bf16 buffer cut into the layout
store = torch.empty(total, dtype=torch.bfloat16, device=dev)
arr = (FksTensor * nt)()
at = 0
for i, n in enumerate(numels):
    arr[i].data, arr[i].numel, arr[i].dtype, arr[i].flags = store.data_ptr() + 2 * at, n, BF16, 0
    at += n
stream = torch.cuda.current_stream(dev).cuda_stream
out = torch.empty(4 * K, dtype=torch.float64, device=dev)
nb = Z(0)
check(L.fks_project_mt_workspace_size(ctypes.addressof(arr), nt, K, ctypes.byref(nb)))
ws1 = torch.empty(nb.value, dtype=torch.uint8, device=dev)
vec = torch.empty(total, dtype=torch.float32, device=dev).normal_()

def project_mt():
    check(L.fks_project_mt(ctypes.addressof(arr), nt, seeds.ctypes.data, K, vec.data_ptr(), 0, 1, out.data_ptr(),
                           ws1.data_ptr(), nb.value, stream))

def project_mt_x4():
    for _ in range(4):
        project_mt()

def vectors(bufs, code, es):
    v = (FksVec * (len(bufs) * nt))()
    for m, b in enumerate(bufs):
        at = 0
        for i, n in enumerate(numels):
            v[m * nt + i].data, v[m * nt + i].dtype = b.data_ptr() + es * at, code
            at += n
    return v

def multi_call(v, M):
    n = Z(0)
    check(L.fks_project_mt_multi_workspace_size(ctypes.addressof(arr), nt, K, M, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device=dev)
    def fn():
        check(L.fks_project_mt_multi(ctypes.addressof(arr), nt, seeds.ctypes.data, K, ctypes.addressof(v), M, 0, 1,
                                     out.data_ptr(), ws.data_ptr(), n.value, stream))
    return fn

ids = {"build_id": L.fks_build_id().decode(), "source_id": L.fks_source_id().decode()}
for what in WHAT:
    if what == "project_mt":
        t = timed(project_mt); seed0 = float(out[0])
    elif what == "project_mt_x4":
        t = timed(project_mt_x4); seed0 = float(out[0])
    elif what == "m1_f32":
        t = timed(multi_call(vectors([vec], F32, 4), 1)); seed0 = float(out[0])
    else:
        M = int(what[1])
        if "half" not in globals():
            half = [torch.empty(total, dtype=torch.bfloat16, device=dev).normal_() for _ in range(4)]
        t = timed(multi_call(vectors(half[:M], BF16, 2), M)); seed0 = float(out[0])
    emit(what, seed0=seed0, **dict(t, **ids))
'''

BASE_WHAT = "project_mt,project_mt_x4"
NEW_WHAT = os.environ.get("AB_NEW_WHAT", "project_mt,m1_f32,m1_bf16,m2,m3,m4")  # a subset: a quick look at variants


def _child(lib, what):
    env = dict(os.environ, ROOT=ROOT, AB_LIB=lib, AB_WHAT=what, AB_CALLS=os.environ.get("AB_CALLS", "10"),
               AB_WARMUP=os.environ.get("AB_WARMUP", "2"), AB_SEEDS=os.environ.get("AB_SEEDS", str(SEEDS)))
    if what == "e2e":
        env["FKS_LIB_OVERRIDE"] = lib
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=600)
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    for row in rows:
        print(json.dumps(row), flush=True)
    if r.returncode != 0:
        print(json.dumps({"lib": lib, "what": what, "error": (r.stderr or r.stdout)[-800:]}), flush=True)
        raise SystemExit(1)  # nothing more on the GPU after a failed child
    return rows


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    intree = os.path.join(ROOT, "fate-llm_amd", "python", "fate_llm", "algo", "fedkseed", "libfks.so")
    base = os.path.abspath(sys.argv[1])
    news = [intree if a == "intree" else os.path.abspath(a) for a in (sys.argv[2:] or ["intree"])]
    rounds = int(os.environ.get("AB_ROUNDS", "3"))
    med = {}
    for r in range(rounds):
        for lib, what in [(base, BASE_WHAT)] + [(n, NEW_WHAT) for n in news]:
            for row in _child(lib, what):
                med.setdefault((os.path.basename(lib) if lib != base else "BASE", row["what"]), []).append(row["ms_median"])
    if os.environ.get("AB_E2E", "1") != "0":
        _child(news[0], "e2e")
    m = {k: statistics.median(v) for k, v in med.items()}
    spread = {k: [min(v), max(v)] for k, v in med.items()}

    def ratio(a, b, times=1):
        return round(m[a] / (times * m[b]), 4) if a in m and b in m else None

    for n in news:
        nm = os.path.basename(n)
        print(json.dumps({"summary": nm, "rounds": rounds, "seeds": int(os.environ.get("AB_SEEDS", str(SEEDS))),
                          "base_project_mt_ms": m["BASE", "project_mt"],
                          "base_project_mt_ms_over_rounds": spread["BASE", "project_mt"],
                          "project_mt_over_base": ratio((nm, "project_mt"), ("BASE", "project_mt")),
                          "m1_f32_over_base_project_mt": ratio((nm, "m1_f32"), ("BASE", "project_mt")),
                          "m1_bf16_over_base_project_mt": ratio((nm, "m1_bf16"), ("BASE", "project_mt")),
                          "m2_over_2_base_project_mt": ratio((nm, "m2"), ("BASE", "project_mt"), 2),
                          "m3_over_3_base_project_mt": ratio((nm, "m3"), ("BASE", "project_mt"), 3),
                          "m4_over_base_project_mt_x4": ratio((nm, "m4"), ("BASE", "project_mt_x4"))}), flush=True)


if __name__ == "__main__":
    main()
