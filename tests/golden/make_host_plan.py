"""Record the host results of a libfks.so into tests/golden/host_plan_parent.json.

Run it against the library of the commit BEFORE a change to the host planning code, on a
machine without a device (the CU count then falls back to 256):
    FKS_LIB_OVERRIDE=/path/to/that/libfks.so python3 tests/golden/make_host_plan.py
tests/test_plan_host.py (which owns the tensor lists and the recorder) asserts that the
tree's library reproduces every number.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fate-llm_amd", "python"), ROOT):
    sys.path.insert(0, p)

N_RECORDED = 120  # of the 200 LCG lists: keeps the file well under 100 KB


def main():
    import test_plan_host as T
    from fate_llm.algo.fedkseed import _native as N
    L = N.load()
    lcg = T.lcg_lists()
    gold = {"source_id": N.source_id(), "lcg_lists_crc": T.lists_crc(lcg),
            "hand": [T.record(N, L, ts) for ts in T.HAND], "lcg": [T.record(N, L, ts) for ts in lcg[:N_RECORDED]]}
    out = os.path.join(HERE, "host_plan_parent.json")
    with open(out, "w") as f:
        json.dump(gold, f, separators=(",", ":"))
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
