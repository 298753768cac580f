"""Record the bits of codec.project_mt of a libfks.so into tests/golden/project_mt_parent.json.

Run it against the library of the commit BEFORE a change to the projection kernels or to
anything they share with the update kernels, on the device the GPU tests run on:
    FKS_LIB_OVERRIDE=/path/to/that/libfks.so python3 tests/golden/make_project_mt_parent.py COMMIT
tests/test_gpu_project_mt.py (which owns the tensor list, the vector, the seeds and the
recorder) asserts that the tree's library reproduces every bit on a device of the same CU count.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fate-llm_amd", "python"), ROOT):
    sys.path.insert(0, p)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    import test_gpu_project_mt as T
    from fate_llm.algo.fedkseed import _native as N
    gold = {"commit": sys.argv[1], "build_id": N.build_id(), "source_id": N.source_id(), "cu_count": T._cu_count(),
            "seeds": T.SEEDS, "bits": T.record_bits()}
    out = os.path.join(HERE, "project_mt_parent.json")
    with open(out, "w") as f:
        json.dump(gold, f, separators=(",", ":"))
        f.write("\n")
    print(out, os.path.getsize(out), "bytes", "build", gold["build_id"], "CUs", gold["cu_count"])


if __name__ == "__main__":
    main()
