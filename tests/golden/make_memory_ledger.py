"""Write tests/golden/memory_ledger.json: cwf_hip_system_memory after each stage of tests/test_gpu_memory_ledger.py
(create, solves, mode switch, modal blocks, caller-order gram, refined solves; a two-rank LOCAL PARITY shard), from
the library CWF_LIB_PATH selects (default: the tree's).

It was run once with CWF_LIB_PATH on a build of the commit before csrc/devmem.hpp gave device memory one owner
(tools/gpu_run.sh's lib_parent), which is what pins that refactor, and any later one, to the same bytes. The numbers
are integers the host layout code decides; a handle is needed to read them, so this runs on a GPU.
Run: CWF_LIB_PATH=civiwave-fem_amd/lib_parent/libcwf_hip.so python tests/golden/make_memory_ledger.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "civiwave-fem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_memory_ledger as T  # noqa: E402

if __name__ == "__main__":
    out = T.record()
    for name, stages in out.items():
        for label, nbytes in stages:
            print(name, label, nbytes)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "memory_ledger.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
