"""Write tests/golden/create_layout.json: the layout counters (device bytes, modelled K_eff traffic) of every
create path of tests/test_gpu_create_paths.py, from the library CWF_LIB_PATH selects (default: the tree's).

The counters are integers decided by create's host layout code; a handle is needed to read them, so this runs
on a GPU. It was run once against the library of the commit before cwf_hip_system_create was split into stages,
which is what pins that refactor (and any later one) to the same layouts.
Run: python tests/golden/make_create_layout.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "civiwave-fem_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_create_paths as T  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in sorted(T.CASES):
        for k in T.KNOBS:
            os.environ.pop(k, None)
        os.environ.update(T.CASES[name][2])
        s, _ = T.build(name)
        kern = T.kernel_name(s)
        out[name] = T.layout_counters(s)
        print(name, kern, out[name])
        s.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "create_layout.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
