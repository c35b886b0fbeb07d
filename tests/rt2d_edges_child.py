"""Child process of test_rt2d_edges_gpu.py::test_environment_variants.

CSM_RT2D_DEPTH and CSM_RT2D_HOSTKEYS are read once per process, so each
variant needs a process of its own. Runs the batch-boundary and tie cases
through Match and prints one JSON list of {"name", "bits", "pose"}: the score
as its float32 bit pattern, the pose as three doubles (repr round-trips them).
Reads nothing outside the repository and needs no oracle."""
import importlib.util
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TESTS)

import rt2d_edges_support as support  # noqa: E402


def load_package():
    pkg_dir = os.path.join(os.path.dirname(TESTS), "cartographer-1_amd")
    spec = importlib.util.spec_from_file_location(
        "cartographer_amd", os.path.join(pkg_dir, "__init__.py"),
        submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["cartographer_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    csm = load_package()
    out = []
    for case in support.child_cases():
        score, pose = case.match(csm)
        out.append({"name": case.name, "bits": int(np.float32(score).view(np.uint32)),
                    "pose": [float(v) for v in pose]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
