#!/usr/bin/env python3
"""Record tests/golden/symmetric_product_bits.json on a GPU: the cases of tests/test_gpu_symmetric_bits.py, computed by the library
as it is built in this tree.

    python tests/golden/make_symmetric_bits.py COMMIT [OUTPUT]

COMMIT is the commit the library was built from; it is written into the file next to the compiler's version line.  The file pins
the summation order of the symmetric kernels: run this only on a build whose symmetric kernels are known to be what they should be
(the commit before a change to them), never to make a failing test pass."""
import importlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_symmetric_bits as T     # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN_FILE
    lam = importlib.import_module("2024-eumaster4hpc-student-challenge_amd")
    ver = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    hipcc = next((l.strip() for l in ver.splitlines() if "HIP version" in l), ver.splitlines()[0].strip() if ver else "unknown")
    cases = {}
    for case in T.CASES:
        cases[T.case_id(case)] = T.record(T.compute(lam, case))
        print(T.case_id(case), cases[T.case_id(case)]["sha256"], flush=True)
    with open(out, "w") as f:
        json.dump({"commit": commit, "hipcc": hipcc, "library_build_id": lam.lib().lam_hip_build_id().decode(),"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
