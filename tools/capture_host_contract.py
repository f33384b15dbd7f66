"""Record the host contract (tests/host_contract_cases.py) of the seven handle-free libraries into tests/golden/host_contract.json.

    python tools/capture_host_contract.py --libs DIR --commit REV

DIR holds the libsta_*.so of the build to record (default: this tree's vista_slam_amd/), REV names the commit they were built from.
The fixture is recorded from the commit BEFORE a change to the libraries' host code and replayed by tests/test_host_contract.py after
it.  No GPU is needed: every call returns before its first HIP call."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import host_contract_cases as HC           # noqa: E402
from vista_slam_amd import _lib            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default=os.path.join(ROOT, "vista_slam_amd"))
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_contract.json"))
    a = ap.parse_args()
    import torch  # noqa: F401      (one HIP runtime per process: see _lib.load())
    libs = {}
    for name in HC.LIBRARIES:
        libs[name] = C.CDLL(os.path.join(a.libs, "libsta_%s.so" % name))
        for fn, (res, args) in HC.signatures(_lib, name).items():
            getattr(libs[name], fn).restype, getattr(libs[name], fn).argtypes = res, args

    def plan(name, fn, args):
        r = HC.call(_lib, libs[name], name, fn, args)
        assert r["rc"] == 0, (fn, args, r)
        return r["sizes"]
    records = []
    for name, kind, fn, args in HC.cases(plan):
        r = HC.call(_lib, libs[name], name, fn, args)
        assert (r["rc"] == 0) == (kind == "plan"), (name, kind, fn, args, r)
        records.append({"lib": name, "kind": kind, "fn": fn, "args": args, **r})
    with open(a.out, "w") as f:
        f.write('{"commit": %s, "records": [\n' % json.dumps(a.commit))
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")
    print(len(records), "records ->", a.out)


if __name__ == "__main__":
    main()
