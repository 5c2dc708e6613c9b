"""Writes tests/golden/abi_status.json: the status every call of the argument-check matrix
(tests/abi_status_cases.py) returns from the library as built, entry -> case -> status.
Record it BEFORE a change to the host code of the entry points, so that
tests/test_abi_status_matrix.py holds the change to what the library returned before it.

Run where no GPU is visible: python tests/golden/make_abi_status.py.  A case that returns
RPKT_E_HIP passed every check and tried to launch: it does not belong in the matrix (drop
the mutation the library accepts), and nothing is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    import torch
    import abi_status_cases as M
    from rpkt_amd import engine
    from rpkt_amd.build import build_gpu
    if torch.cuda.is_available():
        sys.exit("a GPU is visible: the matrix calls use fake device addresses")
    build_gpu()
    L = engine.lib()
    out = {e: {c: M.run(L, e, c) for c in M.cases(e)} for e in M.ENTRIES}
    launched = [(e, c) for e in out for c in out[e] if out[e][c] == M.E_HIP]
    if launched:
        sys.exit("passed the checks and tried to launch: %r" % launched[:20])
    with open(os.path.join(HERE, "abi_status.json"), "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d entries, %d cases" % (len(out), sum(len(v) for v in out.values())))


if __name__ == "__main__":
    main()
