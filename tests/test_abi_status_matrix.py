"""Every checked entry point of the C ABI returns, for every one or two mutations of a valid
call, the status it returned before its argument checks were put on the shared pieces of
rpkt_amd/csrc/rpkt_args.h: tests/golden/abi_status.json, recorded by
tests/golden/make_abi_status.py from the library built before that change.  The order of an
entry's checks, its documented deviations from its family's order included
(include/rpkt_gpu.h, at enum rpkt_err), is therefore pinned.

CPU only, and skipped where a GPU is visible: the calls carry fake device addresses, so a
check dropped by mistake must fail at the launch (RPKT_E_HIP, no device) instead of running
a kernel on them.
"""
import json
import os

import pytest
import torch

import abi_status_cases as M
from rpkt_amd import engine
from rpkt_amd.build import build_gpu

pytestmark = pytest.mark.skipif(torch.cuda.is_available(),
                                reason="fake device addresses: never where a launch could run")


@pytest.fixture(scope="module")
def L():
    build_gpu()
    return engine.lib()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "abi_status.json")) as fh:
        return json.load(fh)


def test_the_golden_file_holds_exactly_the_matrix(golden):
    assert len(M.ENTRIES) == 22
    assert sorted(golden) == sorted(M.ENTRIES)
    for e in M.ENTRIES:
        assert sorted(golden[e]) == sorted(M.cases(e)), e
        assert M.E_HIP not in golden[e].values(), e          # a recorded launch attempt


@pytest.mark.parametrize("entry", list(M.ENTRIES))
def test_statuses_match_the_recording(L, golden, entry):
    got = {c: M.run(L, entry, c) for c in M.cases(entry)}
    assert {c: (got[c], golden[entry][c]) for c in got if got[c] != golden[entry][c]} == {}
