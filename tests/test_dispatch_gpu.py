"""GPU tier (real library, cuda:0) of the conv dispatch edges: every case of dispatch_cases.py.  ``CFUN_PARITY_TABLE=<file>``
appends the printed rows to a file (profiles/dispatch_parity.txt is such a run)."""
import os

import pytest

import dispatch_cases as dc

pytestmark = pytest.mark.gpu


def _emit(line):
    print(line)
    path = os.environ.get("CFUN_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_dispatch_case(gpu, name):
    dc.check_case(gpu, name, emit=_emit)


def test_pointwise_misaligned(gpu):
    dc.check_pointwise_misaligned(gpu)


def test_pointwise_prologue_limit(gpu):
    dc.check_pointwise_prologue_limit(gpu)


def test_wino_workspace_fallback(gpu):
    dc.check_wino_workspace_fallback(gpu)


def test_short_workspace_refused(gpu):
    dc.check_short_workspace_refused(gpu)


def test_algo_mfma_refused(gpu):
    dc.check_algo_mfma_refused(gpu)


@pytest.mark.parametrize("name", sorted(dc.EMPTY_CASES))
def test_empty_problem(gpu, name):
    dc.check_empty(gpu, name)
