"""CPU tier (HIP emulator, same kernel sources) of the conv dispatch edges: every case of dispatch_cases.py."""
import pytest

import dispatch_cases as dc


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_dispatch_case(emu, name):
    dc.check_case(emu, name)


def test_pointwise_misaligned(emu):
    dc.check_pointwise_misaligned(emu)


def test_pointwise_prologue_limit(emu):
    dc.check_pointwise_prologue_limit(emu)


def test_wino_workspace_fallback(emu):
    dc.check_wino_workspace_fallback(emu)


def test_short_workspace_refused(emu):
    dc.check_short_workspace_refused(emu)


def test_algo_mfma_refused(emu):
    dc.check_algo_mfma_refused(emu)


@pytest.mark.parametrize("name", sorted(dc.EMPTY_CASES))
def test_empty_problem(emu, name):
    dc.check_empty(emu, name)
