"""GPU tier of the memory-bound tier (tests/membound_cases.py): the same cases as tests/test_membound_emu.py on the real
libcfun_hip.so -- launch geometry past the 2048-block cap, value-range edges of the norm / activation / pooling kernels, the
optimizer tail, the mask losses on trained-looking logits (here with the device's __expf / __logf in the fused forward).

Every comparison appends a row (e32, the kernel's error, the bound, the ratio) to membound_cases.REPORT.  A module-scoped
fixture owns that list for this file: it empties it before the first selected test and prints the rows of whatever was
selected after the last one; ``CFUN_PARITY_TABLE=<file>`` appends them to a file (profiles/membound_parity.txt is a run of
the whole file)."""
import os

import pytest

import membound_cases as mb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    mb.REPORT.clear()
    yield
    lines = mb.report_lines()
    print("\n".join(lines))
    path = os.environ.get("CFUN_PARITY_TABLE")
    if path and lines:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    mb.REPORT.clear()


def test_launch_constants(gpu):
    mb.check_launch_constants(gpu)


# ---- A. launch geometry
@pytest.mark.parametrize("n", mb.FLAT_SMALL_N)
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3)],
                         ids=lambda o: "offs%d%d%d" % o)
def test_flat_small(gpu, n, offs):
    mb.check_flat_elementwise(gpu, n, offs)


def test_flat_two_sweeps_ragged(gpu):
    mb.check_flat_elementwise(gpu, mb.FLAT_BIG_N)


def test_flat_through_ops(gpu):
    mb.check_flat_through_ops(gpu)


@pytest.mark.parametrize("c", mb.STRIDED_C)
def test_lrelu_strided(gpu, c):
    mb.check_lrelu_strided(gpu, c)


def test_lrelu_strided_too_wide(gpu):
    mb.check_lrelu_strided_too_wide(gpu)


def test_act_bwd(gpu):
    mb.check_act_bwd(gpu)


@pytest.mark.parametrize("shape", [mb.POOL_SHAPE, mb.POOL_SHAPE_VEC4], ids=["vec1", "vec4"])
def test_upsample2_bwd(gpu, shape):
    mb.check_upsample2_bwd(gpu, shape)


def test_maxpool_geometry(gpu):
    mb.check_maxpool_geometry(gpu)


def test_halo_geometry(gpu):
    mb.check_halo_geometry(gpu)


@pytest.mark.parametrize("c", mb.CHANNEL_SUM_C)
@pytest.mark.parametrize("rows", mb.CHANNEL_SUM_ROWS)
def test_channel_sum(gpu, rows, c):
    mb.check_channel_sum(gpu, rows, c)


def test_channel_sum_paths(gpu):
    mb.check_channel_sum_paths(gpu)


@pytest.mark.parametrize("n,v,c", mb.NORM_GEOMETRY)
def test_norm_geometry(gpu, n, v, c):
    mb.check_norm_geometry(gpu, n, v, c)


def test_alignment_contract(gpu):
    mb.check_alignment_contract(gpu)


# ---- B. value range
@pytest.mark.parametrize("name", sorted(mb.NORM_RANGE_SHAPES))
def test_norm_range(gpu, name):
    mb.check_norm_range(gpu, *mb.NORM_RANGE_SHAPES[name])


def test_maxpool_values(gpu):
    mb.check_maxpool_values(gpu)


# ---- C. optimizer tail
@pytest.mark.parametrize("n_a,n_b", [(a, b) for a, b in zip(mb.SUMSQ_N, reversed(mb.SUMSQ_N))])
def test_sumsq_norm(gpu, n_a, n_b):
    mb.check_sumsq_norm(gpu, n_a, n_b)


@pytest.mark.parametrize("name", sorted(mb.SGD_RUNS))
def test_sgd_step(gpu, name):
    mb.check_sgd_step(gpu, name)


def test_flat_sgd_over_cap(gpu):
    mb.check_flat_sgd_over_cap(gpu)


# ---- D. mask losses on trained-looking inputs
@pytest.mark.parametrize("sigma", mb.MASK_RANGE_SIGMAS)
@pytest.mark.parametrize("name", sorted(mb.MASK_RANGE_SHAPES))
def test_mask_losses_range(gpu, name, sigma):
    mb.check_mask_losses_range(gpu, mb.MASK_RANGE_SHAPES[name], sigma)


def test_edge_flat_probs(gpu):
    mb.check_edge_flat_probs(gpu)


def test_edge_flat_logits(gpu):
    mb.check_edge_flat_logits(gpu)

