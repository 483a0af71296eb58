"""CPU tier of the memory-bound tier (tests/membound_cases.py): the non-conv kernels of elementwise.hip, loss.hip and
loss_fused.hip on the HIP emulator, against float64 under the product-shape tier's rule, at launch-geometry and value edges.

The GPU tier (tests/test_membound_gpu.py) runs the same cases on the real library.  No geometry case is left to the GPU
file alone: the largest ones (two grid sweeps and a ragged third: 4.2 M floats for the flat kernels, 1.05 M work items for
act_bwd / pooling / upsample / halo / the optimizer step) take one to four seconds each on the emulator.  The emulator builds
the fused mask-loss forward with expf / logf instead of the device's __expf / __logf, so what the range cases say about those
two intrinsics is said by the GPU tier alone."""
import pytest

import membound_cases as mb


def test_launch_constants(emu):
    mb.check_launch_constants(emu)


# ---- A. launch geometry
@pytest.mark.parametrize("n", mb.FLAT_SMALL_N)
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3)],
                         ids=lambda o: "offs%d%d%d" % o)
def test_flat_small(emu, n, offs):
    mb.check_flat_elementwise(emu, n, offs)


def test_flat_two_sweeps_ragged(emu):
    mb.check_flat_elementwise(emu, mb.FLAT_BIG_N)


def test_flat_through_ops(emu):
    mb.check_flat_through_ops(emu)


@pytest.mark.parametrize("c", mb.STRIDED_C)
def test_lrelu_strided(emu, c):
    mb.check_lrelu_strided(emu, c)


def test_lrelu_strided_too_wide(emu):
    mb.check_lrelu_strided_too_wide(emu)


def test_act_bwd(emu):
    mb.check_act_bwd(emu)


@pytest.mark.parametrize("shape", [mb.POOL_SHAPE, mb.POOL_SHAPE_VEC4], ids=["vec1", "vec4"])
def test_upsample2_bwd(emu, shape):
    mb.check_upsample2_bwd(emu, shape)


def test_maxpool_geometry(emu):
    mb.check_maxpool_geometry(emu)


def test_halo_geometry(emu):
    mb.check_halo_geometry(emu)


@pytest.mark.parametrize("c", mb.CHANNEL_SUM_C)
@pytest.mark.parametrize("rows", mb.CHANNEL_SUM_ROWS)
def test_channel_sum(emu, rows, c):
    mb.check_channel_sum(emu, rows, c)


def test_channel_sum_paths(emu):
    mb.check_channel_sum_paths(emu)


@pytest.mark.parametrize("n,v,c", mb.NORM_GEOMETRY)
def test_norm_geometry(emu, n, v, c):
    mb.check_norm_geometry(emu, n, v, c)


def test_alignment_contract(emu):
    mb.check_alignment_contract(emu)


# ---- B. value range
@pytest.mark.parametrize("name", sorted(mb.NORM_RANGE_SHAPES))
def test_norm_range(emu, name):
    mb.check_norm_range(emu, *mb.NORM_RANGE_SHAPES[name])


def test_maxpool_values(emu):
    mb.check_maxpool_values(emu)


# ---- C. optimizer tail
@pytest.mark.parametrize("n_a,n_b", [(a, b) for a, b in zip(mb.SUMSQ_N, reversed(mb.SUMSQ_N))])
def test_sumsq_norm(emu, n_a, n_b):
    mb.check_sumsq_norm(emu, n_a, n_b)


@pytest.mark.parametrize("name", sorted(mb.SGD_RUNS))
def test_sgd_step(emu, name):
    mb.check_sgd_step(emu, name)


def test_flat_sgd_over_cap(emu):
    mb.check_flat_sgd_over_cap(emu)


# ---- D. mask losses on trained-looking inputs
@pytest.mark.parametrize("sigma", mb.MASK_RANGE_SIGMAS)
@pytest.mark.parametrize("name", sorted(mb.MASK_RANGE_SHAPES))
def test_mask_losses_range(emu, name, sigma):
    mb.check_mask_losses_range(emu, mb.MASK_RANGE_SHAPES[name], sigma)


def test_edge_flat_probs(emu):
    mb.check_edge_flat_probs(emu)


def test_edge_flat_logits(emu):
    mb.check_edge_flat_logits(emu)
