"""GPU tier of the guard-band / poison tier (tests/guard.py): everything in test_kernels_gpu.py (the large conv shapes and the
4096-box NMS included), every seed of test_fuzz_gpu.py, the module cases at the 64x64x32 cfg0 size and the zero-size
contract on the real libcfun_hip.so, with every allocation guarded and 0xFF-poisoned and every dense input shadowed;
``verify()`` at the end of each.  The checks' own assertions and tolerances apply unchanged.  Full-size cfg2/3/4 steps are
left out on purpose: the recorded buffers stay alive until verify().  The last test accounts for the C entries that ran."""
import pytest

import guard
import guard_cases as gc
import module_cases as mc
import test_fuzz_gpu
import test_kernels_gpu

pytestmark = pytest.mark.gpu


def test_guarded_tensor_keeps_the_allocator_alignment(gpu):
    import torch
    from cfun_amd import _lib
    with guard.guarded_memory():
        for shape in ((5, 7), (1,), (3, 4, 5, 6, 20)):
            t = torch.empty(shape, device=gpu)
            assert t.is_contiguous() and t.is_cuda and _lib.ptr(t) == t.data_ptr() and t.data_ptr() % 256 == 0
            assert torch.isnan(t).all()
        assert (torch.empty(9, dtype=torch.int32, device=gpu) == -1).all()
        assert (_lib.workspace(10, t) == 255).all() and _lib.workspace(0, t).numel() == 0
        assert guard.verify() == 6


guard.guarded_copies(test_kernels_gpu, globals(), "kernels")
guard.guarded_copies(test_fuzz_gpu, globals(), "fuzz")


@guard.guarded
def test_guard_cases(gpu):
    gc.check_all(gpu)


@guard.guarded
def test_zero_size_contract(gpu):
    gc.check_zero_size(gpu)


@guard.guarded
def test_unet_golden(gpu):
    mc.check_unet_golden(gpu, "unet_beginning_train")


@guard.guarded
def test_training_step_cfg0_vs_oracle(gpu):
    """BASELINE.json configs[0] shape (64x64x32, b = 20, 96^3 crops, 'beginning'), 2 positive RoIs."""
    from cfun_amd import config
    mc.check_training_step_vs_oracle(gpu, config.heart_config("beginning", 64, 64, 32), n_pos=2)


@guard.guarded
def test_flat_sgd(gpu):
    mc.check_flat_sgd(gpu)


@guard.guarded
def test_unmold_golden(gpu):
    mc.check_unmold_golden(gpu)


@guard.guarded
def test_unmold_lits_golden(gpu):
    mc.check_unmold_lits_golden(gpu)


@guard.guarded
def test_input_pipeline(gpu):
    mc.check_input_pipeline(gpu)


@guard.guarded
def test_resize_kat_device(gpu):
    mc.check_resize_kat_device(gpu)


@guard.guarded
def test_detection_target_layer(gpu):
    mc.check_detection_target_layer(gpu)
    mc.check_detection_target_layer(gpu, lits=True)


@guard.guarded
def test_classifier_golden(gpu):
    mc.check_classifier_golden(gpu)


@guard.guarded
def test_proposal_layer_golden(gpu):
    mc.check_proposal_layer_golden(gpu)


def test_zz_every_launching_entry_ran_under_guard():
    """Runs last in this file: the C entries the proxy saw against _lib.EXPORTS (needs the whole file to have run)."""
    gc.check_coverage(gc.EXEMPT_GPU, "gpu")
