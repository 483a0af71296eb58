"""CPU tier of the guard-band / poison tier (tests/guard.py): the mechanism's self-tests (plain torch), then every case of
test_kernels_emu.py and test_fuzz_emu.py, a set of module cases and the zero-size contract of the wrappers on the HIP
emulator with every allocation guarded and 0xFF-poisoned and every dense input shadowed, ``verify()`` at the end of each.
The checks' own assertions and tolerances apply unchanged.  The last test accounts for the C entries that ran under guard."""
import re

import pytest
import torch

import guard
import guard_cases as gc
import module_cases as mc
import test_fuzz_emu
import test_kernels_emu


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # (as in test_modules_emu.py: module-sized graphs run the direct kernels on the emulator)
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


# ---------------------------------------------------------------------------------------------- the mechanism itself
def _record_of(t):
    return next(r for r in guard._STATE.records if r.buf.untyped_storage().data_ptr() == t.untyped_storage().data_ptr())


@pytest.mark.parametrize("where", ["front", "back", "payload_end_plus_1"])
def test_one_byte_write_into_a_band_is_reported(where):
    with guard.guarded_memory():
        t = torch.empty((3, 5), dtype=torch.float32)          # 60 bytes: the back band starts off any 256-byte boundary
        buf = _record_of(t).buf
        off = {"front": guard.BAND - 3, "back": guard.BAND + 60 + 100, "payload_end_plus_1": guard.BAND + 60}[where]
        buf[off] = 7
        with pytest.raises(guard.GuardError) as e:
            guard.verify()
        msg = str(e.value)
        assert ("front band" if where == "front" else "back band") in msg
        assert "(3, 5)" in msg and "torch.float32" in msg and "1 byte(s) changed" in msg
        assert re.search(r"test_guard_emu\.py:\d+", msg), msg          # the allocation site
        want = {"front": "3 .. 3 bytes BEFORE", "back": "101 .. 101 bytes PAST", "payload_end_plus_1": "1 .. 1 bytes PAST"}[where]
        assert want in msg, msg
        assert guard.verify() == 0                                     # the records were released


def test_workspace_is_exact_and_the_site_inside_the_package_is_named(emu):
    from cfun_amd import _lib, ops
    with guard.guarded_memory():
        ws = _lib.workspace(10, torch.zeros(1))
        assert ws.numel() == 10 and (ws == 255).all()                  # exactly the bytes asked for, no 256-byte floor
        assert _lib.workspace(0, ws).numel() == 0
        _record_of(ws).buf[guard.BAND + 10] = 0
        with pytest.raises(guard.GuardError, match=r"back band of workspace \(10,\) torch.uint8"):
            guard.verify()
        y = ops.add(torch.ones(2, 3), torch.ones(2, 3))                # its output is a torch.empty_like inside ops.py
        _record_of(y).buf[guard.BAND - 1] = 0
        with pytest.raises(guard.GuardError, match=r"front band of empty_like \(2, 3\) torch.float32 \(24 bytes\) allocated at "
                                                   r"cfun_amd/ops\.py:\d+: 1 byte"):
            guard.verify()


def test_untouched_buffers_pass():
    with guard.guarded_memory():
        a = torch.empty(7)
        a.fill_(1.0)
        torch.zeros((2, 3), dtype=torch.int32).add_(1)
        torch.empty_like(a).copy_(a)
        a.new_zeros((0, 4))
        assert guard.verify() == 4


def test_poison_reads_back_as_nan_minus_one_255():
    with guard.guarded_memory():
        assert torch.isnan(torch.empty((4, 3), dtype=torch.float32)).all()
        assert torch.isnan(torch.empty_like(torch.ones(5))).all()
        assert (torch.empty(6, dtype=torch.int32) == -1).all()
        assert (torch.empty(6, dtype=torch.uint8) == 255).all()
        assert torch.isnan(torch.ones(3).new_empty((2, 2))).all()
        z = torch.zeros((2, 2))
        assert (z == 0).all() and (torch.zeros_like(z) == 0).all() and (z.new_zeros(3) == 0).all()
        assert (_record_of(z).buf[:guard.BAND] == 255).all()          # zeros keep their zeros, the bands the poison
        guard.verify()


def test_patching_is_undone_also_after_a_failure():
    from cfun_amd import _lib, loss_ops, ops, optim, weights
    before = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.new_zeros, torch.Tensor.new_empty,
              _lib.load, _lib.ptr, _lib.workspace, ops.ptr, ops.ptr_raw, ops.workspace, weights.ptr, loss_ops.ptr, optim.ptr)
    with pytest.raises(ZeroDivisionError):
        with guard.guarded_memory():
            assert torch.empty is not before[0] and ops.ptr is not before[9] and weights.ptr is not before[12]
            1 / 0
    after = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.new_zeros, torch.Tensor.new_empty,
             _lib.load, _lib.ptr, _lib.workspace, ops.ptr, ops.ptr_raw, ops.workspace, weights.ptr, loss_ops.ptr, optim.ptr)
    assert all(a is b for a, b in zip(before, after))
    assert "new_zeros" not in vars(torch.Tensor) and guard._STATE is None
    assert not torch.isnan(torch.zeros(3)).any()


def test_guarded_tensor_is_a_valid_kernel_argument(emu):
    from cfun_amd import _lib
    plain = torch.empty((5, 7))
    with guard.guarded_memory():
        t = torch.empty((5, 7))
        assert t.is_contiguous() and not t._is_view() and _lib.ptr(t) == t.data_ptr()      # guarded: passed as it is
        assert t.data_ptr() % 64 == 0 and (plain.data_ptr() % 64 != 0 or t.data_ptr() % 64 == 0)
        assert guard.BAND % 256 == 0
        guard.verify()


def test_input_shadow_round_trip(emu):
    """An unguarded input is shadowed (the kernel sees a guarded copy), a piece of it lands in the same shadow, and what
    the kernel wrote through the pointer is copied back."""
    from cfun_amd import _lib, ops
    a, b = torch.arange(24.0).view(2, 3, 4), torch.ones(2, 3, 4)
    with guard.guarded_memory():
        pa = _lib.ptr(a)
        assert pa != a.data_ptr() and _lib.ptr(a) == pa and _lib.ptr(a[1:]) == pa + 48
        guard._copy_back()
        out = torch.full((2, 3, 4), -5.0)                                # (torch.full: not a guarded allocator)
        lib = _lib.load()
        _lib.check(lib.cfun_add(_lib.ptr(a), _lib.ptr(b), _lib.ptr(out), a.numel(), None), "add")
        assert torch.equal(out, a + b) and "cfun_add" in guard.SEEN["emu"]
        assert torch.equal(ops.add(a, b), a + b)
        guard.verify()


# ------------------------------------------------------------------------- every kernel and fuzz case, guarded
guard.guarded_copies(test_kernels_emu, globals(), "kernels")
guard.guarded_copies(test_fuzz_emu, globals(), "fuzz")


@guard.guarded
def test_guard_cases(emu):
    """The small cases that exist for this tier's coverage (entries the other kernel cases do not reach)."""
    gc.check_all(emu)


@guard.guarded
def test_zero_size_contract(emu):
    gc.check_zero_size(emu)


# ----------------------------------------------------------------------------------------------- module cases, guarded
@guard.guarded
def test_unet_golden(emu_direct):
    mc.check_unet_golden(emu_direct, "unet_beginning_train")


@guard.guarded
def test_training_step_vs_oracle(emu_direct):
    # (stage and arguments of test_modules_emu.py::test_training_step_vs_oracle[beginning])
    r = mc.check_training_step_vs_oracle(emu_direct, mc.tiny_config("beginning"), n_pos=1, fp64_bound=False)
    assert all(l == l for l in r["losses"])


@guard.guarded
def test_flat_sgd(emu):
    mc.check_flat_sgd(emu)


@guard.guarded
def test_unmold_golden(emu):
    mc.check_unmold_golden(emu)


@guard.guarded
def test_unmold_lits_golden(emu):
    mc.check_unmold_lits_golden(emu)


@guard.guarded
def test_input_pipeline(emu):
    mc.check_input_pipeline(emu)


@guard.guarded
def test_resize_kat_device(emu):
    mc.check_resize_kat_device(emu)


@guard.guarded
def test_detection_target_layer(emu):
    mc.check_detection_target_layer(emu)
    mc.check_detection_target_layer(emu, lits=True)


@guard.guarded
def test_classifier_golden(emu):
    mc.check_classifier_golden(emu)


@guard.guarded
def test_proposal_layer_golden(emu):
    mc.check_proposal_layer_golden(emu)


# ------------------------------------------------------------------------------------------------ coverage accounting
def test_zz_every_launching_entry_ran_under_guard():
    """Runs last in this file: the C entries the proxy saw against _lib.EXPORTS (needs the whole file to have run)."""
    gc.check_coverage(gc.EXEMPT_EMU, "emu")
