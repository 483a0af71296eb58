"""CPU tier of the product-shape conv check (tests/product_shapes.py): the fp64 box / full-reduction references are
themselves tested against the whole-volume formulation, and the recorder, the signature key and the replay run on the HIP
emulator over the tiny training steps -- the dispatch of the real layer chain at emulator size, not hand-picked shapes.

The cfg0 step (heart_config('beginning', 64, 64, 32), 2 positive RoIs: b = 20 at 96^3) is NOT replayed here: on the emulator
(8 host threads) its forward pass alone did not finish within 15 minutes, before any backward or fp64 reference.  It is recorded
and replayed at full size in the GPU tier instead (tests/test_product_shapes_gpu.py, configuration "cfg0"); at emulator size
tiny_wino_finetune is the configuration whose layer chain reaches the Winograd and MFMA kernels and their remainder tiles
under CFUN_ALGO_AUTO."""
import os

import numpy as np
import pytest
import torch

import kernel_cases as kc
import module_cases as mc
import product_shapes as ps
from cfun_amd._lib import ACT_NONE, ALGO_AUTO, ALGO_DIRECT

REF_TOL = 1e-12


_case_sig = ps.case_sig


@pytest.mark.parametrize("name", sorted(kc.CONV_CASES))
def test_box_reference_equals_whole_volume_fp64(name):
    """No kernel involved: on every kernel_cases.CONV_CASES shape the box reference (y, dx; boxes shrunk to fit the volume)
    and the full-reduction references (dw, dshift, dres) equal the whole-volume float64 ref_conv + autograd to 1e-12."""
    n, dhw, ci, co, k, kw = kc.CONV_CASES[name]
    s = _case_sig(n, dhw, ci, co, k, **kw)
    t = {key: (None if v is None else v.double()) for key, v in ps.make_tensors(s, "cpu").items()}
    leaf = {key: (None if t[key] is None else t[key].clone().requires_grad_(True)) for key in ("x", "w", "shift", "res")}
    y = kc.ref_conv(leaf["x"], leaf["w"], ps._spec(s), t["scale"], leaf["shift"], leaf["res"])
    assert tuple(y.shape) == ps.y_shape(s)
    y.backward(t["gy"])
    box = (2, 2, 3)                      # smaller than the volumes: borders, seams and interior boxes all differ
    yboxes = ps.boxes_for(ps.out_dims(s), s.n, np.random.RandomState(1), box=box)
    assert len(yboxes) >= 4
    for b in yboxes:
        got = ps.ref_y_box(s, b, t["x"], t["w"], t["scale"], t["shift"], t["res"])
        assert kc.rel_err(got, ps.cut_y(s, y.detach(), b)) <= REF_TOL, (name, "y", b)
    gp, g = ps.conv_sum_gradients(s, t["gy"], y.detach(), t["scale"], torch.float64)
    for b in ps.boxes_for(s.dhw, s.n, np.random.RandomState(2), box=box):
        got = ps.ref_dx_box(s, b, t["w"], g)
        sample, (z, y_, x_) = b[0], b[1:]
        want = leaf["x"].grad[sample:sample + 1, z[0]:z[1], y_[0]:y_[1], x_[0]:x_[1]]
        assert float((got - want).abs().max()) <= REF_TOL * float(leaf["x"].grad.abs().max()), (name, "dx", b)
    assert kc.rel_err(ps.ref_dw_full(s, t["x"], g, torch.float64), leaf["w"].grad) <= REF_TOL, (name, "dw")
    if s.has_shift:
        assert kc.rel_err(gp.reshape(-1, gp.shape[-1]).sum(0), leaf["shift"].grad) <= REF_TOL, (name, "dshift")
    if s.res_mode:
        assert kc.rel_err(ps.ref_dres(s, gp), leaf["res"].grad) <= REF_TOL, (name, "dres")


def test_folded_up_conv_reference_fp64():
    """The references' depth-to-space handling with padded parity groups (d2s_cq) and skipped taps -- the folded up-conv of
    the U-Net's decoder -- against nearest x2 -> 3x3x3 conv written out in float64 (host only)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(3)
    n, dhw, ci, co, cqp = 2, (4, 5, 6), 8, 12, 16
    w3 = torch.randn(co, ci, 3, 3, 3, generator=gen, dtype=torch.float64)
    f = torch.zeros(2, 3, 3, dtype=torch.float64)
    for p in range(2):
        for tap in range(3):
            f[p, (p + tap - 1) // 2 + 1, tap] = 1.0
    wf = torch.einsum("oitsr,pat,qbs,ucr->pquoiabc", w3, f, f, f)          # [2,2,2,co,ci,3,3,3]
    w = torch.zeros(8, cqp, ci, 3, 3, 3, dtype=torch.float64)
    w[:, :co] = wf.reshape(8, co, ci, 3, 3, 3)
    w = w.reshape(8 * cqp, ci, 3, 3, 3)
    s = _case_sig(n, dhw, ci, 8 * cqp, (3, 3, 3), d2s=True)._replace(d2s_cq=co, tap_skip=1)
    x = torch.randn(n, *dhw, ci, generator=gen, dtype=torch.float64).requires_grad_(True)
    y = F.conv3d(F.interpolate(x.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest"), w3, padding=1).permute(0, 2, 3, 4, 1)
    gy = torch.randn(*y.shape, generator=gen, dtype=torch.float64)
    assert tuple(y.shape) == ps.y_shape(s)
    y.backward(gy)
    for b in ps.boxes_for(ps.out_dims(s), n, np.random.RandomState(1), box=(3, 3, 4)):
        assert kc.rel_err(ps.ref_y_box(s, b, x.detach(), w, None, None, None), ps.cut_y(s, y.detach(), b)) <= REF_TOL, b
    _, g = ps.conv_sum_gradients(s, gy, y.detach(), None, torch.float64)
    rows = ps.live_rows(s)
    for b in ps.boxes_for(dhw, n, np.random.RandomState(2), box=(3, 3, 4)):
        sample, (z, y_, x_) = b[0], b[1:]
        got = ps.ref_dx_box(s, b, w.index_select(0, rows), g)
        assert kc.rel_err(got, x.grad[sample:sample + 1, z[0]:z[1], y_[0]:y_[1], x_[0]:x_[1]]) <= REF_TOL, b
    # dw of the folded weight on its live taps, pulled back through the fold, is the 3x3x3 weight's gradient
    dwf = ps.ref_dw_full(s, x.detach(), g, torch.float64) * ps.live_tap_mask(s, 8 * co)
    dw3 = torch.einsum("pquoiabc,pat,qbs,ucr->oitsr", dwf.reshape(2, 2, 2, co, ci, 3, 3, 3), f, f, f)
    leaf = w3.clone().requires_grad_(True)
    F.conv3d(F.interpolate(x.detach().permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest"), leaf, padding=1).permute(
        0, 2, 3, 4, 1).backward(gy)
    assert kc.rel_err(dw3, leaf.grad) <= REF_TOL


@pytest.fixture()
def emu_direct(emu, monkeypatch):
    # whole steps on the emulator run on the direct kernels (see test_modules_emu.py); the replays then run each recorded
    # conv under the dispatcher's own choice
    monkeypatch.setenv("CFUN_CONV_ALGO", "direct")
    return emu


def _tiny(which):
    if which == "tiny_lits":
        return mc.tiny_lits_config("finetune")
    if which == "tiny_wino_finetune":
        return mc.tiny_wino_config("finetune")
    return mc.tiny_config(which.split("_", 1)[1])


def _count_forward_launches(monkeypatch):
    """Count the conv forwards at the C ABI (cfun_conv3d_fwd_fused, the only forward entry ops.py calls): a count that does
    not pass through the recorder's hook."""
    from cfun_amd import _lib
    lib, n = _lib.load(), [0]
    entry = lib.cfun_conv3d_fwd_fused

    def counted(*a):
        n[0] += 1
        return entry(*a)

    monkeypatch.setattr(lib, "cfun_conv3d_fwd_fused", counted)
    return n


@pytest.mark.parametrize("which", ["tiny_beginning", "tiny_finetune"])
def test_recorder_is_reproducible_and_complete(emu_direct, monkeypatch, which):
    """A step recorded twice gives the same calls.  Every conv forward the library launches is a recorded call (frozen and
    no-grad convs included: they make no autograd node, so they are counted at the C ABI), and the recorded calls that want a
    gradient are the _Conv3d nodes of the step's autograd graph.  Signatures hold nothing that differs between two runs."""
    cfg = _tiny(which)
    launches = _count_forward_launches(monkeypatch)
    a, nodes = ps.record_step(cfg, emu_direct, n_pos=1, backward=False)
    assert launches[0] == len(a.calls), "%d conv forwards launched, %d recorded" % (launches[0], len(a.calls))
    b, _ = ps.record_step(cfg, emu_direct, n_pos=1, backward=False)
    assert a.calls and a.calls == b.calls
    assert nodes == sum(1 for s in a.calls if any(s.need)), (nodes, len(a.calls))
    assert len(set(a.calls)) < len(a.calls)               # shared shapes de-duplicate
    assert len({ps.sig_id(s) for s in a.sigs}) == len(a.sigs), "two signatures share one id"
    for s in a.sigs:
        assert ps.sig_from_json(ps.sig_to_json(s)) == s and hash(s) == hash(ps.sig_from_json(ps.sig_to_json(s)))


@pytest.mark.parametrize("which", ["tiny_beginning", "tiny_finetune", "tiny_lits", "tiny_wino_finetune"])
def test_replay_recorded_step(emu, which):
    """Record a tiny training step, then replay every distinct conv on its own against fp64 under the rule (the kernel's
    error <= bench.GRAD_FP64_FACTOR x the fp32 formulation's + bench.GRAD_FP64_FLOOR), on the kernels the dispatcher picks
    for it (CFUN_ALGO_AUTO)."""
    rec, _ = ps.record_step(_tiny(which), emu, n_pos=1)
    sigs = sorted(set(rec.calls), key=ps.sig_id)
    assert len(sigs) >= 10 and all(s.algo == ALGO_AUTO for s in sigs)
    assert any(s.pro for s in sigs) and any(s.stats for s in sigs) and any(s.d2s for s in sigs)
    bad = []
    for s in sigs:
        rep = ps.replay(s, emu)
        print(ps.format_row(rep))
        bad += ["%s: %s" % (ps.sig_id(rep["sig"]), f) for f in rep["failures"]]
    assert not bad, "\n".join(bad)
