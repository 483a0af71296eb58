"""GPU tier of the product-shape conv check (tests/product_shapes.py): every distinct conv that the full-size training
steps issue -- cfg0 (64x64x32 'beginning', 2 positive RoIs), cfg2 (the benchmarked 256x256x128 'finetune' step), cfg3
(512x512x256) and both LiTS phases -- replayed on
its own at its true shape against fp64, one test per signature.

The parametrisation comes from tests/golden/product_shapes_signatures.json (``python tests/product_shapes.py
--write-manifest`` on an MI355X), so the ids are known without a GPU and stable from run to run; the steps are recorded
again here and the first test fails, naming the difference, when a model or dispatch change issues a conv the manifest does
not hold.  Nothing is skipped for size.  ``CFUN_PARITY_TABLE=<file>`` appends the printed rows to a file
(profiles/product_shapes_parity.txt is such a run)."""
import os

import pytest
import torch

import product_shapes as ps

pytestmark = pytest.mark.gpu

MANIFEST = ps.load_manifest()
ALL = sorted({s for sigs in MANIFEST.values() for s in sigs}, key=ps.sig_id)
_RECORDED = {}          # configuration -> set of Sig, filled once per session
_REPLAYED = set()


def _recorded(gpu):
    if not _RECORDED:
        for name, (make, n_pos) in ps.product_configs().items():
            rec, _ = ps.record_step(make(), gpu, n_pos=n_pos)
            _RECORDED[name] = set(rec.calls)
            print("%s: %d conv calls, %d distinct signatures" % (name, len(rec.calls), len(_RECORDED[name])))
            torch.cuda.empty_cache()
    return _RECORDED


def _emit(line):
    print(line)
    path = os.environ.get("CFUN_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def test_recorded_signatures_are_the_manifest(gpu):
    """The recorded steps issue exactly the signatures the manifest lists (so every one of them has a test below)."""
    rec = _recorded(gpu)
    assert sorted(rec) == sorted(MANIFEST)
    for name in sorted(rec):
        want = set(MANIFEST[name])
        new = sorted(ps.sig_id(s) for s in rec[name] - want)
        gone = sorted(ps.sig_id(s) for s in want - rec[name])
        assert not new and not gone, ("%s: the step issues convs the manifest does not hold %s / no longer issues %s -- "
                                      "regenerate it (python tests/product_shapes.py --write-manifest)" % (name, new, gone))
    total = set().union(*rec.values())
    _emit("# distinct signatures: " + ", ".join("%s %d" % (n, len(rec[n])) for n in sorted(rec)) + ", all %d" % len(total))


def test_cfg2_covers_every_forward_kernel_kind(gpu):
    kinds = {ps.kernel_info(s)["fwd"] for s in _recorded(gpu)["cfg2"]}
    missing = {"pointwise", "wino", "mfma", "stem"} - kinds
    assert not missing, "the cfg2 step runs no conv on the %s kernels (kinds seen: %s)" % (sorted(missing), sorted(kinds))


def test_bench_layers_table_is_current(gpu):
    """Every plain conv of tools/bench_layers.LAYERS is a conv the cfg2 step really issues: a layer without a recorded
    signature means the timing table is stale."""
    sigs = _recorded(gpu)["cfg2"]
    layers = ps.bench_layers_plain()
    assert len(layers) >= 15
    stale = [L[0] for L in layers if not any(ps.layer_matches(L, s) for s in sigs)]
    assert not stale, "tools/bench_layers.py times layers the cfg2 step does not run: %s" % stale


@pytest.mark.parametrize("sig", ALL, ids=ps.sig_id)
def test_conv_at_product_shape(gpu, sig):
    """y and dx on the boxes, dw / dshift / dres in full, the statistics epilogue and the prologue of ONE recorded conv
    against fp64: error <= bench.GRAD_FP64_FACTOR x (the fp32 host formulation's) + bench.GRAD_FP64_FLOOR."""
    rep = ps.replay(sig, gpu)
    _emit(ps.format_row(rep))
    _REPLAYED.add(sig)
    torch.cuda.empty_cache()
    assert not rep["failures"], "\n".join(rep["failures"])


def test_every_recorded_signature_was_replayed(gpu):
    recorded = set().union(*_recorded(gpu).values())
    assert _REPLAYED == recorded, sorted(ps.sig_id(s) for s in recorded ^ _REPLAYED)
