"""CPU tier: the C-ABI library builds for gfx950, loads, and exports every symbol include/cfun_hip.h declares
(no kernel is launched here); the C restatement of NMS agrees with the golden vectors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "cfun_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))


def test_header_matches_binding():
    from cfun_amd import _lib
    assert header_symbols() == sorted(_lib.EXPORTS)


def test_library_exports_every_symbol(monkeypatch):
    monkeypatch.delenv("CFUN_LIB_PATH", raising=False)
    from cfun_amd import _lib
    if not os.path.exists(_lib.DEFAULT_LIB):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(_lib.DEFAULT_LIB)
    for name in header_symbols():
        assert hasattr(lib, name), name
    lib.cfun_version.restype = ctypes.c_int
    assert lib.cfun_version() == 100
    lib.cfun_error_string.restype = ctypes.c_char_p
    assert b"workspace" in lib.cfun_error_string(-2)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from cfun_amd import _lib
    monkeypatch.setenv("CFUN_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_cpu_tensor_rejected_by_real_library(monkeypatch):
    import torch
    from cfun_amd import _lib, ops
    monkeypatch.delenv("CFUN_LIB_PATH", raising=False)
    if not os.path.exists(_lib.DEFAULT_LIB):
        pytest.skip("library not built")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lrelu(torch.zeros(4))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "f", "tie"])
def test_c_restatement_of_nms(tag):
    so = os.path.join(ROOT, "oracle", "_build", "libnms_ref.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = ctypes.CDLL(so)
    g = load_golden("nms")
    boxes = np.ascontiguousarray(g[tag + "_boxes"], np.float32)
    scores = g[tag + "_scores"]
    thr, mx = g[tag + "_cfg"]
    n = boxes.shape[0]
    order = np.lexsort((-np.arange(n), -scores)).astype(np.int32)   # score desc, ties: higher index first
    keep = np.zeros(max(n, 1), np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lib.cfun_ref_nms.restype = ctypes.c_int32
    cnt = lib.cfun_ref_nms(boxes.ctypes.data_as(fp), order.ctypes.data_as(ip), n, ctypes.c_float(thr), int(mx),
                           keep.ctypes.data_as(ip))
    np.testing.assert_array_equal(keep[:cnt], g[tag + "_keep"])


def test_input_formatting_helpers():
    """utils.mold_image / compose_image_meta / parse_image_meta (model.py:1870-1904) -- host-side, no kernel."""
    import numpy as np
    import torch
    from cfun_amd import utils
    x = np.random.default_rng(0).normal(3.0, 7.0, (4, 5, 6)).astype(np.float32)
    m = utils.mold_image(x)
    assert abs(float(m.mean())) < 1e-5 and abs(float(m.std()) - 1.0) < 1e-5
    np.testing.assert_allclose(utils.mold_image(torch.from_numpy(x)).numpy(), m, rtol=1e-5, atol=1e-6)
    meta = utils.compose_image_meta(7, [1, 32, 64, 64], (0, 0, 0, 32, 64, 64), np.zeros(8, np.int32))[None]
    iid, shape, window, active = utils.parse_image_meta(meta)
    assert int(iid[0]) == 7 and list(shape[0]) == [1, 32, 64, 64] and list(window[0]) == [0, 0, 0, 32, 64, 64]
    assert active.shape == (1, 8)


def test_conv_kernel_selection(emu):
    """Which kernel family AUTO picks for the benchmarked shapes (cfun_conv3d_fwd_kernel): the measured per-shape rules of
    DESIGN section 3.9 must not drift silently.  Host-side logic only (no launch)."""
    import ctypes as C
    from cfun_amd import _lib, ops
    lib = _lib.load()
    DIRECT, MFMA, WINO, STEM, POINTWISE = 0, 1, 2, 3, 4

    def kern(shape, **spec):
        p = ops._params(ops.ConvSpec(**spec), shape, False, False, False)
        return int(lib.cfun_conv3d_fwd_kernel(C.byref(p)))

    k3 = dict(k=(3, 3, 3), pad=(1, 1, 1))
    assert kern((4, 96, 96, 96, 40), co=40, **k3) == WINO                      # conv_norm_lrelu_l4.0, the dominant launch
    assert kern((4, 48, 48, 48, 80), co=80, **k3) == WINO
    assert kern((1, 16, 32, 32, 128), co=256, **k3) == WINO                    # rpn.conv_shared
    assert kern((2, 8, 8, 8, 40), co=40, k=(3, 3, 3), pad=(0, 1, 1)) == WINO   # a depth slab that arrives with its halo
    assert kern((4, 96, 96, 96, 20), co=20, **k3) == MFMA                      # 32-wide tile would pad C_out = 20 by 37 %
    assert kern((4, 96, 96, 96, 40), co=40, algo=_lib.ALGO_MFMA, **k3) == MFMA
    assert kern((4, 96, 96, 96, 20), co=40, stride=2, **k3) == MFMA            # stride 2
    assert kern((4, 48, 48, 48, 40), co=8 * 32, d2s=True, d2s_cq=20, tap_skip=True, **k3) == MFMA   # parity-folded up-conv
    assert kern((4, 96, 96, 96, 8), co=64, d2s=True, **k3) == MFMA             # folded 5x5x5 conv: forward stays direct
    assert kern((4, 96, 96, 96, 1), co=20, **k3) == STEM
    assert kern((4, 96, 96, 96, 40), co=8, k=(1, 1, 1), pad=(0, 0, 0)) == POINTWISE
    assert kern((1, 8, 8, 8, 3), co=5, **k3) == DIRECT                         # channel counts the MFMA tiles cannot take

    def plan(shape, **spec):
        p = ops._params(ops.ConvSpec(**spec), shape, False, False, False)
        out = (C.c_int32 * 4)()
        rc = int(lib.cfun_conv3d_wino_plan(C.byref(p), out))
        return rc, [int(v) for v in out]

    # the Winograd plan: {2-D, subtiles per channel tile, two-waves-per-SIMD 2-D loop, columns computed}
    assert plan((4, 96, 96, 96, 40), co=40, **k3) == (0, [0, 3, 0, 48])        # > 2^19 voxels: x axis only, 48-wide tiles
    assert plan((4, 48, 48, 48, 40), co=40, **k3) == (0, [1, 3, 0, 48])        # 2-D, 192 accumulators: one wave per SIMD
    assert plan((4, 48, 48, 48, 80), co=80, **k3) == (0, [1, 1, 1, 80])        # five 16-wide tiles
    assert plan((4, 24, 24, 24, 160), co=160, **k3) == (0, [1, 2, 1, 160])
    assert plan((4, 96, 96, 96, 64), co=64, **k3) == (0, [0, 2, 0, 64])
    assert plan((4, 96, 96, 96, 20), co=20, **k3)[0] != 0                      # not a Winograd launch


def test_tile_header_matches_binding(monkeypatch):
    """include/cfun_tile.h (the tile queries and cfun_conv3d_bwd_kernels) is bound one to one by _lib.TILE_SIGNATURES and every
    entry is exported by the built library."""
    from cfun_amd import _lib
    txt = open(os.path.join(ROOT, "include", "cfun_tile.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(cfun_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.TILE_EXPORTS) and "cfun_conv3d_bwd_kernels" in names
    assert not set(names) & set(_lib.EXPORTS)
    monkeypatch.delenv("CFUN_LIB_PATH", raising=False)
    if not os.path.exists(_lib.DEFAULT_LIB):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(_lib.DEFAULT_LIB)
    for name in names:
        assert hasattr(lib, name), name


def test_conv_backward_kernel_selection(emu):
    """cfun_conv3d_bwd_kernels, the counterpart of cfun_conv3d_fwd_kernel for the two gradients, at the benchmarked shapes and
    at the shapes whose predicates admitted convs their kernels do not implement (tests/dispatch_cases.py).  Host-side logic
    only (no launch)."""
    import ctypes as C
    from cfun_amd import _lib, ops
    lib = _lib.load()
    DIRECT, MFMA, WINO, S2FOLD, C1 = 0, 1, 2, 3, 4

    def kern(shape, **spec):
        p = ops._params(ops.ConvSpec(**spec), shape, False, False, False)
        out = (C.c_int32 * 2)()
        assert int(lib.cfun_conv3d_bwd_kernels(C.byref(p), out)) == 0
        return int(out[0]), int(out[1])

    k3 = dict(k=(3, 3, 3), pad=(1, 1, 1))
    assert kern((4, 96, 96, 96, 40), co=40, **k3) == (WINO, WINO)                       # conv_norm_lrelu_l4.0
    assert kern((4, 96, 96, 96, 20), co=20, **k3) == (MFMA, MFMA)
    assert kern((4, 96, 96, 96, 20), co=40, stride=2, **k3) == (S2FOLD, MFMA)
    assert kern((4, 95, 96, 96, 20), co=40, stride=2, **k3) == (DIRECT, MFMA)           # an odd extent: no fold
    assert kern((4, 96, 96, 96, 1), co=20, **k3) == (DIRECT, C1)
    assert kern((4, 96, 96, 96, 40), co=8, k=(1, 1, 1), pad=(0, 0, 0)) == (MFMA, MFMA)
    assert kern((1, 8, 8, 8, 3), co=5, **k3) == (DIRECT, DIRECT)
    assert kern((4, 96, 96, 96, 40), co=40, algo=_lib.ALGO_DIRECT, **k3) == (DIRECT, DIRECT)
    assert kern((4, 48, 48, 48, 40), co=8 * 32, d2s=True, d2s_cq=20, tap_skip=True, **k3) == (MFMA, MFMA)   # folded up-conv
    # depth-to-space: the C_in = 1 weight gradient and the folded stride-2 data gradient read g as a plain tensor, the s2d
    # gather of the MFMA data gradient exists for 3x3x3 with whole channel quads per parity only
    assert kern((1, 5, 6, 18, 1), co=16, d2s=True, **k3) == (DIRECT, DIRECT)
    assert kern((1, 8, 8, 12, 4), co=64, stride=2, d2s=True, **k3) == (DIRECT, MFMA)
    assert kern((1, 4, 5, 6, 8), co=32, k=(1, 1, 1), pad=(0, 0, 0), d2s=True) == (DIRECT, MFMA)
    assert kern((1, 4, 5, 6, 8), co=48, d2s=True, **k3) == (DIRECT, DIRECT)
    p = ops._params(ops.ConvSpec(co=16, stride=2, **k3), (1, 8, 8, 8, 8), False, False, False)
    p.stride = 3
    assert int(lib.cfun_conv3d_bwd_kernels(C.byref(p), (C.c_int32 * 2)())) == -1         # refused parameters


def _gfx950_code_objects(path):
    """The gfx950 ELF images inside a HIP shared library: every clang offload bundle of its .hip_fatbin section."""
    import struct
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = data.find(magic)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(magic))
        q = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(magic, pos + 1)


def _kernel_metadata(elf):
    """[(kernel name, private segment (scratch) bytes per lane)] from the NT_AMDGPU_METADATA note of one code object."""
    import struct
    import msgpack
    assert elf[:4] == b"\x7fELF"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    out = []
    for i in range(shnum):
        sh = shoff + i * shentsize
        sh_type, = struct.unpack_from("<I", elf, sh + 4)
        if sh_type != 7:      # SHT_NOTE
            continue
        off, size = struct.unpack_from("<QQ", elf, sh + 0x18)
        p, end = off, off + size
        while p + 12 <= end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            p += 12
            name = elf[p:p + namesz]
            p += (namesz + 3) & ~3
            desc = elf[p:p + descsz]
            p += (descsz + 3) & ~3
            if name.startswith(b"AMDGPU") and ntype == 32:
                md = msgpack.unpackb(desc, raw=False, strict_map_key=False)
                for k in md.get("amdhsa.kernels", []):
                    out.append((k[".name"], int(k.get(".private_segment_fixed_size", 0))))
    return out


def test_no_kernel_of_the_library_uses_scratch():
    """Every kernel of libcfun_hip.so runs out of registers and LDS alone.  Not a style rule: a kernel that spills to scratch on the
    mask head's side stream corrupted 64-byte pieces of tensors the main stream was writing (the runtime's scratch memory and
    freshly cudaMalloc'ed allocator blocks, round 4, tools/probe_repro.py); the code objects are checked here, on the CPU tier,
    because the failure is timing-dependent on the GPU."""
    from cfun_amd import _lib
    path = _lib.DEFAULT_LIB
    if not os.path.exists(path):
        pytest.skip("libcfun_hip.so is not built")
    kernels = [km for co in _gfx950_code_objects(path) for km in _kernel_metadata(co)]
    assert len(kernels) > 200, "expected the library's few hundred gfx950 kernels, found %d" % len(kernels)
    spilling = [(n, s) for n, s in kernels if s]
    assert not spilling, "kernels with scratch: %s" % spilling[:8]
