"""Guard bands and poison for the memory the HIP kernels touch (both tiers; no sanitizer, nothing preloaded).

The parity tests compare values; they do not see WHERE a kernel reads and writes.  Inside ``guarded_memory()``

* every Python-level allocator ``cfun_amd`` uses -- ``torch.empty`` / ``empty_like`` / ``zeros`` / ``zeros_like``,
  ``Tensor.new_empty`` / ``new_zeros`` and ``_lib.workspace`` -- returns a tensor that sits inside a larger byte buffer
  ``[front band | payload | back band]``.  The bands are ``BAND`` bytes each (a multiple of 256, so the payload keeps the base
  allocation's alignment); the back band starts at the payload's exact last byte + 1.  Bands and payload are filled with 0xFF
  (NaN as fp32 at any 4-byte phase, -1 as int32, 255 as uint8; ``zeros`` keep their zeros).  An output element a kernel
  leaves unwritten, or a workspace it accumulates into without initialising, is a NaN in the result; a write outside the
  payload changes a band.  ``_lib.workspace`` hands out exactly the bytes the ``*_workspace_bytes`` function reported
  (no 256-byte floor), so an under-reported size lands in the back band.
* every dense tensor whose pointer goes to the library (``_lib.ptr``, and ``ops.ptr_raw`` when the tensor is dense) and
  that is not guarded already -- the tests' inputs, autograd's gradients, parameters -- is SHADOWED: copied into a guarded
  buffer whose address the kernel gets; after the call the payload is copied back into the original on the same stream
  (some entries write through what looks like an input: ``out=`` slots, ``*_bwd_add``, the optimizer step).  A read outside
  an input therefore reads NaN, and a write outside it hits a band.
* ``_lib.load()`` returns a proxy that records which ``cfun_*`` entries were called (``SEEN``), copies the shadows back after
  each entry that launches work, and with ``CFUN_GUARD_EVERY_CALL=1`` runs ``verify()`` after every such call, so a hit
  is pinned to one C entry (slow: one device synchronisation per launch; a debugging switch).

``verify()`` synchronises, checks every band of every allocation made since the last call in one batched compare per device,
raises ``GuardError`` naming the allocation (shape, dtype, allocation site inside cfun_amd/, band, first / last changed byte,
count) and releases the recorded buffers.  Everything is restored when the context exits, also after a failure.

Known blind spots
* channel-strided views (``ops._slot_view`` / ``ConcatBuffer`` slots, strided gradients handed to ``ops.ptr_raw``, permuted
  volumes of ``ops.resize3d``) are not shadowed: no stride rule is guessed.  The ConcatBuffer itself is guarded as a whole.
* pointers that do not pass ``ptr`` (the InstanceNorm statistics in ``CfunConvFusion``, taken with ``data_ptr()``): guarded when
  ``cfun_amd`` allocated them, never shadowed.  ``RAW_POINTER_USES`` pins the number of such uses per module.
* dense sub-views of a guarded or shadowed tensor (one sample of a BatchBuffer, ``out[1:]``) share their parent's bands.
* a stray access that stays inside a neighbouring LIVE payload farther away than one band is not seen.
* ``empty_like`` of a non-contiguous tensor, pinned memory and ``out=`` allocations fall through to torch unguarded.
"""
import contextlib
import importlib
import operator
import os
import pkgutil
import re
import sys

import torch

BAND = 4096          # bytes per band: a choice (16 rows of 64 fp32 channels), not a measurement; a multiple of 256
POISON = 0xFF

SEEN = {"emu": set(), "gpu": set()}      # cfun_* entries called under guard in this process, per tier (the coverage tests)
COUNTS = {"allocations": 0, "shadows": 0, "verifies": 0, "bytes": 0}

# entries that launch nothing (host-side queries): the proxy does not copy shadows back after them
NO_LAUNCH = frozenset("""cfun_version cfun_error_string cfun_conv3d_fwd_workspace_bytes cfun_conv3d_fwd_kernel cfun_conv3d_wino_plan
cfun_conv3d_fused_support cfun_conv3d_fwd_fused_workspace_bytes cfun_conv3d_bwd_data_workspace_bytes
cfun_conv3d_bwd_weight_workspace_bytes cfun_channel_sum_workspace_bytes cfun_fc_workspace_bytes cfun_fc_bwd_weight_max_rows
cfun_instnorm_workspace_bytes cfun_nms3d_workspace_bytes cfun_loss_workspace_bytes cfun_edge_loss_bwd_workspace_bytes
cfun_mask_fused_workspace_bytes cfun_mask_fused_supported cfun_mask_fused_u_bytes cfun_ce_weighted_workspace_bytes
cfun_edge_raw_dc_bytes cfun_sumsq_partials_count cfun_weight_prepare_kinds cfun_weight_prepare_plan""".split())

# ``.data_ptr()`` occurrences per cfun_amd module that do not go through ptr / ptr_raw, reviewed for this tier: _lib.ptr itself;
# ops: three CfunConvFusion statistics pointers, two storage comparisons, two alignment tests, ptr_raw itself; weights: the
# prepared-operand arena (a torch.empty: guarded); dist / layers: identity comparisons and a cache key.  A new one fails
# guarded_memory() until it is looked at: a pointer that bypasses ptr is neither checked nor shadowed.
RAW_POINTER_USES = {"cfun_amd._lib": 1, "cfun_amd.ops": 8, "cfun_amd.weights": 1, "cfun_amd.dist": 2, "cfun_amd.layers": 1}


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ("buf", "nbytes", "shape", "dtype", "site", "kind")

    def __init__(self, buf, nbytes, shape, dtype, site, kind):
        self.buf, self.nbytes, self.shape, self.dtype, self.site, self.kind = buf, nbytes, shape, dtype, site, kind


class _State:
    def __init__(self):
        self.records = []
        self.storages = set()      # untyped-storage addresses of the live records' buffers
        self.pending = []          # shadows of the call being assembled: (lo, hi, shadow address, shadow, original)
        self.every_call = os.environ.get("CFUN_GUARD_EVERY_CALL", "0") == "1"


_STATE = None
_ORIG = {}
_HERE = os.path.abspath(__file__)
_PKG = os.sep + "cfun_amd" + os.sep


def _site():
    """file:line of the innermost frame inside cfun_amd/ (else of the first frame outside this file)."""
    f = sys._getframe(2)
    first = None
    for _ in range(40):
        if f is None:
            break
        fn = f.f_code.co_filename
        if _PKG in fn:
            return "cfun_amd/%s:%d" % (fn.rsplit(_PKG, 1)[1], f.f_lineno)
        if first is None and os.path.abspath(fn) != _HERE:
            first = "%s:%d" % (os.path.basename(fn), f.f_lineno)
        f = f.f_back
    return first or "?"


def _alloc(shape, dtype, device, zero=False, kind="empty", site=None, requires_grad=False):
    st = _STATE
    dtype = dtype if dtype is not None else torch.get_default_dtype()
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * dtype.itemsize
    buf = _ORIG["empty"](BAND + nbytes + BAND, dtype=torch.uint8, device=device)
    buf.fill_(POISON)
    if zero and nbytes:
        buf[BAND:BAND + nbytes].zero_()
    strides, acc = [], 1
    for s in reversed(shape):
        strides.append(acc)
        acc *= max(s, 1)
    # (set_ on the buffer's storage, not .view(): the result is an ordinary tensor, not an autograd view of the buffer)
    t = _ORIG["empty"](0, dtype=dtype, device=buf.device).set_(buf.untyped_storage(), BAND // dtype.itemsize, shape,
                                                              tuple(reversed(strides)))
    st.records.append(_Record(buf, nbytes, shape, dtype, site or _site(), kind))
    st.storages.add(buf.untyped_storage().data_ptr())
    COUNTS["allocations" if kind != "shadow" else "shadows"] += 1
    COUNTS["bytes"] += nbytes
    if requires_grad:
        t.requires_grad_(True)
    return t


def _size_args(args):
    try:
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        return tuple(operator.index(a) for a in args)
    except TypeError:          # symbolic or tensor sizes: torch's own path
        return None


_PLAIN_KW = {"dtype", "device", "requires_grad", "pin_memory", "layout", "memory_format"}


def _plain(kw, like=None):
    """Can this allocation be served from a guarded buffer?  (dense, pageable, contiguous, no out=)"""
    if _STATE is None or set(kw) - _PLAIN_KW or kw.get("pin_memory") or kw.get("layout", torch.strided) is not torch.strided:
        return False
    mf = kw.get("memory_format")
    if mf not in (None, torch.contiguous_format, torch.preserve_format):
        return False
    if like is not None and (not like.is_contiguous() or like.layout is not torch.strided or like.is_quantized):
        return False
    dev = kw.get("device")
    dev = like.device if dev is None and like is not None else dev
    return dev is None or torch.device(dev).type in ("cpu", "cuda")


def _make_factory(name, zero):
    orig = _ORIG[name]

    def factory(*args, **kw):
        size = _size_args(args) if args else None
        if size is None or not _plain(kw):
            return orig(*args, **kw)
        return _alloc(size, kw.get("dtype"), kw.get("device"), zero, name, requires_grad=kw.get("requires_grad", False))
    return factory


def _make_like(name, zero):
    orig = _ORIG[name]

    def like_factory(t, **kw):
        if not torch.is_tensor(t) or not _plain(kw, t):
            return orig(t, **kw)
        dev = kw.get("device")
        return _alloc(t.shape, kw.get("dtype") or t.dtype, t.device if dev is None else dev, zero, name,
                      requires_grad=kw.get("requires_grad", False))
    return like_factory


def _make_new(name, zero):
    orig = _ORIG[name]

    def new_factory(self, *args, **kw):
        size = _size_args(args) if args else None
        if size is None or not _plain(kw, None):
            return orig(self, *args, **kw)
        dev = kw.get("device")
        return _alloc(size, kw.get("dtype") or self.dtype, self.device if dev is None else dev, zero, name,
                      requires_grad=kw.get("requires_grad", False))
    return new_factory


def _workspace(nbytes, like):
    """_lib.workspace in guard mode: exactly ``nbytes`` (zero included: a valid address with the back band right at it)."""
    return _alloc((int(nbytes),), torch.uint8, like.device, False, "workspace")


def _shadow(t, p):
    st = _STATE
    if st is None or t.untyped_storage().data_ptr() in st.storages:
        return p
    nbytes = t.numel() * t.element_size()
    if nbytes == 0:
        return p
    for lo, hi, sp, _, _ in st.pending:
        if lo <= p and p + nbytes <= hi:       # the same tensor again, or a dense piece of it (g and g[1:]): one shadow
            return sp + (p - lo)
        if p < hi and lo < p + nbytes:         # overlaps without being contained: left alone
            return p
    sh = _alloc(t.shape, t.dtype, t.device, False, "shadow")
    with torch.no_grad():
        sh.copy_(t.detach())
    st.pending.append((p, p + nbytes, sh.data_ptr(), sh, t))
    return sh.data_ptr()


def _ptr(t):
    p = _ORIG["ptr"](t)
    return p if t is None else _shadow(t, p)


def _ptr_raw(t):
    p = _ORIG["ptr_raw"](t)
    return _shadow(t, p) if t.is_contiguous() else p      # (strided slot views: the documented blind spot)


def _copy_back():
    st = _STATE
    if st.pending:
        with torch.no_grad():
            for _, _, _, sh, t in st.pending:
                t.data.copy_(sh)           # (.data: the original's autograd version counter is not this test's business)
        st.pending = []


class _LibProxy:
    """The ctypes library with every cfun_* entry wrapped: record the name, copy shadows back after a launch."""

    def __init__(self, lib, emu):
        self.__dict__["_lib"] = lib
        self.__dict__["_emu"] = emu
        self.__dict__["_wrapped"] = {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cfun_"):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            launches = name not in NO_LAUNCH
            _seen = SEEN["emu" if self._emu else "gpu"]

            def w(*args, _fn=fn, _name=name, _launches=launches):
                _seen.add(_name)
                rc = _fn(*args)
                if _launches and _STATE is not None:
                    _copy_back()
                    if _STATE.every_call:
                        verify(where=_name)
                return rc
            self._wrapped[name] = w
        return w


def _load():
    from cfun_amd import _lib
    lib = _ORIG["load"]()
    return _LibProxy(lib, _lib._is_emulator)


def _check_pointer_bypass(mods):
    for name, mod in mods.items():
        src = getattr(mod, "__file__", None)
        if not src or not os.path.exists(src):
            continue
        with open(src) as f:
            n = len(re.findall(r"\.data_ptr\(\)", f.read()))
        if n != RAW_POINTER_USES.get(name, 0):
            raise GuardError("%s takes %d raw .data_ptr() (tests/guard.py knows of %d): a pointer that reaches the library past "
                             "_lib.ptr / ops.ptr_raw is neither checked nor shadowed -- route it through ptr, or review it and "
                             "update guard.RAW_POINTER_USES" % (name, n, RAW_POINTER_USES.get(name, 0)))


def _package_modules():
    import cfun_amd
    for m in pkgutil.iter_modules(cfun_amd.__path__):
        if os.path.exists(os.path.join(cfun_amd.__path__[0], m.name + ".py")):      # (not the kernel library beside them)
            importlib.import_module("cfun_amd." + m.name)
    return {n: m for n, m in sys.modules.items() if m is not None and (n == "cfun_amd" or n.startswith("cfun_amd."))}


@contextlib.contextmanager
def guarded_memory():
    """Guard mode for the duration of the block (one test).  Not re-entrant."""
    global _STATE
    if _STATE is not None:
        raise RuntimeError("guarded_memory() is already active")
    from cfun_amd import _lib, ops
    mods = _package_modules()
    _check_pointer_bypass(mods)
    _ORIG.update(empty=torch.empty, empty_like=torch.empty_like, zeros=torch.zeros, zeros_like=torch.zeros_like,
                 new_empty=torch.Tensor.new_empty, new_zeros=torch.Tensor.new_zeros,
                 ptr=_lib.ptr, ptr_raw=ops.ptr_raw, workspace=_lib.workspace, load=_lib.load)
    repl = {"ptr": _ptr, "ptr_raw": _ptr_raw, "workspace": _workspace, "load": _load}
    undo = []

    def put(obj, attr, new):
        had = attr in vars(obj)
        undo.append((obj, attr, had, vars(obj).get(attr)))
        setattr(obj, attr, new)

    _STATE = _State()
    try:
        put(torch, "empty", _make_factory("empty", False))
        put(torch, "zeros", _make_factory("zeros", True))
        put(torch, "empty_like", _make_like("empty_like", False))
        put(torch, "zeros_like", _make_like("zeros_like", True))
        put(torch.Tensor, "new_empty", _make_new("new_empty", False))
        put(torch.Tensor, "new_zeros", _make_new("new_zeros", True))
        for mod in mods.values():          # ptr & co. are imported by name into several modules: patch every holder
            for attr, new in repl.items():
                if vars(mod).get(attr) is _ORIG[attr]:
                    put(mod, attr, new)
        yield sys.modules[__name__]
    finally:
        for obj, attr, had, old in reversed(undo):
            if had:
                setattr(obj, attr, old)
            else:
                delattr(obj, attr)
        _STATE = None


def _band_report(rec, which):
    band = rec.buf[:BAND] if which == "front" else rec.buf[BAND + rec.nbytes:]
    idx = (band.cpu() != POISON).nonzero().flatten()
    first, last = int(idx[0]), int(idx[-1])
    if which == "front":
        where = "%d .. %d bytes BEFORE the payload's first byte" % (BAND - first, BAND - last)
    else:
        where = "%d .. %d bytes PAST the payload's last byte" % (first + 1, last + 1)
    return ("%s band of %s %s %s (%d bytes) allocated at %s: %d byte(s) changed, band offsets %d .. %d = %s"
            % (which, rec.kind, tuple(rec.shape), rec.dtype, rec.nbytes, rec.site, idx.numel(), first, last, where))


def verify(release=True, where=None):
    """Check every band of every allocation since the last call (one synchronisation, one batched compare per device);
    raise GuardError on a hit; release the recorded buffers."""
    st = _STATE
    if st is None:
        raise RuntimeError("verify() outside guarded_memory()")
    _copy_back()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
    COUNTS["verifies"] += 1
    recs = st.records
    hits = []
    by_dev = {}
    for r in recs:
        by_dev.setdefault(r.buf.device, []).append(r)
    for dev_recs in by_dev.values():
        for i in range(0, len(dev_recs), 2048):
            chunk = dev_recs[i:i + 2048]
            bands = []
            for r in chunk:
                bands.append(r.buf[:BAND])
                bands.append(r.buf[BAND + r.nbytes:])
            low = torch.cat(bands).view(-1, BAND).amin(dim=1).cpu()      # 0xFF is the largest byte: any change lowers the minimum
            for j in (low != POISON).nonzero().flatten().tolist():
                hits.append(_band_report(chunk[j // 2], "front" if j % 2 == 0 else "back"))
    if release:
        st.records = []
        st.storages = set()
    if hits:
        raise GuardError("guard band hit%s (%d band(s)):\n  %s" % (" after " + where if where else "", len(hits),
                                                                    "\n  ".join(hits[:8])))
    return len(recs)


def guarded(fn):
    """Decorator: run a test under guarded_memory() with verify() at its end (pytest sees the original's signature and marks)."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kw):
        with guarded_memory():
            fn(*args, **kw)
            verify()
    return run


def guarded_copies(module, namespace, prefix):
    """Put a guarded copy of every test function of ``module`` into ``namespace`` (a case added there is guarded too)."""
    names = []
    for name, fn in sorted(vars(module).items()):
        if name.startswith("test_") and callable(fn) and getattr(fn, "__module__", None) == module.__name__:
            g = guarded(fn)
            g.__name__ = g.__qualname__ = "test_%s_%s" % (prefix, name[5:])
            namespace[g.__name__] = g
            names.append(g.__name__)
    return names
