"""Memory-hygiene harness for the engine wrappers (a helper module, not a conftest).

Every buffer the engine writes comes from an uninitialised allocation in a module of the pde_policylearning_amd/functional/
package (`_bytes` of functional/_core.py for `saved`, `xhat` and every workspace; torch.empty / torch.empty_like for outputs and
gradients) or in trainer.py (the dead Adam moments of FusedAdam.sync_dead_slices).  Under torch's caching allocator such a
block usually holds what the same computation left there the last time, so a kernel that skips part of its output, reads a
slab nobody wrote or stores one tile past the end passes every value test.  This module takes the allocator out of the picture:

  poisoned(pattern)   while active, every allocation those modules make through `torch.empty`, `torch.empty_like` and
                      their `_bytes` name is numel + 2 G elements filled with the pattern byte, and the caller gets the
                      contiguous middle.  G * itemsize = GUARD_BYTES (256 KB: more than one 128-pixel x 64-channel fp32 tile,
                      a multiple of 256 bytes, so the middle keeps the alignment a fresh allocation has).  `torch` itself is
                      not patched: the modules' `torch` name is swapped for a proxy that overrides the two allocators and
                      forwards everything else, so the oracle and torch's own code allocate as usual.
  check_guards()      (Poison.check_guards) both guard bands of every registered buffer still hold the pattern, bit for bit.
  guarded(t)          a copy of an input in the middle of a NaN-filled (0xFF) buffer with guard bands: an out-of-bounds read
                      that reaches a result shows up as NaN or as a bitwise difference between runs.
  run_case(...)       the whole check for one case: one plain run, one run under each pattern with guarded inputs; outputs
                      bitwise equal across the four runs and finite, guard bands intact, inputs bitwise unchanged after the
                      forward and after the backward.
  assert_clean(...)   run_case for a test: fails with the case's name and its findings, returns the outputs of the plain run.

Patterns: 0x00; 0xFF (NaN in fp16, fp32 and fp64); 0x7F (fp32 3.396e38: finite, so it survives fmaxf and an integer max of
bit patterns - the magnitude-bound slots are accumulated that way).

Safety: poison only data.  The harness must expose numeric dependence on stale memory, never make a kernel fault, so no
poisoned buffer may hold something a kernel turns into an address.  Checked against fno_abi.hip (carve_spec, carve_model,
carve_saved, carve_fanout, carve_pino, carve_chanflow, carve_proj, fno_lploss_rel_*, the Adam entry points) and the kernel headers:
  - every carved region is float, float2 or packed 16-bit weight data (ModelWs::wa1 / wa3, ProjWs::wa1 / wa3);
  - the partial-sum reductions (k_reduce_jobs) get their job lists (ReduceJobs) as kernel arguments, not from memory;
  - the block backward's barrier counters and the projection's column queue live in LDS (k_block_bwd2.h, k_projection_h2.h);
  - the 64 magnitude-bound slots at the end of `saved` are float bit patterns (atomicMax on their unsigned image,
    fno_dev.h) that only feed scales; the forward clears them (pack_w_layers' zero64) and the backward clears [32, 64)
    unless CallState::bwd_clean says the forward just did;
  - the only integers in device memory are FusedAdam's step counter and scratch (fno_adam_step_dev): torch.zeros, which the
    harness does not replace (the contract is "starts at zero"), like every torch.zeros / zeros_like in the wrappers
    (_fresh_grads: plane-major gradients whose dead planes the host guarantees to be zero).
So nothing is exempt today.  A region that ever holds an index, count, pointer or ticket must be left unpoisoned and listed
here.
"""
import contextlib
import sys

import torch

GUARD_BYTES = 256 * 1024
PATTERNS = {"zero": 0x00, "nan": 0xFF, "big": 0x7F}
_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

_real_empty = torch.empty
_active = []          # the Poison registries in force (innermost last)


def _guard_elems(dtype):
    isz = torch.empty((), dtype=dtype).element_size()
    assert GUARD_BYTES % isz == 0 and GUARD_BYTES % 256 == 0
    return GUARD_BYTES // isz


def _caller_label(depth):
    """the engine wrapper that asked for the allocation: 'Fn.forward' / 'Fn.backward' for autograd functions, else the
    function's name"""
    f = sys._getframe(depth + 1)
    while f.f_code.co_name.startswith("<") and f.f_back is not None:      # a comprehension inside the wrapper
        f = f.f_back
    name = f.f_code.co_name
    ctx = f.f_locals.get("ctx")
    if ctx is not None:
        return f"{type(ctx).__name__.replace('Backward', '')}.{name}"
    return name


class _Buf(object):
    __slots__ = ("base", "g", "numel", "label", "byte")

    def __init__(self, base, g, numel, label, byte):
        self.base, self.g, self.numel, self.label, self.byte = base, g, numel, label, byte


class Poison(object):
    """Registry of the buffers handed out while one `poisoned(pattern)` is active (kept alive until it is dropped)."""

    def __init__(self, byte):
        self.byte = int(byte)
        self.bufs = []

    def alloc(self, shape, dtype, device, label, byte=None, strides=None):
        byte = self.byte if byte is None else int(byte)
        shape = torch.Size(shape)
        n = shape.numel()
        g = _guard_elems(dtype)
        base = _real_empty(n + 2 * g, dtype=dtype, device=device)
        base.view(torch.uint8).fill_(byte)
        mid = base.as_strided(shape, strides, g) if strides is not None else base[g:g + n].view(shape)
        self.bufs.append(_Buf(base, g, n, f"{label} {tuple(shape)} {str(dtype).replace('torch.', '')}", byte))
        return mid

    def check_guards(self):
        """Both guard bands of every registered buffer, bit for bit.  Returns a list of findings (empty: all intact)."""
        if any(b.base.is_cuda for b in self.bufs):
            torch.cuda.synchronize()
        bad = []
        for b in self.bufs:
            isz = b.base.element_size()
            raw = b.base.view(torch.uint8)
            for side, band in (("before", raw[:b.g * isz]), ("after", raw[(b.g + b.numel) * isz:])):
                diff = (band != b.byte).view(-1, isz).any(dim=1)
                cnt = int(diff.sum())
                if cnt:
                    idx = torch.nonzero(diff).view(-1)
                    # the offending element nearest to the tensor, in elements from its first / past its last element
                    where = f"element {int(idx.max()) - b.g}" if side == "before" else f"element numel + {int(idx.min())}"
                    bad.append(f"guard band {side} {b.label}: {cnt} element(s) overwritten, nearest at {where}")
        return bad


class _TorchProxy(object):
    """`torch` as the patched modules see it: empty / empty_like poisoned, every other attribute forwarded."""

    def __init__(self, poison):
        self._poison = poison

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, requires_grad=False, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        t = self._poison.alloc(size, dtype, device, _caller_label(1))
        return t.requires_grad_(True) if requires_grad else t

    def empty_like(self, src, dtype=None, device=None, requires_grad=False, **kw):
        dtype = dtype if dtype is not None else src.dtype
        device = torch.device(device) if device is not None else src.device
        strides = None
        if not src.is_contiguous():
            # preserve_format keeps the strides of a dense permutation (plane-major weights); anything else becomes contiguous
            span = 1 + sum((s - 1) * st for s, st in zip(src.shape, src.stride()))
            if src.numel() > 0 and span == src.numel() and all(st >= 0 for st in src.stride()):
                strides = src.stride()
        t = self._poison.alloc(src.shape, dtype, device, _caller_label(1), strides=strides)
        return t.requires_grad_(True) if requires_grad else t


def _engine_modules():
    """every module found in the functional package (one added later is covered without an edit here), the package itself
    (callers allocate through F.torch / F._bytes too) and trainer"""
    import importlib
    import pkgutil
    from pde_policylearning_amd import functional, trainer
    subs = [importlib.import_module(f"{functional.__name__}.{m.name}") for m in pkgutil.iter_modules(functional.__path__)]
    return subs + [functional, trainer]


@contextlib.contextmanager
def poisoned(pattern, modules=None):
    """Replace the allocations of the engine wrappers (the modules of functional/ and trainer.py, or `modules`) by poisoned,
    guarded buffers.  Each module's own `torch` and `_bytes` names are swapped, whichever of the two it has.  `pattern`: a key
    of PATTERNS or a byte value.  Yields the Poison registry; the patches are undone on exit."""
    byte = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    poison = Poison(byte)
    mods = list(modules) if modules is not None else _engine_modules()
    proxy = _TorchProxy(poison)

    def _bytes(n, device):
        return poison.alloc((max(int(n), 256),), torch.uint8, device, _caller_label(1) + " _bytes")
    saved = []
    for m in mods:
        for name, stand_in in (("torch", proxy), ("_bytes", _bytes)):
            if name in m.__dict__:
                saved.append((m, name, m.__dict__[name]))
                setattr(m, name, stand_in)
    _active.append(poison)
    try:
        yield poison
    finally:
        _active.remove(poison)
        for m, name, val in reversed(saved):
            setattr(m, name, val)


def guarded(t):
    """A copy of `t` (same shape, dtype, device and requires_grad) in the middle of a NaN-filled (0xFF) buffer with guard
    bands, registered with the innermost active poisoned() context when there is one (so its bands are checked too)."""
    p = _active[-1] if _active else Poison(0xFF)
    src = t.detach()
    g = p.alloc(src.shape, src.dtype, src.device, "input", byte=0xFF)
    with torch.no_grad():
        g.copy_(src)
    return g.requires_grad_(True) if t.requires_grad else g


def bits(t):
    """bit image of a tensor on the CPU (an integer view: NaN equals NaN when the bits agree)"""
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.contiguous().reshape(-1)
    return t.view(_INT_OF[t.element_size()]).to("cpu", copy=True)


def describe_diff(a, b, limit=8):
    """'n of N elements differ, first at [...]' for two bit images"""
    d = torch.nonzero(a != b).view(-1)
    return f"{d.numel()} of {a.numel()} elements differ, first at {d[:limit].tolist()}"


def _not_finite(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    if not t.is_floating_point():
        return None
    nf = ~torch.isfinite(t.reshape(-1))
    n = int(nf.sum())
    return f"{n} of {t.numel()} elements not finite, first at {torch.nonzero(nf).view(-1)[:8].tolist()}" if n else None


def run_case(fn, inputs, mutable=(), patterns=tuple(PATTERNS), modules=None):
    """Run `fn(inp, after_forward)` once with plain allocations on `inputs` (dict name -> tensor) and once under each pattern
    on guarded copies.  `fn` returns a dict name -> tensor of everything it produced (outputs, gradients, losses; for an
    optimiser the updated state) and calls `after_forward()` between its forward and its backward.  Inputs named in `mutable`
    are declared outputs that may change in place; every other input must come back bitwise unchanged after the forward and
    after the backward.  Returns (outputs of the plain run, findings); no findings = every output bitwise equal across the
    runs and finite, the guard bands intact, the inputs unchanged."""
    findings = []
    runs = {}

    def one(tag, inp):
        snap = {k: bits(v) for k, v in inp.items() if k not in mutable}

        def unchanged(when):
            for k, b in snap.items():
                now = bits(inp[k])
                if not torch.equal(now, b):
                    findings.append(f"[{tag}] input {k} changed {when}: {describe_diff(now, b)}")
        out = fn(inp, lambda: unchanged("by the forward"))
        unchanged("by the backward")
        for k, v in out.items():
            m = _not_finite(v)
            if m:
                findings.append(f"[{tag}] {k}: {m}")
        return {k: bits(v) for k, v in out.items()}, out

    runs["plain"], plain = one("plain", {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in inputs.items()})
    for pat in patterns:
        with poisoned(pat, modules) as poison:
            inp = {k: guarded(v) for k, v in inputs.items()}
            runs[pat], out = one(pat, inp)
            del out, inp
            findings += [f"[{pat}] {m}" for m in poison.check_guards()]
    for pat in patterns:
        for k, b in runs["plain"].items():
            o = runs[pat].get(k)
            if o is None or o.shape != b.shape:
                findings.append(f"[{pat}] {k}: missing or of another size")
            elif not torch.equal(o, b):
                findings.append(f"[{pat}] {k} differs from the plain run: {describe_diff(o, b)}")
    return plain, findings


def assert_clean(case, fn, inputs, mutable=()):
    """run_case, no findings allowed (the first 40 are in the message).  Returns the outputs of the plain run."""
    out, findings = run_case(fn, inputs, mutable)
    assert not findings, "\n".join([case] + findings[:40])
    return out
