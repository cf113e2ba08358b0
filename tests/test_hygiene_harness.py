"""CPU self-test of the memory-hygiene harness (tests/hygiene.py): fake "engine ops" written in torch allocate through the
names the engine wrappers use (functional.torch.empty / empty_like, functional._bytes), and each planted fault must be
reported by the same check the GPU module runs (run_case) - an output element left unwritten, one element stored past the
end, one element read before the start of an input, an input modified in place - while a correct fake op passes."""
import pytest
import torch

from pde_policylearning_amd import functional as F
from tests import hygiene as H


def _span(t, lo, hi):
    """elements [lo, hi) counted from t's first element, as far as t's storage reaches: what a kernel indexing past the
    tensor would touch (in a plain allocation the storage ends with the tensor, so the span is clipped there)"""
    flat = t.view(-1)
    n_store = t.untyped_storage().nbytes() // t.element_size()
    lo_ok, hi_ok = max(lo, -t.storage_offset()), min(hi, n_store - t.storage_offset())
    if hi_ok <= lo_ok:
        return flat[:0]
    return torch.as_strided(flat, (hi_ok - lo_ok,), (1,), t.storage_offset() + lo_ok)


class _FakeOp(torch.autograd.Function):
    """y = 2 x + 1 through a workspace; dx = 2 dy.  `fault` plants one bug."""

    @staticmethod
    def forward(ctx, x, fault):
        ctx.fault = fault
        n = x.numel()
        ws = F._bytes(4 * n, x.device).view(torch.float32)[:n]          # workspace: fully written before it is read
        y = F.torch.empty_like(x)
        src = x.reshape(-1)
        ws.copy_(src)
        if fault == "read_before":
            before = _span(x, -1, 0)                                     # x[-1]: no such element
            if before.numel():
                ws[0] = ws[0] + 0.0 * before[0]
        if fault == "unwritten":
            y.view(-1)[:-1] = 2.0 * ws[:-1] + 1.0
        else:
            y.view(-1)[:] = 2.0 * ws + 1.0
        if fault == "store_past":
            past = _span(y, n, n + 1)
            if past.numel():
                past.fill_(0.0)
        if fault == "modify_input":
            x.view(-1)[3] += 1.0
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = F.torch.empty(dy.shape, dtype=dy.dtype, device=dy.device)
        dx.copy_(2.0 * dy)
        return dx, None


def _case(fault):
    def fn(inp, after_forward):
        x = inp["x"]
        y = _FakeOp.apply(x, fault)
        after_forward()
        y.backward(inp["dy"])
        return {"y": y.detach(), "dx": x.grad}
    g = torch.Generator().manual_seed(4)
    inputs = {"x": torch.randn(5, 7, generator=g).requires_grad_(True), "dy": torch.randn(5, 7, generator=g)}
    return H.run_case(fn, inputs)[1]


def test_correct_fake_op_passes():
    assert _case(None) == []


@pytest.mark.parametrize("fault,expect", [
    ("unwritten", ["[nan] y: 1 of 35 elements not finite, first at [34]", "[big] y differs from the plain run: 1 of 35",
                   "[nan] y differs from the plain run: 1 of 35"]),
    ("store_past", ["guard band after _FakeOp.forward (5, 7) float32: 1 element(s) overwritten, nearest at element numel + 0"]),
    ("read_before", ["[nan] y: 1 of 35 elements not finite, first at [0]"]),
    ("modify_input", ["[plain] input x changed by the forward: 1 of 35 elements differ, first at [3]",
                      "[nan] input x changed by the forward"]),
])
def test_planted_fault_is_reported(fault, expect):
    findings = _case(fault)
    text = "\n".join(findings)
    for e in expect:
        assert e in text, (e, findings)


def test_patterns_and_guard_report():
    """pattern bytes read as the documented values; a guard-band hit names the buffer, the side, the nearest offending
    element and the count; the patches are gone afterwards"""
    real_torch, real_bytes = F.torch, F._bytes
    with H.poisoned("nan") as p:
        assert F.torch is not torch and F._bytes is not real_bytes and F.torch.zeros is torch.zeros
        a = F.torch.empty((3, 4))
        assert torch.isnan(a).all()
        b = F._bytes(10, torch.device("cpu"))
        assert b.numel() == 256 and bool((b == 0xFF).all())
        assert (a.data_ptr() - p.bufs[0].base.data_ptr()) == H.GUARD_BYTES
        _span(a, -3, -1).fill_(1.0)
        _span(a, 12, 13).fill_(1.0)
        bad = p.check_guards()
    assert F.torch is real_torch and F._bytes is real_bytes
    assert any("guard band before test_patterns_and_guard_report (3, 4) float32: 2 element(s) overwritten, nearest at element -2"
               in m for m in bad), bad
    assert any("guard band after" in m and "1 element(s)" in m and "numel + 0" in m for m in bad), bad
    with H.poisoned("big"):
        assert float(F.torch.empty(2).max()) == pytest.approx(3.3961514e38, rel=1e-6)
    with H.poisoned("zero"):
        assert float(F.torch.empty_like(torch.ones(4)).abs().max()) == 0.0
    # a dense permutation keeps its strides (plane-major weights), like torch.empty_like's preserve_format
    pm = F.to_plane_major(torch.randn(2, 3, 4))
    with H.poisoned("nan"):
        e = F.torch.empty_like(pm)
    assert e.stride() == pm.stride() and e.shape == pm.shape


def _package_modules():
    """every module of the functional package, found the way an import would find it (not through the harness's own list)"""
    import importlib
    import pkgutil
    found = [importlib.import_module(f"{F.__name__}.{m.name}") for m in pkgutil.iter_modules(F.__path__)]
    assert len(found) >= 10 and F._bytes.__module__ in [m.__name__ for m in found]
    return found + [F]


def test_every_module_of_the_package_is_poisoned():
    """The wrappers live in one module per family: inside poisoned() each of them must see the proxy under its own `torch`
    name and the poisoning allocator under its own `_bytes` name (a module left out would allocate unpoisoned while every
    hygiene test stayed green), and both names come back on exit."""
    mods = _package_modules()
    before = {m.__name__: (m.__dict__.get("torch"), m.__dict__.get("_bytes")) for m in mods}
    assert sum(t is torch for t, _ in before.values()) >= 10 and sum(b is F._bytes for _, b in before.values()) >= 5
    with H.poisoned("nan") as p:
        for m in mods:
            if "torch" in m.__dict__:
                assert m.torch is not torch and isinstance(m.torch, H._TorchProxy), m.__name__
            if "_bytes" in m.__dict__:
                assert m._bytes is F._bytes and m._bytes is not before[m.__name__][1], m.__name__
                n0 = len(p.bufs)
                b = m._bytes(10, torch.device("cpu"))
                assert len(p.bufs) == n0 + 1 and b.numel() == 256 and bool((b == 0xFF).all()), m.__name__
    for m in mods:
        assert (m.__dict__.get("torch"), m.__dict__.get("_bytes")) == before[m.__name__], m.__name__
