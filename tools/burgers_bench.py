"""Time the Burgers PINO step on the engine against the same step composed from torch operations, on the same GPU in the same
process (GPU box).

  python tools/burgers_bench.py [--out profiles/r20_burgers_bench.txt] [--blocks 7] [--iters 50] [--only loss|step]

Shape: B 20, grid (nt 101, nx 128), FNO2d(modes1=[15,12,9,9], modes2=[15,12,9,9], layers=[64]*5, fc_dim=128, in_dim=3), visc 0.01.
  (a) loss   the loss alone, forward + backward: functional.burgers_loss (k_burgers_loss.h: two launches forward, one backward)
             against the reference's operation sequence (libs/pino_utils/losses.py:200-243: fft, two multiplies, two irfft,
             slices, mse_loss and their autograd twins).
  (b) step   model forward, data LpLoss, PINO_loss, backward, torch.optim.Adam: engine model + engine losses against the model
             composed from torch.fft.rfft2 / einsum / irfft2 / Conv1d / gelu with the torch losses.  Two models, one set of
             initial values.
Method: the outputs of the two versions are compared at the timed shape first.  After warm-up the two versions take turns in
BLOCKS blocks of ITERS steps, each block bracketed by device events; median, min and max of the per-step times.  GPU
dispatches per step are counted by torch.profiler around one extra step of each version (outside the timed blocks); the
engine's own launches also come from the library's launch log.  For per-kernel times run this script once under
`rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the host)."""
import argparse
import copy
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pde_policylearning_amd import _lib      # noqa: E402
from pde_policylearning_amd import functional as F      # noqa: E402
from pde_policylearning_amd.libs.models.pino_models import FNO2d      # noqa: E402
from pde_policylearning_amd.libs.pino_utils.losses import LpLoss, PINO_loss      # noqa: E402

B, NT, NX, VISC = 20, 101, 128, 0.01
MODES, LAYERS = [15, 12, 9, 9], [64] * 5
W_IC, W_F, W_XY = 5.0, 1.0, 1.0
WARM = 5


def torch_burgers_loss(u, u0, v):
    """libs/pino_utils/losses.py:200-243 as written there"""
    batchsize, nt, nx = u.shape
    dt = 1 / (nt - 1)
    u_h = torch.fft.fft(u, dim=2)
    k_max = nx // 2
    k_x = torch.cat((torch.arange(start=0, end=k_max, step=1, device=u.device),
                     torch.arange(start=-k_max, end=0, step=1, device=u.device)), 0).reshape(1, 1, nx)
    ux_h = 2j * math.pi * k_x * u_h
    uxx_h = 2j * math.pi * k_x * ux_h
    ux = torch.fft.irfft(ux_h[:, :, :k_max + 1], dim=2, n=nx)
    uxx = torch.fft.irfft(uxx_h[:, :, :k_max + 1], dim=2, n=nx)
    ut = (u[:, 2:, :] - u[:, :-2, :]) / (2 * dt)
    Du = ut + (ux * u - v * uxx)[:, 1:-1, :]
    index_t = torch.zeros(nx, device=u.device).long()
    index_x = torch.arange(nx, device=u.device).long()
    loss_u = TF.mse_loss(u[:, index_t, index_x], u0)
    loss_f = TF.mse_loss(Du, torch.zeros(Du.shape, device=u.device))
    return loss_u, loss_f


def torch_lploss(x, y):
    n = x.size(0)
    return torch.mean(torch.norm(x.reshape(n, -1) - y.reshape(n, -1), 2, 1) / torch.norm(y.reshape(n, -1), 2, 1))


def torch_model(m, x):
    """fourier2d.py:53-87 of the reference from torch operations, on the engine model's parameters (no padding)"""
    h = m.fc0(x).permute(0, 3, 1, 2)
    bs, sx, sy = h.shape[0], h.shape[-2], h.shape[-1]
    last = len(m.ws) - 1
    for i, (sp, w) in enumerate(zip(m.sp_convs, m.ws)):
        hf = torch.fft.rfftn(h, dim=[2, 3])
        out = torch.zeros(bs, sp.out_channels, sx, sy // 2 + 1, device=h.device, dtype=torch.cfloat)
        out[:, :, :sp.modes1, :sp.modes2] = torch.einsum("bixy,ioxy->boxy", hf[:, :, :sp.modes1, :sp.modes2], sp.weights1)
        out[:, :, -sp.modes1:, :sp.modes2] = torch.einsum("bixy,ioxy->boxy", hf[:, :, -sp.modes1:, :sp.modes2], sp.weights2)
        h = torch.fft.irfftn(out, s=(sx, sy), dim=[2, 3]) + w(h.view(bs, m.layers[i], -1)).view(bs, m.layers[i + 1], sx, sy)
        if i != last:
            h = TF.gelu(h)
    h = h.permute(0, 2, 3, 1)
    return m.fc3(TF.gelu(m.fc2(TF.gelu(m.fc1(h)))))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def dispatches(fn):
    """GPU kernels of one call, counted by torch.profiler (None where the profiler is unavailable)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if getattr(e, "device_type", None) is not None
                   and "cuda" in str(e.device_type).lower())
    except Exception as exc:      # noqa: BLE001
        print(f"  (torch.profiler unavailable: {exc})")
        return None


def alternate(name, engine, composed, blocks, iters, lines):
    for fn in (engine, composed):
        timed(fn, WARM)
    with _lib.launch_log() as log:
        engine()
        torch.cuda.synchronize()
    ne, nt_ = dispatches(engine), dispatches(composed)
    lines.append(f"  {name}: engine-library launches per step {len(log.records)}; GPU dispatches per step (torch.profiler): "
                 f"engine version {ne}, torch composition {nt_}")
    t = {"engine": [], "torch": []}
    for _ in range(blocks):
        for key, fn in (("engine", engine), ("torch", composed)):
            t[key].append(timed(fn, iters))
    for key in ("engine", "torch"):
        v = t[key]
        lines.append(f"  {name}: {key:7s} median {statistics.median(v):.4f} ms per step  min {min(v):.4f}  max {max(v):.4f}  "
                     f"({blocks} blocks of {iters} steps)")
    lines.append(f"  {name}: torch composition / engine = {statistics.median(t['torch']) / statistics.median(t['engine']):.2f} x; "
                 f"engine's slowest block {max(t['engine']):.4f} ms vs the composition's fastest {min(t['torch']):.4f} ms: "
                 f"{'engine not slower' if max(t['engine']) <= min(t['torch']) else 'ENGINE SLOWER OR WITHIN THE SPREAD'}")


def inputs(dev):
    g = torch.Generator(device=dev).manual_seed(1)
    xs = torch.arange(NX, device=dev, dtype=torch.float32) / NX
    ts = torch.linspace(0, 1, NT, device=dev)
    phase = torch.rand(B, 1, generator=g, device=dev)
    a = torch.sin(2 * math.pi * (xs[None] + phase)) + 0.5 * torch.sin(4 * math.pi * (xs[None] - phase))      # (B, NX)
    x = torch.stack((a[:, None, :].expand(B, NT, NX), xs[None, None, :].expand(B, NT, NX), ts[None, :, None].expand(B, NT, NX)), -1)
    y = a[:, None, :] * torch.exp(-ts)[None, :, None]
    return x.contiguous(), y.contiguous(), a.contiguous()


def rel(p, q):
    return float((p.double() - q.double()).norm() / q.double().norm())


def bench_loss(dev, blocks, iters, lines):
    x, y, a = inputs(dev)
    u = (y + 0.05 * torch.sin(37.0 * x[..., 1] + 11.0 * x[..., 2])).requires_grad_(True)

    def engine():
        lu, lf = F.burgers_loss(u, a, VISC)
        return lu, lf, torch.autograd.grad(W_IC * lu + W_F * lf, u)[0]

    def composed():
        lu, lf = torch_burgers_loss(u, a, VISC)
        return lu, lf, torch.autograd.grad(W_IC * lu + W_F * lf, u)[0]
    (lue, lfe, ge), (lut, lft, gt) = engine(), composed()
    lines.append(f"  loss: engine vs torch composition (float32 both): loss_u {abs(float(lue) - float(lut)) / float(lut):.3e}, "
                 f"loss_f {abs(float(lfe) - float(lft)) / float(lft):.3e}, du rel L2 {rel(ge, gt):.3e}")
    alternate("loss", engine, composed, blocks, iters, lines)


def bench_step(dev, blocks, iters, lines):
    x, y, a = inputs(dev)
    torch.manual_seed(0)
    me = FNO2d(modes1=MODES, modes2=MODES, layers=LAYERS, fc_dim=128, in_dim=3).to(dev)
    mt = copy.deepcopy(me)
    lines.append(f"  step: the engine covers lifting and layers at this shape: {me.route(x) == 'chain'}")
    with torch.no_grad():
        lines.append(f"  step: model output, engine vs torch composition on the same parameters: rel L2 {rel(me(x), torch_model(mt, x)):.3e}")
    oe, ot = torch.optim.Adam(me.parameters(), lr=1e-3), torch.optim.Adam(mt.parameters(), lr=1e-3)
    lp = LpLoss(size_average=True)

    def engine():
        out = me(x).reshape(y.shape)
        data = lp(out, y)
        lu, lf = PINO_loss(out, a, VISC)
        total = lu * W_IC + lf * W_F + data * W_XY
        oe.zero_grad()
        total.backward()
        oe.step()
        return total

    def composed():
        out = torch_model(mt, x).reshape(y.shape)
        data = torch_lploss(out, y)
        lu, lf = torch_burgers_loss(out, a, VISC)
        total = lu * W_IC + lf * W_F + data * W_XY
        ot.zero_grad()
        total.backward()
        ot.step()
        return total
    te, tt = float(engine()), float(composed())
    lines.append(f"  step: total loss of the first step, engine {te:.6e} vs torch composition {tt:.6e}: {abs(te - tt) / abs(tt):.3e}")
    alternate("step", engine, composed, blocks, iters, lines)
    te, tt = float(engine()), float(composed())
    lines.append(f"  step: total loss after the timed steps, engine {te:.6e} vs torch composition {tt:.6e}: {abs(te - tt) / abs(tt):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "loss", "step"])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"## Burgers PINO step: B {B}, grid ({NT}, {NX}), FNO2d modes {MODES} layers {LAYERS} fc_dim 128, visc {VISC}, "
             f"{torch.cuda.get_device_name(0)}"]
    if args.only in ("", "loss"):
        bench_loss(dev, args.blocks, args.iters, lines)
    if args.only in ("", "step"):
        bench_step(dev, args.blocks, args.iters, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
