"""PINO observers with the reference surface (libs/models/pino_models/pinobserver.py:
MultiplicativeNet :14-63, PINObserver2d :129-233, PlanePredHead :236-273,
PINObserverFullField :276-375, PolicyModel2D :378-463).  SpectralConv3d runs in the HIP engine; the channels-last
Linear / Conv1d(k=1) glue is torch."""
import math

import torch
import torch.nn.functional as TF
from torch import nn
from torch.nn import init

from .basics import SpectralConv3d
from .... import functional as F
from .... import layer_stack as LS


def _activation(name):
    table = {"tanh": torch.tanh, "gelu": TF.gelu, "relu": TF.relu_, "elu": TF.elu_, "leaky_relu": TF.leaky_relu_}
    if name not in table:
        raise ValueError(f"{name} is not supported")
    return table[name]


def _pad_last(x, num_pad):
    return TF.pad(x, (num_pad[0], num_pad[1]), "constant", 0) if max(num_pad) > 0 else x


def _unpad_last(x, num_pad):
    return x[..., num_pad[0]:-num_pad[1]] if max(num_pad) > 0 else x


class MultiplicativeNet(nn.Module):
    """out = B x1 + A x2 + bias, x1 (N, X, Y, T, in1) channels-last, x2 (N, in2) a per-sample code."""

    def __init__(self, in1_features, in2_features, out_features, device=None, dtype=None):
        super().__init__()
        self.in1_features, self.in2_features, self.out_features = in1_features, in2_features, out_features
        self.A = nn.Parameter(torch.empty(out_features, in2_features))
        self.B = nn.Parameter(torch.empty(out_features, in1_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        self.reset_parameters()

    def reset_parameters(self):
        init.kaiming_uniform_(self.A, a=math.sqrt(5))
        init.kaiming_uniform_(self.B, a=math.sqrt(5))
        bound = 1 / math.sqrt(self.in1_features)
        init.uniform_(self.bias, -bound, bound)

    def forward(self, input1, input2):
        if input2.dim() < 2:
            input2 = input2.unsqueeze(-1)
        code = (input2 @ self.A.t())[:, None, None, None, :]
        return input1 @ self.B.t() + code + self.bias


def _code(mn, re):
    """the per-sample Re-conditioning code A re, (B, C)"""
    return (re if re.dim() >= 2 else re.unsqueeze(-1)) @ mn.A.t()


def _lift_front(fc0, mn, x, re):
    """multiplicative_net1(fc0(x), re) as a channels-first tensor (pinobserver.py:205-207, 356-358).  fc0 followed by the
    Re-conditioning affine is ONE linear map of the <= 4 input channels: when the shape allows it the two small matrices are
    composed (autograd differentiates the composition) and applied by the engine's lifting kernels; an input that asks for
    its gradient gets it from them too (functional.lifting)."""
    xc = x.permute(0, 4, 1, 2, 3)
    if LS.lift_covered(xc, fc0):
        return F.lifting(xc.contiguous(), mn.B @ fc0.weight, mn.B @ fc0.bias + mn.bias) + _code(mn, re)[:, :, None, None, None]
    return mn(fc0(x), re).permute(0, 4, 1, 2, 3)


def _recondition_tail(x, re, mn, fc1, fc2, act, engine=True):
    """fc2(act(fc1(multiplicative_net2(x, re)))) of the channels-first x, channels-last (pinobserver.py:228-233, 257-273).  On
    the engine: the Re-conditioning affine as a pointwise mix with the per-sample code added, then fc1 -> GELU -> fc2 for all
    planes in the projection kernels (hidden tensor never materialised)."""
    if engine and act is TF.gelu and LS.head_covered(x, fc1, fc2):
        h = F.pointwise_conv_add(x.contiguous(), mn.B, mn.bias, None) + _code(mn, re)[:, :, None, None, None]
        return F.projection_head(h, fc1.weight, fc1.bias, fc2.weight, fc2.bias).permute(0, 2, 3, 4, 1)
    return fc2(act(fc1(mn(x.permute(0, 2, 3, 4, 1), re))))


class _SpectralStack(nn.Module):
    """layers of  x <- act(SpectralConv3d(x) + Conv1d_{k=1}(x)), no activation after the last."""

    ROUTES = LS.RUNGS

    def _build_stack(self, layers, modes1, modes2, modes3):
        self.sp_convs = nn.ModuleList([SpectralConv3d(i, o, m1, m2, m3)
                                       for i, o, m1, m2, m3 in zip(layers, layers[1:], modes1, modes2, modes3)])
        self.ws = nn.ModuleList([nn.Conv1d(i, o, 1) for i, o in zip(layers, layers[1:])])

    def stack(self, x):
        """the stack for an input shaped like x; engine_call announces the live last-dim slices before any weight is read"""
        uniform = self.act is TF.gelu and len(set(self.layers)) == 1
        return LS.conv_stack(self.sp_convs, self.ws, self.act, [conv.engine_call(x) for conv in self.sp_convs] if uniform else None)

    def _run_stack(self, x):
        return LS.run(x, self.stack(x), self.ROUTES)


def _num_pad(pad_ratio, size_z):
    """zeros in front of / behind the last axis: round(size_z * r) of the extent the reference reads (dim -2, :353)"""
    return [round(size_z * r) for r in pad_ratio] if max(pad_ratio) > 0 else [0, 0]


def _pad_ratio(pad_ratio):
    if isinstance(pad_ratio, float):
        return [pad_ratio, pad_ratio]
    assert len(pad_ratio) == 2, 'Cannot add padding in more than 2 directions.'
    return pad_ratio


class PINObserver2d(_SpectralStack):
    def __init__(self, modes1, modes2, modes3, width=16, fc_dim=128, layers=None, in_dim=4, out_dim=1,
                 act='gelu', pad_ratio=[0., 0.], use_fourier_layer=False):
        super().__init__()
        if use_fourier_layer:
            raise NotImplementedError("use_fourier_layer=True is outside the accelerated hot path")
        self.pad_ratio = _pad_ratio(pad_ratio)
        self.modes1, self.modes2, self.modes3, self.in_dim = modes1, modes2, modes3, in_dim
        self.layers = [width] * 4 if layers is None else layers
        self.use_fourier_layer, self.fourier_layer1 = False, None
        self.fc0 = nn.Linear(in_dim, self.layers[0])
        self.multiplicative_net1 = MultiplicativeNet(self.layers[0], 1, self.layers[0])
        self._build_stack(self.layers, modes1, modes2, modes3)
        self.multiplicative_net2 = MultiplicativeNet(self.layers[-1], 1, self.layers[-1])
        self.fc1 = nn.Linear(self.layers[-1], fc_dim)
        self.fc2 = nn.Linear(fc_dim, out_dim)
        self.act = _activation(act)

    def forward(self, x, re):
        re = re.float()
        num_pad = _num_pad(self.pad_ratio, x.shape[-2])
        y = self._forward_padded(x, re, num_pad)
        if y is not None:
            return y
        x = _lift_front(self.fc0, self.multiplicative_net1, x, re)
        x = _unpad_last(self._run_stack(_pad_last(x, num_pad).contiguous()), num_pad)
        return _recondition_tail(x, re, self.multiplicative_net2, self.fc1, self.fc2, self.act)

    PER_SAMPLE_MAX = 16      # the per-sample-bias kernels are launched once per sample

    def _forward_padded(self, x, re, num_pad):
        """The whole forward on the PADDED grid, channels-first, with no layout or padding copies of the 64-channel tensors:
        the in_dim-channel INPUT is padded (C / in_dim times cheaper), lifted per sample with the Re-conditioning code folded
        into the bias, and the pad columns are zeroed in place (= F.pad of the lifted tensor, pinobserver.py:208-213); the
        tail (second Re-conditioning affine with its code as a per-sample bias, fc1 -> GELU -> fc2) runs on the padded tensor
        too - it is pointwise, the pad columns are dropped from the 1-channel output (:228).  None when the engine's
        lifting / pointwise / projection kernels do not cover the shape."""
        B = x.shape[0]
        if (x.requires_grad or self.act is not TF.gelu or len(set(self.layers)) != 1 or self.layers[0] not in (32, 64)
                or B > self.PER_SAMPLE_MAX or self.fc2.out_features != 1):
            return None
        p0, p1 = num_pad
        xc = TF.pad(x.permute(0, 4, 1, 2, 3), (p0, p1)) if p0 + p1 > 0 else x.permute(0, 4, 1, 2, 3).contiguous()
        C = self.layers[0]
        like = LS.probe(xc, C)                              # a (B, C, X, Y, T') view for the shape predicates (no memory)
        if not (LS.lift_covered(xc, self.fc0) and F.pointwise_supported(like) and LS.head_covered(like, self.fc1, self.fc2)):
            return None
        fc0, mn1, mn2 = self.fc0, self.multiplicative_net1, self.multiplicative_net2
        w = mn1.B @ fc0.weight                                             # (C, in_dim): fc0 then the Re-conditioning mix
        bias = (mn1.B @ fc0.bias + mn1.bias)[None, :] + _code(mn1, re)     # (B, C): + the per-sample code
        h = F.zero_last_pads_(F.lifting_per_sample_bias(xc, w, bias), p0, p1)
        h = self._run_stack(h)
        h = F.pointwise_conv_per_sample_bias(h, mn2.B, mn2.bias[None, :] + _code(mn2, re))
        y = F.projection_head(h, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)
        if p0 + p1 > 0:
            y = y[..., p0:y.shape[-1] - p1]
        return y.permute(0, 2, 3, 4, 1)


class PlanePredHead(_SpectralStack):
    def __init__(self, layers, modes1, modes2, modes3, fc_dim, out_dim, act):
        super().__init__()
        self.layers, self.modes1, self.modes2, self.modes3 = layers, modes1, modes2, modes3
        self._build_stack(layers, modes1, modes2, modes3)
        self.fc1 = nn.Linear(layers[-1], fc_dim)
        self.fc2 = nn.Linear(fc_dim, out_dim)
        self.act = _activation(act)

    def forward(self, x, num_pad, re, multiplicative_net2):
        x = _unpad_last(self._run_stack(x), num_pad)
        return _recondition_tail(x, re, multiplicative_net2, self.fc1, self.fc2, self.act,
                                 not getattr(self, "no_engine_tail", False))


class PINObserverFullField(nn.Module):
    def __init__(self, plane_num, modes1, modes2, modes3, width=16, fc_dim=128, layers=None, in_dim=4, out_dim=1,
                 act='gelu', pad_ratio=[0., 0.], use_fourier_layer=False):
        super().__init__()
        if use_fourier_layer:
            raise NotImplementedError("use_fourier_layer=True is outside the accelerated hot path")
        self.plane_num, self.pad_ratio = plane_num, _pad_ratio(pad_ratio)
        self.modes1, self.modes2, self.modes3 = modes1, modes2, modes3
        self.max_re, self.in_dim = 1000, in_dim
        self.layers = [width] * 4 if layers is None else layers
        self.use_fourier_layer, self.fourier_layer1 = False, None
        self.fc0 = nn.Linear(in_dim, self.layers[0])
        self.multiplicative_net1 = MultiplicativeNet(self.layers[0], 1, self.layers[0])
        self.multiplicative_net2 = MultiplicativeNet(self.layers[-1], 1, self.layers[-1])
        self.observer_head = PlanePredHead(self.layers, modes1, modes2, modes3, fc_dim, out_dim * plane_num, act)

    def forward(self, x, re):
        re = re.float() / self.max_re
        num_pad = _num_pad(self.pad_ratio, x.shape[-2])
        x = _lift_front(self.fc0, self.multiplicative_net1, x, re)
        pred = self.observer_head(_pad_last(x, num_pad).contiguous(), num_pad, re, self.multiplicative_net2)
        return pred.permute(0, 4, 1, 2, 3)     # (B, planes, X, Y, T)


class PolicyModel2D(nn.Module):
    """The policy network of `optimal-policy-observer` (pinobserver.py:378-463): PINObserverFullField with the head named
    `pred_net`, out_dim outputs and the output left channels-last (B, X, Y, T, out_dim).  The reference ends its constructor
    by zeroing EVERY parameter, which makes its run degenerate: fc2.weight's gradient is dy (x) gelu(0) = 0 and everything
    upstream receives fc2.weight^T dy = 0, so only pred_net.fc2.bias ever changes and the policy is one scalar offset of the
    whole plane.  zero_init (beyond the reference's signature): True - the reference; "head" - the ordinary initialisation
    with only pred_net.fc2 zeroed, so the correction still starts at zero but gradients reach every layer from the second
    step on; False - the ordinary initialisation."""

    def __init__(self, modes1, modes2, modes3, width=16, fc_dim=128, layers=None, in_dim=4, out_dim=1,
                 act='gelu', pad_ratio=[0., 0.], use_fourier_layer=False, zero_init=True):
        super().__init__()
        if use_fourier_layer:
            raise NotImplementedError("use_fourier_layer=True is outside the accelerated hot path")
        if zero_init not in (True, False, "head"):
            raise ValueError(f"PolicyModel2D: zero_init must be True, False or 'head' (got {zero_init!r})")
        self.pad_ratio = _pad_ratio(pad_ratio)
        self.modes1, self.modes2, self.modes3 = modes1, modes2, modes3
        self.max_re, self.in_dim, self.out_dim = 1000, in_dim, out_dim
        self.layers = [width] * 4 if layers is None else layers
        self.use_fourier_layer, self.fourier_layer1 = False, None
        self.fc0 = nn.Linear(in_dim, self.layers[0])
        self.multiplicative_net1 = MultiplicativeNet(self.layers[0], 1, self.layers[0])
        self.multiplicative_net2 = MultiplicativeNet(self.layers[-1], 1, self.layers[-1])
        self.pred_net = PlanePredHead(self.layers, modes1, modes2, modes3, fc_dim, out_dim, act)
        with torch.no_grad():
            zero = list(self.parameters()) if zero_init is True else list(self.pred_net.fc2.parameters()) if zero_init == "head" else []
            for prm in zero:
                prm.zero_()

    def forward(self, x, re):
        re = re.float() / self.max_re
        num_pad = _num_pad(self.pad_ratio, x.shape[-2])
        x = _lift_front(self.fc0, self.multiplicative_net1, x, re)
        return self.pred_net(_pad_last(x, num_pad).contiguous(), num_pad, re, self.multiplicative_net2)      # (B, X, Y, T, out_dim)
