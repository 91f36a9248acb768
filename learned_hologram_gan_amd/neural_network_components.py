"""Network building blocks with the reference's class names and ``state_dict`` schema
(ref: learnedMethodForHologram/neural_network_components.py:6-95, 241-315), computed by the
HIP ops of hip_ops.py on NHWC activations.

``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.ConvTranspose2d`` objects are used as PARAMETER
CONTAINERS only (same key names, OIHW / IOHW fp32 shapes, running statistics and
``num_batches_tracked`` as the reference checkpoints); their ``forward`` is never called.
The reference's lazy layers infer ``in_channels`` on the first call; here it is an explicit
constructor argument with the value the hot path uses.
"""

from __future__ import annotations

import os

import torch
from torch import nn

from . import hip_ops as ops
from .hip_ops import ACT_NONE, ACT_RELU, OutSlot


def _bn_eval_affine(bn: nn.BatchNorm2d):
    """(scale, shift) of an eval-mode BatchNorm, folded into the conv epilogues — cached on the module while its five tensors are
    unchanged: an inference frame re-derived them with five small ATen launches per layer (90 per generator forward, ~1 ms of a 4K
    frame).  The stamp: storage and version counter of weight / bias / running statistics, plus ``num_batches_tracked``'s version —
    the train-mode kernels update the running statistics through raw pointers (no version bump), but every train-mode forward counts
    its batch (flush_batch_counters), and the optimiser step bumps the parameters' versions (hip_ops.bump_version)."""
    ts = (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    stamp = tuple((t.data_ptr(), t._version) for t in ts)
    hit = bn.__dict__.get("_lhg_eval_affine")
    if hit is not None and hit[0] == stamp and not _PENDING_COUNTERS:
        return hit[1]
    with torch.no_grad():
        affine = ops.batch_norm_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if not _PENDING_COUNTERS:  # (a train-mode forward whose batch counts are not flushed yet: its statistics are not stamped)
        bn.__dict__["_lhg_eval_affine"] = (stamp, affine)
    return affine


def eval_grad_wanted(module: nn.Module, *inputs) -> bool:
    """Eval-mode forward that autograd records: grad mode on and an input or a parameter of ``module`` requires grad.  Otherwise eval mode
    runs the inference kernels under no_grad (the same kernels and bits as ``with torch.no_grad()``)."""
    if module.training or not torch.is_grad_enabled():
        return False
    return any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in module.parameters())


def _conv_bn_eval(conv: nn.Conv2d, bn: nn.BatchNorm2d, x, stride, res, out, act=ACT_RELU, slope=0.0, cached=True):
    """act(BN_running(conv(x)) [+ res]), differentiable.  Frozen gamma / beta: the conv with the folded affine in its epilogue (the
    inference call, same bits; ``cached``: the affine from _bn_eval_affine, as the caller's inference path takes it); a trained gamma or
    beta needs the pre-BN conv output for d gamma: the conv, then the BatchNorm op (nothing cached)."""
    if not (bn.weight.requires_grad or bn.bias.requires_grad):
        if cached:
            scale, shift = _bn_eval_affine(bn)
        else:
            with torch.no_grad():
                scale, shift = ops.batch_norm_eval_affine(bn.weight, bn.bias, bn.running_mean, bn.running_var)
        return ops.ConvBNEvalFn.apply(x, conv.weight, conv.bias, stride, scale, shift, res, act, slope, out)
    y = ops.Conv2dFn.apply(x, conv.weight, conv.bias, stride, None)  # (no "feeds_bn": the bias gradient is scale * sum g here, not zero)
    return ops.BatchNormEvalFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, res, act, slope, out)


_PENDING_COUNTERS: list = []
_THIN_RES = os.environ.get("LHG_THIN_RES", "1") != "0"  # 0: the first block's 1x1 shortcut as a tensor of its own (A/B measurements)
_THIN_NCHW = os.environ.get("LHG_THIN_NCHW", "1") != "0"  # 0: the eval-mode generator converts its NCHW input to NHWC(32) first (A/B measurements)


def _count_batch(*bns):
    """``num_batches_tracked += 1`` (nn.BatchNorm2d bookkeeping, checkpoint parity), batched: one multi-tensor launch per network
    forward (``flush_batch_counters``) instead of one tiny kernel per BatchNorm layer."""
    _PENDING_COUNTERS.extend(b.num_batches_tracked for b in bns)


def flush_batch_counters():
    if _PENDING_COUNTERS:
        # a layer counted twice (two stacked batches through one pass: WGANGPDiscriminator192.forward_pair) gets ONE add of 2 — the
        # multi-tensor kernel must not see the same tensor twice
        counts = {}
        for t in _PENDING_COUNTERS:
            key = id(t)
            counts[key] = (t, counts[key][1] + 1) if key in counts else (t, 1)
        tensors, scalars = [v[0] for v in counts.values()], [v[1] for v in counts.values()]
        if all(c == 1 for c in scalars):
            torch._foreach_add_(tensors, 1)
        else:
            torch._foreach_add_(tensors, scalars)
        _PENDING_COUNTERS.clear()


class ResidualBlock(nn.Module):
    """relu(BN2(conv3x3(relu(BN1(conv3x3(X))))) + conv1x1(X)). ref: neural_network_components.py:6-32."""

    def __init__(self, num_channels, use_1x1conv=False, strides=1, in_channels=None):
        super().__init__()
        in_channels = num_channels if in_channels is None else in_channels
        self.in_channels, self.num_channels, self.strides = in_channels, num_channels, strides
        self.convolution_layer_1 = nn.Conv2d(in_channels, num_channels, kernel_size=3, padding=(1, 1), stride=strides)
        self.convolution_layer_2 = nn.Conv2d(num_channels, num_channels, kernel_size=3, padding=(1, 1))
        self.convolution_layer_3 = nn.Conv2d(in_channels, num_channels, kernel_size=1, stride=strides) if use_1x1conv else None
        self.batch_norm_layer_1 = nn.BatchNorm2d(num_channels)
        self.batch_norm_layer_2 = nn.BatchNorm2d(num_channels)

    # NHWC in (channels padded to 32), NHWC out; `out` optionally names the destination view
    def forward_nhwc(self, x, out: OutSlot | None = None, x_nchw=None):
        """``x_nchw`` (eval mode, thin first block only): the block's input as the reference's NCHW tensor — read directly by the two
        thin-input convs, ``x`` may then be None (no NCHW -> NHWC conversion of the network input)."""
        c1, c2, c3 = self.convolution_layer_1, self.convolution_layer_2, self.convolution_layer_3
        b1, b2 = self.batch_norm_layer_1, self.batch_norm_layer_2
        if self.training:
            # (the RGBD first layer, 4 -> 64, is routed to the direct thin-convolution kernels inside the op)
            # X has two consumers; the gradient of the skip path is added inside the first conv's input-gradient GEMM
            y, xs = ops.conv2d_shared_input(x, c1.weight, c1.bias, self.strides, "feeds_bn")
            y = ops.BatchNormTrainFn.apply(y, b1.weight, b1.bias, b1.running_mean, b1.running_var, None, ACT_RELU, 0.0, None)
            y = ops.Conv2dFn.apply(y, c2.weight, c2.bias, 1, "feeds_bn")
            skip = ops.Conv2dFn.apply(xs, c3.weight, c3.bias, self.strides, None) if c3 is not None else xs
            _count_batch(b1, b2)
            return ops.BatchNormTrainFn.apply(y, b2.weight, b2.bias, b2.running_mean, b2.running_var, skip, ACT_RELU, 0.0, out)
        if eval_grad_wanted(self, x):
            # eval mode under autograd: the running-statistics BatchNorms as differentiable ops (hip_ops.ConvBNEvalFn / BatchNormEvalFn)
            y = _conv_bn_eval(c1, b1, x, self.strides, None, None)
            skip = ops.Conv2dFn.apply(x, c3.weight, c3.bias, self.strides, None) if c3 is not None else x
            return _conv_bn_eval(c2, b2, y, 1, skip, out)
        with torch.no_grad():
            s1, t1 = _bn_eval_affine(b1)
            s2, t2 = _bn_eval_affine(b2)
            if x_nchw is not None:  # thin first block: both convs read the NCHW input as it is
                y = ops.conv2d_thin_forward_nchw(x_nchw, c1.weight, c1.bias, act=ACT_RELU, scale=s1, shift=t1, measure_out=True)
                if _THIN_RES:  # the 1x1 shortcut evaluated by the second conv's epilogue: the shortcut tensor is never written (same bits)
                    z = ops.conv2d_forward_thin_res(y, c2.weight, c2.bias, x_nchw, c3.weight, c3.bias, act=ACT_RELU, scale=s2, shift=t2, out=out,
                                                    measure_out=True)
                    if z is not None:
                        return z
                skip = ops.conv2d_thin_forward_nchw(x_nchw, c3.weight, c3.bias)
                return ops.conv2d_forward_raw(y, c2.weight, c2.bias, 1, act=ACT_RELU, scale=s2, shift=t2, res=skip, out=out, measure_out=True)
            y = ops.conv2d_forward_raw(x, c1.weight, c1.bias, self.strides, act=ACT_RELU, scale=s1, shift=t1, measure_out=True)
            skip = ops.conv2d_forward_raw(x, c3.weight, c3.bias, self.strides) if c3 is not None else x
            return ops.conv2d_forward_raw(y, c2.weight, c2.bias, 1, act=ACT_RELU, scale=s2, shift=t2, res=skip, out=out, measure_out=True)

    def forward(self, X):
        x = ops.ToNHWC.apply(X, ops.pad_to(X.shape[1], 32))
        y = ops.ToNCHW.apply(self.forward_nhwc(x), self.num_channels)
        flush_batch_counters()
        return y


class SymmetricConv2d(nn.Module):
    """1-channel 3x3 conv whose taps share one parameter per squared distance from the centre
    (index 0 centre, 1 edge, 2 corner) + scalar bias. ref: neural_network_components.py:35-75.
    Evaluated as a 9-term shifted sum (pointwise on a 384^2 plane), not as a GEMM."""

    def __init__(self, kernel_size=3, padding=1):
        super().__init__()
        if kernel_size != 3 or padding != 1:
            raise NotImplementedError("the hot path uses kernel_size=3, padding=1")
        self.kernel_size, self.padding, self.center = kernel_size, padding, kernel_size // 2
        self.params = nn.Parameter(torch.abs(torch.randn(3)))
        self.bias = nn.Parameter(torch.zeros(1))
        self.distance_map = torch.tensor([[2, 1, 2], [1, 0, 1], [2, 1, 2]], dtype=torch.long)  # plain attribute, as in the reference

    def forward(self, x):
        p = torch.nn.functional.pad(x, (1, 1, 1, 1))
        H, W = x.shape[-2], x.shape[-1]
        win = lambda dy, dx: p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]  # noqa: E731
        edge = win(-1, 0) + win(1, 0) + win(0, -1) + win(0, 1)
        corner = win(-1, -1) + win(-1, 1) + win(1, -1) + win(1, 1)
        return self.params[0] * x + self.params[1] * edge + self.params[2] * corner + self.bias


class ChannelWiseSymmetricConv(nn.Module):
    """One SymmetricConv2d per colour. ref: neural_network_components.py:78-95."""

    def __init__(self, kernel_size=3, padding=1):
        super().__init__()
        self.conv_r = SymmetricConv2d(kernel_size, padding)
        self.conv_g = SymmetricConv2d(kernel_size, padding)
        self.conv_b = SymmetricConv2d(kernel_size, padding)

    def forward(self, x):
        return torch.cat((self.conv_r(x[:, 0:1]), self.conv_g(x[:, 1:2]), self.conv_b(x[:, 2:3])), dim=1)

    def taps_and_bias(self):
        """(3,3) taps [colour][centre, edge, corner] and (3,) biases for the fused inference kernel."""
        convs = (self.conv_r, self.conv_g, self.conv_b)
        return torch.stack([c.params for c in convs]).contiguous(), torch.cat([c.bias for c in convs]).contiguous()


class fakeChannelWiseSymmetricConv(nn.Module):
    def __init__(self, kernel_size=3, padding=1):
        super().__init__()

    def forward(self, x):
        return x


class UNet(nn.Module):
    """Four-level residual UNet, widths 64..1024, MaxPool 2x2 down, ConvTranspose 2x2 up, 1x1 sigmoid head.
    ref: neural_network_components.py:241-315.  Skip concatenations are channel slices of one NHWC
    buffer written in place by their producers (skip first, as torch.cat((encoderN, up), 1))."""

    def __init__(self, output_channels=6, in_channels=4):
        super().__init__()
        self.output_channels, self.in_channels = output_channels, in_channels
        pool = lambda: nn.MaxPool2d(kernel_size=2, stride=2)  # noqa: E731  (parameter-less; keeps the Sequential indices)
        self.encoder1 = nn.Sequential(self.conv_block(64, in_channels))
        self.encoder2 = nn.Sequential(pool(), self.conv_block(128, 64))
        self.encoder3 = nn.Sequential(pool(), self.conv_block(256, 128))
        self.encoder4 = nn.Sequential(pool(), self.conv_block(512, 256))
        self.bottleneck = nn.Sequential(pool(), self.conv_block(1024, 512), nn.ConvTranspose2d(1024, 512, kernel_size=2, stride=2))
        self.decoder1 = nn.Sequential(self.conv_block(512, 1024), nn.ConvTranspose2d(512, 256, kernel_size=2, stride=2))
        self.decoder2 = nn.Sequential(self.conv_block(256, 512), nn.ConvTranspose2d(256, 128, kernel_size=2, stride=2))
        self.decoder3 = nn.Sequential(self.conv_block(128, 256), nn.ConvTranspose2d(128, 64, kernel_size=2, stride=2))
        self.decoder4 = self.conv_block(64, 128)
        self.final_layer = nn.Sequential(nn.Conv2d(64, output_channels, kernel_size=1), nn.Sigmoid())

    def conv_block(self, out_channels, in_channels=None):
        return nn.Sequential(ResidualBlock(out_channels, use_1x1conv=True, in_channels=in_channels))

    @staticmethod
    def _block(seq_entry):
        return seq_entry[0] if isinstance(seq_entry, nn.Sequential) else seq_entry

    def _up(self, convt: nn.ConvTranspose2d, x, out: OutSlot, record: bool):
        if record:
            return ops.ConvTranspose2x2Fn.apply(x, convt.weight, convt.bias, out)
        with torch.no_grad():
            return ops.ConvTranspose2x2Fn.apply(x, convt.weight, convt.bias, out)

    def _cat(self, skip, up, buf, share, record: bool):
        if record:
            return ops.CatViewsFn.apply(skip, up, OutSlot(buf, share))
        return share.tag(buf)

    def forward(self, X):
        if X.shape[1] != self.in_channels or X.shape[2] % 16 or X.shape[3] % 16:
            raise ValueError(f"UNet expects (B,{self.in_channels},H,W) with H, W multiples of 16, got {tuple(X.shape)}")
        N, _, H, W = X.shape
        dev = X.device
        blk1 = self._block(self.encoder1[0])
        # eval mode: the first block's two thin-input convs (4 -> 64, 3x3 and the 1x1 shortcut) read the NCHW frame directly
        direct = (_THIN_NCHW and not self.training and not torch.is_grad_enabled() and X.is_cuda and X.dtype == torch.float32 and blk1.strides == 1
                  and blk1.convolution_layer_3 is not None and ops.activation_storage() == "fp32"
                  and ops.thin_mode(self.in_channels, 64, 3, 1) == 1 and ops.thin_mode(self.in_channels, 64, 1, 1) == 1)
        # train mode, or an eval-mode forward that autograd records: the transposed convs, concatenations and the head as autograd ops
        record = self.training or eval_grad_wanted(self, X)
        x = None if direct else ops.ToNHWC.apply(X, 32)
        new = lambda h, w, c: ops.new_nhwc(N, h, w, c, dev)  # noqa: E731  (fp32, or bf16 in the bf16 storage mode)
        buf4, buf3, buf2, buf1 = new(H, W, 128), new(H // 2, W // 2, 256), new(H // 4, W // 4, 512), new(H // 8, W // 8, 1024)
        # one max|.| slot per concatenation buffer: the encoder block and the transposed conv that fill its halves both measure into it
        sh4, sh3, sh2, sh1 = (ops.AmaxShare(dev, buf=b_) for b_ in (buf4, buf3, buf2, buf1))

        # (an encoder output feeds the pool and the skip concatenation: maxpool2x2_with_skip hands back an alias for the skip, and the
        #  pool's backward kernel adds the skip's gradient itself)
        pool_skip = ops.maxpool2x2_with_skip
        e1 = blk1.forward_nhwc(x, OutSlot(buf4[..., :64], sh4), x_nchw=X if direct else None)
        p1, e1 = pool_skip(e1)
        e2 = self._block(self.encoder2[1]).forward_nhwc(p1, OutSlot(buf3[..., :128], sh3))
        p2, e2 = pool_skip(e2)
        e3 = self._block(self.encoder3[1]).forward_nhwc(p2, OutSlot(buf2[..., :256], sh2))
        p3, e3 = pool_skip(e3)
        e4 = self._block(self.encoder4[1]).forward_nhwc(p3, OutSlot(buf1[..., :512], sh1))
        p4, e4 = pool_skip(e4)
        b = self._block(self.bottleneck[1]).forward_nhwc(p4)
        u = self._up(self.bottleneck[2], b, OutSlot(buf1[..., 512:], sh1), record)
        d = self._block(self.decoder1[0]).forward_nhwc(self._cat(e4, u, buf1, sh1, record))
        u = self._up(self.decoder1[1], d, OutSlot(buf2[..., 256:], sh2), record)
        d = self._block(self.decoder2[0]).forward_nhwc(self._cat(e3, u, buf2, sh2, record))
        u = self._up(self.decoder2[1], d, OutSlot(buf3[..., 128:], sh3), record)
        d = self._block(self.decoder3[0]).forward_nhwc(self._cat(e2, u, buf3, sh3, record))
        u = self._up(self.decoder3[1], d, OutSlot(buf4[..., 64:], sh4), record)
        d = self._block(self.decoder4).forward_nhwc(self._cat(e1, u, buf4, sh4, record))
        head = self.final_layer[0]
        flush_batch_counters()
        if record:
            return ops.SigmoidHeadFn.apply(d, head.weight, head.bias)
        with torch.no_grad():
            return ops.conv2d_forward_raw(d, head.weight, head.bias, 1, act=ops.ACT_SIGMOID, planar=True)


_ = ACT_NONE
