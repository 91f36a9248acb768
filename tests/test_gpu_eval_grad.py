"""Eval-mode forward under autograd: the backward of a BatchNorm that normalises with its running statistics (lhg_bn_eval_backward,
hip_ops.ConvBNEvalFn / BatchNormEvalFn) and the modules that use it — frozen-BatchNorm fine-tuning, a frozen critic as a loss, input
gradients through a frozen generator.  ref: model.eval() only switches BatchNorm to the running statistics
(learnedMethodForHologram/neural_network_components.py:26-32, watermelon_hologram/discriminator.py:34-40).

Gradients are checked against a float64 evaluation of the same maths: the fp32 GPU error must be within a small multiple of the fp32 CPU
oracle's own error (the pattern of test_gpu_path.test_unet_train_gradients_vs_fp64_truth), in relative L2 — max-pool argmax and ReLU
masks are discontinuous, so two fp32 evaluations route a few element gradients differently."""

import itertools

import pytest
import torch

from conftest import rel_err
from oracle import nets, optics, seeded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WL = torch.tensor([638e-9, 520e-9, 450e-9])
PITCH = 3.74e-6


def l2_err(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _is_bn(key):
    """BatchNorm affine parameter: ...batch_norm_layer_N.* of the UNet, blockN.1.* of the critic."""
    return "batch_norm_layer_" in key or (key.startswith("block") and ".1." in key)


def _unet_sd():
    return {k[len("part1.part1."):]: v for k, v in seeded.generator_state_dict().items() if k.startswith("part1.part1.")}


def _dtype(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _set_trainable(named, setting):
    """"all": every parameter trains (BatchNorm affine too: the unfused route); "bn_frozen": BatchNorm gamma / beta frozen, convs train
    (the fused route); "input_only": everything frozen, only the input gradient is wanted."""
    for k, p in named:
        if nets.is_buffer_key(k):
            continue
        p.requires_grad_(setting == "all" or (setting == "bn_frozen" and not _is_bn(k)))


def _buffers(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items() if nets.is_buffer_key(k)}


# ----------------------------------------------------------------------------- 1. op level: lhg_bn_eval_backward
def _act_mask(z, act):
    from learned_hologram_gan_amd.hip_ops import ACT_LEAKY, ACT_RELU

    if act == ACT_RELU:
        return (z > 0).double()
    if act == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.2))
    return torch.ones_like(z)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_bn_eval_backward_op(storage):
    """Every act x residual x sums x y case, on channel slices of wider buffers (ld != C for gz, z, y, gy and gres) and a pixel count that
    is not a multiple of any tile: gy, gres and the sums within fp32 rounding of a float64 evaluation of the same stored inputs; in fp32
    storage max|gy| and the per-channel maxima exactly those of the stored gy."""
    from learned_hologram_gan_amd import hip_ops as ops
    from learned_hologram_gan_amd import native
    from learned_hologram_gan_amd.native import call, ptr, stream_ptr

    N, H, W, C, LD, OFF = 2, 13, 11, 64, 96, 16
    P = N * H * W
    g = torch.Generator().manual_seed(5)
    with ops.precision("default", storage=storage):
        dt = ops.act_dtype()
        wide = lambda: torch.randn((N, H, W, LD), generator=g).to(dt).to(DEV)  # noqa: E731
        gz_b, z_b, y_b = wide(), wide(), wide()
        z_b[..., OFF:OFF + C][(torch.rand((N, H, W, C), generator=g) < 0.1).to(DEV)] = 0  # exact zeros: the mask's edge
        gz, z, y = gz_b[..., OFF:OFF + C], z_b[..., OFF:OFF + C], y_b[..., OFF:OFF + C]
        scale = (torch.rand((C,), generator=g) + 0.5).to(DEV)
        stats = torch.cat((torch.randn((C,), generator=g) * 0.1, torch.rand((C,), generator=g) + 0.5)).to(DEV)
        fp32 = storage == "fp32"
        for act, res, want_sums, with_y in itertools.product((ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY), (False, True), (False, True), (False, True)):
            if with_y and not want_sums:
                continue
            gy_b = torch.full((N, H, W, LD), 7.0, dtype=dt, device=DEV)
            gres_b = torch.full((N, H, W, LD), 7.0, dtype=dt, device=DEV)
            gy, gres = gy_b[..., 8:8 + C], gres_b[..., 24:24 + C]
            sums = torch.full(((2 if with_y else 1) * C,), 7.0, device=DEV) if want_sums else None
            ws = torch.empty((4096 * C,), device=DEV) if want_sums else None
            amax = torch.zeros((1,), device=DEV) if fp32 else None
            rows = int(native.load().lhg_chanmax_partial_rows(P, C))
            cpart = torch.empty((rows * C,), device=DEV) if fp32 else None
            call("lhg_bn_eval_backward", ptr(gz), LD, ptr(z), LD, ptr(y) if with_y else None, LD, P, C, ptr(scale), ptr(stats) if with_y else None,
                 act, 0.2, ptr(gy), LD, ptr(gres) if res else None, LD, ptr(sums), ptr(ws), ptr(amax), ptr(cpart), stream_ptr())
            torch.cuda.synchronize()
            case = (storage, act, res, want_sums, with_y)
            gz64, z64, y64 = gz.cpu().double(), z.cpu().double(), y.cpu().double()
            gg = gz64 * _act_mask(z64, act)
            gy_ref = gg * scale.cpu().double()
            tol = 1e-6 if fp32 else 2 ** -8
            assert (gy.cpu().double() - gy_ref).abs().max().item() <= tol * gy_ref.abs().max().item(), case
            # nothing outside the views is touched
            assert (gy_b[..., :8] == 7).all() and (gy_b[..., 8 + C:] == 7).all(), case
            if res:
                assert (gres.cpu().double() - gg).abs().max().item() <= tol * gg.abs().max().item(), case
                assert (gres_b[..., :24] == 7).all() and (gres_b[..., 24 + C:] == 7).all(), case
            else:
                assert (gres_b == 7).all(), case
            if want_sums:
                s = sums.cpu().double()
                ref = gg.sum((0, 1, 2))
                bound = 1e-5 * gg.abs().sum((0, 1, 2)) + 1e-6
                assert ((s[:C] - ref).abs() <= bound).all(), case
                if with_y:
                    xh = (y64 - stats[:C].cpu().double()) * stats[C:].cpu().double()
                    ref1, b1 = (gg * xh).sum((0, 1, 2)), 1e-5 * (gg * xh).abs().sum((0, 1, 2)) + 1e-6
                    assert ((s[C:] - ref1).abs() <= b1).all(), case
            if fp32:
                stored = gy.abs()
                assert amax.item() == stored.max().item(), case
                cmax = torch.empty((C,), device=DEV)
                call("lhg_channel_absmax_finish", ptr(cpart), P, C, ptr(cmax), stream_ptr())
                assert torch.equal(cmax, stored.amax((0, 1, 2))), case


# ----------------------------------------------------------------------------- 2-4. UNet in eval mode
@pytest.mark.parametrize("setting", ["all", "bn_frozen", "input_only"])
def test_unet_eval_gradients_vs_fp64_truth(setting):
    """Eval-mode UNet forward + backward in the three parameter settings: the input gradient and every trainable parameter's gradient
    (conv biases in front of the BatchNorms included: NOT zero in eval mode) against float64 truth; in the two frozen-affine settings the
    forward has the bits of the no_grad eval forward; no BatchNorm buffer changes."""
    from learned_hologram_gan_amd.neural_network_components import UNet

    rows, batch = 32, 2
    sd32 = _unet_sd()
    rgbd, _, _ = seeded.smooth_batch(batch, rows, rows, seed=23)
    proj = torch.randn((batch, 6, rows, rows), generator=torch.Generator().manual_seed(9))

    def run_oracle(dtype):
        sd = nets.as_parameters(_dtype(sd32, dtype))
        _set_trainable(sd.items(), setting)
        x = rgbd.detach().clone().to(dtype).requires_grad_(True)
        y = nets.unet(sd, "", x, False)
        (y * proj.to(dtype)).sum().backward()
        return y.detach().double(), x.grad.double(), {k: v.grad.double() for k, v in sd.items() if v.requires_grad}

    y64, dx64, gw64 = run_oracle(torch.float64)
    y32, dx32, gw32 = run_oracle(torch.float32)
    net = UNet(6, 4)
    net.load_state_dict(sd32)
    net.to(DEV).eval()
    _set_trainable(net.named_parameters(), setting)
    before = _buffers(net)
    x = rgbd.detach().clone().to(DEV).requires_grad_(True)
    with torch.no_grad():
        y_nograd = net(x)
    y = net(x)
    assert y.grad_fn is not None
    (y * proj.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    if setting != "all":
        assert torch.equal(y.detach(), y_nograd), "the fused route must give the no_grad eval forward's bits"
    for k, v in _buffers(net).items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    e_y = rel_err(y.detach().cpu().double(), y64)
    assert e_y <= max(4 * rel_err(y32, y64), 1e-5), e_y
    e_dx = l2_err(x.grad.cpu().double(), dx64)
    assert e_dx <= max(6 * l2_err(dx32, dx64), 5e-3), e_dx
    named = dict(net.named_parameters())
    assert set(gw64) == {k for k, p in named.items() if p.requires_grad}
    for k, ref in gw64.items():
        assert named[k].grad is not None, k
        e_gpu, e_cpu = l2_err(named[k].grad.cpu().double(), ref), l2_err(gw32[k], ref)
        assert e_gpu <= max(6 * e_cpu, 5e-3), (k, e_gpu, e_cpu)


# ----------------------------------------------------------------------------- 5. critic in eval mode
def _critic(requires_grad_setting=None):
    from learned_hologram_gan_amd.watermelon_hologram.discriminator import WGANGPDiscriminator192

    D = WGANGPDiscriminator192(None, 32, True)
    D.load_state_dict(seeded.critic_state_dict())
    D.to(DEV).eval()
    if requires_grad_setting is not None:
        _set_trainable(D.named_parameters(), requires_grad_setting)
    return D


@pytest.mark.parametrize("setting", ["all", "bn_frozen"])
def test_critic_eval_gradients_vs_fp64_truth(setting):
    """The critic's input and parameter gradients in eval mode (LeakyReLU 0.2 masks read from the BatchNorm outputs; stride-2 layers)."""
    batch, rows = 2, 64
    sd32 = seeded.critic_state_dict()
    x0 = torch.rand((batch, 3, rows, rows), generator=torch.Generator().manual_seed(4))
    proj = torch.randn((batch, (rows // 8) ** 2), generator=torch.Generator().manual_seed(6))

    def run_oracle(dtype):
        sd = nets.as_parameters(_dtype(sd32, dtype))
        _set_trainable(sd.items(), setting)
        x = x0.clone().to(dtype).requires_grad_(True)
        (nets.critic(sd, x, False) * proj.to(dtype)).sum().backward()
        return x.grad.double(), {k: v.grad.double() for k, v in sd.items() if v.requires_grad}

    dx64, gw64 = run_oracle(torch.float64)
    dx32, gw32 = run_oracle(torch.float32)
    D = _critic(setting)
    before = _buffers(D)
    x = x0.clone().to(DEV).requires_grad_(True)
    (D(x) * proj.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for k, v in _buffers(D).items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    e_dx = l2_err(x.grad.cpu().double(), dx64)
    assert e_dx <= max(6 * l2_err(dx32, dx64), 5e-3), e_dx
    named = dict(D.named_parameters())
    for k, ref in gw64.items():
        e_gpu, e_cpu = l2_err(named[k].grad.cpu().double(), ref), l2_err(gw32[k], ref)
        assert e_gpu <= max(6 * e_cpu, 5e-3), (k, e_gpu, e_cpu)


def _generator(rows, cols, pad):
    from learned_hologram_gan_amd.watermelon_hologram.generator import Generator

    G = Generator(rows, cols, pad, 0.45, 3, PITCH, WL, torch.tensor([1e-3]))
    G.load_state_dict(seeded.generator_state_dict())
    return G.to(DEV)


def _optics(rows, cols, pad, dtype):
    o = optics.make_optics(rows, cols, pad, 0.45, PITCH, WL)
    Hf = optics.transfer_function(o.w, torch.tensor([1e-3]))[0]
    if dtype == torch.float64:
        o = optics.Optics(o.rows0, o.cols0, o.pad_r, o.pad_c, o.rows, o.cols, o.w.double(), o.mask.double())
        Hf = Hf.to(torch.complex128)
    return o, Hf


def test_frozen_critic_as_generator_loss():
    """D.eval().requires_grad_(False) as the adversarial loss of a train-mode generator: d(-mean D(hat_amps)) / d hat_amps and / d G's
    parameters, with hat_amps the generator's reconstructed amplitude (POH -> fixed-distance propagation), against float64 truth.

    The generator's parameters with fewer than 16 elements (the symmetric stencils' taps and scalar biases, AP2POH.py:107-110) are left
    out: each is a sum over every pixel with heavy cancellation, a property of the train-mode generator and not of the critic
    (test_gpu_truth._score_param_grads scores them as one group for that reason; `part2.part1.conv_g.bias` at 64^2 sits 5 - 24 x the
    CPU's error from float64 there)."""
    rows, pad, batch = 64, 32, 2
    rgbd, _, _ = seeded.smooth_batch(batch, rows, rows, seed=31)
    sdD32 = seeded.critic_state_dict()

    def run_oracle(dtype):
        o, Hf = _optics(rows, rows, pad, dtype)
        sdG = nets.as_parameters(_dtype(seeded.generator_state_dict(), dtype))
        sdD = _dtype(sdD32, dtype)
        poh = nets.generator(sdG, o, Hf, rgbd.to(dtype), True)
        amp, _ = optics.poh_to_amp_phase(o, Hf, poh)
        amp.retain_grad()
        (-nets.critic(sdD, amp, False).mean()).backward()
        return amp.grad.double(), {k: v.grad.double() for k, v in sdG.items() if v.requires_grad and v.grad is not None}

    (da64, g64), (da32, g32) = run_oracle(torch.float64), run_oracle(torch.float32)
    G = _generator(rows, rows, pad).train()
    D = _critic()
    D.requires_grad_(False)
    before = _buffers(D)
    poh = G(rgbd.to(DEV))
    hat_amps, _ = G.part2.propagator.propagate_POH2AP_forward(poh)
    hat_amps.retain_grad()
    loss = -D(hat_amps).mean()
    assert loss.grad_fn is not None
    loss.backward()
    torch.cuda.synchronize()
    for k, v in _buffers(D).items():
        assert torch.equal(v, before[k]), f"the frozen critic changed {k}"
    e_da = l2_err(hat_amps.grad.cpu().double(), da64)
    assert e_da <= max(6 * l2_err(da32, da64), 5e-3), e_da
    named = dict(G.named_parameters())
    for k, ref in g64.items():
        if k.endswith(("convolution_layer_1.bias", "convolution_layer_2.bias")) or ref.numel() < 16:
            continue  # analytically zero (the generator's BatchNorms are in train mode) / scalar sums with heavy cancellation (docstring)
        e_gpu, e_cpu = l2_err(named[k].grad.cpu().double(), ref), l2_err(g32[k], ref)
        assert e_gpu <= max(6 * e_cpu, 2e-2), (k, e_gpu, e_cpu)


# ----------------------------------------------------------------------------- 6. frozen-BatchNorm fine-tune step
def test_frozen_bn_finetune_step_flat_adam():
    """G.eval() with frozen BatchNorm affine parameters, a reconstruction loss, one step of optim.FusedAdam on optim.FlatParams.  The
    flat-buffer slot gradients equal autograd's .grad of an unregistered copy bit for bit (every parameter receives ONE contribution, by
    the same kernels, into a zeroed slot or as autograd's first gradient); the post-step weights match an eval-mode oracle step with
    torch.optim.Adam within the bound of the train-mode step test."""
    from learned_hologram_gan_amd import optim

    rows, pad, batch, lr = 64, 32, 2, 1e-3
    rgbd, tamp, _ = seeded.smooth_batch(batch, rows, rows, seed=41)

    def frozen_bn(G):
        G.eval()
        for k, p in G.named_parameters():
            p.requires_grad_(not _is_bn(k))
        return G

    def loss_of(G):
        hat_amps, _ = G.part2.propagator.propagate_POH2AP_forward(G(rgbd.to(DEV)))
        return ((hat_amps - tamp.to(DEV)) ** 2).mean()

    G = frozen_bn(_generator(rows, rows, pad))
    flat = optim.FlatParams(G)
    opt = optim.FusedAdam(flat, lr=lr)
    before = _buffers(G)
    opt.zero_grad()
    loss_of(G).backward()
    torch.cuda.synchronize()
    slot_grads = {k: p.grad.detach().clone() for k, p in G.named_parameters() if p.requires_grad}
    G2 = frozen_bn(_generator(rows, rows, pad))
    loss_of(G2).backward()
    torch.cuda.synchronize()
    for k, p in G2.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, slot_grads[k]), k
    opt.step()
    torch.cuda.synchronize()
    for k, v in _buffers(G).items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"

    o, Hf = _optics(rows, rows, pad, torch.float32)
    sd = nets.as_parameters(seeded.generator_state_dict())
    for k, v in sd.items():
        if v.requires_grad and _is_bn(k):
            v.requires_grad_(False)
    trainable = {k: v for k, v in sd.items() if v.requires_grad}
    ref_opt = torch.optim.Adam(list(trainable.values()), lr=lr)
    amp, _ = optics.poh_to_amp_phase(o, Hf, nets.generator(sd, o, Hf, rgbd, False))
    ((amp - tamp) ** 2).mean().backward()
    ref_opt.step()
    post = G.state_dict()
    for k, v in trainable.items():
        d = (post[k].cpu() - v.detach()).abs()
        bad = d > 2e-4 + 1e-3 * v.detach().abs()
        assert bad.float().mean().item() <= max(2e-2, 6.0 / v.numel()), (k, int(bad.sum()), v.numel())
        assert not bad.any() or d[bad].max().item() <= 2.1 * lr, (k, d[bad].max().item())
    for k in sd:
        if _is_bn(k) and not nets.is_buffer_key(k):
            assert torch.equal(post[k].cpu(), sd[k]), f"frozen {k} moved"


# ----------------------------------------------------------------------------- 7. double backward
def test_eval_critic_double_backward_raises():
    """A gradient penalty through an eval-mode critic would need the double backward of the running-statistics BatchNorm: it raises,
    it never returns silent zeros."""
    D = _critic()
    x = torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="eval-mode BatchNorm"):
        (gx,) = torch.autograd.grad(D(x).sum(), x, create_graph=True)
        gx.pow(2).sum().backward()


def test_eval_no_grad_paths_unchanged():
    """Eval mode under no_grad, or with nothing requiring grad, returns outputs without a graph (the inference kernels)."""
    G = _generator(64, 64, 32).eval()
    rgbd, _, _ = seeded.smooth_batch(1, 64, 64, seed=3)
    with torch.no_grad():
        a = G(rgbd.to(DEV))
    G.requires_grad_(False)
    b = G(rgbd.to(DEV))
    assert a.grad_fn is None and b.grad_fn is None
    assert torch.equal(a, b)
