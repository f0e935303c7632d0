"""LTX-Video feed-forward adapters (ff.net.0.proj, ff.net.2) on the MI355X: the gelu_from_pre kernel against fp64 and against the GELU GEMM's own bits, the
ten-adapter block stack against the CPU oracle (tests/ltx_ff_lora_reference.py) with the yardstick measured inside the test, exact zeros, the backward's
schedules against each other, the fused step and its DCP training state, the sampler, and the refusals of the ftmi_ltx_ff_* entries.  Run on the MI355X box: pytest -m gpu.

Geometry: the suite's smallest LTX case -- 2 blocks, B = 2, F x H x W = 3 x 4 x 6, i.e. M = 144 token rows (no multiple of 64: the K = 8192 down-projection
and the TN launches see a ragged row tile), text masks of 32 and 96 valid keys."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
CONTROL = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"
LAYERS, B, F_, H_, W_ = 2, 2, 3, 4, 6
D, FF = 2048, 8192
ROPE_SCALE = [1 / (25 / 8), 32, 32]
FLOOR_FACTOR, FLOOR_FACTOR_WORST, PRED_FACTOR = 1.5, 2.0, 1.5  # tests/test_gpu_dit.py's factors and the latent-sampling tests' 1.5
ATOMIC_BOUND = 2e-6  # tools/ltx_digest.py: the project's bound for split-token fp32 atomics
FF_NAMES = ("ff.net.0.proj.lora_A", "ff.net.0.proj.lora_B", "ff.net.2.lora_A", "ff.net.2.lora_B")


def _dev():
    return torch.device("cuda", 0)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------------------------- 1. gelu_from_pre
def _ordered(t):
    """bf16 bit patterns as integers ordered like the values (-0 == +0): neighbours differ by 1."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def _gelu64(z):
    """The tanh-GELU in fp64, 0.5 x (1 + tanh u) with u = sqrt(2 / pi) (x + 0.044715 x^3), evaluated as x sigmoid(2u): the same function, without the
    cancellation of 1 + tanh u.  At x = -10 the true value is -1.2e-37, a normal bf16 number 548 steps from zero, and fp64's tanh has long rounded to -1
    there: the literal formula returns -0 and would fault a kernel that is right."""
    x = z.double()
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def _gemm_gelu(zvals):
    """(g, z) an EPI_GELU GEMM launch writes for pre-activations ``zvals`` (any shape): x = the values as [M, 128] rows, W = the 128 x 128 identity, no bias, so
    every accumulator holds one value exactly and the stashed z is the input."""
    from finetrainers_amd import _lib, ops

    flat = zvals.reshape(-1)
    n = flat.numel()
    rows = -(-n // 128)
    x = torch.zeros(rows * 128, dtype=bf16, device=flat.device)
    x[:n] = flat
    eye = torch.eye(128, dtype=bf16, device=flat.device)
    g, z = ops.gemm_nt(x.view(rows, 128), eye, epilogue=_lib.EPI_GELU, want_out2=True)
    return g.reshape(-1)[:n].reshape(zvals.shape), z.reshape(-1)[:n].reshape(zvals.shape)


@pytest.mark.parametrize("width", [8, 136, 8192])
@pytest.mark.parametrize("rows", [1, 63, 144])
def test_gelu_from_pre_vs_fp64_and_the_gemm_epilogue(rows, width):
    from finetrainers_amd import ops

    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(rows * 10007 + width)
    ldz, ldg = width + 24, width + 40  # leading dimensions larger than the width (multiples of 8: the vector path)
    zbuf = (torch.randn((rows, ldz), generator=g, device=dev) * 2.0).to(bf16)
    big = torch.finfo(bf16).max
    planted = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 3.0, -3.0, 10.0, -10.0, 30.0, -30.0, big, -big], device=dev).to(bf16)
    zflat = zbuf[:, :width].reshape(-1)
    idx = torch.randperm(zflat.numel(), generator=g, device=dev)[:min(planted.numel(), zflat.numel())]
    zflat[idx] = planted[:idx.numel()]
    # the kernel's input is what a GELU GEMM stashed: the planted values go through the identity GEMM first (its stash holds them value for value; a -0 comes
    # back as the accumulator's +0, which is why the kernel is fed the stash itself)
    g_gemm, z_gemm = _gemm_gelu(zflat.view(rows, width).contiguous())
    assert torch.equal(_ordered(z_gemm), _ordered(zflat.view(rows, width))), "the identity GEMM must stash its input as z"
    zbuf[:, :width] = z_gemm
    z = zbuf[:, :width]
    poison = torch.full((rows + 2, ldg), -7.0, dtype=bf16, device=dev)  # a guard row before and after, guard columns to the right
    out = poison[1:rows + 1, :width]
    ops.gelu_from_pre(z, out=out)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    # (c) nothing outside the rows x width window was written
    assert (poison[0] == -7.0).all() and (poison[rows + 1] == -7.0).all() and (poison[1:rows + 1, width:] == -7.0).all()
    # (b) bit-equal to the g an EPI_GELU GEMM launch wrote next to its stashed z
    assert torch.equal(out.contiguous().view(torch.int16), g_gemm.view(torch.int16))
    # (a) every element is the bf16 rounding of the fp64 tanh-GELU of that bf16 z, or its bf16 neighbour; the neighbour share is at most the GEMM's own
    want = _ordered(_gelu64(z).to(bf16))
    d_k = (_ordered(out) - want).abs()
    d_g = (_ordered(g_gemm) - want).abs()
    share_k, share_g = (d_k == 1).float().mean().item(), (d_g == 1).float().mean().item()
    print(f"[gelu_from_pre {rows}x{width}] neighbour share {share_k:.4f} (EPI_GELU GEMM on the same z: {share_g:.4f}); max step {d_k.max().item()}")
    assert d_k.max().item() <= 1
    assert share_k <= share_g
    # the contiguous default output and a base that breaks the 16-byte alignment (element path) give the same bits
    assert torch.equal(ops.gelu_from_pre(z).view(torch.int16), out.contiguous().view(torch.int16))
    if width > 8:
        odd = ops.gelu_from_pre(zbuf[:, 1:width])
        assert torch.equal(odd.view(torch.int16), out[:, 1:].contiguous().view(torch.int16))


def test_gelu_from_pre_empty_is_no_launch():
    from finetrainers_amd import _lib

    assert _lib.load().ftmi_gelu_from_pre(None, 8, None, 8, 0, 8, None) == 0
    assert _lib.load().ftmi_gelu_from_pre(None, 8, None, 8, -3, 8, None) == 0
    assert _lib.load().ftmi_gelu_from_pre(None, 8, None, 8, 4, 8, None) != 0  # rows > 0 with null tensors: refused


# ---------------------------------------------------------------------------------------------------------------- shared builders
def _inputs(cfg, seed=3):
    from oracle import ltx

    inp = ltx.synth_inputs(cfg, B, F_, H_, W_, seed=seed, mask_lens=[32, 96], sigmas=[0.25, 0.7])
    inp.latents_mean = torch.randn(cfg.in_channels, generator=torch.Generator().manual_seed(5)) * 0.1
    inp.latents_std = 1.0 + 0.2 * torch.rand(cfg.in_channels, generator=torch.Generator().manual_seed(6))
    return inp


def _gpu_model(omodel, rank, alpha, target=CONTROL):
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification

    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=LAYERS))
    gmodel = spec.load_diffusion_models(state_dict=omodel.state_dict(), device=_dev())["transformer"]
    gmodel.add_adapter(r=rank, lora_alpha=alpha, target_modules=target)
    lora = {k: v for k, v in omodel.state_dict().items() if "lora_" in k}
    if target != CONTROL:
        lora = {k: v for k, v in lora.items() if ".ff.net." not in k}
    gmodel.load_lora_state_dict(lora)
    return spec, gmodel


def _gpu_forward(spec, gmodel, inp):
    dev = _dev()
    return spec.forward(
        transformer=gmodel,
        condition_model_conditions={"encoder_hidden_states": inp.encoder_hidden_states.to(dev), "encoder_attention_mask": inp.encoder_attention_mask.to(dev)},
        latent_model_conditions={"latents": inp.latents.to(dev), "latents_mean": inp.latents_mean, "latents_std": inp.latents_std,
                                 "num_frames": F_, "height": H_, "width": W_},
        sigmas=inp.sigmas.view(-1, 1, 1, 1, 1).to(dev), noise=inp.noise.to(dev), first_frame_sigma=None, force_first_frame_branch=False)


def _clear_grads(gmodel):
    for p in gmodel.parameters():
        p.grad = None


def _backward(spec, gmodel, inp, clear=True):
    from finetrainers_amd.trainer import sft_loss

    if clear:
        _clear_grads(gmodel)
    pred, target, sig = _gpu_forward(spec, gmodel, inp)
    sft_loss(pred, target, sig, "none").backward()
    torch.cuda.synchronize()
    return pred.detach().clone(), {k: v.detach().float().cpu().clone() for k, v in gmodel.lora_grad_views().items()}


@pytest.fixture(scope="module")
def rank64():
    """The rank-64 oracle pair and GPU model, shared by the tests that do not change the parameters."""
    import ltx_ff_lora_reference as ref
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel, m32 = ref.build_pair(cfg, 64, 64.0)
    inp = _inputs(cfg)
    spec, gmodel = _gpu_model(omodel, 64, 64.0)
    return cfg, omodel, m32, inp, spec, gmodel


# ---------------------------------------------------------------------------------------------------------------- 2. block-stack parity
def _parity(cfg, omodel, m32, inp, spec, gmodel, tag):
    import ltx_ff_lora_reference as ref
    from oracle import ltx

    loss_ref, pred_ref, _ = ltx.forward_loss(omodel, inp, contiguous_hidden_states=True)
    for p in omodel.parameters():
        p.grad = None
    loss_ref.backward()
    g_ref = {n.replace(".default", ""): p.grad.detach().clone() for n, p in ltx.lora_parameters(omodel)}
    inp32 = ref.float_inputs(inp)
    loss32, pred32, _ = ltx.forward_loss(m32, inp32, contiguous_hidden_states=True)
    for p in m32.parameters():
        p.grad = None
    loss32.backward()
    g_32 = {n.replace(".default", ""): p.grad.detach().clone() for n, p in ltx.lora_parameters(m32)}
    assert len(g_ref) == 20 * LAYERS == len(g_32)

    pred, gv = _backward(spec, gmodel, inp)
    assert set(gv) == set(g_ref)
    d_oracle, d_oracle_worst = ltx.grads_rel_l2(g_ref, g_32)
    d_kernel, d_kernel_worst = ltx.grads_rel_l2(gv, g_32)
    p_oracle, p_kernel = rel_l2(pred_ref.detach(), pred32.detach()), rel_l2(pred, pred32.detach())
    print(f"[ltx-ff {tag}] prediction: kernel vs fp32 {p_kernel:.3e}, bf16 oracle vs fp32 {p_oracle:.3e}, ratio {p_kernel / p_oracle:.2f}")
    print(f"[ltx-ff {tag}] all gradients: kernel {d_kernel:.3e} / worst {d_kernel_worst:.3e}; bf16 oracle {d_oracle:.3e} / worst {d_oracle_worst:.3e}; "
          f"ratio {d_kernel / d_oracle:.2f} / {d_kernel_worst / d_oracle_worst:.2f}")
    for l in range(LAYERS):
        for n in FF_NAMES:
            k = f"transformer_blocks.{l}.{n}.weight"
            dk, do = rel_l2(gv[k], g_32[k]), rel_l2(g_ref[k], g_32[k])
            print(f"[ltx-ff {tag}] {k:56s} kernel {dk:.3e} oracle {do:.3e} ratio {dk / do:.2f} |g| {g_32[k].norm().item():.3e}")
    # the eight attention adapters of the ten-adapter model on their own: they now receive dn2 and dz through extended launches
    attn = [k for k in g_32 if ".ff.net." not in k]
    ka, _ = ltx.grads_rel_l2({k: gv[k] for k in attn}, {k: g_32[k] for k in attn})
    oa, _ = ltx.grads_rel_l2({k: g_ref[k] for k in attn}, {k: g_32[k] for k in attn})
    print(f"[ltx-ff {tag}] the eight attention adapters: kernel {ka:.3e} oracle {oa:.3e} ratio {ka / oa:.2f}")
    for v in gv.values():
        assert torch.isfinite(v).all()
    assert p_kernel <= PRED_FACTOR * p_oracle
    assert d_kernel <= FLOOR_FACTOR * d_oracle
    assert d_kernel_worst <= FLOOR_FACTOR_WORST * d_oracle_worst
    assert ka <= FLOOR_FACTOR * oa


def test_block_stack_parity_rank64(rank64):
    _parity(*rank64, "r64")


@pytest.mark.parametrize("rank", [128, 32])
def test_block_stack_parity_other_ranks(rank):
    """Rank 128: two K-extension steps per plane.  Rank 32: padded storage."""
    import ltx_ff_lora_reference as ref
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel, m32 = ref.build_pair(cfg, rank, float(rank))
    inp = _inputs(cfg)
    spec, gmodel = _gpu_model(omodel, rank, float(rank))
    _parity(cfg, omodel, m32, inp, spec, gmodel, f"r{rank}")


# ---------------------------------------------------------------------------------------------------------------- 3. exact properties
def test_zero_b_gives_exactly_zero_a_gradients(rank64):
    cfg, omodel, m32, inp, spec, gmodel = rank64
    keep = gmodel.lora_flat.detach().clone()
    try:
        with torch.no_grad():
            gmodel.lora_ff_B1.zero_()
            gmodel.lora_ff_B2.zero_()
        _, gv = _backward(spec, gmodel, inp)
        assert gmodel.lora_ff_A1.grad.abs().max().item() == 0.0 and gmodel.lora_ff_A2.grad.abs().max().item() == 0.0
        assert gmodel.lora_ff_B1.grad.abs().max().item() > 0.0 and gmodel.lora_ff_B2.grad.abs().max().item() > 0.0
        assert gmodel.lora_A.grad.abs().max().item() > 0.0
    finally:
        with torch.no_grad():
            gmodel.lora_flat.copy_(keep)
        gmodel._lora_versions = None
        _clear_grads(gmodel)


def test_rank32_padding_is_exactly_zero_in_gradients_and_after_two_steps():
    import ltx_ff_lora_reference as ref
    from finetrainers_amd.trainer import MI355XSFTStep
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel = ltx.build_model(cfg, seed=0, rank=32, alpha=32.0, lora_b_std=0.02)
    ref.add_ff_lora(omodel, 32, 32.0)
    inp = _inputs(cfg)
    spec, gmodel = _gpu_model(omodel, 32, 32.0)
    dev = _dev()
    _backward(spec, gmodel, inp)
    n_ab = gmodel._lora_A_full.numel() + gmodel._lora_B_full.numel()
    ga1, gb1, ga2, gb2 = gmodel._ff_views(gmodel._grad_flat[n_ab:].view_as(gmodel._lora_ff_full), padded=True)
    for t, pad in ((ga1, ga1[:, 32:, :]), (gb1, gb1[:, :, 32:]), (ga2, ga2[:, 32:, :]), (gb2, gb2[:, :, 32:])):
        assert pad.abs().max().item() == 0.0 and t.abs().max().item() > 0.0
    assert tuple(gmodel.lora_ff_A2.grad.shape) == (LAYERS, 32, FF) and tuple(gmodel.lora_ff_B1.grad.shape) == (LAYERS, FF, 32)
    _clear_grads(gmodel)
    step = MI355XSFTStep(gmodel, spec, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0)
    cond = {"encoder_hidden_states": inp.encoder_hidden_states.to(dev), "encoder_attention_mask": inp.encoder_attention_mask.to(dev)}
    lat = {"latents": inp.latents.to(dev), "latents_mean": inp.latents_mean, "latents_std": inp.latents_std, "num_frames": F_, "height": H_, "width": W_}
    before = gmodel.lora_flat.detach().clone()
    for _ in range(2):
        out = step.step(cond, lat, sigmas=inp.sigmas.to(dev), noise=inp.noise.to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item() and out["grad_norm"].item() > 0
    a1, b1, a2, b2 = gmodel._ff_views(gmodel._lora_ff_full, padded=True)
    for pad in (a1[:, 32:, :], b1[:, :, 32:], a2[:, 32:, :], b2[:, :, 32:]):
        assert pad.abs().max().item() == 0.0
    assert gmodel._lora_A_full[:, :, 32:, :].abs().max().item() == 0.0 and gmodel._lora_B_full[:, :, :, 32:].abs().max().item() == 0.0
    assert not torch.equal(gmodel._lora_ff_full, before[n_ab:].view_as(gmodel._lora_ff_full))


# ---------------------------------------------------------------------------------------------------------------- 4. schedules agree
def _assert_grads_close(got, want, what):
    worst = max(rel_l2(got[k], want[k]) for k in want)
    print(f"[ltx-ff schedules] {what}: worst adapter gradient rel_l2 {worst:.3e} (bound {ATOMIC_BOUND:.0e})")
    assert set(got) == set(want)
    assert worst < ATOMIC_BOUND


def test_backward_schedules_agree(rank64):
    cfg, omodel, m32, inp, spec, gmodel = rank64
    pred0, g0 = _backward(spec, gmodel, inp)
    # checkpoint = 1 against 0
    gmodel.enable_gradient_checkpointing()
    try:
        pred1, g1 = _backward(spec, gmodel, inp)
    finally:
        gmodel.disable_gradient_checkpointing()
    assert torch.equal(pred1.view(torch.int16), pred0.view(torch.int16))
    _assert_grads_close(g1, g0, "checkpoint = 1")
    # one range per block against one range, with the hook's calls recorded
    calls = []
    prev = gmodel._grad_bucket_hook, gmodel._grad_bucket_finish, gmodel.grad_bucket_blocks
    gmodel._grad_bucket_hook, gmodel._grad_bucket_finish, gmodel.grad_bucket_blocks = (lambda lo, hi, *ts: calls.append((lo, hi, [(t.data_ptr(), t.numel(), t.is_contiguous()) for t in ts]))), None, 1
    try:
        pred2, g2 = _backward(spec, gmodel, inp)
        gflat = gmodel._grad_flat
    finally:
        gmodel._grad_bucket_hook, gmodel._grad_bucket_finish, gmodel.grad_bucket_blocks = prev
    assert torch.equal(pred2.view(torch.int16), pred0.view(torch.int16))
    _assert_grads_close(g2, g0, "one range per block")
    assert [(lo, hi) for lo, hi, _ in calls] == [(l, l + 1) for l in reversed(range(LAYERS))]
    cover = torch.zeros(gflat.numel(), dtype=torch.int32)
    for _, _, ts in calls:
        assert len(ts) == 3  # the range's A, B and feed-forward slices
        for p, n, contiguous in ts:
            assert contiguous and (p - gflat.data_ptr()) % 4 == 0
            o = (p - gflat.data_ptr()) // 4
            assert 0 <= o and o + n <= gflat.numel()
            cover[o:o + n] += 1
    assert bool((cover == 1).all()), "the hook's slices must cover every element of the gradient buffer exactly once"
    assert gflat.numel() == gmodel.lora_flat.numel()
    # two accumulated micro-steps against the sum of two single backwards (same inputs: twice the single gradient)
    _backward(spec, gmodel, inp)
    pred3, g3 = _backward(spec, gmodel, inp, clear=False)
    assert torch.equal(pred3.view(torch.int16), pred0.view(torch.int16))
    _assert_grads_close(g3, {k: 2 * v for k, v in g0.items()}, "two accumulated micro-steps")
    # foreign .grad tensors: autograd accumulates into them
    _clear_grads(gmodel)
    for p in gmodel.parameters():
        p.grad = torch.ones_like(p)
    _gpu_pred, target, sig = _gpu_forward(spec, gmodel, inp)
    from finetrainers_amd.trainer import sft_loss

    sft_loss(_gpu_pred, target, sig, "none").backward()
    torch.cuda.synchronize()
    g4 = {k: v.detach().float().cpu() - 1.0 for k, v in gmodel.lora_grad_views().items()}
    worst = max(((g4[k] - g0[k]).norm() / (g0[k].norm() + g0[k].numel() ** 0.5 * 2.0 ** -24)).item() for k in g0)  # (1 + g) - 1 in fp32: 2^-24 absolute per element
    print(f"[ltx-ff schedules] foreign .grad: worst {worst:.3e}")
    assert worst < 1.0
    _clear_grads(gmodel)


# ---------------------------------------------------------------------------------------------------------------- 5. fused step
def test_two_fused_steps_match_the_oracle_and_resume():
    """Two MI355XSFTStep.step calls on the ten-adapter model against the oracle's torch.optim.AdamW over the same parameters, by the acceptance rule of
    tests/test_gpu_dit.py::test_full_step_matches_oracle_step (AdamW's first steps are sign-like: few sign flips of the update, close agreement where the gradient
    is well above its noise); then state_dict -> load_state_dict -> third step against the uninterrupted third step."""
    import ltx_ff_lora_reference as ref
    from finetrainers_amd.trainer import MI355XSFTStep
    from oracle import ltx

    cfg = ltx.LTXConfig.production(num_layers=LAYERS)
    omodel = ltx.build_model(cfg, seed=0, rank=64, alpha=64.0, lora_b_std=0.02)
    ref.add_ff_lora(omodel, 64, 64.0)
    inp = _inputs(cfg, seed=11)
    spec, gmodel = _gpu_model(omodel, 64, 64.0)
    hyper = dict(lr=5e-5, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4)
    opt = ltx.make_optimizer(omodel, **hyper)
    before = {n.replace(".default", ""): p.detach().clone() for n, p in ltx.lora_parameters(omodel)}
    assert len(before) == 20 * LAYERS
    loss_ref, gn_ref, grads_ref = ltx.sft_step(omodel, opt, inp, max_grad_norm=1.0, contiguous_hidden_states=True)
    grads_ref = {k.replace(".default", ""): v for k, v in grads_ref.items()}
    ltx.sft_step(omodel, opt, inp, max_grad_norm=1.0, contiguous_hidden_states=True)

    dev = _dev()
    step = MI355XSFTStep(gmodel, spec, max_grad_norm=1.0, **hyper)
    assert step.exp_avg.numel() == gmodel.lora_flat.numel()
    cond = {"encoder_hidden_states": inp.encoder_hidden_states.to(dev), "encoder_attention_mask": inp.encoder_attention_mask.to(dev)}
    lat = {"latents": inp.latents.to(dev), "latents_mean": inp.latents_mean, "latents_std": inp.latents_std}
    kw = dict(sigmas=inp.sigmas.to(dev), noise=inp.noise.to(dev), force_first_frame_branch=False)
    out = step.step(cond, lat, **kw)
    loss, gn = out["loss"].item(), out["grad_norm"].item()
    print(f"[ltx-ff step] loss {loss:.6f} vs {loss_ref.item():.6f}; grad_norm {gn:.6e} vs {gn_ref.item():.6e}")
    assert abs(loss - loss_ref.item()) / abs(loss_ref.item()) < 1e-3
    assert abs(gn - gn_ref.item()) / gn_ref.item() < 5e-3
    step.step(cond, lat, **kw)
    torch.cuda.synchronize()
    after = gmodel.lora_state_dict()
    flips = total = 0
    num = den = 0.0
    ff_flips = ff_total = 0
    for n, p in ltx.lora_parameters(omodel):
        k = n.replace(".default", "")
        d_ref = (p.detach() - before[k]).float()
        d_got = (after[k].detach().cpu() - before[k]).float()
        f = (torch.sign(d_ref) != torch.sign(d_got)).sum().item()
        flips, total = flips + f, total + d_ref.numel()
        if ".ff.net." in k:
            ff_flips, ff_total = ff_flips + f, ff_total + d_ref.numel()
        big = grads_ref[k].abs() > 0.05 * grads_ref[k].abs().mean()
        num += (d_got[big] - d_ref[big]).pow(2).sum().item()
        den += d_ref[big].pow(2).sum().item()
    upd = (num / max(den, 1e-30)) ** 0.5
    print(f"[ltx-ff step] after two steps: update sign flips {flips}/{total} = {flips / total:.2e} (feed-forward adapters {ff_flips}/{ff_total}); "
          f"update rel_l2 on entries with a non-negligible gradient = {upd:.3e}")
    assert ff_total > 0 and flips / total < 3e-3
    assert upd < 2e-2

    # resume: the moments and the counter travel in state_dict; the parameters are the model's
    sd = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in step.state_dict().items()}
    p2 = gmodel.lora_flat.detach().clone()
    step.step(cond, lat, **kw)
    torch.cuda.synchronize()
    p3 = gmodel.lora_flat.detach().clone()
    with torch.no_grad():
        gmodel.lora_flat.copy_(p2)
    gmodel._lora_versions = None
    step_b = MI355XSFTStep(gmodel, spec, max_grad_norm=1.0, **hyper)
    step_b.load_state_dict(sd)
    step_b.step(cond, lat, **kw)
    torch.cuda.synchronize()
    p3b = gmodel.lora_flat.detach().clone()
    # same parameters, moments, counter and inputs: the two third steps differ by the order of the fp32 atomics in the gradients only (relative ATOMIC_BOUND),
    # which AdamW passes on to the update at that order wherever |g| is above it; 1e-3 of the update's norm leaves room for the entries whose gradient is not
    d = ((p3b - p3).double().norm() / (p3 - p2).double().norm()).item()
    print(f"[ltx-ff step] resumed third step vs uninterrupted: |diff| / |update| = {d:.3e}")
    assert not torch.equal(p3, p2)
    assert d < 1e-3


def test_dcp_training_state_round_trips_the_feed_forward_moments(tmp_path):
    """wire.save_training_state / load_training_state on the ten-adapter model: the AdamW moments of the four feed-forward parameters travel under their peft
    names, come back bit for bit into a fresh step object, and the resumed third step lands on the uninterrupted run's parameters (tests/test_gpu_wire.py's
    acceptance for the eight: 1e-6 relative, fp32 atomics in the weight-gradient GEMMs)."""
    import os

    from finetrainers_amd import wire
    from finetrainers_amd.trainer import MI355XSFTStep

    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(5)
    lat = {"latents": torch.randn((2, 128, 2, 4, 4), generator=g, device=dev).to(bf16), "latents_mean": torch.zeros(128, device=dev), "latents_std": torch.ones(128, device=dev)}
    cond = {"encoder_hidden_states": torch.randn((2, 128, 4096), generator=g, device=dev).to(bf16), "encoder_attention_mask": torch.ones(2, 128, device=dev, dtype=bf16)}
    kw = dict(sigmas=torch.tensor([0.3, 0.7], device=dev), noise=torch.randn((2, 128, 2, 4, 4), generator=g, device=dev).to(bf16), force_first_frame_branch=False)

    def fresh(seed):
        from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification

        spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=1))
        model = spec.load_diffusion_models(device=dev, random_init_seed=0)["transformer"]
        model.add_adapter(r=32, lora_alpha=32.0, target_modules=CONTROL)  # rank 32: the moments are cut out of rank-padded storage
        gg = torch.Generator(device=dev).manual_seed(seed)
        with torch.no_grad():
            for p_ in model.parameters():
                p_.copy_(torch.randn(p_.shape, generator=gg, device=dev) * 0.01)
        return spec, model, MI355XSFTStep(model, spec, lr=1e-3, betas=(0.9, 0.99), weight_decay=1e-2)

    spec, model, step = fresh(0)
    for _ in range(2):
        step.step(dict(cond), dict(lat), **kw)
    ckpt = wire.save_training_state(str(tmp_path), 2, model, step, train_state={"step": 2, "observed_data_samples": 4})
    assert os.path.exists(os.path.join(ckpt, ".metadata"))
    import torch.distributed.checkpoint as dcp

    keys = set(dcp.FileSystemReader(ckpt).read_metadata().state_dict_metadata.keys())
    for n in ("ff.net.0.proj.lora_A", "ff.net.0.proj.lora_B", "ff.net.2.lora_A", "ff.net.2.lora_B"):
        fqn = f"transformer_blocks.0.{n}.default.weight"
        assert f"model.{fqn}" in keys and f"optimizer.state.{fqn}.exp_avg" in keys and f"optimizer.state.{fqn}.exp_avg_sq" in keys and f"optimizer.state.{fqn}.step" in keys
    m1, m2, p2 = step.exp_avg.clone(), step.exp_avg_sq.clone(), model.lora_flat.clone()
    step.step(dict(cond), dict(lat), **kw)
    torch.cuda.synchronize()
    want = model.lora_flat.clone()

    spec2, model2, step2 = fresh(9)
    ts = wire.load_training_state(ckpt, model2, step2)
    assert ts == {"step": 2, "observed_data_samples": 4} and step2.step_count == 2
    assert torch.equal(model2.lora_flat, p2) and torch.equal(step2.exp_avg, m1) and torch.equal(step2.exp_avg_sq, m2)
    n_ab = model2._lora_A_full.numel() + model2._lora_B_full.numel()
    assert step2.exp_avg[n_ab:].abs().max().item() > 0  # the feed-forward region is not empty
    step2.step(dict(cond), dict(lat), **kw)
    torch.cuda.synchronize()
    rel = ((model2.lora_flat - want).norm() / want.norm()).item()
    print(f"[ltx-ff dcp] parameters after the resumed third step vs the uninterrupted run: rel diff {rel:.2e}")
    assert rel < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 6. sampler
def _random_model(target, seed=3):
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification

    dev = _dev()
    spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=LAYERS))
    model = spec.load_diffusion_models(device=dev, random_init_seed=0)["transformer"]
    model.add_adapter(r=64, lora_alpha=64.0, target_modules=target)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        # the random-init scale_shift_table (randn / sqrt(D)) gates the feed-forward branch down to a few percent of the residual stream, and whatever sits on it
        # with it; a trained model's gate is of order one: gate_mlp (row 5 of the block's table) = 1 in both models
        model.tables[:, 5] = 1.0
    with torch.no_grad():  # trained-looking adapters: A and B both non-zero; the first [A | B] elements are the same draws in both models
        model.lora_flat.copy_(torch.randn(model.lora_flat.shape, generator=g, device=dev) * 0.01)
        if model.lora_ff:
            # feed-forward adapters as strong as the layers they sit on, so that the comparison with the eight-adapter model is about the adapters and not about
            # rounding: A at peft's init scale (uniform within 1 / sqrt(fan_in), rms 1 / sqrt(3 fan_in) -- the rms of the base weight's own default init) and
            # B ~ N(0, 1 / sqrt(r)): per output, s x A^T B^T then has the rms of x W^T (rms(A) sqrt(r) sigma_B = rms(W))
            for a_, b_ in ((model.lora_ff_A1, model.lora_ff_B1), (model.lora_ff_A2, model.lora_ff_B2)):
                bound = 1.0 / math.sqrt(a_.shape[-1])
                a_.copy_((torch.rand(a_.shape, generator=g, device=dev) * 2 - 1) * bound)
                b_.copy_(torch.randn(b_.shape, generator=g, device=dev) / math.sqrt(64))
    return model


def _compose(model, text_c, text_u, mask_c, mask_u, x0, sigmas, timesteps, guidance, hold_frames):
    """The denoising loop in Python: model.forward at batch 2B (unconditional rows first) + the step kernel."""
    from finetrainers_amd import ops

    Bv, S, C = x0.shape
    text, mask = torch.cat([text_u, text_c]).contiguous(), torch.cat([mask_u, mask_c]).contiguous()
    x = x0.clone()
    xin = torch.cat([x.to(bf16)] * 2).contiguous()
    hold = hold_frames * (S // F_) * C
    with torch.no_grad():
        for i in range(timesteps.numel()):
            if hold_frames:
                ft = timesteps[i].expand(2 * Bv, F_).clone()
                ft[:, :hold_frames] = 0
                pred = model(xin, text, None, mask, F_, H_, W_, ROPE_SCALE, frame_timestep=ft)["sample"]
                xin = ops.ltx_cfg_euler_step_held(pred, x, sigmas[i].expand(Bv).contiguous(), sigmas[i + 1].expand(Bv).contiguous(), guidance, hold)
            else:
                pred = model(xin, text, timesteps[i].expand(2 * Bv).contiguous(), mask, F_, H_, W_, ROPE_SCALE)["sample"]
                xin = ops.ltx_cfg_euler_step(pred, x, sigmas[i].expand(Bv).contiguous(), sigmas[i + 1].expand(Bv).contiguous(), guidance)
    torch.cuda.synchronize()
    return x


def test_sampler_is_the_composition_bit_for_bit_and_sees_the_feed_forward_adapters():
    """2 blocks, 72 tokens, cond + uncond, 3 Euler steps, guidance 3: MI355XLTXLatentSampler on the ten-adapter model against the Python composition of
    model.forward at batch 2B and the step kernel, text-to-video and with the first latent frame held; and against the eight-adapter model."""
    from finetrainers_amd import ops
    from finetrainers_amd.ltx_video.sampler import MI355XLTXLatentSampler

    dev = _dev()
    ten, eight = _random_model(CONTROL), _random_model(None)
    n8 = eight.lora_flat.numel()
    assert torch.equal(ten.lora_flat[:n8], eight.lora_flat) and ten.lora_flat.numel() > n8
    assert ten.lora_ff_B1.abs().max().item() > 0 and ten.lora_ff_B2.abs().max().item() > 0
    T, C, S = 128, 128, F_ * H_ * W_
    g = torch.Generator(device=dev).manual_seed(17)
    text_c = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
    text_u = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
    mask_c, mask_u = torch.zeros((1, T), dtype=bf16, device=dev), torch.zeros((1, T), dtype=bf16, device=dev)
    mask_c[:, :96], mask_u[:, :32] = 1, 1
    lat0 = torch.randn((1, C, F_, H_, W_), generator=g, device=dev)
    sig = [1.0, 0.71, 0.33, 0.0]
    sigmas = torch.tensor(sig, device=dev)
    timesteps = (sigmas[:-1] * 1000.0).contiguous()
    m0, s1 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    x0 = MI355XLTXLatentSampler.initial_state(1, C, F_, H_, W_, dev, latents=lat0)
    for hold in (0, 1):
        kw = dict(num_frames=F_, height=H_, width=W_, guidance_scale=3.0, sigmas=sig, timesteps=timesteps.cpu().tolist(), latents=lat0)
        if hold:
            kw["cond_frames"] = 1
        got = MI355XLTXLatentSampler(ten).sample(text_c, mask_c, text_u, mask_u, **kw)
        torch.cuda.synchronize()
        want_x = _compose(ten, text_c, text_u, mask_c, mask_u, x0, sigmas, timesteps, 3.0, hold)
        want = ops.ltx_unpack_denorm(want_x, m0, s1, F_, H_, W_)
        assert torch.isfinite(got.float()).all() and got.shape == (1, C, F_, H_, W_)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"hold {hold}: rel_l2 {rel_l2(got, want):.3e}"
        if hold:
            assert torch.equal(got[:, :, :1].view(torch.int16), lat0[:, :, :1].to(bf16).view(torch.int16))
        base = MI355XLTXLatentSampler(eight).sample(text_c, mask_c, text_u, mask_u, **kw)
        torch.cuda.synchronize()
        moved = got.float()[:, :, hold:] - base.float()[:, :, hold:]
        spacing = 2.0 ** (torch.floor(torch.log2(base.float()[:, :, hold:].abs().clamp_min(2.0 ** -126))) - 7)  # bf16 spacing of each state element
        rms_ratio = (moved.pow(2).mean().sqrt() / spacing.pow(2).mean().sqrt()).item()
        steps = moved.abs() / spacing
        print(f"[ltx-ff sampler hold={hold}] ten- vs eight-adapter latents: rms difference / rms bf16 spacing = {rms_ratio:.1f}; "
              f"largest difference {steps.max().item():.1f} spacings, share of elements beyond 10 spacings {(steps > 10).float().mean().item():.3f}")
        # (over all elements, in units of the bf16 spacing of the state: a same-model-up-to-rounding pair would sit at about one)
        assert rms_ratio > 10.0


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_ff_entries_refuse_before_any_launch(rank64):
    from finetrainers_amd import _lib
    from finetrainers_amd._lib import ptr, stream_ptr

    cfg_, omodel, m32, inp, spec, gmodel = rank64
    lib = _lib.load()
    dev = _dev()
    S, T = F_ * H_ * W_, inp.encoder_hidden_states.shape[1]
    cos, sin = gmodel.rope_tables(F_, H_, W_, ROPE_SCALE)
    gmodel.refresh_lora_copies()
    cfg = gmodel._c_config(B, S, T)
    good = gmodel._c_weights(cos, sin)
    assert isinstance(good, _lib.LtxFfWeights)
    ws_bytes = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(good))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    x_t = torch.zeros((B, S, 128), dtype=bf16, device=dev)
    text = inp.encoder_hidden_states.to(dev).to(bf16).contiguous()
    tv = torch.tensor([250.0, 700.0], device=dev)

    def forward(c, w, nbytes):
        pred = torch.full((B, S, 128), -7.0, dtype=bf16, device=dev)
        rc = lib.ftmi_ltx_ff_forward(ctypes.byref(c), ctypes.byref(w), ptr(x_t), ptr(text), None, ptr(tv), ptr(pred), ptr(ws), nbytes, stream_ptr())
        torch.cuda.synchronize()
        return rc, bool((pred == -7.0).all())

    def variant(**changes):
        w = _lib.LtxFfWeights()
        ctypes.memmove(ctypes.byref(w), ctypes.byref(good), ctypes.sizeof(w))
        for k, v in changes.items():
            setattr(w, k, v)
        return w

    rc, untouched = forward(cfg, good, ws_bytes)
    assert rc == 0 and not untouched  # the accepted call does run
    refusals = (_lib.FTMI_ERR_INVALID, _lib.FTMI_ERR_UNSUPPORTED)
    # only some of the eight operand pointers set
    rc, untouched = forward(cfg, variant(ff_b2_ext=None), ws_bytes)
    assert rc in refusals and untouched
    rc, untouched = forward(cfg, variant(**{n: None for n in _lib.LTX_FF_WEIGHT_FIELDS[1:]}), ws_bytes)
    assert rc in refusals and untouched
    # r = 0 with feed-forward pointers set
    c0 = _lib.LtxConfig.from_buffer_copy(bytes(cfg))
    c0.r = 0
    rc, untouched = forward(c0, good, ws_bytes)
    assert rc in refusals and untouched
    # a workspace sized for the eight
    eight_bytes = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(variant(**{n: None for n in _lib.LTX_FF_WEIGHT_FIELDS})))
    assert eight_bytes < ws_bytes
    rc, untouched = forward(cfg, good, eight_bytes)
    assert rc in refusals and untouched
    # the backward and the sampler refuse the same way
    ga = torch.zeros(gmodel.lora_flat.numel(), device=dev)
    dpred = torch.zeros((B, S, 128), dtype=bf16, device=dev)
    n_a, n_b = gmodel._lora_A_full.numel(), gmodel._lora_B_full.numel()
    rc = lib.ftmi_ltx_ff_backward_range(ctypes.byref(cfg), ctypes.byref(variant(ff_a1_sp=None)), None, None, ptr(dpred), ptr(ga), ptr(ga[n_a:]), ptr(ga[n_a + n_b:]),
                                        ptr(ws), ws_bytes, LAYERS, 0, 0, stream_ptr())
    torch.cuda.synchronize()
    assert rc in refusals and ga.abs().max().item() == 0.0
    rc = lib.ftmi_ltx_ff_backward_range(ctypes.byref(cfg), ctypes.byref(good), None, None, ptr(dpred), ptr(ga), ptr(ga[n_a:]), None, ptr(ws), ws_bytes, LAYERS, 0, 0,
                                        stream_ptr())
    assert rc in refusals  # feed-forward adapters without their gradient buffer
    assert lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), ctypes.byref(variant(ff_a2_sp=None)), 1) == 0
