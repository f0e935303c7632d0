"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol the header declares, host logic of the
ModelSpecification / attention-provider / step mirrors, and the product path's refusal to run without the GPU."""

import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def lib():
    from finetrainers_amd import _lib

    if not _lib.lib_available():
        from finetrainers_amd.csrc.build import build

        build()
    return _lib.load()


def test_c_abi_exports_every_declared_symbol(lib):
    from finetrainers_amd import _lib

    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"#ifdef FTMI_EXPERIMENTAL.*?#endif", "", header, flags=re.S)  # research-build section: not part of the product ABI
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"libftmi355.so does not export {name}"
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)
    # the full-argument entries of the LTX row-wise launchers (tests/test_gpu_rowwise_contract.py launches through them)
    assert {"ftmi_norm_modulate_fwd_ex", "ftmi_norm_modulate_bwd_ex", "ftmi_qknorm_rope_fwd_ex", "ftmi_qknorm_rope_bwd_ex"} <= declared
    assert lib.ftmi_version() >= 100


def test_c_abi_error_reporting(lib):
    """int status + ftmi_last_error, converted to ValueError (invalid / unsupported), without touching a GPU."""
    import ctypes

    from finetrainers_amd import _lib

    cfg = _lib.LtxConfig(B=2, S=2688, T=128, D=2048, H=32, L=28, C_in=128, C_out=128, D_ff=8192, D_cap=4096, r=64, lora_scale=1.0,
                         eps_norm=1e-6, eps_qk=1e-5, gemm_variant=8)
    w = ctypes.byref(_lib.LtxFfWeights())  # (no feed-forward adapters; a planner never dereferences the weights)
    ws = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), w)
    assert 8 * 2**30 < ws < 16 * 2**30  # ~10.4 GB of activations at the headline shape
    off = ctypes.c_size_t(0)
    assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), w, b"qkv", 3, ctypes.byref(off)) == 0 and 0 < off.value < ws
    rc = lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), w, b"no_such_tensor", 0, ctypes.byref(off))
    assert rc == _lib.FTMI_ERR_INVALID and "unknown name" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "ftmi_ltx_ff_workspace_offset")
    # NULL tensors are rejected before any launch
    rc = lib.ftmi_gemm_nt(128, 128, 64, None, 64, None, 64, None, 1.0, None, 128, 0, None, None, None, 0, None, 0, 0, None)
    assert rc == _lib.FTMI_ERR_INVALID
    desc = _lib.AttnDesc(B=1, H=1, Sq=64, Sk=64, d=32, scale=0.1)
    rc = lib.ftmi_attn_fwd(ctypes.byref(desc), None, None, None, None, None, None, None)
    assert rc == _lib.FTMI_ERR_UNSUPPORTED and "head_dim" in _lib.last_error()
    # messages are kept per failing thread: another thread's failure does not replace the one this thread is about to read
    import threading

    def other():
        d2 = _lib.AttnDesc(B=0, H=1, Sq=64, Sk=64, d=64, scale=0.1)
        q = ctypes.c_void_p(16)
        assert lib.ftmi_attn_fwd(ctypes.byref(d2), q, q, q, q, None, None, None) == _lib.FTMI_ERR_INVALID
        assert "empty problem" in _lib.last_error()

    th = threading.Thread(target=other)
    th.start()
    th.join()
    assert "head_dim" in _lib.last_error()


def test_product_path_never_imports_the_oracle():
    bad = []
    for dp, _, files in os.walk(os.path.join(ROOT, "finetrainers_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                    bad.append(os.path.join(dp, f))
    assert not bad, f"product code imports the oracle: {bad}"


def test_product_path_fails_loudly_without_gpu():
    from finetrainers_amd import ops
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoTransformer3DModel

    q = torch.zeros(1, 2, 64, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        ops.attn_fwd(q, q, q)
    model = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=1), device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.zeros(1, 32, 128), torch.zeros(1, 128, 4096), torch.tensor([500]), torch.ones(1, 128), 2, 4, 4)
    with pytest.raises(ValueError, match="production geometry"):
        MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_attention_heads=4, attention_head_dim=8), device=torch.device("cpu"))


def test_adapter_surface_is_peft_compatible():
    """sft_trainer/trainer.py:121-136: add_adapter(LoraConfig(r, lora_alpha, init_lora_weights=True, target_modules)); fp32 params;
    names as get_peft_model_state_dict would emit them."""
    from types import SimpleNamespace

    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoTransformer3DModel
    from finetrainers_amd.ltx_video.transformer import DEFAULT_TARGET_MODULES

    model = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=2), device=torch.device("cpu"))
    with pytest.raises(ValueError):
        model.add_adapter(r=0, lora_alpha=1)
    with pytest.raises(ValueError):
        model.add_adapter(SimpleNamespace(r=64, lora_alpha=64, target_modules="ff.net.0.proj"))
    model.add_adapter(SimpleNamespace(r=64, lora_alpha=64, target_modules=DEFAULT_TARGET_MODULES, init_lora_weights=True))
    params = dict(model.named_parameters())
    assert set(params) == {"lora_A", "lora_B"} and all(p.dtype == torch.float32 and p.requires_grad for p in params.values())
    assert params["lora_A"].shape == (2, 8, 64, 2048) and params["lora_B"].shape == (2, 8, 2048, 64)
    assert params["lora_B"].abs().max() == 0 and params["lora_A"].abs().max() > 0  # B = 0, A kaiming-uniform
    bound = (6.0 / (6.0 * 2048)) ** 0.5
    assert params["lora_A"].abs().max() <= bound
    assert params["lora_A"].data_ptr() == model.lora_flat.data_ptr()  # views into one flat buffer [A | B]
    assert params["lora_B"].data_ptr() == model.lora_flat.data_ptr() + 4 * params["lora_A"].numel()
    sd = model.lora_state_dict()
    assert len(sd) == 2 * 8 * 2
    assert sd["transformer_blocks.1.attn2.to_out.0.lora_B.weight"].shape == (2048, 64)
    assert sd["transformer_blocks.0.attn1.to_q.lora_A.weight"].shape == (64, 2048)
    # 224 adapters / 58 720 256 parameters at the production depth
    assert 28 * 8 == 224 and 28 * 8 * 2 * 64 * 2048 == 58_720_256
    with pytest.raises(ValueError):
        model.add_adapter(r=64, lora_alpha=64)  # already attached


def test_adapter_rank_that_is_not_a_multiple_of_64_is_zero_padded():
    """The reference's LTX example trains with --rank 32 --lora_alpha 32 (examples/training/sft/ltx_video/crush_smol_lora/train.sh:75-76): the
    parameters, their state dict and the saved file have rank 32; the storage the kernels see is padded to 64 with zeros."""
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoTransformer3DModel

    model = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=2), device=torch.device("cpu"))
    model.add_adapter(r=32, lora_alpha=32)
    assert model.lora_rank == 32 and model.lora_rank_padded == 64
    assert model.lora_A.shape == (2, 8, 32, 2048) and model.lora_B.shape == (2, 8, 2048, 32)
    assert model.lora_flat.numel() == 2 * 2 * 8 * 64 * 2048
    assert model._lora_A_full[:, :, 32:, :].abs().max() == 0 and model._lora_A_full[:, :, :32, :].abs().max() > 0
    model._assert_flat_aliasing()
    with torch.no_grad():
        model.lora_B.normal_(0, 0.02)  # writes through the view: only the real columns change
    assert model._lora_B_full[:, :, :, 32:].abs().max() == 0 and model._lora_B_full[:, :, :, :32].abs().max() > 0
    sd = model.lora_state_dict()
    assert sd["transformer_blocks.1.attn2.to_out.0.lora_B.weight"].shape == (2048, 32)
    assert sd["transformer_blocks.0.attn1.to_q.lora_A.weight"].shape == (32, 2048)
    other = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=2), device=torch.device("cpu"))
    other.add_adapter(r=32, lora_alpha=32)
    other.load_lora_state_dict(sd)
    assert torch.equal(other.lora_flat, model.lora_flat)
    assert model._c_config(1, 32, 128).r == 64 and abs(model._c_config(1, 32, 128).lora_scale - 1.0) < 1e-7


def test_lr_schedules_match_reference(golden):
    """finetrainers/optimizer.py:191-226: the seven --lr_scheduler multipliers, pinned to values produced by the reference's own functions,
    and the LambdaLR clock (rate before the first step = base * f(0); one step() per optimiser step)."""
    from finetrainers_amd.utils.lr_schedule import LRSchedule, lr_multiplier

    cases = {
        "constant": dict(name="constant"),
        "constant_with_warmup": dict(name="constant_with_warmup", num_warmup_steps=7),
        "piecewise_constant": dict(name="piecewise_constant", step_rules="1:10,0.1:20,0.01:30,0.005"),
        "linear": dict(name="linear", num_warmup_steps=5, num_training_steps=50),
        "cosine": dict(name="cosine", num_warmup_steps=5, num_training_steps=50, num_cycles=1),
        "cosine_half": dict(name="cosine", num_warmup_steps=5, num_training_steps=50, num_cycles=0.5),
        "cosine_with_restarts": dict(name="cosine_with_restarts", num_warmup_steps=5, num_training_steps=50, num_cycles=3),
        "polynomial": dict(name="polynomial", num_warmup_steps=5, num_training_steps=50, lr_init=5e-5, lr_end=1e-7, power=2.0),
    }
    for key, kw in cases.items():
        f = lr_multiplier(**kw)
        ref = golden[f"lr.{key}"]
        got = torch.tensor([f(t) for t in range(ref.numel())], dtype=torch.float64)
        assert torch.equal(got, ref), (key, (got - ref).abs().max())
    with pytest.raises(ValueError):
        lr_multiplier("nope")
    # clock: identical to torch's LambdaLR around a real optimiser
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=5e-5)
    ref = torch.optim.lr_scheduler.LambdaLR(opt, lr_multiplier("constant_with_warmup", num_warmup_steps=4))
    mine = LRSchedule.from_args(5e-5, "constant_with_warmup", num_warmup_steps=4)
    for _ in range(8):
        assert mine.get_last_lr() == ref.get_last_lr()
        opt.step()
        ref.step()
        mine.step()
    again = LRSchedule.from_args(5e-5, "constant_with_warmup", num_warmup_steps=4)
    again.load_state_dict(mine.state_dict())
    assert again.current_lr() == mine.current_lr()


def test_rope_tables_match_upstream_formula():
    from finetrainers_amd.ltx_video.transformer import ltx_rope_tables
    from oracle import ltx

    scale = [1 / (25 / 8), 32, 32]
    cos_c, sin_c = ltx_rope_tables(3, 4, 6, scale)
    rope = ltx.LTXVideoRotaryPosEmbed(dim=2048)
    cos_f, sin_f = rope(torch.zeros(2, 72, 128), 3, 4, 6, scale)
    assert torch.equal(cos_f[0], cos_f[1])  # identical across the batch -> one table per clip shape
    assert torch.equal(cos_f[0, :, 0::2], cos_f[0, :, 1::2]) and torch.equal(sin_f[0, :, 0::2], sin_f[0, :, 1::2])
    assert torch.equal(cos_c, cos_f[0, :, 0::2]) and torch.equal(sin_c, sin_f[0, :, 0::2])


def test_spec_mirror_collation_and_scheduler():
    from finetrainers_amd.ltx_video import MI355XLTXVideoModelSpecification
    from finetrainers_amd.ltx_video.specification import FlowMatchSigmas
    from oracle import ltx

    spec = MI355XLTXVideoModelSpecification()
    assert spec._resolution_dim_keys == {"latents": (2, 3, 4)}
    items = [{"latents": torch.ones(1, 128, 2, 4, 4) * i, "latents_mean": torch.zeros(128), "num_frames": 2} for i in range(3)]
    out = spec.collate_latents(items)
    assert out["latents"].shape == (3, 128, 2, 4, 4) and out["latents_mean"].shape == (128,) and out["num_frames"] == 2
    assert torch.equal(FlowMatchSigmas().sigmas, ltx.scheduler_sigmas())
    with pytest.raises(ValueError):
        MI355XLTXVideoModelSpecification(transformer_dtype=torch.float16)
    with pytest.raises(NotImplementedError):
        spec.load_latent_models()


def test_sigma_sampling_mirror_matches_reference(golden):
    from finetrainers_amd.ltx_video.specification import FlowMatchSigmas
    from finetrainers_amd.utils import diffusion as D

    sch = FlowMatchSigmas()
    for scheme in ("none", "logit_normal", "mode"):
        gen = torch.Generator().manual_seed(21)
        s = D.prepare_sigmas(sch, sch.sigmas, 16, 1000, flow_weighting_scheme=scheme, generator=gen)
        assert torch.equal(s, golden[f"sigmas.{scheme}"])
    sig = torch.tensor([0.25, 0.7])
    assert torch.equal(D.prepare_loss_weights(sch, sigmas=sig, flow_weighting_scheme="none"), torch.ones(2))
    torch.testing.assert_close(D.prepare_loss_weights(sch, sigmas=sig, flow_weighting_scheme="sigma_sqrt"), sig**-2.0)


def test_attention_provider_registry_semantics():
    from finetrainers_amd import attention_dispatch as ad

    reg = ad._AttentionProviderRegistry
    assert ad.AttentionProvider("mi355x") in reg.list_providers()
    name, fn = reg.get_active_provider()
    assert name == ad.AttentionProvider.MI355X and fn is ad._mi355x_attention
    assert not reg.supports_context_parallel(ad.AttentionProvider.MI355X)
    with pytest.raises(ValueError):
        with ad.attention_provider(ad.AttentionProvider.MI355X, mesh=object()):
            pass
    # constraint checks raise ValueError like the reference's (attention_dispatch.py:460-519)
    q = torch.zeros(1, 2, 16, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        ad._check_device_gpu(query=q, key=q, value=q)
    with pytest.raises(ValueError, match="bfloat16"):
        ad._check_qkv_dtype_bf16(query=q.float(), key=q, value=q)
    with pytest.raises(ValueError, match="head_dim"):
        ad._check_head_dim(query=q[..., :32], key=q, value=q)
    with pytest.raises(ValueError):
        ad._check_no_dropout_causal_gqa(is_causal=True)
    # kwargs the provider does not name are dropped by the dispatcher (attention_dispatch.py:442)
    seen = {}

    def fake(query, key, value, attn_mask=None):
        seen.update(attn_mask=attn_mask)
        return query

    old = reg._providers[ad.AttentionProvider.MI355X], reg._supported_arg_names[ad.AttentionProvider.MI355X]
    try:
        reg.register(ad.AttentionProvider.MI355X)(fake)
        out = ad.attention_dispatch(q, q, q, attn_mask=None, dropout_p=0.0, is_causal=False, scale=0.5, enable_gqa=False,
                                    attention_kwargs={"unknown_kw": 1})
        assert out is q and "attn_mask" in seen
    finally:
        reg._providers[ad.AttentionProvider.MI355X], reg._supported_arg_names[ad.AttentionProvider.MI355X] = old
    # LTX's [B, H, 1, T] additive mask -> per-key bias
    m = ((1 - torch.tensor([[1.0, 1, 0, 0], [1, 0, 0, 0]]).to(torch.bfloat16)) * -10000.0).unsqueeze(1)
    m4 = m.repeat_interleave(3, dim=0).view(2, 3, 1, 4)
    kb = ad._key_bias_from_mask(m4, 2, 3, 4)  # materialised per head (diffusers' prepare_attention_mask): honoured per head
    assert kb.shape == (2, 3, 4) and kb[0, 1, 2] == -9984.0 and kb[0, 2, 0] == 0 and kb.dtype == torch.float32
    kb = ad._key_bias_from_mask(m.unsqueeze(1).expand(2, 3, 1, 4), 2, 3, 4)  # an expanded view of one mask -> one row per sample
    assert kb.shape == (2, 4) and kb[0, 2] == -9984.0 and kb[0, 0] == 0 and kb[1, 1] == -9984.0
    # torch SDPA aligns mask dimensions to the RIGHT: a 3-D [X, 1, S_k] mask is per HEAD, not per sample
    kb = ad._key_bias_from_mask(torch.zeros(3, 1, 4), 2, 3, 4)
    assert kb.shape == (2, 3, 4)
    with pytest.raises(ValueError):
        ad._key_bias_from_mask(torch.zeros(2, 1, 4), 2, 3, 4)  # would silently treat the batch axis as heads
    with pytest.raises(ValueError):
        ad._key_bias_from_mask(torch.zeros(2, 3, 5, 4), 2, 3, 4)  # per-query masks are not supported
    # bool masks / -inf: masked keys become a large FINITE negative (weight exactly 0, never NaN)
    kb = ad._key_bias_from_mask(torch.tensor([[True, False, True, True]]), 2, 3, 4)
    assert kb.shape == (2, 4) and kb[1, 1] < -1e29 and torch.isfinite(kb).all() and kb[0, 0] == 0
    kb = ad._key_bias_from_mask(torch.tensor([[0.0, float("-inf"), 0.0, 0.0]]), 2, 3, 4)
    assert torch.isfinite(kb).all() and kb[0, 1] < -1e29
    assert ad.register_into_finetrainers() is False  # the reference package is not importable in this image


def _dp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from finetrainers_amd.parallel import DataParallelBackend

    par = DataParallelBackend(backend="gloo")
    try:
        g = torch.arange(10, dtype=torch.float32) * (rank + 1)
        par.all_reduce_mean_(g)
        m = par.reduce_step_metrics(torch.tensor(1.0 + rank), torch.tensor(10.0 * (rank + 1)))
        w = torch.full((4,), float(rank))
        par.broadcast_(w, src=0)
        q.put((rank, g.tolist(), {k: v.item() for k, v in m.items()}, list(par.shard_indices(7)), w.tolist(), par.is_main_process))
    finally:
        par.destroy()


def test_data_parallel_backend_world_size_2_gloo():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() % 200)
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, g, m, shard, w, main in res:
        assert g == [1.5 * i for i in range(10)]  # mean of g and 2g
        assert m["global_avg_loss"] == 1.5 and m["global_max_loss"] == 2.0 and m["grad_norm"] == 15.0
        assert shard == list(range(rank, 7, 2))
        assert w == [0.0] * 4
        assert main == (rank == 0)


def _bucket_worker(rank, world, port, q):
    """Two ranks drive GradBucketReducer exactly as the DiT backward does: block ranges in descending order, the slices of ONE flat
    [A | B] buffer reported as each range becomes final, later ranges still being 'computed' (written) after earlier ones were issued."""
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from finetrainers_amd.parallel import DataParallelBackend, GradBucketReducer

    par = DataParallelBackend(backend="gloo")
    try:
        L, per = 10, 6  # 10 "blocks", 6 floats of A and of B per block
        flat = torch.zeros(2 * L * per)
        ga, gb = flat[: L * per].view(L, per), flat[L * per:].view(L, per)
        red = GradBucketReducer(par)
        order = []
        hi, step = L, 4
        while hi > 0:
            lo = max(0, hi - step)
            for l in range(lo, hi):  # this range's gradients become final only now
                ga[l] = float(rank + 1) * (l + 1)
                gb[l] = -float(rank + 1) * (l + 1)
            red.bucket_ready(lo, hi, ga[lo:hi], gb[lo:hi])
            order.append((lo, hi))
            hi = lo
        red.finish()
        q.put((rank, flat.tolist(), order, red.buckets_issued))
    finally:
        par.destroy()


def test_bucketed_gradient_exchange_world_size_2_gloo():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 200)
    procs = [ctx.Process(target=_bucket_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    L, per = 10, 6
    want = [1.5 * (l + 1) for l in range(L) for _ in range(per)] + [-1.5 * (l + 1) for l in range(L) for _ in range(per)]
    for rank, flat, order, n in res:
        assert flat == want           # every rank ends with the mean over ranks, A and B slices of every bucket
        assert order == [(6, 10), (2, 6), (0, 2)] and n == 3   # same schedule on every rank: a function of L alone


def _backend_worker(rank, world, port, q):
    """Two ranks drive MI355XParallelBackend the way SFTTrainer does (trainer.py:185-189, 333-336): construct with the PTD arguments, apply_ddp on the
    model, then a 'backward' that reports block ranges through the hooks apply_ddp installed and ends the exchange itself."""
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from finetrainers_amd.parallel import MI355XParallelBackend

    class _Model:  # what apply_ddp touches of MI355XLTXVideoTransformer3DModel: the flat adapter buffer, the two parameters, the hook attributes
        def __init__(self):
            L, per = 8, 4
            self.lora_flat = torch.full((2 * L * per,), float(rank + 1))  # ranks start with DIFFERENT adapters (peft draws A per process)
            self.lora_A, self.lora_B = self.lora_flat[: L * per].view(L, per), self.lora_flat[L * per:].view(L, per)
            self.grad = torch.zeros_like(self.lora_flat)
            self._grad_bucket_hook = self._grad_bucket_finish = None
            self._lora_versions = "stale"

        def backward(self, blocks_per_range):
            L, per = self.lora_A.shape
            ga, gb = self.grad[: L * per].view(L, per), self.grad[L * per:].view(L, per)
            hi = L
            while hi > 0:
                lo = max(0, hi - blocks_per_range)
                ga[lo:hi] = float(rank + 1) * torch.arange(lo, hi, dtype=torch.float32)[:, None]
                gb[lo:hi] = -float(rank + 1)
                if self._grad_bucket_hook is not None:
                    self._grad_bucket_hook(lo, hi, ga[lo:hi], gb[lo:hi])
                hi = lo
            if self._grad_bucket_finish is not None:
                self._grad_bucket_finish()

    b = MI355XParallelBackend(world_size=world, pp_degree=1, dp_degree=world, dp_shards=-1, cp_degree=1, tp_degree=1, backend="gloo", timeout=60,
                              logging_dir="logs", output_dir="/tmp/ftmi_backend_test", gradient_accumulation_steps=1)
    try:
        b.enable_determinism(1234)
        m = b.apply_ddp(_Model(), b.get_mesh())
        after_bcast = m.lora_flat.clone()
        m.backward(m.grad_bucket_blocks if hasattr(m, "grad_bucket_blocks") else 3)
        metrics = b.reduce_step_metrics(torch.tensor(1.0 + rank), torch.tensor(3.0))
        # the reference trainer INDEXES the mesh (trainer.py:512 `get_mesh()["dp_cp"]`, :595 `get_mesh()["dp"]`) and reduces over the sub-mesh
        # (parallel/utils.py:6-19 dist_mean / dist_max): both flattened names must exist and span both ranks
        import torch.distributed as dist

        mesh_sums = []
        for nm in ("dp_cp", "dp"):
            sub = b.get_mesh()[nm]
            t = torch.tensor(float(rank + 1))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=sub.get_group())
            mesh_sums.append((nm, sub.size(), t.item(), b.get_mesh(nm).size()))
        metrics["mesh"] = torch.tensor(float(all(sz == world and tot == 3.0 and sz2 == world for _, sz, tot, sz2 in mesh_sums)))
        with b.main_process_first():
            pass
        b.wait_for_everyone()
        q.put((rank, after_bcast.tolist(), m.grad.tolist(), b.reducer.buckets_issued, m._lora_versions, {k: v.item() for k, v in metrics.items()},
               (b.world_size, b.rank, b.data_parallel_enabled, b.data_replication_enabled, b.data_sharding_enabled, b._dp_degree)))
    finally:
        b.destroy()


def test_parallel_backend_drives_the_exchange_world_size_2_gloo():
    """N2 / a17: the BaseParallelBackend-shaped backend on two real processes (gloo here, RCCL on GPUs): apply_ddp broadcasts rank 0's adapters and
    installs the hooks; after the model's backward every rank holds the rank-AVERAGED gradient -- DDP's contract at that point of the trainer loop."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29400 + (os.getpid() % 150)
    procs = [ctx.Process(target=_backend_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    L, per = 8, 4
    want = [1.5 * l for l in range(L) for _ in range(per)] + [-1.5] * (L * per)
    for rank, bcast, grad, nb, ver, metrics, props in res:
        assert bcast == [1.0] * (2 * L * per)      # rank 0's adapters everywhere
        assert grad == want                        # mean over the two ranks, A and B slices of every bucket
        assert nb == 2 and ver is None             # default 7 blocks per range over 8 blocks -> 2 buckets; stale operand copies invalidated
        assert metrics["global_avg_loss"] == 1.5 and metrics["global_max_loss"] == 2.0
        assert metrics["mesh"] == 1.0              # get_mesh()["dp_cp"] / ["dp"] exist, span both ranks, and reduce over them
        assert props == (2, rank, True, True, False, 2)


def test_wire_formats_roundtrip(tmp_path):
    """LoRA checkpoint (transformer.-prefixed peft keys + lora_config / format metadata), diffusers transformer directory
    (sharded safetensors + index), precomputed-sample files and the prefetching feeder."""
    import json

    from safetensors import safe_open
    from safetensors.torch import save_file

    from finetrainers_amd import wire
    from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification, MI355XLTXVideoTransformer3DModel
    from finetrainers_amd.ltx_video.transformer import DEFAULT_TARGET_MODULES

    # --- LoRA checkpoint through the spec's _save_lora_weights, exactly as trainer.py:283-298 calls it
    model = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=1), device=torch.device("cpu"))
    model.add_adapter(r=64, lora_alpha=64)
    with torch.no_grad():
        model.lora_B.normal_(0, 0.02)
    peft_sd = {k.replace(".default.", "."): v for k, v in model.state_dict().items() if "lora_" in k}  # get_peft_model_state_dict
    assert len(peft_sd) == 16
    spec = MI355XLTXVideoModelSpecification(pretrained_model_name_or_path=str(tmp_path / "nowhere"))
    out_dir = str(tmp_path / "lora_weights" / "000010")
    from finetrainers_amd.ltx_video.specification import FlowMatchSigmas

    spec._save_lora_weights(out_dir, peft_sd, FlowMatchSigmas(), wire.lora_config_metadata(64, 64, DEFAULT_TARGET_MODULES))
    path = os.path.join(out_dir, "pytorch_lora_weights.safetensors")
    with safe_open(path, framework="pt") as f:
        md = f.metadata()
        keys = list(f.keys())
    assert md["format"] == "pt" and json.loads(md["lora_config"]) == {"r": 64, "lora_alpha": 64, "init_lora_weights": True, "target_modules": DEFAULT_TARGET_MODULES}
    assert all(k.startswith("transformer.transformer_blocks.0.attn") and ".default." not in k for k in keys) and len(keys) == 16
    assert os.path.exists(os.path.join(out_dir, "scheduler", "scheduler_config.json"))
    sd2, cfg2 = wire.load_lora_weights(out_dir)
    assert cfg2["r"] == 64
    fresh = MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=1), device=torch.device("cpu"))
    fresh.add_adapter(r=cfg2["r"], lora_alpha=cfg2["lora_alpha"], target_modules=cfg2["target_modules"])
    fresh.load_state_dict(sd2, strict=False)
    assert torch.equal(fresh.lora_A, model.lora_A) and torch.equal(fresh.lora_B, model.lora_B)
    with pytest.raises(ValueError):
        fresh.load_state_dict(sd2, assign=True)

    # --- base weights: load_diffusion_models() with NO arguments must load from disk or raise, never random-init
    with pytest.raises(FileNotFoundError, match="never trains on random weights"):
        spec.load_diffusion_models(device=torch.device("cpu"))
    tdir = tmp_path / "snapshot" / "transformer"
    tdir.mkdir(parents=True)
    base = {k: torch.randn(v.shape).to(torch.bfloat16) for k, v in MI355XLTXVideoTransformer3DModel(
        LTXTransformerConfig(num_layers=1), device=torch.device("cpu")).state_dict().items() if v.numel() < 1_000_000}
    names = sorted(base)
    shards = {"diffusion_pytorch_model-00001-of-00002.safetensors": names[: len(names) // 2], "diffusion_pytorch_model-00002-of-00002.safetensors": names[len(names) // 2:]}
    for fn, ks in shards.items():
        save_file({k: base[k] for k in ks}, str(tdir / fn))
    with open(tdir / "diffusion_pytorch_model.safetensors.index.json", "w") as f:
        json.dump({"metadata": {}, "weight_map": {k: fn for fn, ks in shards.items() for k in ks}}, f)
    with open(tdir / "config.json", "w") as f:
        json.dump({"_class_name": "LTXVideoTransformer3DModel", "num_layers": 1, "num_attention_heads": 32, "attention_head_dim": 64}, f)
    assert wire.resolve_transformer_dir(str(tmp_path / "snapshot")) == str(tdir)
    got = wire.load_transformer_state_dict(str(tdir))
    assert set(got) == set(base) and all(torch.equal(got[k], base[k]) for k in base)
    assert wire.load_transformer_config(str(tdir))["num_layers"] == 1

    # --- precomputed samples + feeder (rank 1 of 2, batch 2, two resolutions interleaved)
    pdir = str(tmp_path / "out" / wire.PRECOMPUTED_DATA_DIR)
    for i in range(8):
        hw = 4 if i % 2 == 0 else 6
        wire.save_precomputed_item({"latents": torch.full((1, 128, 2, hw, hw), float(i)), "num_frames": 2, "height": hw, "width": hw,
                                    "latents_mean": torch.zeros(128), "latents_std": torch.ones(128)}, i, pdir, "latent")
        wire.save_precomputed_item({"encoder_hidden_states": torch.full((1, 128, 8), float(i)), "encoder_attention_mask": torch.ones(1, 128)}, i, pdir, "condition")
    assert wire.load_precomputed_item(3, pdir, "latent")["latents"][0, 0, 0, 0, 0] == 3
    feeder = wire.PrecomputedSampleFeeder(str(tmp_path / "out"), rank=1, world_size=2, batch_size=2, collate_conditions=spec.collate_conditions,
                                          collate_latents=spec.collate_latents, resolution_dim_keys=spec._resolution_dim_keys)
    try:
        assert len(feeder) == 4
        seen = []
        for _ in range(4):
            cb, lb = next(feeder)
            assert lb["latents"].shape[0] == 2 and cb["encoder_hidden_states"].shape[0] == 2 and lb["latents_mean"].shape == (128,)
            ids = lb["latents"][:, 0, 0, 0, 0].tolist()
            assert cb["encoder_hidden_states"][:, 0, 0].tolist() == ids      # latents stay paired with their conditions
            assert len({int(i) % 2 for i in ids}) == 1                        # one resolution per batch
            seen += ids
        assert set(seen) == {4.0, 5.0, 6.0, 7.0}                              # rank 1 owns indices [4, 8) and cycles through them
    finally:
        feeder.close()


def test_dp_gradient_average_equals_large_batch_gradient():
    """The DP contract of the step: averaging per-rank LoRA gradients (each the mean over its own samples) equals the gradient
    of the global-batch loss -- checked on the oracle (tiny config), world 2 emulated in-process."""
    from oracle import ltx

    cfg = ltx.LTXConfig.dummy()
    m = ltx.build_model(cfg, seed=0, rank=4, alpha=4.0, dtype=torch.float32, lora_b_std=0.02)
    inp = ltx.synth_inputs(cfg, 2, 2, 4, 4, dtype=torch.float32)
    loss, _, _ = ltx.forward_loss(m, inp)
    loss.backward()
    full = {n: p.grad.clone() for n, p in ltx.lora_parameters(m)}
    per_rank = []
    for r in range(2):
        m.zero_grad()
        sub = ltx.StepInputs(inp.latents[r:r + 1], inp.latents_mean, inp.latents_std, inp.encoder_hidden_states[r:r + 1],
                             inp.encoder_attention_mask[r:r + 1], inp.sigmas[r:r + 1], inp.noise[r:r + 1])
        l, _, _ = ltx.forward_loss(m, sub)
        l.backward()
        per_rank.append({n: p.grad.clone() for n, p in ltx.lora_parameters(m)})
    for n in full:
        torch.testing.assert_close((per_rank[0][n] + per_rank[1][n]) / 2, full[n], rtol=1e-4, atol=1e-7)


def test_bench_and_entry_points_exist():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"metric"', '"roofline"', '"cpu_baseline"', '"ms_per_step"', '"vs_baseline"', "--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert key in src
    import __graft_entry__ as ge

    assert callable(ge.build) and callable(ge.smoke)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")  # no device visible, on a GPU machine too
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], capture_output=True, text=True, env=env)
    assert out.returncode != 0 and "MI355X" in (out.stderr + out.stdout)  # refuses to run without the GPU


def test_loss_weighting_and_density_schemes_match_oracle():
    """Host mirrors of utils/diffusion.py (density sampling for every --flow_weighting_scheme, SD3 loss weights) against the
    oracle's restatement, same generator state: bit-identical."""
    from finetrainers_amd.utils import diffusion as host
    from oracle import ltx

    sig = torch.tensor([0.05, 0.25, 0.5, 0.7, 0.999])
    for scheme in ("none", "sigma_sqrt", "cosmap", "logit_normal", "mode"):
        assert torch.equal(host.compute_loss_weighting_for_sd3(scheme, sig), ltx.compute_loss_weighting_for_sd3(scheme, sig)), scheme
    for scheme in ("none", "logit_normal", "mode"):
        g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
        a = host.compute_density_for_timestep_sampling(scheme, 16, logit_mean=0.0, logit_std=1.0, mode_scale=1.29, device=torch.device("cpu"), generator=g1)
        b = ltx.compute_density_for_timestep_sampling(scheme, 16, logit_mean=0.0, logit_std=1.0, mode_scale=1.29, generator=g2)
        assert torch.equal(a, b), scheme
        assert (a >= 0).all() and (a <= 1).all()


def test_cogvideox_host_tables_match_oracle():
    """CogVideoX host-side constants (no kernels): the 3-D sincos position table, the timestep embedding, the DDIM alphas and the sigma table."""
    from finetrainers_amd.cogvideox import CogVideoXDDIMTables, CogVideoXTransformerConfig
    from finetrainers_amd.cogvideox.model import sincos_position_table, timestep_embedding
    from oracle import cogvideox as cvx
    from oracle import ltx

    ocfg, cfg = cvx.CogVideoXConfig(), CogVideoXTransformerConfig()
    for (h, w, f) in ((60, 90, 13), (10, 14, 3)):
        ref = cvx.get_3d_sincos_pos_embed(ocfg.inner_dim, (w // 2, h // 2), f, ocfg.spatial_interpolation_scale, ocfg.temporal_interpolation_scale).flatten(0, 1)
        assert torch.equal(sincos_position_table(cfg, h, w, f), ref)
    t = torch.tensor([0, 31, 874, 999])
    assert torch.equal(timestep_embedding(t, 1920), ltx.get_timestep_embedding(t, 1920))
    tab, osch = CogVideoXDDIMTables(), cvx.CogVideoXDDIMScheduler()
    assert torch.equal(tab.alphas_cumprod, osch.alphas_cumprod)
    ts = torch.tensor([3, 500, 998])
    assert torch.equal(tab.loss_weights(ts), 1 / (1 - osch.alphas_cumprod[ts]))
    assert dict(cfg.__dict__, use_rotary_positional_embeddings=False, patch_size_t=None, ofs_embed_dim=None) == ocfg.__dict__  # the 2b defaults agree


def test_wan_host_tables_layouts_and_spec_ops_match_oracle():
    """Wan host-side pieces (no kernels): the rotary tables against the oracle's complex table, the flat parameter layouts (diffusers names, fused q|k|v
    and cross k|v views contiguous, 16-byte aligned slices, the 1.3B parameter count), the config loader, and the spec-level torch arithmetic
    (moment normalisation, flow-match mix, target) on the CPU against oracle/wan.py -- the posterior draw is the library's and is tested on the GPU."""
    from finetrainers_amd.wan.block import WanBlockLayout
    from finetrainers_amd.wan.model import RootLayout, WanTransformerConfig, rotary_tables
    from finetrainers_amd.wan.specification import MI355XWanSpecOps
    from oracle import wan

    cfg, ocfg = WanTransformerConfig(), wan.WanConfig()
    for (f, h, w) in ((21, 64, 64), (3, 8, 12)):
        cos, sin = rotary_tables(cfg, f, h, w)
        freqs = wan.WanRotaryPosEmbed(ocfg)(torch.zeros(1, 16, f, h, w))[0, 0]  # complex128 [S, 64]
        assert cos.shape == (f * (h // 2) * (w // 2), 64) and torch.equal(cos, freqs.real.float()) and torch.equal(sin, freqs.imag.float())
    lay = WanBlockLayout(cfg.inner_dim, cfg.ffn_dim)
    oblk = wan.WanTransformerBlock(ocfg)
    names = {n.replace("ffn.proj_in.", "ffn.net.0.proj.").replace("ffn.proj_out.", "ffn.net.2."): tuple(p.shape) for n, p in oblk.named_parameters()}
    assert {n: s for n, s in lay.entries} == names and lay.total == sum(p.numel() for p in oblk.parameters())
    assert all(off % 8 == 0 for off, _ in lay.offsets.values())
    flat = torch.arange(lay.total, dtype=torch.float32)
    D = cfg.inner_dim
    qkv = lay.view(flat, "w_qkv1")
    assert qkv.shape == (3 * D, D) and torch.equal(qkv[D:2 * D], lay.view(flat, "attn1.to_k.weight")) and torch.equal(qkv[2 * D:], lay.view(flat, "attn1.to_v.weight"))
    kv = lay.view(flat, "w_kv2")
    assert torch.equal(kv[:D], lay.view(flat, "attn2.to_k.weight")) and torch.equal(lay.view(flat, "b_kv2")[D:], lay.view(flat, "attn2.to_v.bias"))
    root = RootLayout(cfg)
    omodel_names = {k: tuple(v.shape) for k, v in wan.WanTransformer3DModel(wan.WanConfig(num_layers=0)).state_dict().items()}
    omodel_names["patch_embedding.weight"] = (D, 64)  # the Conv3d weight in its GEMM shape
    assert {n: s for n, s in root.entries} == omodel_names
    assert 30 * lay.total + sum(math.prod(s) for _, s in root.entries) == 1_418_996_800  # Wan2.1-T2V-1.3B
    assert WanTransformerConfig.from_dict({"patch_size": [1, 2, 2], "num_layers": 2, "_class_name": "WanTransformer3DModel"}).num_layers == 2

    # spec ops around the posterior draw
    g = torch.Generator().manual_seed(0)
    mom = torch.randn(2, 32, 3, 8, 12, generator=g).bfloat16()
    mean, std = 0.1 * torch.randn(16, generator=g), 1 + 0.2 * torch.rand(16, generator=g)
    spec = MI355XWanSpecOps()
    assert spec._resolution_dim_keys == {"latents": (2, 3, 4)}
    assert torch.equal(spec.normalize_latents(mom[:, :16], mean, std), wan.normalize_latents(mom[:, :16], mean, std))


def test_hunyuan_host_tables_and_key_maps_match_oracle():
    """HunyuanVideo host-side pieces (no kernels): the 3-axis rotary table bit-identical to the oracle's, and the frozen-front / block parameter names and
    shapes equal to the oracle model's (translated to the diffusers names) -- what ``load_diffusers_state_dict`` will ask a checkpoint for."""
    from finetrainers_amd.hunyuan_video.block import MI355XHunyuanDualBlock, MI355XHunyuanSingleBlock
    from finetrainers_amd.hunyuan_video.model import HunyuanVideoTransformerConfig, _front_keys, rotary_tables
    from oracle import hunyuan as hy

    cfg, ocfg = HunyuanVideoTransformerConfig(), hy.HunyuanVideoConfig()
    for (f, h, w) in ((16, 68, 120), (3, 8, 12)):
        a, b = rotary_tables(cfg, f, h, w), hy.rotary_tables(ocfg, f, h, w)
        assert a[0].shape == (f * (h // 2) * (w // 2), 128) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    def to_diffusers(k):
        k = k.replace("context_embedder.refiner_blocks.", "context_embedder.token_refiner.refiner_blocks.").replace(".norm_out_linear.", ".norm_out.linear.")
        if k.startswith("norm_out_linear."):
            k = "norm_out.linear." + k[len("norm_out_linear."):]
        if k.startswith("x_embedder."):
            k = "x_embedder.proj." + k[len("x_embedder."):]
        for a_ in ("ff_context", "ff"):
            k = k.replace(f"{a_}.proj_in.", f"{a_}.net.0.proj.").replace(f"{a_}.proj_out.", f"{a_}.net.2.")
        return k

    kw = dict(num_attention_heads=2, attention_head_dim=128, num_layers=1, num_single_layers=1, num_refiner_layers=2, text_embed_dim=64, pooled_projection_dim=64)
    sd = {to_diffusers(k): tuple(v.shape) for k, v in hy.HunyuanVideoTransformer3DModel(hy.HunyuanVideoConfig(**kw)).state_dict().items()}
    front = {k: v for k, v in sd.items() if not k.startswith(("transformer_blocks", "single_transformer_blocks"))}
    front["x_embedder.proj.weight"] = (256, 64)  # the Conv3d weight in its GEMM shape
    assert front == dict(_front_keys(HunyuanVideoTransformerConfig(**kw)))
    dev = torch.device("cpu")
    for prefix, blk in (("transformer_blocks.0.", MI355XHunyuanDualBlock(256, 2, device=dev)), ("single_transformer_blocks.0.", MI355XHunyuanSingleBlock(256, 2, device=dev))):
        want = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        assert want == {k: tuple(getattr(blk, n).shape) for k, n in blk._KEYS.items()}


def test_wan_and_hunyuan_specification_collation_and_guards():
    """Spec mirrors, host-only parts: ``latents_mean`` / ``latents_std`` pass through the Wan collation uncollated (modeling_utils.py:22), tensors are
    concatenated on dim 0, non-bf16 transformer dtypes are refused, encoders / VAE / validation stay with the reference."""
    from finetrainers_amd.hunyuan_video.specification import MI355XHunyuanVideoModelSpecification
    from finetrainers_amd.wan.specification import IGNORE_KEYS_FOR_COLLATION, MI355XWanModelSpecification

    wspec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
    items = [{"latents": torch.zeros(1, 32, 2, 4, 4), "latents_mean": torch.arange(16.0), "latents_std": torch.ones(16)} for _ in range(3)]
    out = wspec.collate_latents(items)
    assert out["latents"].shape == (3, 32, 2, 4, 4) and out["latents_mean"].shape == (16,) and {"latents_mean", "latents_std"} <= IGNORE_KEYS_FOR_COLLATION
    hspec = MI355XHunyuanVideoModelSpecification(pretrained_model_name_or_path=None)
    cond = hspec.collate_conditions([{"encoder_hidden_states": torch.zeros(1, 5, 8), "encoder_attention_mask": torch.ones(1, 5, dtype=torch.long), "pooled_projections": torch.zeros(1, 4)}] * 2)
    assert cond["encoder_hidden_states"].shape == (2, 5, 8) and cond["encoder_attention_mask"].shape == (2, 5) and hspec.scaling_factor == 0.476986
    for cls in (MI355XWanModelSpecification, MI355XHunyuanVideoModelSpecification):
        with pytest.raises(ValueError):
            cls(transformer_dtype=torch.float16)
        spec = cls(pretrained_model_name_or_path=None)
        for fn in (spec.load_condition_models, spec.load_latent_models, spec.validation):
            with pytest.raises(NotImplementedError):
                fn()
        with pytest.raises(FileNotFoundError):
            spec.load_diffusion_models()  # nothing to load from: never random weights


def test_hunyuan_step_rehomes_adapters_into_one_flat_buffer_and_saves_peft_keys(tmp_path):
    """Host-only parts of the HunyuanVideo step: the 200 (here 7) adapters' Parameters become views of ONE flat fp32 buffer (what the fused clip + AdamW
    launch updates), and ``lora_state_dict`` carries the peft names the reference's ``_save_lora_weights`` writes."""
    from finetrainers_amd import wire
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoSFTStep, MI355XHunyuanVideoTransformer3DModel

    cfg = HunyuanVideoTransformerConfig(num_attention_heads=2, num_layers=1, num_single_layers=1, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
    model = MI355XHunyuanVideoTransformer3DModel(cfg, device=torch.device("cpu"))
    model.add_adapter(r=64, lora_alpha=32.0)
    with torch.no_grad():
        model.single_transformer_blocks[0].lora_B.normal_()
    before = model.single_transformer_blocks[0].lora_B.detach().clone()
    step = MI355XHunyuanVideoSFTStep(model)
    n = sum(p.numel() for p in model.lora_parameters())
    assert step.flat.numel() == n == (4 + 3) * 2 * 64 * 256
    lo, hi = step.flat.data_ptr(), step.flat.data_ptr() + 4 * n
    assert all(lo <= p.data_ptr() < hi for p in model.lora_parameters()) and torch.equal(model.single_transformer_blocks[0].lora_B, before)
    step.flat.zero_()
    assert float(model.transformer_blocks[0].lora_A.detach().abs().max()) == 0.0 and model.transformer_blocks[0].lora_scale == 0.5
    sd = model.lora_state_dict()
    assert len(sd) == 14 and "transformer_blocks.0.attn.to_out.0.lora_B.weight" in sd and "single_transformer_blocks.0.attn.to_v.lora_A.weight" in sd
    wire.save_lora_weights(str(tmp_path), sd, wire.lora_config_metadata(64, 32.0, ["to_q", "to_k", "to_v", "to_out.0"]))
    tensors, _ = wire.load_lora_weights(str(tmp_path))
    assert len(tensors) == 14


def test_training_state_checkpoint_is_the_reference_dcp_layout(tmp_path):
    """wire.training_state_dict / save_training_state produce the dictionary PTDCheckpointer hands to torch.distributed.checkpoint
    (finetrainers/parallel/ptd.py:296-352): model.<fqn>, optimizer.state.<fqn>.{step, exp_avg, exp_avg_sq}, optimizer.param_groups.<fqn>.*,
    lr_scheduler.*, train_state.*.  Checked both ways against torch's own Stateful plumbing on a small peft-shaped module: (1) key for key and
    value for value against get_model_state_dict / get_optimizer_state_dict(flatten) / LambdaLR.state_dict() of a torch AdamW run;
    (2) a checkpoint written from the flat, rank-padded buffers loads into a FRESH torch model + optimizer through the reference's wrappers."""
    import functools
    import io

    import torch.distributed.checkpoint as dcp
    import torch.nn as nn
    from torch.distributed.checkpoint.state_dict import StateDictOptions, get_model_state_dict, get_optimizer_state_dict, set_model_state_dict, set_optimizer_state_dict
    from torch.distributed.checkpoint.stateful import Stateful

    from finetrainers_amd import wire

    D, r, r_pad = 8, 2, 4

    class LoraLinear(nn.Module):  # peft's module tree: base_layer + lora_A / lora_B ModuleDicts keyed by the adapter name
        def __init__(self):
            super().__init__()
            self.base_layer = nn.Linear(D, D)
            self.lora_A = nn.ModuleDict({"default": nn.Linear(D, r, bias=False)})
            self.lora_B = nn.ModuleDict({"default": nn.Linear(r, D, bias=False)})

        def forward(self, x):
            return self.base_layer(x) + self.lora_B["default"](self.lora_A["default"](x))

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.to_q, self.to_k, self.norm = LoraLinear(), LoraLinear(), nn.LayerNorm(D)

        def forward(self, x):
            return self.norm(self.to_q(x) + self.to_k(x))

    def make(seed):
        torch.manual_seed(seed)
        m = Tiny()
        for n, p in m.named_parameters():
            p.requires_grad_("lora_" in n)
        # as the reference does (finetrainers/optimizer.py:36-38): the optimizer is built over ALL parameters, the frozen ones included
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-4, fused=False)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
        return m, opt, sch

    m, opt, sch = make(0)
    for _ in range(2):
        m(torch.randn(3, D)).pow(2).sum().backward()
        opt.step(); sch.step(); opt.zero_grad()

    # ---- the same state as the MI355X step holds it: stacked rank-padded storage [L = 1, 2 adapters, r_pad, D] / [1, 2, D, r_pad] ----
    paths = ["to_q", "to_k"]
    mods = [m.to_q, m.to_k]

    def stack(get):
        a = torch.zeros(1, 2, r_pad, D)
        b = torch.zeros(1, 2, D, r_pad)
        for i, mod in enumerate(mods):
            a[0, i, :r] = get(mod.lora_A["default"].weight)
            b[0, i, :, :r] = get(mod.lora_B["default"].weight)
        return a, b

    ea, eb = stack(lambda p: opt.state[p]["exp_avg"])
    qa, qb = stack(lambda p: opt.state[p]["exp_avg_sq"])
    ours = wire.training_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, paths, r, ea, eb, qa, qb, step_count=2,
                                    hyper={"lr": sch.get_last_lr()[0], "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 1e-4, "initial_lr": 1e-3},
                                    lr_scheduler_state=wire.lambda_lr_state(1e-3, sch.last_epoch, sch.get_last_lr()[0]),
                                    train_state={"step": 2, "observed_data_samples": 6, "global_avg_losses": [0.5, 0.25], "global_max_losses": [0.75, 0.5], "log_steps": [1, 2]})

    # (1) key for key, value for value
    ref_model = get_model_state_dict(m)
    ref_opt = get_optimizer_state_dict(m, opt, options=StateDictOptions(flatten_optimizer_state_dict=True))
    assert set(ours["model"]) == set(ref_model) and all(torch.equal(ours["model"][k], ref_model[k]) for k in ref_model)
    assert set(ours["optimizer"]) == set(ref_opt), sorted(set(ours["optimizer"]) ^ set(ref_opt))[:6]
    for k, v in ref_opt.items():
        if torch.is_tensor(v):
            assert torch.equal(ours["optimizer"][k], v), k
        else:
            assert ours["optimizer"][k] == v, (k, ours["optimizer"][k], v)
    assert ours["lr_scheduler"] == sch.state_dict()
    assert int(ours["train_state"]["step"]) == 2 and ours["train_state"]["step"].dtype == torch.int32
    ours["train_state"]["global_avg_losses"].seek(0)
    assert torch.load(ours["train_state"]["global_avg_losses"]) == [0.5, 0.25]

    # (2) written by this side, read by the reference's side (its wrappers, restated from parallel/ptd.py:280-294 and optimizer.py:48-62)
    ckpt = str(tmp_path / f"{wire.DCP_PREFIX}_2")
    dcp.save(ours, checkpoint_id=ckpt)

    class ModelWrapper(Stateful):
        def __init__(self, model):
            self.model = model

        def state_dict(self):
            return get_model_state_dict(self.model)

        def load_state_dict(self, sd):
            set_model_state_dict(self.model, model_state_dict=sd, options=StateDictOptions(strict=False))

    class OptimizerWrapper(Stateful):
        def __init__(self, model, optim):
            self.model, self.optim = model, optim

        def state_dict(self):
            return get_optimizer_state_dict(self.model, self.optim, options=StateDictOptions(flatten_optimizer_state_dict=True))

        def load_state_dict(self, sd):
            set_optimizer_state_dict(self.model, self.optim, optim_state_dict=sd, options=StateDictOptions(flatten_optimizer_state_dict=True))

    m2, opt2, sch2 = make(1)  # different weights, empty optimizer
    m2(torch.randn(3, D)).sum().backward()
    opt2.step(); opt2.zero_grad()  # the reference loads after the optimizer exists; its state gets overwritten
    class DataLoaderState(Stateful):  # DPDataLoader's Stateful face (finetrainers/data/dataloader.py:27-40)
        loaded = None

        def state_dict(self):
            return {"dp_rank_0": b""}

        def load_state_dict(self, sd):
            import pickle
            self.loaded = pickle.loads(sd["dp_rank_0"])

    dl = DataLoaderState()
    states = {"model": ModelWrapper(m2), "optimizer": OptimizerWrapper(m2, opt2), "lr_scheduler": sch2, "dataloader": dl}
    dcp.load(states, checkpoint_id=ckpt)  # strict planner: every key the reference asks for is in the checkpoint
    assert dl.loaded == {}
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2), n1
    for p1, p2 in zip([p for p in m.parameters() if p.requires_grad], [p for p in m2.parameters() if p.requires_grad]):
        assert torch.equal(opt.state[p1]["exp_avg"], opt2.state[p2]["exp_avg"]) and torch.equal(opt.state[p1]["exp_avg_sq"], opt2.state[p2]["exp_avg_sq"])
        assert float(opt2.state[p2]["step"]) == 2.0
    assert sch2.last_epoch == sch.last_epoch and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]


@pytest.mark.parametrize("ntiles,nk,ov", [(168, 32, 7), (168, 32, 4), (168, 128, 7), (168, 96, 13), (504, 32, 7), (672, 32, 4), (84, 32, 7), (255, 32, 4), (257, 4, 4),
                                           (300, 3, 1), (512, 32, 4), (513, 32, 4), (100, 64, 4)])
def test_stream_k_plan_invariants(ntiles, nk, ov):
    """ftmi_gemm_sk_plan (host-only, pure): the split of the persistent GEMM's tail tiles over 256 workgroups.  Every (tile, K iteration) of the
    stream-K tiles is computed exactly once; every tile is finished (extension + epilogue) by exactly one workgroup -- the one holding its
    iteration 0 --; an owner's contributor mask names exactly the workgroups that open with a partial of its tile; no piece is shorter than
    min_piece; the shares are balanced (the largest costs at most ~ half a forbidden zone more than the mean)."""
    import ctypes

    from finetrainers_amd import _lib

    lib = _lib.load()
    G, minp, pc, ac = 256, min(4, max(1, nk // 2)), 1, 2
    buf = (ctypes.c_int * (G * 8))()
    if not hasattr(lib, "ftmi_gemm_sk_plan"):
        pytest.skip("the stream-K planner lives in FTMI_EXPERIMENTAL builds of the library")
    assert lib.ftmi_gemm_sk_plan(ntiles, G, nk, ov, minp, pc, ac, buf) == 0
    W = [list(buf[i * 8:i * 8 + 8]) for i in range(G)]
    sk = ntiles % G
    cover, finished, cost = {}, {}, [0] * G
    for v, (t0, k0, t1, k1, kinds, nf, mask, _) in enumerate(W):
        part, own = kinds & 1, (kinds >> 1) & 1
        segs = []
        if part:
            kb = k1 if t1 == t0 else nk
            assert kb - k0 >= minp
            segs.append((t0, k0, kb))
            cost[v] += pc
        for i in range(nf):
            segs.append((t0 + part + i, 0, nk))
            finished[t0 + part + i] = finished.get(t0 + part + i, 0) + 1
            cost[v] += ov
        if own:
            assert k1 >= minp
            segs.append((t1, 0, k1))
            finished[t1] = finished.get(t1, 0) + 1
            want = [u for u in range(v + 1, G) if W[u][0] == t1 and (W[u][4] & 1)]
            assert want == [v + 1 + i for i in range(31) if (mask >> i) & 1]
            cost[v] += ov + ac * len(want)
        else:
            assert mask == 0
        for t, a, b in segs:
            for k in range(a, b):
                assert (t, k) not in cover
                cover[(t, k)] = v
            cost[v] += b - a
    assert len(cover) == sk * nk and all(finished.get(t, 0) == 1 for t in range(sk))
    if sk * (nk + ov) >= G * 2 * (ov + 2 * minp):  # enough work for every workgroup: balanced within a forbidden zone
        mean = sum(cost) / G
        assert max(cost) <= mean + (ov + 2 * minp) + pc + ac, (max(cost), mean)


def test_cogvideox_15_host_tables_and_patch_layout():
    """CogVideoX 1.5 host logic against the oracle restatement: the integer-position rotary tables (finetrainers/models/cogvideox/utils.py:38-51, the
    ``patch_size_t`` branch -> [upstream] get_3d_rotary_pos_embed(grid_type="slice")) bit for bit, and the (channel, frame, row, column) patch layout of the
    Linear patch embedding / proj_out, forth and back."""
    from finetrainers_amd.cogvideox.model import CogVideoXTransformerConfig, patches_3d, rotary_tables, unpatches_3d
    from oracle import cogvideox as cvx

    cfg = CogVideoXTransformerConfig(num_attention_heads=2, num_layers=1, sample_width=12, sample_height=8, patch_size_t=2, use_rotary_positional_embeddings=True)
    for frames, h, w in ((4, 8, 12), (3, 6, 10)):
        cos, sin = rotary_tables(cfg, h, w, frames)
        co, so = cvx.prepare_rotary_positional_embeddings(h * 8, w * 8, frames, 8, 2, 2, 64, cfg.sample_height * 8, cfg.sample_width * 8)
        assert torch.equal(cos, co) and torch.equal(sin, so)
    x = torch.randn(2, 4, 16, 8, 12)
    t = patches_3d(x, 2, 2)
    ref = x.permute(0, 1, 3, 4, 2).reshape(2, 2, 2, 4, 2, 6, 2, 16).permute(0, 1, 3, 5, 7, 2, 4, 6).flatten(4, 7).flatten(1, 3)  # [upstream] CogVideoXPatchEmbed
    assert torch.equal(t, ref)
    assert torch.equal(unpatches_3d(t, 4, 16, 8, 12, 2, 2), x)
    back = t.reshape(2, 2, 4, 6, -1, 2, 2, 2).permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5).flatten(1, 2)  # [upstream] the model's final reshape
    assert torch.equal(back, x)


def test_block_orchestrator_planners_agree_with_the_python_layouts():
    """Host-only entry points of the per-block C orchestrators (no kernel is launched): the Wan block's flat parameter layout has the same length in C
    (csrc/wan_dit.hip Offsets) as in Python (WanBlockLayout) for several geometries, and the saved / scratch planners of the three block kinds return sizes
    that cover at least the tensors the Python compositions keep."""
    import ctypes

    from finetrainers_amd import _lib
    from finetrainers_amd.wan.block import WanBlockLayout

    lib = _lib.load()
    for D, H, F in ((256, 2, 512), (1536, 12, 8960), (5120, 40, 13824)):
        if D > 4096:  # the row-wise kernels' width limit: the planner still answers, the forward would refuse
            continue
        cfg = _lib.WanBlockConfig(B=1, S=256, T=64, D=D, H=H, F=F, eps=1e-6, gemm_variant=8)
        assert lib.ftmi_wan_block_param_elements(ctypes.byref(cfg)) == WanBlockLayout(D, F).total
        M, Mt = 256, 64
        kept = 2 * (M * D * 13 + M * 3 * D + Mt * 3 * D + 2 * M * F) + 2 * 4 * H * M  # n1 qkv qn kn o1 a1 x1 n2 q2 q2n o2 x2 n3 f | kv2 k2n | act pre | lse
        saved = lib.ftmi_wan_block_saved_bytes(ctypes.byref(cfg))
        assert kept <= saved <= kept + 64 * 256, (D, kept, saved)
        assert lib.ftmi_wan_block_scratch_bytes(ctypes.byref(cfg)) >= 2 * (7 * D * D + 2 * D * F)  # the seven transposed weights alone
    hs = _lib.HySingleConfig(B=1, T=256, S=1024, D=3072, H=24, mlp=12288, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    M = 1280
    kept = 2 * M * 3072 * 7 + 2 * M * 12288 + 3 * 2 * M * 192 + 4 * 24 * M  # n q k v qn kn o | pre | xa x 3 | lse
    saved = lib.ftmi_hy_single_saved_bytes(ctypes.byref(hs))
    assert kept <= saved <= kept + 64 * 256 + 6 * 2 * 3072
    assert lib.ftmi_hy_single_scratch_bytes(ctypes.byref(hs)) >= 2 * M * (3072 + 12288)  # the [attention | MLP] feature buffer
    hd = _lib.HyDualConfig(T=256, S=1024, D=3072, H=24, mlp=12288, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    assert lib.ftmi_hy_dual_saved_bytes(ctypes.byref(hd)) > 2 * (1024 * 3072 * 4 + 1280 * 3072 * 4 + 1280 * 12288)
    bad = _lib.HySingleConfig(B=1, T=8, S=64, D=3072, H=23, mlp=12288, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)  # heads x 128 != width
    assert lib.ftmi_hy_single_saved_bytes(ctypes.byref(bad)) > 0  # planners do not validate; the forward does (FTMI_ERR_UNSUPPORTED)


def test_spec_classes_subclass_the_reference_when_it_is_importable():
    """B1 as a drop-in: the MI355X specification classes are the MI355X overrides ON TOP of the reference's own specification class when one is
    importable.  The reference package cannot be imported here (no diffusers), so a stand-in with the reference's surface is injected as the base: a
    ModelSpecification that takes the reference constructor's keyword arguments and carries the methods SFTTrainer calls, and an LTX-Video subclass
    whose constructor installs the default processors (one for the conditions, one for the latents) and which defines its own loaders / forward."""
    from finetrainers_amd.ltx_video import specification as ltx_spec
    from finetrainers_amd.utils.reference_base import REFERENCE_CTOR_KEYS, StandaloneModelSpecification, as_drop_in

    inherited = ("prepare_conditions", "prepare_latents", "load_condition_models", "load_latent_models", "load_pipeline", "validation", "collate_conditions",
                 "collate_latents", "_trainer_init")
    own = ("load_diffusion_models", "forward", "_save_lora_weights")

    def method(name):
        def f(self, *args, **kwargs):
            return name
        f.__name__ = name
        return f

    def base_init(self, **kwargs):
        unknown = set(kwargs) - set(REFERENCE_CTOR_KEYS)
        assert not unknown, unknown  # as_drop_in hands the base the reference's own keyword arguments only
        for k in REFERENCE_CTOR_KEYS:
            setattr(self, k, kwargs.get(k))
        self.condition_model_processors = kwargs.get("condition_model_processors") or []
        self.latent_model_processors = kwargs.get("latent_model_processors") or []

    def ltx_init(self, pretrained_model_name_or_path="Lightricks/LTX-Video", condition_model_processors=None, latent_model_processors=None, **kwargs):
        condition_model_processors = condition_model_processors or [("text", ["encoder_hidden_states", "encoder_attention_mask"])]
        latent_model_processors = latent_model_processors or [("latents", ["latents", "num_frames", "height", "width", "latents_mean", "latents_std"])]
        base_init(self, pretrained_model_name_or_path=pretrained_model_name_or_path, condition_model_processors=condition_model_processors,
                  latent_model_processors=latent_model_processors, **kwargs)

    ns = {"ModelSpecification": type("ModelSpecification", (), {"__init__": base_init, **{n: method(n) for n in inherited + own}})}
    Ref = type("LTXVideoModelSpecification", (ns["ModelSpecification"],), {"__init__": ltx_init, **{n: method(n) for n in own}})

    overrides = ltx_spec.MI355XLTXVideoModelSpecification.MI355X_OVERRIDES
    Spec = as_drop_in(overrides, "finetrainers.models.ltx_video", "LTXVideoModelSpecification", base_override=Ref)
    spec = Spec(pretrained_model_name_or_path="somewhere/LTX-Video", transformer_dtype=torch.bfloat16)
    assert isinstance(spec, Ref) and isinstance(spec, ns["ModelSpecification"]) and Spec.IS_REFERENCE_SUBCLASS
    # inherited from the reference, untouched: what SFTTrainer calls outside the denoiser path (trainer.py:380-383, 834-835, 877, 896)
    for name in ("prepare_conditions", "prepare_latents", "load_condition_models", "load_latent_models", "load_pipeline", "validation", "collate_conditions",
                 "collate_latents", "_trainer_init"):
        assert getattr(Spec, name) is getattr(Ref, name) or getattr(Spec, name) is getattr(ns["ModelSpecification"], name), name
    # overridden by the MI355X backend
    for name in ("load_diffusion_models", "forward", "_save_lora_weights"):
        assert getattr(Spec, name) is getattr(overrides, name) and getattr(Spec, name) is not getattr(Ref, name), name
    # the reference constructor ran: its default processors are in place (one each), ours did not wipe them
    assert len(spec.condition_model_processors) == 1 and len(spec.latent_model_processors) == 1 and spec._resolution_dim_keys == {"latents": (2, 3, 4)}
    assert spec.pretrained_model_name_or_path == "somewhere/LTX-Video" and spec.first_frame_conditioning_p == 0.1

    # without the reference: the same overrides on the generic half of ModelSpecification; the model-specific loaders raise the base's error
    assert not ltx_spec.MI355XLTXVideoModelSpecification.IS_REFERENCE_SUBCLASS and issubclass(ltx_spec.MI355XLTXVideoModelSpecification, StandaloneModelSpecification)
    alone = ltx_spec.MI355XLTXVideoModelSpecification()
    with pytest.raises(NotImplementedError, match="load_condition_models"):
        alone.load_condition_models()
    assert alone.prepare_latents(processors=[lambda **kw: {"latents": kw["image"] * 2}], image=torch.ones(1))["latents"].item() == 2.0  # the generic processor loop
    for mod, cls in (("cogvideox", "MI355XCogVideoXModelSpecification"), ("wan", "MI355XWanModelSpecification"), ("hunyuan_video", "MI355XHunyuanVideoModelSpecification")):
        import importlib
        C = getattr(importlib.import_module(f"finetrainers_amd.{mod}.specification"), cls)
        assert issubclass(C, StandaloneModelSpecification) and hasattr(C, "prepare_conditions") and hasattr(C, "load_pipeline") and hasattr(C, "apply_tensor_parallel")


def test_gemm_dispatch_rule_matches_the_design(lib):
    """The automatic NT-GEMM kernel choice as a pure host function (ftmi_gemm_nt_plan; no device): pinned to what DESIGN.md section 3 / 6 state for the
    LTX step's shapes (M = 2 x 2688 tokens) -- the 16 x 16 x 32 pipeline (80 = 256-row tiles, 86 = 192-row tiles, 87 = 224-row tiles where they save a share of a
    round) on every launch with several rounds of tiles or a long K, 192 x 128 two-per-CU tiles (42) on the single-round N = 2048 / K = 2048 launches, 128 x 128 (44) for few rows or few tiles."""
    M = 2 * 2688
    EPI_STORE, EPI_GELU, EPI_RESID, EPI_DGELU = 0, 1, 2, 3
    plan = lambda *a: lib.ftmi_gemm_nt_plan(*a)
    assert plan(M, 6144, 2048, 192, EPI_STORE) == 80     # fused q|k|v forward with the LoRA K-extension: 21 x 24 tiles of 256 x 256, two rounds
    assert plan(M, 8192, 2048, 0, EPI_GELU) == 87        # ff1 forward (GELU + stash): 24 x 32 tiles of 224 x 256 = exactly three rounds of the 256 CUs (round 6)
    assert plan(M, 8192, 2048, 0, EPI_DGELU) == 87       # ff2 input gradient (GELU')
    assert plan(M, 2048, 8192, 0, EPI_RESID) == 1386     # ff2 forward: K = 8192, 28 x 8 tiles of 192 x 256 in one round -- W on the three-slot direct-to-LDS ring (round 6)
    assert plan(M, 2048, 8192, 0, EPI_STORE) == 1386     # ff1 input gradient
    assert plan(M, 2048, 6144, 192, EPI_STORE) == 1386   # fused q|k|v input gradient
    assert plan(M, 2048, 2048, 192, EPI_RESID) == 1386   # to_out forward: one round, short K -- 192 x 256 tiles since round 6
    assert plan(M, 2048, 2048, 192, EPI_STORE) == 1386   # attn2.to_q forward   (FTMI_NT16_SHORT=0: 42, the 192 x 128 two-per-CU kernel of rounds 1-5)
    assert plan(2688, 2048, 2048, 0, EPI_STORE) == 44    # batch 1: 224 tiles of 192 x 128 would half-fill the machine
    assert plan(256, 4096, 2048, 192, EPI_STORE) == 44   # the text side (few rows)
    assert plan(M, 192, 2048, 0, EPI_STORE) == 2         # narrow plain store over many rows: the LDS-ring skinny kernel, whatever N % 128 is
    assert plan(M, 128, 2048, 0, EPI_STORE) == 2 and plan(M, 256, 2048, 0, EPI_STORE) == 2
    assert plan(256, 192, 2048, 0, EPI_STORE) == 1       # few rows, N % 128 != 0: the 128 x 64 tile kernel
    assert plan(M, 192, 2048, 192, EPI_STORE) == 1       # a K-extension keeps it off the skinny route
    assert plan(M, 2048, 100, 0, EPI_STORE) == 0 and plan(M, 100, 2048, 0, EPI_STORE) == 0
    # Wan-1.3B's widths (1536, 4608, 8960 = 35 x 256) take the same pipeline; CogVideoX-2b's 1920 = 7.5 x 256 keeps the 32 x 32 x 16 kernels
    assert plan(21504, 4608, 1536, 0, EPI_STORE) in (80, 86, 87, 2286, 1386, 1387, 1380) and plan(21504, 8960, 1536, 0, EPI_GELU) in (80, 86, 87, 2286, 1386, 1387, 1380)
    assert plan(17776, 1920, 1920, 0, EPI_STORE) not in (80, 86, 87, 2286, 1386, 1387, 1380) and plan(17776, 7680, 1920, 0, EPI_GELU) in (80, 86, 87, 2286, 1386, 1387, 1380)


def test_gemm_plan_is_the_recorded_one(lib):
    """ftmi_gemm_nt_plan over a grid that reaches every branch of the routing (refusals, skinny, 128 x 64, every automatic tile choice, K-extensions, all four
    epilogues), at the default switches, against tests/golden/gemm_nt_plan_grid.txt: the values the library returned BEFORE gemm_nt() and the plan were put on one
    routing function (recorded from that library, never from the code under test)."""
    import os

    axes, rows = {}, []
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_nt_plan_grid.txt")) as f:
        for line in f:
            if line.startswith("#"):
                name, _, vals = line[1:].partition(":")
                if name.strip() in ("M", "N", "K", "K2"):
                    axes[name.strip()] = [int(v) for v in vals.split()]
            else:
                rows.append([int(v) for v in line.split()])
    assert [len(axes[n]) for n in ("M", "N", "K", "K2")] == [11, 14, 6, 3] and len(rows) == 11 * 14 and all(len(r) == 6 * 3 * 4 for r in rows)
    assert not [k for k in os.environ if k.startswith("FTMI_NT") or k.startswith("FTMI_SK")], "the grid is the plan at the default switches"
    bad = []
    for mi, M in enumerate(axes["M"]):
        for ni, N in enumerate(axes["N"]):
            want = iter(rows[mi * len(axes["N"]) + ni])
            for K in axes["K"]:
                for K2 in axes["K2"]:
                    for epi in range(4):
                        w, got = next(want), lib.ftmi_gemm_nt_plan(M, N, K, K2, epi)
                        if got != w:
                            bad.append(((M, N, K, K2, epi), w, got))
    assert not bad, f"{len(bad)} of 11088 plans moved, first (shape, recorded, now): {bad[:5]}"
    assert {v for r in rows for v in r} >= {0, 1, 2, 42, 44, 80, 87, 1386}  # the grid does reach every default route


def test_parallel_backend_has_the_reference_surface():
    """N2: every method / property of BaseParallelBackend (finetrainers/parallel/base.py:9-115) exists on MI355XParallelBackend with the
    reference's signatures where the trainer passes arguments; degrees the path does not implement are refused at construction.  The lists are those of
    the surveyed reference: BaseParallelBackend's methods / properties, PytorchDTensorParallelBackend.__init__ and PTDCheckpointer.__init__ arguments."""
    import inspect

    from finetrainers_amd.parallel import MI355XCheckpointer, MI355XParallelBackend

    names = ["enable_determinism", "apply_ddp", "apply_fsdp2", "apply_context_parallel", "prepare_model", "prepare_dataset", "prepare_dataloader", "prepare_optimizer",
             "get_mesh", "get_checkpointer", "initialize_trackers", "log", "wait_for_everyone", "main_process_first", "destroy", "world_size", "rank", "local_rank",
             "is_main_process", "is_local_main_process", "device", "pipeline_parallel_enabled", "data_parallel_enabled", "data_replication_enabled",
             "data_sharding_enabled", "context_parallel_enabled", "tensor_parallel_enabled"]
    ref_ctor_args = ["world_size", "pp_degree", "dp_degree", "dp_shards", "cp_degree", "tp_degree", "backend", "timeout", "logging_dir", "output_dir", "gradient_accumulation_steps"]
    ref_ckpt_args = ["dataloader", "model_parts", "optimizers", "schedulers", "states", "checkpointing_steps", "checkpointing_limit", "output_dir", "enable", "_callback_fn", "_prefix"]
    assert len(names) >= 27
    for n in names:
        assert n in MI355XParallelBackend.__dict__ or any(n in k.__dict__ for k in MI355XParallelBackend.__mro__[1:-1]), n
    own = list(inspect.signature(MI355XParallelBackend.__init__).parameters)[1:]
    assert own[:len(ref_ctor_args)] == ref_ctor_args
    assert list(inspect.signature(MI355XCheckpointer.__init__).parameters)[1:1 + len(ref_ckpt_args)] == ref_ckpt_args
    b = MI355XParallelBackend(world_size=1, dp_degree=1, backend="gloo", output_dir="/tmp/x", logging_dir="logs")
    assert (b.world_size, b.rank, b.local_rank, b.is_main_process, b.is_local_main_process) == (1, 0, 0, True, True)
    assert not (b.pipeline_parallel_enabled or b.data_parallel_enabled or b.data_replication_enabled or b.data_sharding_enabled or b.context_parallel_enabled or b.tensor_parallel_enabled)
    assert b.get_mesh() is None and b._dp_degree == 1 and b.prepare_optimizer(1, 2) == (1, 2) and b.prepare_model("m") == "m"
    with b.main_process_first():
        pass
    for kw in (dict(pp_degree=2), dict(cp_degree=2), dict(tp_degree=2), dict(dp_shards=2)):
        with pytest.raises(NotImplementedError):
            MI355XParallelBackend(world_size=2, dp_degree=1, **kw)
    with pytest.raises(ValueError):
        MI355XParallelBackend(world_size=2, dp_degree=1)
    assert isinstance(b.get_checkpointer(output_dir="/tmp/x", checkpointing_steps=5), MI355XCheckpointer)


def test_checkpointer_round_trip_with_the_trainers_own_torch_optimizer(tmp_path):
    """SFTTrainer hands the checkpointer ITS optimizer (finetrainers/trainer/sft_trainer/trainer.py:309-320: `optimizers=self.optimizer`, an
    OptimizerWrapper around torch's AdamW), not an MI355XSFTStep: save() must write a DCP training state from it (and ALWAYS run the model hook that
    writes the adapters), load() must bring model, both AdamW moments, the step counter and the schedule clock back.  CPU, plain torch.optim.AdamW
    and the reference's wrapper shape (an object with `.optimizers` + Stateful state_dict / load_state_dict)."""
    import torch.nn as nn
    from torch.distributed.checkpoint.state_dict import StateDictOptions, get_optimizer_state_dict, set_optimizer_state_dict
    from torch.distributed.checkpoint.stateful import Stateful

    from finetrainers_amd.parallel import MI355XCheckpointer

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.base = nn.Linear(6, 6)
            self.lora_A = nn.Parameter(torch.randn(2, 6) * 0.1)
            self.lora_B = nn.Parameter(torch.randn(6, 2) * 0.1)
            self.base.requires_grad_(False)

        def forward(self, x):
            return self.base(x) + x @ self.lora_A.t() @ self.lora_B.t()

    class OptimizerWrapper(Stateful):  # finetrainers/optimizer.py:17-61, restated
        def __init__(self, parts, opts):
            self.model_parts, self.optimizers = parts, opts

        def state_dict(self):
            o = StateDictOptions(flatten_optimizer_state_dict=True)
            return {k: v for m, oo in zip(self.model_parts, self.optimizers) for k, v in get_optimizer_state_dict(m, oo, options=o).items()}

        def load_state_dict(self, sd):
            o = StateDictOptions(flatten_optimizer_state_dict=True)
            for m, oo in zip(self.model_parts, self.optimizers):
                set_optimizer_state_dict(m, oo, optim_state_dict=sd, options=o)

    class Schedulers:
        def __init__(self, sch):
            self.sch = sch

        def get_lr_scheduler_state(self):
            return {"lr_scheduler": self.sch}  # LRScheduler objects are Stateful-compatible for DCP through state_dict()/load_state_dict()

    class TrainState:
        step = 0
        observed_data_samples = 0

    def make(seed, wrap):
        torch.manual_seed(seed)
        m = Tiny()
        opt = torch.optim.AdamW(m.parameters(), lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-4, fused=False)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1 + s))
        return m, (OptimizerWrapper([m], [opt]) if wrap else opt), opt, sch

    for wrap in (True, False):  # the reference's wrapper, and a bare torch optimizer
        out = tmp_path / f"ckpt_{int(wrap)}"
        m, handed, opt, sch = make(0, wrap)
        for _ in range(3):
            m(torch.randn(4, 6)).pow(2).sum().backward()
            opt.step(); sch.step(); opt.zero_grad()
        hooked = []
        ck = MI355XCheckpointer(dataloader=None, model_parts=[m], optimizers=handed, schedulers=None, states={}, checkpointing_steps=2, checkpointing_limit=2,
                                output_dir=str(out), enable=True, _callback_fn=lambda sd: hooked.append(sorted(sd)))
        assert ck.save(step=3) is None and not hooked            # not a checkpointing step
        path = ck.save(step=4)
        assert path is not None and os.path.isdir(path) and len(hooked) == 1 and "lora_A" in hooked[0]   # the model hook ran
        assert ck.save(step=5, force=True) is not None and ck.save(step=7, force=True) is not None and len(hooked) == 3
        assert sorted(p.name for p in out.glob("finetrainers_step_*")) == ["finetrainers_step_5", "finetrainers_step_7"]  # limit 2: the oldest is purged
        want_a, want_m = m.lora_A.detach().clone(), opt.state[m.lora_A]["exp_avg"].clone()

        m2, handed2, opt2, sch2 = make(1, wrap)  # a FRESH model + optimizer (different weights, no moments)
        m2(torch.randn(4, 6)).pow(2).sum().backward()
        opt2.step(); opt2.zero_grad()             # torch needs the state entries to exist before set_optimizer_state_dict fills them
        ck2 = MI355XCheckpointer(dataloader=None, model_parts=[m2], optimizers=handed2, schedulers=None, states={}, checkpointing_steps=2, checkpointing_limit=2,
                                 output_dir=str(out), enable=True)
        assert ck2.load(step=-1) is True          # the latest (step 7)
        assert torch.equal(m2.lora_A.detach(), want_a) and torch.equal(opt2.state[m2.lora_A]["exp_avg"], want_m)
        assert float(opt2.state[m2.lora_A]["step"]) == 3.0
        assert ck2.load(step=6) is False          # no such directory

    # a failing training-state write must not swallow the adapters: the hook still runs
    class Boom:
        optimizers = [None]

    m, _, _, _ = make(2, False)
    hooked = []
    ck = MI355XCheckpointer(model_parts=[m], optimizers=Boom(), states={}, checkpointing_steps=1, output_dir=str(tmp_path / "boom"), _callback_fn=lambda sd: hooked.append(1))
    with pytest.raises(Exception):
        ck.save(step=1, force=True)
    assert hooked == [1]


def test_bench_two_ranks_rehearsal_emits_the_multi_gpu_schema():
    """The first multi-GPU run of bench.py happens on the driver's clock.  Everything that only exists at N > 1 -- the self-spawn under
    torch.distributed.run on 127.0.0.1, the process group, the adapter broadcast, the bucket schedule of the 28-block backward, barrier + max-over-ranks
    timing, rank 0's single JSON line with `exchange`, `exposed_comm_ms`, `buckets_per_step` -- is executed here end to end, on CPU over gloo
    (FTMI_BENCH_REHEARSAL_CPU=1: no kernels, the line says "rehearsal").  The exchange block must come from the COMMUNICATOR (group size, one record per
    rank), so that the driver can check N ranks on N devices from the line alone."""
    import json
    import subprocess

    env = dict(os.environ, FTMI_BENCH_REHEARSAL_CPU="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # ONE line, from rank 0
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "exchange", "exposed_comm_ms", "buckets_per_step"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert "rehearsal" in d and d["config"]["global_batch"] == 4 and d["config"]["parallelism"] == "dp2"
    ex = d["exchange"]
    assert ex["backend"] == "gloo" and ex["world_size"] == 2 and ex["group_size"] == 2 and ex["group_rank"] == 0
    assert sorted(r["rank"] for r in ex["rank_devices"]) == [0, 1] and "algo" in ex and "proto" in ex and "hsa_env_set_before_hip_init" in ex
    assert d["buckets_per_step"] == 4.0                 # 28 blocks in ranges of 7, every step (warm-up included in the count and in the divisor)
    assert isinstance(d["exposed_comm_ms"], float) and d["exposed_comm_ms"] >= 0.0
    assert d["value"] > 0 and d["ms_per_step"] > 0


def _bench_rehearsal(*argv):
    import json
    import subprocess

    env = dict(os.environ, FTMI_BENCH_REHEARSAL_CPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]  # ONE line, from rank 0
    return json.loads(lines[0])


def test_bench_eight_ranks_rehearsal_ltx():
    """The driver's scaling run is `bench.py --gpus 8` (parallel/ptd.py:462-463 in the reference: replicate() over 8 ranks).  The same harness on 8 gloo ranks
    on CPU: one line, the communicator reports 8 ranks with 8 distinct rank records, and the 28-block backward is exchanged as 4 buckets per step on every
    step -- so the first real 8-GPU run cannot trip over anything that only exists at N = 8."""
    d = _bench_rehearsal("--gpus", "8", "--steps", "2", "--warmup", "1")
    ex = d["exchange"]
    assert d["n_gpus"] == 8 and d["config"]["parallelism"] == "dp8" and d["config"]["global_batch"] == 16 and d["scaling"] == "weak"
    assert ex["group_size"] == 8 and ex["world_size"] == 8 and ex["backend"] == "gloo"
    assert sorted(r["rank"] for r in ex["rank_devices"]) == list(range(8)) and len({r["local_rank"] for r in ex["rank_devices"]}) == 8
    assert d["buckets_per_step"] == 4.0
    assert isinstance(d["exposed_comm_ms"], float) and d["value"] > 0


def test_bench_plain_run_leaves_the_extras_to_full(monkeypatch):
    """A plain `bench.py` run times the steps and nothing else: the in-stream event profiler and the CPU baseline only run under --full."""
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4"])
    a = bench.parse()
    assert (a.full, a.no_prof, a.no_cpu_baseline, a.steps) == (False, True, True, 4)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--steps", "4"])
    a = bench.parse()
    assert (a.full, a.no_prof, a.no_cpu_baseline, a.steps) == (True, False, False, 4)


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs DIR: the last step's outputs as DIR/<name>.npy (rehearsal on CPU: the step's loss); a large output is written as a fixed sample,
    the same elements in every run, in float32 (float64 kept), within the 64 MB budget."""
    import numpy as np

    import bench

    d = _bench_rehearsal("--gpus", "2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "run"))
    assert d["steps"] == 2
    loss = np.load(tmp_path / "run" / "loss.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,)
    big = torch.arange(3 * bench.DUMP_SAMPLE, dtype=torch.bfloat16)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": torch.ones(3, dtype=torch.float64)})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert np.load(tmp_path / "a" / "small.npy").dtype == np.float64
    with pytest.raises(RuntimeError, match="MB"):
        bench.dump_outputs(str(tmp_path / "c"), {f"t{i}": torch.zeros(bench.DUMP_SAMPLE) for i in range(17)})


@pytest.mark.parametrize("n", [2, 8])
def test_bench_rehearsal_wan_parameter_sharding(n):
    """BASELINE config 4 (`--workload wan`, parallel/ptd.py:466-499: fully_shard per block + root): the real ParameterSharder on n gloo ranks walks the
    step's gather / reduce-scatter schedule over 1 + 30 flat units and every rank checks its shard of every averaged gradient (bench.py raises otherwise).
    Per step: the root and 30 blocks are gathered for the forward, 28 blocks again for the backward (the last two are still resident in the two rotating
    buffers) = 59 all-gathers, and 31 reduce-scatters -- whatever the number of ranks."""
    d = _bench_rehearsal("--gpus", str(n), "--workload", "wan", "--steps", "2", "--warmup", "1")
    ex, sh = d["exchange"], d["sharder"]
    assert d["n_gpus"] == n and d["config"]["parallelism"] == f"fsdp{n}" and ex["group_size"] == n
    assert sorted(r["rank"] for r in ex["rank_devices"]) == list(range(n))
    assert sh == {"units": 31, "gathers_per_step": 59.0, "scatters_per_step": 31.0, "world": n}


def test_committed_attention_streams_are_what_the_generator_writes(tmp_path, monkeypatch):
    """The hand-placed attention kernels #include statement lists written by tools/gen_attn_pl.py (csrc/attn_pl_*.inc, committed: the build does not run the
    generator).  Regenerate them into a scratch directory and compare byte for byte, so that an edit of the generator without a regenerate -- or a hand edit
    of a generated file -- cannot ship."""
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_attn_pl", os.path.join(root, "tools", "gen_attn_pl.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out, exp = tmp_path / "csrc", tmp_path / "experimental"
    out.mkdir()
    exp.mkdir()
    monkeypatch.setattr(gen, "OUT", str(out))
    monkeypatch.setattr(gen, "EXP_OUT", str(exp))
    gen.main()
    made = sorted(os.listdir(out))
    committed_dir = os.path.join(root, "finetrainers_amd", "csrc")
    committed = sorted(f for f in os.listdir(committed_dir) if f.startswith("attn_pl_") and f.endswith(".inc"))
    assert made == committed, (made, committed)
    for f in made:
        assert (out / f).read_bytes() == open(os.path.join(committed_dir, f), "rb").read(), f"{f}: committed stream differs from the generator's output"
    for f in sorted(os.listdir(exp)):
        assert (exp / f).read_bytes() == open(os.path.join(root, "tools", "experimental", f), "rb").read(), f"{f}: committed experimental stream differs"


def test_generated_attention_streams_keep_the_mfma_to_valu_distance():
    """hipcc inserts no wait states between `asm volatile` statements, so the generator (tools/gen_attn_pl.py) places every VALU instruction that reads an MFMA
    result at least two MFMAs behind the MFMA that wrote it (the rule the kernels' header states).  Check it statically on the committed streams: walk each
    loop body twice (the loop wraps around) and, for every VALU statement, look up when each accumulator tile it reads was last written."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dirs = [os.path.join(root, "finetrainers_amd", "csrc"), os.path.join(root, "tools", "experimental")]
    files = [os.path.join(d, f) for d in dirs for f in sorted(os.listdir(d)) if f.startswith("attn_pl_") and f.endswith(".inc")]
    assert len(files) >= 12
    stmt = re.compile(r'asm volatile\("([^"]*)"\s*(?::\s*([^:;]*?))?\s*(?::\s*([^:;]*?))?\s*(?::[^;]*)?\);')
    operand = re.compile(r'"([^"]+)"\(([^()]*(?:\([^()]*\)[^()]*)*)\)')
    checked = 0
    for path in files:
        if "_nomfma" in path:  # (time-only ablation without the MFMAs)
            continue
        body = [m for m in stmt.finditer(open(path).read())]
        last_write = {}  # accumulator tile -> index (in MFMAs issued) of the MFMA that last wrote it
        n_mfma = 0
        for rep in range(2):
            for m in body:
                text, outs, ins = m.group(1), m.group(2) or "", m.group(3) or ""
                if text.startswith("v_mfma"):
                    n_mfma += 1
                    for cons, expr in operand.findall(outs):
                        last_write[expr.strip()] = n_mfma
                elif text.startswith("v_") and not text.startswith("v_accvgpr"):
                    for cons, expr in operand.findall(ins):
                        e = expr.strip()
                        for tile, when in last_write.items():
                            if e.startswith(tile + "[") and rep == 1:
                                checked += 1
                                assert n_mfma - when >= 2, f"{os.path.basename(path)}: `{text}` reads {e} {n_mfma - when} MFMA(s) behind the MFMA that wrote {tile}"
    assert checked > 500


def test_head_dim_128_stream_waits_for_every_lds_fragment_it_consumes():
    """attn_bwd_dkdv_pl128_kernel never drains the LDS queue inside a slot: tools/gen_attn_pl.py computes a COUNTED `s_waitcnt lgkmcnt(n)` in front of each consumer
    from the issue order (LDS reads return in order; the counter saturates at 15).  Replay the committed stream on a model of that queue -- two trips through the
    loop body, so the reads the previous trip left in flight are covered -- and require that no MFMA is issued while one of the fragment registers it reads is still
    outstanding, and that no read overwrites a register whose previous content was never consumed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "finetrainers_amd", "csrc", "attn_pl_dkv128_v1.inc")).read()
    stmt = re.compile(r'asm volatile\("([^"]*)"\s*(?::\s*([^:;]*?))?\s*(?::\s*([^:;]*?))?\s*(?::[^;]*)?\);|(HAND_OVER\(\);)')
    operand = re.compile(r'"([^"]+)"\(([^()]*(?:\([^()]*\)[^()]*)*)\)')

    def regs(expr):
        e = expr.strip()
        m = re.fullmatch(r"TRF\((\d+)\)", e)
        if m:
            return [f"trlo[{m.group(1)}]", f"trhi[{m.group(1)}]"]
        if e == "LSI":
            return [f"lsi[{i}]" for i in range(4)]
        if e == "DLI":
            return [f"dli[{i}]" for i in range(4)]
        return [e]

    queue, consumed, n_checked = [], {}, 0  # outstanding reads (oldest first); register -> was its last load consumed by an MFMA
    for trip in range(2):
        for m in stmt.finditer(text):
            if m.group(4):  # HAND_OVER: wave 0 drains the queue inside it, the other waves do not -- model the other waves
                continue
            t, outs, ins = m.group(1), m.group(2) or "", m.group(3) or ""
            if t.startswith("ds_read"):
                dst = operand.findall(outs)[0][1].strip()
                if trip == 1:
                    assert consumed.get(dst, True), f"{dst} is reloaded before its previous content was used"
                consumed[dst] = False
                queue.append(dst)  # (pessimistic model: a read retires only when a wait says so)
            elif t.startswith("s_waitcnt lgkmcnt("):
                n = int(t[len("s_waitcnt lgkmcnt("):].split(")")[0])
                while len(queue) > n:
                    queue.pop(0)
            elif t.startswith("v_mfma"):
                for _, expr in operand.findall(ins):
                    for r in regs(expr):
                        if r in consumed:
                            n_checked += 1
                            assert r not in queue, f"`{t}` reads {r} while its load is still in flight ({len(queue)} outstanding)"
                            consumed[r] = True
    assert n_checked >= 2 * (32 + 32 + 16 + 8)  # per trip: 16 + 16 transposed-fragment halves x 2 slots ..., row fragments, accumulator-input rows


def test_no_accumulator_is_read_before_the_matrix_pipe_has_written_it():
    """tools/mfma_hazard_lint.py on the built code objects: the MFMAs of the hand-placed kernels sit inside asm statements, so hipcc's hazard recogniser does not
    know their results are matrix-pipe results -- a copy it inserts at a loop exit (live-range split of an accumulator tile) can come passes + 3 wait states too
    early.  Round 6 met exactly that (one accumulator register of the 224-row GELU' kernel wrong); the kernels now settle on every exit path and this test
    proves the distance on every kernel whose MFMAs are asm, for whatever register allocation this build produced."""
    import importlib.util

    build = os.path.join(ROOT, "finetrainers_amd", "csrc", "build")
    objs = [os.path.join(build, f) for f in ("gemm.hip.o", "attention.hip.o")]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip("no object files: run __graft_entry__.build() first")
    spec = importlib.util.spec_from_file_location("mfma_hazard_lint", os.path.join(ROOT, "tools", "mfma_hazard_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    for o in objs:
        early = [x for x in lint.lint(lint.disassemble(o)) if any(k in x[0] for k in lint.ASM_KERNELS)]
        assert not early, f"{o}: {len(early)} early accumulator reads, first: {early[0]}"


def test_narrow_ltx_layout_embeds_the_reference_dummy_in_the_wide_one():
    """finetrainers_amd/ltx_video/narrow.py, host logic: every parameter of the reference's dummy transformer (tests/models/ltx_video/base_specification.py:47-58; the
    oracle builds the same module tree) has a layout rule, widening is zero padding (same sum of magnitudes, narrow entries recovered exactly), heads land on 64-channel
    strides, RoPE pairs follow their channels, and geometries the embedding cannot hold are refused."""
    from finetrainers_amd.ltx_video import LTXTransformerConfig, NarrowLayout
    from finetrainers_amd.ltx_video.narrow import is_native
    from oracle import ltx

    cfg = ltx.LTXConfig.dummy()
    tcfg = LTXTransformerConfig(in_channels=8, out_channels=8, num_attention_heads=4, attention_head_dim=8, cross_attention_dim=32, num_layers=1, caption_channels=32)
    assert not is_native(tcfg) and is_native(LTXTransformerConfig())
    lay = NarrowLayout(tcfg)
    assert (lay.wide.inner_dim, lay.wide.in_channels, lay.wide.caption_channels) == (2048, 64, 64)
    assert lay.idx_h.tolist()[:10] == [0, 1, 2, 3, 4, 5, 6, 7, 64, 65] and lay.idx_pair.tolist()[:5] == [0, 1, 2, 3, 32]
    model = ltx.build_model(cfg, seed=0, rank=4, alpha=4.0)
    n = 0
    for k, v in model.state_dict().items():
        if "lora_" in k:
            continue
        sp = lay.spaces_of(k)
        w = lay.widen(v, *sp)
        assert torch.equal(lay.narrow(w, *sp), v) and w.double().abs().sum() == v.double().abs().sum(), k  # float64: exact for bf16 values, in any summation order
        n += 1
    assert n == 15 + 25  # 15 top-level tensors, 25 of the block
    w = lay.widen(model.state_dict()["transformer_blocks.0.attn1.to_q.base_layer.weight"], "h", "d")
    assert w.shape == (2048, 2048) and w[8:64].abs().sum() == 0 and w[:, 32:].abs().sum() == 0 and w[64:72, :32].abs().sum() > 0
    cos, sin = torch.rand(5, 16), torch.rand(5, 16)
    wc, ws = lay.rope_wide(cos, sin)
    assert wc.shape == (5, 1024) and torch.equal(wc[:, lay.idx_pair], cos) and torch.equal(ws[:, lay.idx_pair], sin)
    rest = torch.ones(1024, dtype=torch.bool)
    rest[lay.idx_pair] = False
    assert bool((wc[:, rest] == 1).all()) and bool((ws[:, rest] == 0).all())  # the identity rotation on every padded pair
    assert lay.lora_spaces(3) == ("h", "d") and lay.lora_spaces(0) == ("d", "h") and lay.lora_spaces(5) == ("d", "h")
    for bad in (dict(num_attention_heads=4, attention_head_dim=7, cross_attention_dim=28), dict(num_attention_heads=40, attention_head_dim=8, cross_attention_dim=320),
                dict(num_attention_heads=4, attention_head_dim=10, cross_attention_dim=40)):
        with pytest.raises(ValueError):
            NarrowLayout(LTXTransformerConfig(in_channels=8, out_channels=8, num_layers=1, caption_channels=32, **bad))


def test_no_register_is_reused_while_its_load_is_in_flight():
    """tools/inflight_reg_lint.py: the second hazard class of asm-load kernels that round 6 met (a dead fragment read handed its register to a load's address while
    the LDS read was still in flight: memory fault).  The replay of the in-order wait counters must (a) flag that pattern in a hand-written listing and accept it once
    the wait is there, (b) find nothing in the built GEMM and attention code objects -- which also proves that no instantiation that spills in-flight load destinations
    (224-row register-staged tiles with a K-extension) is in the library at all."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("inflight_reg_lint", os.path.join(ROOT, "tools", "inflight_reg_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    bad = ("0000 <k1>:\n\tds_read_b128 v[2:5], v210 offset:2048\n\tv_mfma_f32_16x16x32_bf16 a[0:3], v[38:41], v[6:9], a[0:3]\n"
           "\tv_cndmask_b32_e32 v2, v104, v102, vcc\n\tbuffer_load_dwordx4 v2, s[0:3], s4 offen lds\n\ts_waitcnt lgkmcnt(0)\n")
    found = lint.lint(bad)
    assert found and found[0][2] == "writes" and found[0][3] == "v2"
    assert lint.lint(bad.replace("\tv_cndmask", "\ts_waitcnt lgkmcnt(0)\n\tv_cndmask")) == []
    counted = ("0000 <k2>:\n\tbuffer_load_dwordx4 a[0:3], v0, s[8:11], s20 offen\n\tbuffer_load_dwordx4 v[8:11], v1, s[8:11], s20 offen\n\ts_waitcnt vmcnt(1)\n"
               "\tds_write_b128 v20, a[0:3]\n\tds_write_b128 v20, v[8:11]\n")
    found = lint.lint(counted)  # vmcnt(1) retires the older load only: the first store is fine, the second reads a destination still in flight
    assert len(found) == 1 and "v[8:11]" in found[0][1]
    build = os.path.join(ROOT, "finetrainers_amd", "csrc", "build")
    objs = [os.path.join(build, f) for f in ("gemm.hip.o", "attention.hip.o")]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip("no object files: run __graft_entry__.build() first")
    for o in objs:
        pr = lint.lint(lint.disassemble(o))
        assert not pr, f"{o}: {len(pr)} uses of a register whose load is in flight, first: {pr[0]}"
