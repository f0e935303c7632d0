"""Wan-T2V LoRA fine-tuning over a frozen base, the parts that need no GPU: the C ABI of the LoRA block (exported, declared, its saved-activation plan against the
full fine-tune's), the adapter set ``add_adapter`` attaches against the recipe's regex applied to the oracle's module names, the save -> load round trip
of the adapter file, and the data-parallel bucket schedule of ``MI355XWanLoRAStep`` on two gloo ranks."""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE_REGEX = "blocks.*(to_q|to_k|to_v|to_out.0)"  # examples/training/sft/wan/*/train.sh --target_modules
SMALL = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)


def test_c_abi_exports_and_declares_the_wan_lora_block():
    """The one LoRA entry family, ``ftmi_wan_lora_ffn_block_*``, is declared, bound and exported; the eight names of the two narrow families folded into it
    are neither declared nor exported."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", header))
    wan_lora_bytes.assert_only_the_wide_family(lib, declared, set(_lib.EXPORTED_SYMBOLS))
    assert not re.search(r"\bftmi_wan_(i2v_)?lora_block_config\b", header)  # their configuration typedefs went with them
    assert lib.ftmi_version() == 101


def test_lora_block_keeps_less_than_the_full_finetune_block():
    """At the recipe's bucket (49 x 480 x 832 -> 20 280 video + 512 text tokens, Wan2.1-T2V-1.3B geometry) the frozen base drops a1, n3, act and f:
    the saved buffer must be smaller than the full fine-tune's by at least the activation `act` (B S F 2 bytes), also with the rank-64 down-projections kept."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    B, S, T, D, F = 1, 20280, 512, 1536, 8960
    full = lib.ftmi_wan_block_saved_bytes(ctypes.byref(_lib.WanBlockConfig(B=B, S=S, T=T, D=D, H=12, F=F, eps=1e-6, gemm_variant=8)))
    for r in (0, 64, 128):
        lora, scratch = wan_lora_bytes.planned(B, S, T, D, 12, F, r)
        print(f"[wan-lora] saved bytes per block at {S}+{T} tokens: full fine-tune {full / 1e9:.3f} GB, LoRA r={r} {lora / 1e9:.3f} GB")
        assert 0 < lora and full - lora >= B * S * F * 2
        assert scratch > 0
    r0 = wan_lora_bytes.planned(B, S, T, D, 12, F, 0)[0]
    assert full - r0 >= B * S * (3 * D + F) * 2  # the four dropped buffers


def test_wan_planners_return_the_recorded_bytes():
    """The four byte planners and ``param_elements`` against tests/golden/wan_block_bytes.txt, recorded once from the library as it was before the full and
    the LoRA block shared one buffer plan: the callers' allocations (and what a checkpoint of ``saved`` would hold) must not move by a byte.  The LoRA
    columns are read through the one LoRA entry at TI = 0, ffn = 0."""
    import wan_lora_bytes
    from finetrainers_amd import _lib

    lib = _lib.load()
    rows = [ln.split() for ln in open(os.path.join(ROOT, "tests", "golden", "wan_block_bytes.txt")) if ln.strip() and not ln.startswith("#")]
    assert len(rows) == 18  # six geometries x r in {0, 64, 128}
    for row in rows:
        B, S, T, D, H, F, r, full_saved, full_scratch, elements, lora_saved, lora_scratch = map(int, row)
        full = ctypes.byref(_lib.WanBlockConfig(B=B, S=S, T=T, D=D, H=H, F=F, eps=1e-6, gemm_variant=8))
        got = (lib.ftmi_wan_block_saved_bytes(full), lib.ftmi_wan_block_scratch_bytes(full), lib.ftmi_wan_block_param_elements(full)) + \
            wan_lora_bytes.planned(B, S, T, D, H, F, r)
        assert got == (full_saved, full_scratch, elements, lora_saved, lora_scratch), (row, got)


def test_the_one_lora_entry_plans_the_recorded_bytes_of_all_three_families():
    """Every row of tests/golden/wan_lora_entry_bytes.txt -- seven geometries x r in {0, 64, 128} x TI in {0, 257, 320} x ffn in {0, 1}, and the refused
    configurations (0 0) -- through ``ftmi_wan_lora_ffn_block_*``, to the byte.  The file was recorded when the library still had the two narrow families
    and they returned the same numbers wherever they accepted the row: what their callers allocated has not moved."""
    import wan_lora_bytes

    plans = wan_lora_bytes.recorded()
    assert len(plans) == 123 and sum(v == (0, 0) for v in plans.values()) == 18
    assert {k[6:] for k, v in plans.items() if v != (0, 0)} == {(r, TI, ffn) for r in (0, 64, 128) for TI in (0, 257, 320) for ffn in (0, 1) if r or not ffn}
    for key, want in plans.items():
        assert wan_lora_bytes.planned(*key) == want, (key, want)


def _models(layers, rank=32, alpha=32.0):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig
    from oracle import wan

    omodel = wan.WanTransformer3DModel(wan.WanConfig(num_layers=layers, **SMALL))
    model = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, **SMALL), device=torch.device("cpu"))
    model.add_adapter(rank, alpha, target_modules=RECIPE_REGEX)
    return omodel, model


def test_add_adapter_selects_what_the_recipe_regex_selects():
    omodel, model = _models(30)
    # peft: a string target_modules is re.fullmatch'ed against every module name
    targets = [n for n, _ in omodel.named_modules() if re.fullmatch(RECIPE_REGEX, n)]
    assert len(targets) == 240  # 30 blocks x 2 attentions x 4 projections
    want = {f"{n}.lora_{ab}.weight" for n in targets for ab in "AB"}
    sd = model.lora_state_dict()
    assert set(sd) == want
    D = 256
    for k, v in sd.items():
        assert tuple(v.shape) == ((32, D) if ".lora_A." in k else (D, 32)) and v.dtype == torch.float32, k
        if ".lora_B." in k:
            assert float(v.abs().max()) == 0.0  # peft's init: B = 0
        else:
            assert 0.0 < float(v.abs().max()) <= (1.0 / D) ** 0.5  # kaiming_uniform_(a = sqrt(5)): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert len(model.lora_parameters()) == 60 and all(p.requires_grad and p.dtype == torch.float32 for p in model.lora_parameters())
    assert not any(blk.flat.requires_grad for blk in model.blocks) and not model.root.requires_grad
    for blk in model.blocks:  # ranks below the kernels' 64-row groups are stored zero-padded
        assert float(blk.lora_A.data[:, 32:].abs().max()) == 0.0


@pytest.mark.parametrize("bad", ["blocks.*(to_q|to_v)", "blocks.*attn1.(to_q|to_k|to_v|to_out.0)", ["to_q", "to_k", "to_v", "to_out.0", "ffn.net.2"], "ffn.*"])
def test_add_adapter_refuses_other_target_modules(bad):
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    model = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=1, **SMALL), device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match=re.escape(str(bad))[:12]):
        model.add_adapter(32, 32.0, target_modules=bad)
    assert model.lora_config is None and model.blocks[0].lora_A is None


def test_lora_file_round_trip(tmp_path):
    from finetrainers_amd import wire
    from finetrainers_amd.wan import MI355XWanModelSpecification

    _, model = _models(2, rank=32, alpha=16.0)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for v in model.lora_state_dict().values():
            v.copy_(0.02 * torch.randn(v.shape, generator=g))
    want = {k: v.clone() for k, v in model.lora_state_dict().items()}
    spec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
    spec._save_lora_weights(str(tmp_path), model.lora_state_dict(), scheduler=None, metadata=wire.lora_config_metadata(32, 16.0, RECIPE_REGEX))
    sd, cfg = wire.load_lora_weights(str(tmp_path))
    assert cfg["r"] == 32 and cfg["lora_alpha"] == 16.0 and cfg["target_modules"] == RECIPE_REGEX
    _, fresh = _models(2, rank=cfg["r"], alpha=cfg["lora_alpha"])
    fresh.load_lora_state_dict(sd)
    got = fresh.lora_state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert all(float(blk.lora_A.data[:, 32:].abs().max()) == 0.0 and float(blk.lora_B.data[:, :, 32:].abs().max()) == 0.0 for blk in fresh.blocks)
    with pytest.raises(KeyError):
        fresh.load_lora_state_dict({k: v for k, v in sd.items() if "blocks.1.attn2.to_out.0" not in k})
    assert json.dumps(cfg)  # plain JSON types


def _bucket_worker(rank, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from finetrainers_amd.parallel import DataParallelBackend
    from finetrainers_amd.wan import MI355XWanLoRAStep

    par = DataParallelBackend(backend="gloo", device=torch.device("cpu"))
    try:
        torch.manual_seed(100 + rank)  # different adapters per rank: the step object broadcasts rank 0's
        _, model = _models(7)
        step = MI355XWanLoRAStep(model, parallel=par, grad_bucket_blocks=3)
        n = step.flat.numel()
        first = step.flat[:64].clone()
        # the backward as the blocks drive it: last block first, each adds its gradient into its two views, then reports itself finished
        step._begin_exchange(True)
        for i in reversed(range(7)):
            blk = model.blocks[i]
            blk._grad_a_view.add_(float(rank + 1) * (i + 1))
            blk._grad_b_view.add_(float(rank + 1) * (i + 1) + 0.5)
            blk._backward_done()
        step._finish_exchange()
        log = list(step.bucket_log)
        ok = step.buckets_issued == 3 and len(log) == 3  # 7 blocks in buckets of 3: {6,5,4}, {3,2,1}, {0}
        ok &= log[0][1] == n and log[-1][0] == 0 and all(log[j][0] == log[j + 1][1] for j in range(len(log) - 1))  # contiguous, cover the buffer once
        for i, blk in enumerate(model.blocks):  # mean over the ranks of (rank + 1) = 1.5
            ok &= bool(torch.allclose(blk._grad_a_view, torch.full_like(blk._grad_a_view, 1.5 * (i + 1))))
            ok &= bool(torch.allclose(blk._grad_b_view, torch.full_like(blk._grad_b_view, 1.5 * (i + 1) + 0.5)))
        ok &= all(blk._grad_hook is None for blk in model.blocks)
        q.put((rank, bool(ok), log, first.numpy().tolist()))
    finally:
        par.destroy()


def test_lora_step_bucket_schedule_world2_gloo():
    """``MI355XWanLoRAStep``'s gradient exchange on two CPU ranks over gloo: every rank issues the same bucket sequence, the slices are contiguous and
    cover the flat gradient once, every element is averaged exactly once, and both ranks hold rank 0's adapters after construction."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 97
    procs = [ctx.Process(target=_bucket_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [r[:2] for r in res] == [(0, True), (1, True)]
    assert res[0][2] == res[1][2] and res[0][3] == res[1][3]
