"""Wan first/last-frame image-to-video LoRA on the GPU (a config with ``pos_embed_seq_len``: two images, 2 x 257 = 514 image keys in every attn2): the wide
second-context kernels (``ftmi_attn_ctx2w_fwd / _dq``) against fp64, bit for bit against the narrow pair where both apply, their tail and saturation
behaviour; the block with a second image (TI2) against tests/wan_i2v_reference.py's block, C call against Python composition, recomputation against kept
activations and its degenerations; model, LoRA step and latent sampler against tests/wan_flf_reference.py.

The block, model and step checks ARE the image-to-video file's (tests/test_gpu_wan_i2v.py): its test bodies run here on first/last-frame pairs and batches,
so the margins are its margins by construction."""
import functools

import pytest
import torch

import test_gpu_wan_i2v as i2v

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
SMALL, BIG = i2v.SMALL, i2v.BIG
TI = TI2 = 257
NPOS = TI + TI2


def _dev():
    return torch.device("cuda", 0)


# ---- 1 - 3: the kernels -----------------------------------------------------------------------------------------------------------------------------------------
def _run(c, kv=None, wide=True, inplace=False):
    """i2v._run_ctx2 through the wide pair (``wide`` False: the narrow pair); ``inplace``: dq written into a copy of dq_t."""
    from finetrainers_amd import ops

    dev = _dev()
    k, v = i2v._kv_views((c["kv"] if kv is None else kv).to(dev), c["Sk"], c["H"])
    q, o_t, do, dq_t = (c[n].to(dev) for n in ("q", "o_t", "do", "dq_t"))
    assert q.stride(1) == 128 and q.stride(2) == c["H"] * 128 and (c["Sk"] == 1 or k.stride(2) == 2 * c["H"] * 128)
    fwd, dq_fn = (ops.attn_ctx2w_fwd, ops.attn_ctx2w_dq) if wide else (ops.attn_ctx2_fwd, ops.attn_ctx2_dq)
    o, lse = fwd(q, k, v, o_t)
    if inplace:
        first = dq_t.clone(memory_format=torch.preserve_format)
        assert first.stride() == dq_t.stride()
        dq = dq_fn(q, k, v, lse, do, first, inplace=True)
        assert dq.data_ptr() == first.data_ptr()
    else:
        dq = dq_fn(q, k, v, lse, do, dq_t)
    torch.cuda.synchronize()
    return o.cpu(), dq.cpu(), lse.cpu()


def _check_wide(monkeypatch, c, tag):
    """i2v._check_ctx2 -- o and dq within 2 x the bf16-storage graph's distance from fp64, lse within 4e-3 + 1e-5 |lse| -- with the wide pair under it."""
    monkeypatch.setattr(i2v, "_run_ctx2", _run)
    return i2v._check_ctx2(c, tag)


@pytest.mark.parametrize("Sk", [321, 384, 514, 575, 640])  # a tail of one, whole tiles, the real shape (tail of two), a tail of 63, the limit
@pytest.mark.parametrize("B,H,Sq", [(1, 1, 1), (2, 2, 48), (1, 3, 200)])
def test_wide_kernels_against_fp64(monkeypatch, B, H, Sq, Sk):
    _check_wide(monkeypatch, i2v._ctx2_case(B, H, Sq, Sk, seed=B * 100000 + Sq * 1000 + Sk), f"wide B={B} H={H} Sq={Sq} Sk={Sk}")


@pytest.mark.parametrize("Sk", [1, 64, 257, 320])
@pytest.mark.parametrize("B,H,Sq", [(2, 2, 48), (1, 3, 200)])
def test_wide_pair_returns_the_narrow_pairs_bits(B, H, Sq, Sk):
    """Same arithmetic in the same order, another staging: o, lse and dq of the wide pair are the narrow pair's bits for every key count both take, with dq
    out of place and in place."""
    c = i2v._ctx2_case(B, H, Sq, Sk, seed=Sq * 1000 + Sk, alloc=Sk + 3)
    want = _run(c, wide=False)
    for inplace in (False, True):
        for wide in (True, False):
            got = _run(c, wide=wide, inplace=inplace)
            for name, a, b in zip(("o", "dq", "lse"), want, got):
                assert torch.equal(a, b), (name, "wide" if wide else "narrow", "in place" if inplace else "out of place")


def test_wide_tail_keys_and_saturated_rows(monkeypatch):
    """Sk = 514 (eight full tiles and a tail of two) in an allocation of 640 rows.  Query row 0 of every head: all real logits below -100; row 1: dominated by
    key 513, the last one; row 2: by key 512, the first of the tail tile.  o, lse and dq finite and within the bounds of the test above; NaN in rows 514 .. 639
    of k_i / v_i changes no bit."""
    B, H, Sq, Sk, A = 1, 2, 48, NPOS, 640
    c = i2v._ctx2_case(B, H, Sq, Sk, seed=5, alloc=A)
    g = torch.Generator().manual_seed(6)
    u = torch.full((128,), 128 ** -0.5)
    w1, w2 = torch.zeros(128), torch.zeros(128)
    w1[0], w1[1] = 2 ** -0.5, -(2 ** -0.5)  # unit, orthogonal to u and to each other
    w2[2], w2[3] = 2 ** -0.5, -(2 ** -0.5)
    kv = c["kv"].float().view(B, A, 2, H, 128)
    kv[:, :, 0] = 12.0 * u + 0.3 * torch.randn(B, A, H, 128, generator=g)
    kv[:, Sk - 1, 0] += 6.0 * w1
    kv[:, Sk - 2, 0] += 6.0 * w2
    c["kv"] = kv.view(B, A, 2 * H * 128).to(bf16)
    q = c["q"].float().clone()
    q[:, :, 0] = -110.0 * u + 0.1 * torch.randn(B, H, 128, generator=g)
    q[:, :, 1] = 40.0 * w1
    q[:, :, 2] = 40.0 * w2
    c["q"] = q.permute(0, 2, 1, 3).contiguous().to(bf16).permute(0, 2, 1, 3)
    k, _ = i2v._kv_views(c["kv"], Sk, H)
    logits = (c["q"].double() @ k.double().transpose(-1, -2)) / 128 ** 0.5
    assert logits[:, :, 0].max() < -100.0
    for row, key in ((1, Sk - 1), (2, Sk - 2)):
        others = torch.cat([logits[:, :, row, :key], logits[:, :, row, key + 1:]], dim=-1)
        assert (logits[:, :, row, key] - others.max(-1).values).min() > 10.0
    o, dq, lse = _check_wide(monkeypatch, c, "wide: saturated rows + tail keys")
    poisoned = c["kv"].clone()
    poisoned[:, Sk:] = float("nan")
    o2, dq2, lse2 = _run(c, kv=poisoned)
    assert torch.equal(o, o2) and torch.equal(dq, dq2) and torch.equal(lse, lse2)


# ---- 4: the block -----------------------------------------------------------------------------------------------------------------------------------------------
def _flf_block_pair(geom, rank, oracle=True, seed=0, second=TI2):
    """i2v._block_pair with the second image declared on the MI355X block (the reference block takes whatever image rows it is handed)."""
    oblk, gblk = _I2V_BLOCK_PAIR(geom, rank, oracle=oracle, seed=seed)
    gblk.second_image_tokens = second
    return oblk, gblk


_I2V_BLOCK_PAIR, _I2V_INPUTS, _I2V_BATCH = i2v._block_pair, i2v._inputs, i2v._batch  # the originals: the tests below put their own in i2v's namespace


def _as_flf(monkeypatch):
    """The image-to-video file's block tests, run on blocks with TI = TI2 = 257 and 514 image rows."""
    monkeypatch.setattr(i2v, "_block_pair", _flf_block_pair)
    monkeypatch.setattr(i2v, "_inputs", functools.partial(_I2V_INPUTS, ti=NPOS))


BLOCK_CASES = [(SMALL, 2, 48, 16), (SMALL, 1, 77, 16)]  # S = 77: a ragged last query tile and rows that are no multiple of any GEMM tile


@pytest.mark.parametrize("rank", [32, 64])
@pytest.mark.parametrize("geom,B,S,T", BLOCK_CASES)
def test_flf_block_parity(monkeypatch, geom, B, S, T, rank):
    """out, dx, d text and the 16 adapter gradients against the reference block on 514 image tokens: test_i2v_block_parity's body and bounds."""
    _as_flf(monkeypatch)
    i2v.test_i2v_block_parity(geom, B, S, T, rank)


@pytest.mark.parametrize("geom,B,S,T,rank", [c + (r,) for c in BLOCK_CASES for r in (32, 64)] + [(BIG, 1, 136, 16, 64)])
def test_flf_block_c_call_python_composition_and_recomputation(monkeypatch, geom, B, S, T, rank):
    """``ftmi_wan_lora_ffn_block_*`` with TI2 > 0 against the composition from Python (``ops.attn_ctx2w_*``) and recomputation against kept activations:
    test_i2v_block_c_call_python_composition_and_recomputation's body and bits.  BIG: 40 heads, the 14B geometry."""
    _as_flf(monkeypatch)
    i2v.test_i2v_block_c_call_python_composition_and_recomputation(geom, B, S, T, rank)


@pytest.mark.parametrize("native", [True, False])
def test_flf_block_degenerations(native):
    """Step a: TI2 = 0 on 257 image rows is the image-to-video block (the narrow pair), and declaring the last of those rows a second image (TI = 256,
    TI2 = 1: the wide pair on the same 257 keys) changes no bit.  Step b: TI = 257, TI2 = 63 -- the block issues the wide pair on 320 keys -- against the same
    block run as a single image of 320 tokens, whose Python composition calls ``ops.attn_ctx2_fwd / _dq`` directly: the bit contract, in place."""
    geom, B, S, T = SMALL, 2, 48, 16
    _, gblk = _I2V_BLOCK_PAIR(geom, 32, oracle=False)
    rope, _ = i2v._rope_tables(S, 128, seed=4)
    x, enc, temb, dout, img = _I2V_INPUTS(B, S, T, geom[0], seed=S + 3, ti=320)

    def run(second, rows, nat):
        gblk.native, gblk.second_image_tokens = nat, second
        return i2v._run_gpu(gblk, x, enc, temb, dout, rope, img[:, :rows])

    one = run(0, TI, native)
    i2v._same(one, run(1, TI, native), "TI = 256, TI2 = 1 against TI = 257, TI2 = 0")
    narrow_direct = run(0, 320, False)
    assert not torch.equal(narrow_direct[0], one[0])
    i2v._same(narrow_direct, run(63, 320, native), "TI = 257, TI2 = 63 against the narrow pair on 320 keys")
    with pytest.raises(ValueError):  # more second-image tokens than rows
        run(320, 257, native)
    gblk.second_image_tokens = 0


# ---- 5, 6: model, step, sampler ---------------------------------------------------------------------------------------------------------------------------------
def _flf_model_pair(layers=2, rank=32):
    """i2v._model_pair for a config with pos_embed_seq_len = 514; ``pos_embed`` drawn non-zero."""
    import wan_flf_reference as ref
    from finetrainers_amd.wan import MI355XWanTransformer3DModel, WanTransformerConfig

    torch.manual_seed(0)
    omodel = ref.WanFLFTransformer3DModel(ref.WanFLFConfig(num_layers=layers, pos_embed_seq_len=NPOS, **i2v.KW))
    g = torch.Generator().manual_seed(7)
    i2v._perturb(omodel, g)
    with torch.no_grad():
        pe = omodel.condition_embedder.image_embedder.pos_embed
        pe.copy_(0.5 * torch.randn(pe.shape, generator=g))
    omodel = omodel.to(bf16)
    gmodel = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=layers, in_channels=36, pos_embed_seq_len=NPOS, **i2v.KW), device=_dev())
    gmodel.load_diffusers_state_dict({i2v._fix(k): v for k, v in omodel.state_dict().items()})
    assert float(gmodel.rparam("condition_embedder.image_embedder.pos_embed").abs().max()) > 0
    for p in omodel.parameters():
        p.requires_grad_(False)
    for blk in omodel.blocks:
        for attn in (blk.attn1, blk.attn2):
            i2v._wrap(attn, rank, float(rank), g)
    gmodel.add_adapter(rank, float(rank))
    gmodel.load_lora_state_dict({k: v.detach() for k, v in i2v._lora_keys(omodel).items()})
    return omodel, gmodel


@functools.lru_cache(maxsize=None)
def _flf_batch():
    """i2v._batch with the CLIP tokens of two images per sample, [B, 514, image_dim]."""
    g = torch.Generator().manual_seed(12)
    b = dict(_I2V_BATCH())
    b["image"] = torch.randn(b["image"].shape[0], NPOS, b["image"].shape[2], generator=g).to(bf16)
    return b


def _model_as_flf(monkeypatch):
    monkeypatch.setattr(i2v, "_model_pair", _flf_model_pair)
    monkeypatch.setattr(i2v, "_batch", _flf_batch)


def test_flf_model_parity(monkeypatch):
    """2 blocks, pos_embed_seq_len = 514: prediction, loss and the 32 adapter gradients against wan_flf_reference -- test_i2v_model_parity's body and bounds."""
    _model_as_flf(monkeypatch)
    i2v.test_i2v_model_parity()


def test_flf_model_takes_both_input_layouts():
    """[B, 514, image_dim] and [2B, 257, image_dim] (rows 2b, 2b + 1 = sample b's first and last image, upstream's view): the same prediction bits; and the
    images matter -- swapping first and last changes the prediction."""
    from finetrainers_amd.wan import MI355XWanSpecOps

    _, gmodel = _flf_model_pair()
    dev, b, spec = _dev(), _flf_batch(), MI355XWanSpecOps()

    def predict(image):
        kw = dict(i2v._gpu_kwargs(b), encoder_hidden_states_image=image.to(dev))
        with torch.no_grad():
            return spec.forward(gmodel, b["moments"].to(dev), b["text"].to(dev), b["sigmas"].to(dev), b["mean"].to(dev), b["std"].to(dev), **kw)[0].clone()

    B = b["image"].shape[0]
    want = predict(b["image"])
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(want, predict(b["image"].reshape(2 * B, TI, -1)))
    assert not torch.equal(want, predict(torch.cat([b["image"][:, TI:], b["image"][:, :TI]], dim=1)))
    with pytest.raises(ValueError, match="514"):
        predict(b["image"][:, :TI])


def test_flf_lora_step_with_and_without_checkpointing(monkeypatch):
    """Two ``MI355XWanLoRAStep`` steps on the first/last-frame model: test_i2v_lora_step_with_and_without_checkpointing's body and bounds."""
    _model_as_flf(monkeypatch)
    i2v.test_i2v_lora_step_with_and_without_checkpointing()


def test_flf_sampler_is_its_composition_bit_for_bit():
    """A two-step ``ftmi_wan_sample`` loop (guidance 5) on the first/last-frame model, ``condition_latents`` = [condition_mask(use_last_frame) | condition]:
    final state and final model input against ``model.forward`` + ``ops.wan_sample_step`` from Python, the assertion of
    test_one_call_loop_is_its_composition_bit_for_bit; then the same through ``MI355XWanLatentSampler.sample``."""
    import test_gpu_wan_sampling as smp
    import wan_sampling_reference as sref
    from finetrainers_amd import ops
    from finetrainers_amd.wan import MI355XWanLatentSampler, MI355XWanModelSpecification

    dev = _dev()
    _, gmodel = _flf_model_pair(rank=64)
    sref.randomize_adapters(gmodel)
    sampler = MI355XWanLatentSampler(gmodel)
    F_, H, W, T, C = smp.F_, smp.H, smp.W, smp.T, smp.C
    g = torch.Generator().manual_seed(31)
    mask = MI355XWanModelSpecification.condition_mask(4 * (F_ - 1) + 1, H, W, use_last_frame=True)
    assert tuple(mask.shape) == (1, 4, F_, H, W) and mask[0, :, 0].min() == 1 and mask[0, 3, -1].min() == 1 and mask[0, :3, -1].max() == 0
    c = dict(latents=torch.randn(1, C, F_, H, W, generator=g).to(dev), pos=torch.randn(1, T, 64, generator=g).to(bf16).to(dev),
             neg=torch.randn(1, T, 64, generator=g).to(bf16).to(dev), image=torch.randn(1, NPOS, 128, generator=g).to(bf16).to(dev),
             extra=torch.cat([mask.to(bf16), torch.randn(1, C, F_, H, W, generator=g).to(bf16)], dim=1).to(dev))
    sigmas = [1.0, 0.6, 0.0]
    x1, cols1, _ = smp._one_call(sampler, c, sigmas, 5.0)
    x2, cols2 = smp._composition(sampler, "i2v", c, sigmas, 5.0)
    x0 = sref.patchify(c["latents"].cpu())
    assert bool(torch.isfinite(x1).all()) and sref.rel_l2(x1, x0) > 0.05
    assert torch.equal(smp._bits(x1), smp._bits(x2)), "final state"
    assert torch.equal(smp._bits(cols1), smp._bits(cols2)), "final model input"
    out = sampler.sample(c["pos"], c["neg"], F_, H, W, guidance_scale=5.0, sigmas=sigmas, latents=c["latents"], image_embeds=c["image"], condition_latents=c["extra"])
    torch.cuda.synchronize()
    want = ops.wan_sample_finish(sampler.geometry(1, F_, H, W, guidance=True), x1, torch.zeros(C, device=dev), torch.ones(C, device=dev))
    assert torch.equal(smp._bits(out), smp._bits(want)), "sample() returns the loop's final state"
    pairs = sampler.sample(c["pos"], c["neg"], F_, H, W, guidance_scale=5.0, sigmas=sigmas, latents=c["latents"], image_embeds=c["image"].view(2, TI, 128),
                           condition_latents=c["extra"])
    assert torch.equal(smp._bits(out), smp._bits(pairs))
