"""CogVideoX latent sampling, the parts that need no GPU: the DDIM tables against the scheduler's formulas and their rotation closed form, the torch
restatement (tests/cog_sampling_reference.py: the loop the GPU trajectory test drives the oracle with), every refusal of the sampler with its reason, the
argument checks of the C entry points (they run before any launch), the workspace plan and the ABI table."""
import ctypes
import math
import os
import re

import pytest
import torch

import cog_sampling_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16 = torch.bfloat16
NEW_SYMBOLS = ("ftmi_cog_sample_init", "ftmi_cog_sample_step", "ftmi_cog_sample_finish", "ftmi_cog_sample_workspace_bytes", "ftmi_cog_sample")
CONFIGS = [None, {"snr_shift_scale": 1.0, "rescale_betas_zero_snr": False}, {"snr_shift_scale": 1.0}, {"rescale_betas_zero_snr": False}]


def _tables(cfg):
    from finetrainers_amd.cogvideox import CogVideoXDDIMTables
    from finetrainers_amd.cogvideox.sampler import COG_SCHEDULER_CONFIG

    c = dict(COG_SCHEDULER_CONFIG, **(cfg or {}))
    return CogVideoXDDIMTables(snr_shift_scale=c["snr_shift_scale"], rescale_betas_zero_snr=c["rescale_betas_zero_snr"])


def _full(cfg):
    from finetrainers_amd.cogvideox.sampler import COG_SCHEDULER_CONFIG

    return None if cfg is None else dict(COG_SCHEDULER_CONFIG, **cfg)


# ---- the schedule and the folded step ------------------------------------------------------------------------------------------------------------------------
def test_timesteps_are_the_trailing_ones_and_prev_is_upstreams():
    from finetrainers_amd.cogvideox import cog_ddim_tables
    from finetrainers_amd.cogvideox.sampler import cog_ddim_schedule

    ts, coef = cog_ddim_tables(50)
    assert ts.dtype == torch.int64 and coef.dtype == torch.float32 and coef.shape == (50, 2)
    assert ts.tolist() == list(range(999, 0, -20)) and ts.tolist()[-1] == 19
    t3, p3, a_t, a_prev = cog_ddim_schedule(3)
    assert t3 == [999, 666, 332] and p3 == [666, 333, -1], "prev is t - N // n, not the next timestep"
    ac = _tables(None).alphas_cumprod.double()
    assert float(a_prev[0]) == float(ac[666]) and float(a_prev[1]) == float(ac[333]) and float(a_t[2]) == float(ac[332])
    assert float(a_prev[2]) == 1.0, "the last step uses final_alpha_cumprod = 1 (set_alpha_to_one)"
    for n in (1, 4, 50):
        assert float(cog_ddim_schedule(n)[3][-1]) == 1.0


@pytest.mark.parametrize("n", [1, 3, 4, 50])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_coefficients_match_the_literal_step_and_the_rotation(n, cfg):
    """coef (fp64, before the fp32 rounding) against a literal transcription of the a / b formulas applied to the basis vectors, and against
    cx = cos(theta_t - theta_prev), cv = -sin(theta_t - theta_prev) with theta = atan2(sqrt(1 - ab), sqrt(ab)); cx^2 + cv^2 = 1."""
    from finetrainers_amd.cogvideox import cog_ddim_tables
    from finetrainers_amd.cogvideox.sampler import cog_ddim_coefficients_f64

    ts, coef = cog_ddim_coefficients_f64(n, _full(cfg))
    sched = ref.ddim_schedule(n, _tables(cfg).alphas_cumprod)
    assert ts.tolist() == [s[0] for s in sched] and coef.dtype == torch.float64 and bool(torch.isfinite(coef).all())
    for i, (_, a_t, a_prev) in enumerate(sched):
        cx, cv = float(coef[i, 0]), float(coef[i, 1])
        assert abs(cx - ref.ddim_step(1.0, 0.0, a_t, a_prev)) < 1e-12 and abs(cv - ref.ddim_step(0.0, 1.0, a_t, a_prev)) < 1e-12
        th = lambda a: math.atan2(math.sqrt(1 - a), math.sqrt(a))
        d = th(a_t) - th(a_prev)
        assert abs(cx - math.cos(d)) < 1e-12 and abs(cv + math.sin(d)) < 1e-12
        assert abs(cx * cx + cv * cv - 1.0) < 1e-12
    t32, c32 = cog_ddim_tables(n, _full(cfg))
    assert torch.equal(t32, ts) and torch.equal(c32, coef.float())


def test_zero_snr_first_step_from_pure_noise_is_minus_v():
    from finetrainers_amd.cogvideox import cog_ddim_tables

    _, coef = cog_ddim_tables(1)
    assert coef.tolist() == [[0.0, -1.0]], "alpha_bar_999 = 0 with the zero-SNR rescale, alpha_bar_prev = 1: x <- -v exactly"


def test_tables_refuse_what_is_not_restated():
    from finetrainers_amd.cogvideox import cog_ddim_tables

    with pytest.raises(ValueError, match="between 1 and 1000 steps"):
        cog_ddim_tables(0)
    with pytest.raises(NotImplementedError, match="CogVideoXDPMScheduler is a multistep solver"):
        cog_ddim_tables(4, {"_class_name": "CogVideoXDPMScheduler"})
    with pytest.raises(NotImplementedError, match="trailing"):
        cog_ddim_tables(4, {"timestep_spacing": "leading"})
    with pytest.raises(NotImplementedError, match="v_prediction"):
        cog_ddim_tables(4, {"prediction_type": "epsilon"})


# ---- the torch restatement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_,H,W,pt", [(1, 2, 2, 1), (3, 4, 6, 1), (2, 4, 8, 2)])
def test_reference_layout_round_trips_and_orders_columns_as_the_patch_embedding(F_, H, W, pt):
    from finetrainers_amd.cogvideox.model import patches_3d

    lat = torch.randn(2, F_, 16, H, W, generator=torch.Generator().manual_seed(F_ + W))
    x, cols = ref.init_ref(lat, 2, pt, P=2)
    S, Kc = (F_ // pt) * (H // 2) * (W // 2), 64 * pt
    assert x.shape == (2, S, Kc) and cols.shape == (2 * 2 * S, Kc)
    assert torch.equal(x, patches_3d(lat, 2, pt)) and torch.equal(ref.unpatchify(x, F_, 16, H, W, 2, pt), lat)
    assert torch.equal(cols[:2 * S], cols[2 * S:]) and torch.equal(cols[:2 * S], x.reshape(-1, Kc).to(bf16))
    assert torch.equal(ref.finish_ref(x, 1.0, F_, 16, H, W, 2, pt).float(), lat)
    if pt == 2:
        assert torch.equal(ref.finish_ref(x, 0.5, F_, 16, H, W, 2, pt, drop=1).float(), 0.5 * lat[:, 1:])
        assert float(x[0, 0, 9]) == float(lat[0, 0, 1, 0, 1]) and float(x[0, 0, 12]) == float(lat[0, 1, 1, 0, 0])  # column ((c pt + dt) p + dy) p + dx
    else:
        assert float(x[0, 0, 5]) == float(lat[0, 0, 1, 0, 1]) and float(x[0, 0, 6]) == float(lat[0, 0, 1, 1, 0])


def test_reference_trajectory_with_a_linear_model_is_the_product_of_the_step_maps():
    """A stand-in model v = M x that mixes the two latent channels with a 2 x 2 matrix M: every step is x <- (cx I + cv M) x on the channel pair, so the
    trajectory is the product of those 2 x 2 maps -- the literal scheduler step of the helper against the folded table of the sampler module."""
    from finetrainers_amd.cogvideox.sampler import cog_ddim_coefficients_f64

    M = torch.tensor([[0.3, -0.7], [0.5, 0.2]], dtype=torch.float64)
    fn = lambda hidden_states, encoder_hidden_states, timestep, image_rotary_emb, return_dict: (torch.einsum("ij,bfjhw->bfihw", M, hidden_states),)
    lat = torch.randn(1, 2, 2, 4, 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    text = torch.zeros(1, 2, 8, dtype=torch.float64)
    for n in (3, 4):
        sched = ref.ddim_schedule(n, _tables(None).alphas_cumprod)
        got = ref.trajectory(fn, torch.float64, lat, text, text, sched, 6.0, round_state=False)
        _, coef = cog_ddim_coefficients_f64(n)
        total = torch.eye(2, dtype=torch.float64)
        for cx, cv in coef.tolist():
            total = (cx * torch.eye(2, dtype=torch.float64) + cv * M) @ total
        want = torch.einsum("ij,bfjhw->bfihw", total, lat)
        assert torch.allclose(got, want, rtol=0, atol=1e-12 * float(want.abs().max()))
        assert float((got - lat).norm() / lat.norm()) > 0.1


def test_reference_step_combines_unconditional_rows_first():
    x = torch.zeros(1, 2, 64)
    u, c = torch.full((1, 2, 64), 1.0), torch.full((1, 2, 64), 3.0)
    out = ref.step_ref(torch.cat([u, c]).to(bf16), x, 0.5, -0.25, 6.0)
    assert torch.equal(out, torch.full((1, 2, 64), -0.25 * (1.0 + 6.0 * 2.0), dtype=torch.float64))
    assert torch.equal(ref.step_ref(c.to(bf16), x, 0.5, -0.25, 1.0), torch.full((1, 2, 64), -0.75, dtype=torch.float64))


# ---- what the sampler refuses ----------------------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel

    cfg = dict(num_layers=1, num_attention_heads=2, text_embed_dim=64, **ref.SMALL)
    cfg.update(kw)
    return MI355XCogVideoXTransformer3DModel(CogVideoXTransformerConfig(**cfg), device=torch.device("cpu"))


def _embeds(B=1, T=16):
    return torch.zeros(B, T, 64, dtype=bf16)


def test_sampler_refusals_name_their_reason():
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    noise = torch.zeros(1, 2, 16, 8, 12)
    s = MI355XCogVideoXLatentSampler(_model())
    with pytest.raises(ValueError, match="guidance_scale != 1 needs negative_prompt_embeds"):
        s.sample(noise, _embeds())
    with pytest.raises(ValueError, match="shaped like prompt_embeds"):
        s.sample(noise, _embeds(), _embeds(B=2))
    with pytest.raises(ValueError, match="expects 16 text tokens"):
        s.sample(noise, _embeds(T=8), _embeds(T=8))
    with pytest.raises(ValueError, match="prompt_embeds must be"):
        s.sample(noise, torch.zeros(1, 16, 32), guidance_scale=1.0)
    with pytest.raises(ValueError, match="latents must be"):
        s.sample(torch.zeros(1, 2, 8, 8, 12), _embeds(), _embeds())
    with pytest.raises(ValueError, match="multiples of patch_size"):
        s.sample(torch.zeros(1, 2, 16, 7, 12), _embeds(), _embeds())
    with pytest.raises(ValueError, match="drop_frames"):
        s.sample(noise, _embeds(), _embeds(), drop_frames=1)
    with pytest.raises(NotImplementedError, match="use_dynamic_cfg"):
        s.sample(noise, _embeds(), _embeds(), use_dynamic_cfg=True)
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):
        s.sample(noise, _embeds(), _embeds())
    with pytest.raises(NotImplementedError, match="CogVideoXDPMScheduler"):
        MI355XCogVideoXLatentSampler(_model(), {"_class_name": "CogVideoXDPMScheduler"}).sample(noise, _embeds(), _embeds())

    v15 = MI355XCogVideoXLatentSampler(_model(patch_size_t=2, use_rotary_positional_embeddings=True, patch_bias=False))
    with pytest.raises(ValueError, match="multiple of patch_size_t = 2"):
        v15.sample(torch.zeros(1, 3, 16, 8, 12), _embeds(), _embeds())
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):  # a padded clip with its one leading frame to drop passes every input check
        v15.sample(torch.zeros(1, 4, 16, 8, 12), _embeds(), _embeds(), drop_frames=1)
    with pytest.raises(NotImplementedError, match="ofs embedding or in_channels != out_channels"):
        MI355XCogVideoXLatentSampler(_model(patch_size_t=2, use_rotary_positional_embeddings=True, ofs_embed_dim=512)).sample(noise, _embeds(), _embeds())
    with pytest.raises(NotImplementedError, match="ofs embedding or in_channels != out_channels"):
        MI355XCogVideoXLatentSampler(_model(in_channels=32)).sample(torch.zeros(1, 2, 32, 8, 12), _embeds(), _embeds())


def test_specification_gains_validation_latents_and_keeps_the_inherited_validation():
    from finetrainers_amd.cogvideox import MI355XCogVideoXModelSpecification

    cls = MI355XCogVideoXModelSpecification
    assert callable(getattr(cls, "validation_latents"))
    assert all("validation" not in vars(b) for b in cls.__mro__ if b.__module__.startswith("finetrainers_amd.cogvideox"))
    spec = cls(pretrained_model_name_or_path=None)
    with pytest.raises(ValueError, match="guidance_scale != 1 needs negative_prompt_embeds"):
        spec.validation_latents(_model(), _embeds(), None, 2, 8, 12, latents=torch.zeros(1, 2, 16, 8, 12))
    v15 = _model(patch_size_t=2, use_rotary_positional_embeddings=True, patch_bias=False)
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):  # 3 frames -> 4 drawn, 1 dropped: the inputs pass, the unloaded model does not
        spec.validation_latents(v15, _embeds(), _embeds(), 3, 8, 12, generator=torch.Generator().manual_seed(0))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------------------------
def _geo(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, C=16, F=2, H=8, W=12, p=2, pt=1, P=2, drop=0)
    base.update(kw)
    return _lib.CogSampleGeometry(**base)


def test_c_abi_declares_exports_and_binds_the_sampling_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name


def test_layout_kernels_check_their_arguments_before_any_launch():
    from finetrainers_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    step = lambda geo, pred=p, x=p, cols=p, g=6.0, coef=p: lib.ftmi_cog_sample_step(ctypes.byref(geo), pred, x, coef, 0, g, cols, None)
    bad = [(dict(C=15), _lib.FTMI_ERR_UNSUPPORTED, "multiple of 8"), (dict(W=13), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(H=7), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"), (dict(pt=2, F=3), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
           (dict(pt=3, F=3), _lib.FTMI_ERR_UNSUPPORTED, "patch_size_t is 1 or 2"), (dict(P=3), _lib.FTMI_ERR_INVALID, "P is 2"),
           (dict(drop=1), _lib.FTMI_ERR_INVALID, "drop"), (dict(pt=2, drop=2), _lib.FTMI_ERR_INVALID, "drop"), (dict(B=0), _lib.FTMI_ERR_INVALID, "positive")]
    for kw, code, msg in bad:
        assert step(_geo(**kw)) == code and msg in _lib.last_error(), (kw, _lib.last_error())
    assert step(_geo(), pred=ctypes.c_void_p(264)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), x=ctypes.c_void_p(260)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(_geo(), g=1.0) == _lib.FTMI_ERR_INVALID and "guidance" in _lib.last_error()
    assert step(_geo(), coef=None) == _lib.FTMI_ERR_INVALID and "coefficient table" in _lib.last_error()
    assert step(_geo(), pred=None, cols=None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_cog_sample_init(ctypes.byref(_geo(W=13)), p, p, p, None) == _lib.FTMI_ERR_UNSUPPORTED
    assert lib.ftmi_cog_sample_init(ctypes.byref(_geo()), p, p, ctypes.c_void_p(258), None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_cog_sample_init(ctypes.byref(_geo()), None, p, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_cog_sample_finish(ctypes.byref(_geo(pt=2, drop=2)), p, 1.0, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_cog_sample_finish(ctypes.byref(_geo()), None, 1.0, p, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_cog_sample_finish(ctypes.byref(_geo()), p, 1.0, ctypes.c_void_p(264), None) == _lib.FTMI_ERR_INVALID


def _cfg(L=2, guidance=6.0, **kw):
    from finetrainers_amd import _lib

    base = dict(geo=_geo(P=2 if guidance != 1.0 else 1), T=16, D_text=64, D=256, heads=4, L=L, D_ff=1024, D_temb=512, r=64, lora_scale=1.0, eps_norm=1e-5,
                eps_qk=1e-6, gemm_variant=8, steps=3, guidance=guidance)
    base.update(kw)
    return _lib.CogSampleConfig(**base)


def _train_cfg(L):
    from finetrainers_amd import _lib

    return _lib.CogConfig(B=2, T=16, S=48, D=256, H=4, L=L, D_ff=1024, D_temb=512, r=64, lora_scale=1.0, eps_norm=1e-5, eps_qk=1e-6, gemm_variant=8)


def test_workspace_plan_is_forward_only():
    """The plan grows with L only through the modulation GEMM's output [P B, L, 2, 6 D] and the tables [L, 2, 3, P B, 2, D] (bf16, each entry rounded to 256
    bytes); it is below the training workspace at the same shape from L = 2 on; without guidance (conditional rows only) it needs less; nothing per step."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    ws = lambda **kw: lib.ftmi_cog_sample_workspace_bytes(ctypes.byref(_cfg(**kw)))
    r256 = lambda n: (n + 255) // 256 * 256
    rows, D = 2, 256
    mod = lambda L: r256(rows * L * 2 * 6 * D * 2) + r256(L * 2 * 3 * rows * 2 * D * 2)
    assert ws(L=2) > 0 and ws(L=4) - ws(L=2) == mod(4) - mod(2) == 2 * (rows * 2 * 6 * D * 2 + 2 * 3 * rows * 2 * D * 2)
    assert ws(L=30) - ws(L=2) == mod(30) - mod(2)
    for L in (2, 4, 30):
        train = lib.ftmi_cog_workspace_bytes(ctypes.byref(_train_cfg(L)))
        assert 0 < ws(L=L) < train, (L, ws(L=L), train)
    assert ws(L=30) < lib.ftmi_cog_workspace_bytes(ctypes.byref(_train_cfg(30))) // 8
    assert ws(guidance=1.0) < ws(guidance=6.0)
    assert ws(steps=50) == ws(steps=3), "nothing is kept per step"
    assert ws(r=0) > 0
    # refused configurations plan 0 bytes, with the reason in ftmi_last_error
    for kw, msg in ((dict(r=32), "LoRA rank"), (dict(steps=0), "positive"), (dict(geo=_geo(P=1)), "P is 2"), (dict(heads=3), "heads x 64"),
                    (dict(geo=_geo(C=8)), "multiples of 64"), (dict(geo=_geo(W=13)), "whole patches"), (dict(D_text=100), "multiples of 64")):
        assert ws(**kw) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())


def test_sample_refuses_a_small_workspace_and_missing_weights():
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg = _cfg()
    need = lib.ftmi_cog_sample_workspace_bytes(ctypes.byref(cfg))
    p = ctypes.c_void_p(256)
    w = _lib.CogSampleWeights()
    call = lambda nbytes, ws=p: lib.ftmi_cog_sample(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, p, ws, nbytes, None)
    assert call(need - 1) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert call(need, ctypes.c_void_p(264)) == _lib.FTMI_ERR_INVALID and "256-byte aligned" in _lib.last_error()
    assert call(need) == _lib.FTMI_ERR_INVALID and "weights missing" in _lib.last_error()
    for f in _lib.COG_SAMPLE_WEIGHT_FIELDS:
        if f != "pos":
            setattr(w, f, 256)
    w.blocks.mod_w = w.blocks.w_qkv = 256
    assert call(need) == _lib.FTMI_ERR_INVALID and "working copies" in _lib.last_error()
    w.blocks.lora_a_sp = w.blocks.lora_b_ext = 256
    assert call(need) == _lib.FTMI_ERR_INVALID and "one of the two" in _lib.last_error()  # neither the sincos table nor the rotary tables
    w.blocks.rope_cos = 256
    assert call(need) == _lib.FTMI_ERR_INVALID and "come as a pair" in _lib.last_error()
    assert lib.ftmi_cog_sample(ctypes.byref(cfg), ctypes.byref(w), None, p, p, p, p, p, p, p, need, None) == _lib.FTMI_ERR_INVALID
