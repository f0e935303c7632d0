"""The DPM multistep scheduler of CogVideoX validation sampling, the parts that need no GPU: the folded rows of finetrainers_amd/cogvideox/sampler.py against the
stepwise restatement of tests/cog_dpm_reference.py, the structure of the rows at the infinities, the order of the noise draws, the dynamic-CFG table, every
refusal, the ABI of the multistep entry points and the specification's choice of scheduler."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import cog_dpm_reference as dref
import cog_sampling_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ftmi_cog_sample_step_dpm", "ftmi_cog_sample_pack", "ftmi_cog_sample_ms_workspace_bytes", "ftmi_cog_sample_ms")
f64 = torch.float64
bf16 = torch.bfloat16


def _config(zero_snr=True, shift=1.0, **kw):
    from finetrainers_amd.cogvideox import COG_DPM_SCHEDULER_CONFIG

    return dict(COG_DPM_SCHEDULER_CONFIG, rescale_betas_zero_snr=zero_snr, snr_shift_scale=shift, **kw)


def _alphas(zero_snr, shift):
    from finetrainers_amd.cogvideox import CogVideoXDDIMTables

    return CogVideoXDDIMTables(snr_shift_scale=shift, rescale_betas_zero_snr=zero_snr).alphas_cumprod


def _apply(row, x, v, old, z):
    """One folded fp64 row: -> (x', x0).  A zero coefficient leaves its term out, as the kernel does."""
    sa, sb, m0, e0, e1, mn = row[:6].tolist()
    x0 = sa * x - sb * v
    out = m0 * x + e0 * x0
    if e1 != 0.0:
        out = out + e1 * old
    if mn != 0.0:
        out = out + mn * z
    return out, x0


# ---- the folded rows ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1.0, 3.0])
@pytest.mark.parametrize("zero_snr", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 50, 1000])
def test_rows_reproduce_the_stepwise_scheduler(n, zero_snr, shift):
    """The folded fp64 rows over random fp64 (x, v_i, z_i) give the stepwise scheduler's whole trajectory to 1e-12 relative, every row is finite, and the
    fp32 table is the fp64 one rounded once.  ``old`` starts as NaN on both sides: nothing may read it before a step wrote it."""
    from finetrainers_amd.cogvideox import cog_dpm_coefficients_f64, cog_dpm_tables

    ts, rows = cog_dpm_coefficients_f64(n, _config(zero_snr, shift))
    assert rows.dtype == f64 and rows.shape == (n, 8) and bool(torch.isfinite(rows).all())
    ts32, rows32 = cog_dpm_tables(n, _config(zero_snr, shift))
    assert rows32.dtype == torch.float32 and torch.equal(rows32, rows.float()) and torch.equal(ts32, ts)
    sched = dref.dpm_schedule(n, _alphas(zero_snr, shift))
    assert ts.tolist() == [s[0] for s in sched]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(64, dtype=f64, generator=g)
    xs, old_s, xf, old_f = x.clone(), None, x.clone(), torch.full((64,), float("nan"), dtype=f64)
    for i, (t, prev, a_t, a_prev, a_back) in enumerate(sched):
        v, z = torch.randn(64, dtype=f64, generator=g), torch.randn(64, dtype=f64, generator=g)
        xs, old_s = dref.dpm_step(xs, v, old_s, z, prev, a_t, a_prev, a_back)
        xf, old_f = _apply(rows[i], xf, v, old_f, z)
        scale = float(xs.abs().max())
        assert float((xf - xs).abs().max()) <= 1e-12 * scale, (i, float((xf - xs).abs().max()) / scale)
        assert float((old_f - old_s).abs().max()) <= 1e-12 * max(float(old_s.abs().max()), 1e-300), i
    assert bool((rows[:, 6] == 6.0).all()) and bool((rows[:, 7] == 0.0).all())


@pytest.mark.parametrize("shift", [1.0, 3.0])
@pytest.mark.parametrize("zero_snr", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 50, 1000])
def test_rows_have_the_structure_the_loop_relies_on(n, zero_snr, shift):
    from finetrainers_amd.cogvideox import cog_dpm_coefficients_f64
    from finetrainers_amd.cogvideox.sampler import cog_ddim_schedule

    _, rows = cog_dpm_coefficients_f64(n, _config(zero_snr, shift))
    _, prev, a_t, a_prev = cog_ddim_schedule(n, dict(_config(zero_snr, shift), _class_name="CogVideoXDDIMScheduler"))
    assert float(rows[0, 4]) == 0.0, "row 0 has no history"
    if prev[-1] < 0:
        want = torch.tensor([float(a_t[-1].sqrt()), float((1 - a_t[-1]).sqrt()), 0.0, 1.0, 0.0, 0.0], dtype=f64)
        assert torch.allclose(rows[-1, :6], want, rtol=0, atol=1e-15), "the last step returns x0, with no noise"
        assert float(rows[-1, 5]) == 0.0 and float(rows[-1, 2]) == 0.0 and float(rows[-1, 4]) == 0.0
    for i in range(n):
        single = i == 0 or prev[i] < 0
        assert (float(rows[i, 4]) == 0.0) == (single or (zero_snr and i == 1)), i
        if not (prev[i] < 0):
            assert float(rows[i, 5]) > 0.0, "every step whose target is not the clean sample adds noise"
    if zero_snr:
        want = torch.tensor([0.0, 1.0, 0.0, float(a_prev[0].sqrt()), 0.0, float((1 - a_prev[0]).sqrt())], dtype=f64)
        assert torch.allclose(rows[0, :6], want, rtol=0, atol=1e-15) and float(rows[0, 0]) == 0.0 and float(rows[0, 2]) == 0.0
        if n > 1:
            assert float(rows[1, 4]) == 0.0, "r = inf: the history first enters at step 2"


def test_the_quoted_rows_at_four_steps():
    from finetrainers_amd.cogvideox import cog_dpm_coefficients_f64

    _, on = cog_dpm_coefficients_f64(4, _config(True, 3.0))
    assert torch.allclose(on[:, 4], torch.tensor([0.0, 0.0, -0.20779, 0.0], dtype=f64), rtol=0, atol=1e-5)
    assert math.copysign(1.0, float(on[1, 4])) == -1.0, "mult1 / inf keeps mult1's sign: -0"
    assert torch.allclose(on[:, 5], torch.tensor([0.99450, 0.89978, 0.71299, 0.0], dtype=f64), rtol=0, atol=1e-5)
    _, off = cog_dpm_coefficients_f64(4, _config(False, 3.0))
    assert torch.allclose(off[1, :6], torch.tensor([0.14005, 0.99014, 0.37573, 0.38791, -0.10351, 0.86488], dtype=f64), rtol=0, atol=1e-5)
    assert torch.allclose(off[2, :6], torch.tensor([0.33702, 0.94150, 0.35077, 0.75902, -0.23727, 0.69381], dtype=f64), rtol=0, atol=1e-5)


def test_default_config_is_the_5b_checkpoints():
    from finetrainers_amd.cogvideox import COG_DPM_SCHEDULER_CONFIG, COG_SCHEDULER_CONFIG, cog_dpm_coefficients_f64

    c = COG_DPM_SCHEDULER_CONFIG
    assert c["_class_name"] == "CogVideoXDPMScheduler" and c["snr_shift_scale"] == 1.0 and c["rescale_betas_zero_snr"] is True
    for k in ("num_train_timesteps", "beta_start", "beta_end", "timestep_spacing", "prediction_type", "set_alpha_to_one"):
        assert c[k] == COG_SCHEDULER_CONFIG[k], k
    assert torch.equal(cog_dpm_coefficients_f64(5)[1], cog_dpm_coefficients_f64(5, dict(c))[1])


def test_each_table_folds_its_own_scheduler_only():
    from finetrainers_amd.cogvideox import COG_SCHEDULER_CONFIG, cog_ddim_tables, cog_dpm_tables

    with pytest.raises(NotImplementedError, match="CogVideoXDDIMScheduler is not the multistep solver"):
        cog_dpm_tables(4, COG_SCHEDULER_CONFIG)
    with pytest.raises(NotImplementedError, match="CogVideoXDPMScheduler is a multistep solver"):
        cog_ddim_tables(4, _config())


# ---- the noise ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 7])
def test_step_noise_is_the_pipelines_sequence_of_draws(n):
    """One draw per step, a second one on a multistep row (i > 0 and prev >= 0) with the second kept; the last step draws too, though its row (prev < 0 at
    n = 1 and 4) never uses the draw: the generator ends where the pipeline's ends.  n = 7: the last step has prev = 0, a multistep row with noise."""
    from finetrainers_amd.cogvideox import cog_dpm_step_noise
    from finetrainers_amd.cogvideox.sampler import cog_ddim_schedule

    _, prev, _, _ = cog_ddim_schedule(n)
    assert (prev[-1] < 0) == (n != 7)
    shape = (2, 3, 4, 2, 2)
    got = cog_dpm_step_noise(shape, n, prev, torch.Generator().manual_seed(11), "cpu")
    assert got.dtype == torch.float32 and got.shape == (n,) + shape
    g = torch.Generator().manual_seed(11)
    for i in range(n):
        z = torch.randn(shape, generator=g, dtype=bf16)
        if i > 0 and prev[i] >= 0:
            z = torch.randn(shape, generator=g, dtype=bf16)
        assert torch.equal(got[i], z.float()), i
    g2 = torch.Generator().manual_seed(11)
    cog_dpm_step_noise(shape, n, prev, g2, "cpu")
    assert torch.equal(g.get_state(), g2.get_state())
    assert cog_dpm_step_noise(shape, n, prev, torch.Generator().manual_seed(11), "cpu", dtype=torch.float32).dtype == torch.float32


# ---- guidance per step ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 50])
def test_dynamic_cfg_table_is_the_formula(n):
    from finetrainers_amd.cogvideox import cog_dpm_coefficients_f64, cog_guidance_table

    ts, rows = cog_dpm_coefficients_f64(n, _config(), 6.0, True)
    want = [1 + 6.0 * ((1 - math.cos(math.pi * ((n - t) / n) ** 5.0)) / 2) for t in ts.tolist()]
    assert rows[:, 6].tolist() == pytest.approx(want, rel=1e-15) and want == pytest.approx([dref.dynamic_cfg(6.0, n, t) for t in ts.tolist()], rel=1e-15)
    assert all(1.0 <= w <= 7.0 for w in want) and len(set(want)) > 1
    assert cog_guidance_table(n, ts.tolist(), 6.0, False) == [6.0] * n
    _, const = cog_dpm_coefficients_f64(n, _config(), 6.0, False)
    assert torch.equal(const[:, :6], rows[:, :6]), "the scale does not touch the solver's numbers"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_scheduler_settings_are_refused_by_name():
    from finetrainers_amd.cogvideox import cog_dpm_tables

    with pytest.raises(NotImplementedError, match="v_prediction"):
        cog_dpm_tables(4, _config(prediction_type="epsilon"))
    with pytest.raises(NotImplementedError, match="trailing"):
        cog_dpm_tables(4, _config(timestep_spacing="leading"))
    with pytest.raises(NotImplementedError, match="set_alpha_to_one"):
        cog_dpm_tables(4, _config(set_alpha_to_one=False))
    with pytest.raises(ValueError, match="between 1 and 1000 steps"):
        cog_dpm_tables(0, _config())
    with pytest.raises(ValueError, match="guidance_scale = 1"):
        cog_dpm_tables(4, _config(), 1.0, True)


def _model(**kw):
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel

    cfg = dict(num_layers=1, num_attention_heads=2, text_embed_dim=64, **ref.SMALL)
    cfg.update(kw)
    return MI355XCogVideoXTransformer3DModel(CogVideoXTransformerConfig(**cfg), device=torch.device("cpu"))


def test_sampler_refusals_of_the_multistep_path():
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    noise, emb = torch.zeros(1, 2, 16, 8, 12), torch.zeros(1, 16, 64, dtype=bf16)
    s = MI355XCogVideoXLatentSampler(_model(), _config())
    with pytest.raises(ValueError, match="pass generator .* or step_noise") as e:
        s.sample(noise, emb, emb)
    assert isinstance(e.value, NotImplementedError), "what this call raised before the scheduler was restated: callers that catch it still do"
    with pytest.raises(ValueError, match="use_dynamic_cfg"):
        s.sample(noise, emb, guidance_scale=1.0, use_dynamic_cfg=True, generator=torch.Generator())
    with pytest.raises(NotImplementedError, match="use_dynamic_cfg .* CogVideoXDDIMScheduler"):  # the DDIM loop takes one scale per call
        MI355XCogVideoXLatentSampler(_model()).sample(noise, emb, emb, use_dynamic_cfg=True)
    # with its noise source named, a DPM run passes every input check, with dynamic CFG too (the model here has no weights loaded)
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):
        s.sample(noise, emb, emb, generator=torch.Generator())
    with pytest.raises(RuntimeError, match="load_diffusers_state_dict first"):
        s.sample(noise, emb, emb, use_dynamic_cfg=True, step_noise=torch.zeros(4, 1, 2, 16, 8, 12))
    i2v = MI355XCogVideoXLatentSampler(_model(in_channels=32, use_rotary_positional_embeddings=True), _config())
    with pytest.raises(NotImplementedError, match="text-to-video only"):
        i2v.sample(torch.zeros(1, 2, 32, 8, 12), emb, emb, generator=torch.Generator())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------------------
def _geo(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, C=16, F=2, H=4, W=6, p=2, pt=1, P=2, drop=0)
    base.update(kw)
    return _lib.CogSampleGeometry(**base)


def _cfg(solver=1, guidance=6.0, **kw):
    from finetrainers_amd import _lib

    geo = _geo(**{k: kw.pop(k) for k in list(kw) if k in ("B", "C", "F", "H", "W", "p", "pt", "P", "drop")})
    base = dict(geo=geo, T=16, D_text=64, D=1920, heads=30, L=2, D_ff=7680, D_temb=512, r=64, lora_scale=1.0, eps_norm=1e-5, eps_qk=1e-6, gemm_variant=8,
                steps=4, guidance=guidance)
    base.update(kw)
    return _lib.CogSampleMsConfig(base=_lib.CogSampleConfig(**base), solver=solver)


def test_c_abi_declares_exports_and_binds_the_multistep_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "ftmi355.h")) as f:
        declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", f.read()))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name


def test_ms_config_has_the_ddim_config_as_its_prefix():
    from finetrainers_amd import _lib

    assert ctypes.sizeof(_lib.CogSampleConfig) == 9 * 4 + 14 * 4, "ftmi_cog_sample_config keeps its size: 9 geometry ints and 14 four-byte fields"
    assert _lib.CogSampleMsConfig.base.offset == 0 and _lib.CogSampleMsConfig.solver.offset == ctypes.sizeof(_lib.CogSampleConfig)
    assert ctypes.sizeof(_lib.CogSampleMsConfig) == ctypes.sizeof(_lib.CogSampleConfig) + 4
    assert [n for n, _ in _lib.CogSampleConfig._fields_][-2:] == ["steps", "guidance"]


def test_ms_workspace_is_the_ddim_workspace_plus_one_state_buffer():
    from finetrainers_amd import _lib

    lib = _lib.load()
    for kw in (dict(), dict(B=2), dict(pt=2, F=4), dict(P=1, guidance=1.0)):
        cfg = _cfg(**kw)
        g = cfg.base.geo
        state = g.B * (g.F // g.pt) * (g.H // 2) * (g.W // 2) * g.C * g.pt * 4 * 4
        base = int(lib.ftmi_cog_sample_workspace_bytes(ctypes.byref(cfg.base)))
        assert base > 0 and int(lib.ftmi_cog_sample_ms_workspace_bytes(ctypes.byref(cfg))) == base + (state + 255) // 256 * 256, kw
    for kw, msg in ((dict(solver=0), "solver"), (dict(solver=2), "solver"), (dict(steps=0), "positive"), (dict(W=5), "whole patches")):
        assert int(lib.ftmi_cog_sample_ms_workspace_bytes(ctypes.byref(_cfg(**kw)))) == 0 and msg in _lib.last_error(), (kw, _lib.last_error())


def test_ms_entry_points_check_their_arguments_before_any_launch():
    """Every refusal below returns before a kernel is launched: the pointers are made-up addresses."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p

    def step(geo=None, **kw):
        a = dict(pred=p(4096), x=p(8192), old=p(12288), noise=p(16384), row=p(20480), cols=p(24576))
        a.update(kw)
        return lib.ftmi_cog_sample_step_dpm(ctypes.byref(geo or _geo()), a["pred"], a["x"], a["old"], a["noise"], a["row"], a["cols"], None)

    for kw, code, msg in [(dict(C=15), _lib.FTMI_ERR_UNSUPPORTED, "multiple of 8"), (dict(W=5), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"),
                          (dict(pt=3, F=3), _lib.FTMI_ERR_UNSUPPORTED, "patch_size_t"), (dict(P=3), _lib.FTMI_ERR_INVALID, "P is 2"),
                          (dict(B=0), _lib.FTMI_ERR_INVALID, "positive")]:
        assert step(_geo(**kw)) == code and msg in _lib.last_error(), (kw, _lib.last_error())
    assert step(old=p(12292)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(noise=p(16388)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(old=p(8192)) == _lib.FTMI_ERR_INVALID and "three buffers" in _lib.last_error()
    assert step(noise=p(8192)) == _lib.FTMI_ERR_INVALID and "three buffers" in _lib.last_error()
    for missing in ("pred", "x", "old", "row"):
        assert step(**{missing: None}) == _lib.FTMI_ERR_INVALID, missing
    pack = lambda n, geo=None, src=p(4096), dst=p(8192): lib.ftmi_cog_sample_pack(ctypes.byref(geo or _geo()), src, n, dst, None)
    assert pack(0) == _lib.FTMI_ERR_INVALID and "positive" in _lib.last_error()
    assert pack(1, src=None) == _lib.FTMI_ERR_INVALID and pack(1, dst=None) == _lib.FTMI_ERR_INVALID
    assert pack(1, dst=p(8196)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert pack(1, _geo(W=5)) == _lib.FTMI_ERR_UNSUPPORTED and "whole patches" in _lib.last_error()
    # the loop: solver, workspace size, noise and noise_steps, all before the weights are looked at
    w = _lib.CogSampleWeights()
    cfg = _cfg()
    need = int(lib.ftmi_cog_sample_ms_workspace_bytes(ctypes.byref(cfg)))

    def call(c, ws_bytes, noise=p(28672), k=3, coef=p(20480)):
        return lib.ftmi_cog_sample_ms(ctypes.byref(c), ctypes.byref(w), p(24576), p(8192), p(256), p(512), p(768), p(1024), coef, noise, k, p(1 << 20), ws_bytes, None)

    assert call(_cfg(solver=2), need) == _lib.FTMI_ERR_UNSUPPORTED and "solver" in _lib.last_error()
    assert call(_cfg(solver=0), need) == _lib.FTMI_ERR_UNSUPPORTED and "solver" in _lib.last_error()
    assert call(cfg, need, k=5) == _lib.FTMI_ERR_INVALID and "noise_steps" in _lib.last_error()
    assert call(cfg, need, k=-1) == _lib.FTMI_ERR_INVALID and "noise_steps" in _lib.last_error()
    assert call(cfg, need, noise=None, k=3) == _lib.FTMI_ERR_INVALID and "noise goes with" in _lib.last_error()
    assert call(cfg, need, k=0) == _lib.FTMI_ERR_INVALID and "noise goes with" in _lib.last_error()
    assert call(cfg, need - 1) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert call(cfg, need, coef=None) == _lib.FTMI_ERR_INVALID
    assert call(cfg, need) == _lib.FTMI_ERR_INVALID and "weights missing" in _lib.last_error()
    assert call(cfg, need, noise=None, k=0) == _lib.FTMI_ERR_INVALID and "weights missing" in _lib.last_error()


# ---- which scheduler validation runs ----------------------------------------------------------------------------------------------------------------------------------
def test_validation_scheduler_config_is_the_checkpoints_or_the_geometrys_default(tmp_path):
    from finetrainers_amd.cogvideox import (COG_DPM_SCHEDULER_CONFIG, COG_SCHEDULER_CONFIG, CogVideoXTransformerConfig, MI355XCogVideoXModelSpecification,
                                            cog_dpm_tables)

    conf = dict(COG_DPM_SCHEDULER_CONFIG, _diffusers_version="0.33.0.dev0", snr_shift_scale=2.0)
    os.makedirs(tmp_path / "scheduler")
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(conf, f)
    spec = MI355XCogVideoXModelSpecification(pretrained_model_name_or_path=str(tmp_path))
    assert spec.validation_scheduler_config() == conf
    assert torch.equal(cog_dpm_tables(4, spec.validation_scheduler_config())[1], cog_dpm_tables(4, conf)[1])
    rotary = CogVideoXTransformerConfig(num_layers=1, use_rotary_positional_embeddings=True, **ref.SMALL)
    sincos = CogVideoXTransformerConfig(num_layers=1, **ref.SMALL)
    hub = lambda c: MI355XCogVideoXModelSpecification(pretrained_model_name_or_path="THUDM/CogVideoX1.5-5B", transformer_config=c)
    assert hub(rotary).validation_scheduler_config() == COG_DPM_SCHEDULER_CONFIG
    assert hub(sincos).validation_scheduler_config() == COG_SCHEDULER_CONFIG
    assert hub(None).validation_scheduler_config(_model(use_rotary_positional_embeddings=True)) == COG_DPM_SCHEDULER_CONFIG
    with pytest.raises(ValueError, match="no transformer config"):
        hub(None).validation_scheduler_config()
