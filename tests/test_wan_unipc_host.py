"""The UniPC multistep scheduler of Wan validation sampling, the parts that need no GPU: the schedule against its closed form, the folded tables of
finetrainers_amd/wan/sampler.py against the stepwise restatement of tests/wan_unipc_reference.py, the order-1 identity with Euler, the solver's accuracy on a
flow with a known endpoint, every refusal, the dispatch of the sampler, the ABI and the scheduler-config loading."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

import wan_unipc_reference as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ftmi_wan_sample_step_unipc", "ftmi_wan_sample_ms_workspace_bytes", "ftmi_wan_sample_ms")
UNIPC = {"_class_name": "UniPCMultistepScheduler"}
f64 = torch.float64


def _linear_model(seed):
    """v = a x + c with per-step, per-element random a, c in fp64: every history slot carries different values."""
    g = torch.Generator().manual_seed(seed)
    a, c = torch.randn(64, 5, dtype=f64, generator=g) * 0.5, torch.randn(64, 5, dtype=f64, generator=g)
    return lambda i, x: a[i % 64] * x + c[i % 64]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---- the folded tables --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disable", ["none", "first", "all"])
@pytest.mark.parametrize("solver_order", [1, 2])
@pytest.mark.parametrize("shift", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 50])
def test_tables_reproduce_the_stepwise_scheduler(n, shift, solver_order, disable):
    from finetrainers_amd.wan import wan_unipc_schedule, wan_unipc_tables

    skip = {"none": [], "first": [0], "all": list(range(n))}[disable]
    sig, _ = wan_unipc_schedule(n, dict(UNIPC, flow_shift=shift))
    table = wan_unipc_tables(sig, solver_order, skip, dtype=f64)
    assert table.shape == (n, 8) and table.dtype == f64 and bool(torch.isfinite(table).all())
    assert wan_unipc_tables(sig, solver_order, skip).dtype == torch.float32
    model = _linear_model(n + int(shift))
    x0 = torch.randn(5, dtype=f64, generator=torch.Generator().manual_seed(1))
    want, solver = uref.run_stepwise(model, x0, sig.tolist(), solver_order, skip)
    got = uref.run_folded(model, x0, sig.tolist(), table)
    assert _rel(got, want) <= 1e-12, _rel(got, want)
    # the orders the stepwise scheduler ran with, exactly, and the rows the corrector skipped
    assert solver.orders == [min(solver_order, n - i, i + 1) for i in range(n)]
    if solver_order == 2 and n >= 3:
        assert solver.orders == [1] + [2] * (n - 2) + [1]
    for i in range(n):
        cx, cl, c1, c2, ct, px, p0, p1 = table[i].tolist()
        runs = i >= 1 and (i - 1) not in skip
        assert solver.corrected[i] == runs
        if runs:
            assert cx == 0.0 and cl != 0.0 and c1 != 0.0 and ct != 0.0
            assert (c2 != 0.0) == (solver.orders[i - 1] == 2)
        else:
            assert (cx, cl, c1, c2, ct) == (1.0, 0.0, 0.0, 0.0, 0.0)
        assert (p1 != 0.0) == (solver.orders[i] == 2)
    assert table[-1, 5:].tolist() == [0.0, 1.0, 0.0], "the last step lands on its data prediction"


def test_tables_refuse_a_table_they_cannot_fold():
    from finetrainers_amd.wan import wan_unipc_tables

    with pytest.raises(ValueError, match="n \\+ 1 values"):
        wan_unipc_tables([0.0])
    with pytest.raises(ValueError, match="decrease strictly"):
        wan_unipc_tables([1.0, 0.5, 0.0])  # lambda(1) = -inf
    with pytest.raises(ValueError, match="decrease strictly"):
        wan_unipc_tables([0.9, 0.5, 0.1])
    with pytest.raises(NotImplementedError, match="solver_order"):
        wan_unipc_tables([0.9, 0.5, 0.0], solver_order=3)


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("n", [1, 4, 50])
def test_schedule_is_the_closed_form(n, shift):
    from finetrainers_amd.wan import wan_unipc_schedule

    sig, ts = wan_unipc_schedule(n, dict(UNIPC, flow_shift=shift))
    f = lambda s: shift * s / (1 + (shift - 1) * s)
    assert sig.dtype == f64 and sig.shape == (n + 1,) and ts.shape == (n,)
    # two fp64 operation orders of values <= 1 (the scheduler's 1 - linspace against the closed form): a handful of roundings of 2^-53 each, absolute
    assert torch.allclose(sig, torch.tensor(uref.flow_sigmas(n, shift), dtype=f64), rtol=0, atol=1e-15)
    assert abs(float(sig[0]) - f(0.999)) < 1e-15 and float(sig[-1]) == 0.0
    assert bool((sig[1:] < sig[:-1]).all())
    assert torch.equal(ts, torch.floor(sig[:-1] * 1000)) and bool((ts == ts.round()).all())
    if shift == 3.0:
        assert float(ts[0]) == 999.0  # sigma_0 N = 999.67: truncated, not rounded
    if shift == 1.0:
        assert float(ts[0]) == 999.0 and abs(float(sig[0]) - 0.999) < 1e-15


def test_schedule_defaults_are_the_checkpoint_config():
    from finetrainers_amd.wan import wan_unipc_schedule

    assert torch.equal(wan_unipc_schedule(6)[0], wan_unipc_schedule(6, dict(UNIPC, flow_shift=3.0, num_train_timesteps=1000))[0])
    with pytest.raises(ValueError, match="at least one step"):
        wan_unipc_schedule(0)


# ---- order 1 without a corrector is Euler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1.0, 3.0])
@pytest.mark.parametrize("n", [1, 4, 50])
def test_order_1_without_corrector_is_the_euler_update(n, shift):
    """x_{i+1} = (t / s) x - alpha_t expm1(-h) (x - s v), expm1(-h) = (t alpha_s) / (s alpha_t) - 1:  the factor of x is t / s + alpha_t - t alpha_s / s = 1
    (alpha_t - t alpha_s / s = 1 - t / s), the factor of v is s alpha_t expm1(-h) = t - s."""
    from finetrainers_amd.wan import wan_unipc_schedule, wan_unipc_tables

    sig, _ = wan_unipc_schedule(n, dict(UNIPC, flow_shift=shift))
    table = wan_unipc_tables(sig, 1, list(range(n)), dtype=f64)
    model = _linear_model(7)
    x0 = torch.randn(5, dtype=f64, generator=torch.Generator().manual_seed(2))
    got = uref.run_folded(model, x0, sig.tolist(), table)
    want = uref.run_euler(model, x0, sig.tolist())
    assert _rel(got, want) <= 1e-12
    stepwise, _ = uref.run_stepwise(model, x0, sig.tolist(), 1, list(range(n)))
    assert _rel(stepwise, want) <= 1e-12


# ---- it is a higher-order solver ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("n", [40, 80])
def test_endpoint_error_on_the_gaussian_flow_is_4x_below_euler(n, shift):
    """Scalar flow with data ~ N(0.7, 0.25): the exact posterior mean is the model, the exact endpoint of the ODE is mu + s z.  A wrong sign, a swapped history
    slot or a wrong rho puts UniPC at Euler's error or above; right, it is 9x or more below on these six tables."""
    from finetrainers_amd.wan import wan_unipc_schedule, wan_unipc_tables

    sig, _ = wan_unipc_schedule(n, dict(UNIPC, flow_shift=shift))
    s = sig.tolist()
    x0 = torch.tensor([-1.5, -0.4, 0.3, 1.1, 2.0], dtype=f64)
    model = lambda i, x: uref.gaussian_flow_velocity(s[i], x)
    exact = uref.gaussian_flow_endpoint(s[0], x0)
    e_unipc = float((uref.run_folded(model, x0, s, wan_unipc_tables(sig, 2, (), dtype=f64)) - exact).abs().max())
    e_step = float((uref.run_stepwise(model, x0, s, 2, ())[0] - exact).abs().max())
    e_euler = float((uref.run_euler(model, x0, s) - exact).abs().max())
    print(f"[unipc gaussian flow n={n} shift={shift}] endpoint error: UniPC {e_unipc:.3e}, Euler {e_euler:.3e}, ratio {e_euler / e_unipc:.1f}")
    assert abs(e_unipc - e_step) <= 1e-12
    assert 4.0 * e_unipc <= e_euler


# ---- refusals and dispatch --------------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [("solver_order", 3), ("solver_order", 0), ("solver_type", "bh1"), ("predict_x0", False), ("prediction_type", "epsilon"), ("use_flow_sigmas", False),
           ("use_karras_sigmas", True), ("use_exponential_sigmas", True), ("use_beta_sigmas", True), ("thresholding", True), ("solver_p", "dpm"),
           ("final_sigmas_type", "sigma_min")]


@pytest.mark.parametrize("key,value", REFUSED)
def test_every_refusal_names_its_key(key, value):
    from finetrainers_amd.wan import MI355XWanLatentSampler, wan_unipc_schedule

    with pytest.raises(NotImplementedError, match=key):
        wan_unipc_schedule(4, dict(UNIPC, **{key: value}))
    with pytest.raises(NotImplementedError, match=key):
        MI355XWanLatentSampler(None, dict(UNIPC, **{key: value}))


def test_dispatch_follows_the_class_name_and_euler_stays_as_it_is():
    from finetrainers_amd.wan import MI355XWanLatentSampler, wan_flow_match_sigmas, wan_unipc_schedule

    for cfg in (None, {"num_train_timesteps": 1000, "shift": 1.0}, {"_class_name": "FlowMatchEulerDiscreteScheduler", "shift": 3.0},
                {"shift": 3.0, "flow_shift": 7.0, "solver_order": 9}):  # no UniPC class name: UniPC's keys are not read
        s = MI355XWanLatentSampler(None, cfg)
        assert not s.unipc
        sig, ts = s.schedule(5, None, None)
        assert sig.dtype == torch.float32 and torch.equal(sig, wan_flow_match_sigmas(5, cfg))
        assert torch.equal(ts, sig[:-1] * 1000.0)
    s = MI355XWanLatentSampler(None, dict(UNIPC, flow_shift=5.0))
    assert s.unipc
    sig, ts = s.schedule(5, None, None)
    want_sig, want_ts = wan_unipc_schedule(5, dict(UNIPC, flow_shift=5.0))
    assert sig.dtype == f64 and torch.equal(sig, want_sig) and ts.dtype == torch.float32 and torch.equal(ts.double(), want_ts)
    assert s.unipc_tables(sig).shape == (5, 8)
    # the overrides of sample stay: given sigmas, truncated timesteps of them; given timesteps, those
    sig, ts = s.schedule(0, [0.9, 0.5005, 0.0], None)
    assert ts.tolist() == [900.0, 500.0]
    sig, ts = s.schedule(0, [0.9, 0.5, 0.0], [7.0, 3.0])
    assert ts.tolist() == [7.0, 3.0]
    with pytest.raises(ValueError, match="one value per step"):
        s.schedule(0, [0.9, 0.5, 0.0], [7.0])
    # disable_corrector of the config reaches the tables
    s = MI355XWanLatentSampler(None, dict(UNIPC, disable_corrector=[0], solver_order=1))
    t = s.unipc_tables(want_sig)
    assert t[1, :5].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and float(t[2, 0]) == 0.0 and bool((t[:, 7] == 0).all())


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _geo(**kw):
    from finetrainers_amd import _lib

    base = dict(B=1, C=16, Cx=0, F=2, H=8, W=12, pt=1, ph=2, pw=2, Kp=64, copies=1, P=2, po=64)
    base.update(kw)
    return _lib.WanSampleGeometry(**base)


def _cfg(L=2, guidance=5.0, solver=1, **kw):
    from finetrainers_amd import _lib

    geo = kw.pop("geo", None) or _geo(P=2 if guidance != 1.0 else 1)
    base = dict(geo=geo, T=16, TI=0, D=256, heads=2, ffn_dim=512, L=L, eps=1e-6, gemm_variant=8, r=64, lora_scale=1.0, ffn=0, patch_fold=0, patch_r=0,
                patch_scale=0.0, steps=3, guidance=guidance)
    base.update(kw)
    return _lib.WanSampleMsConfig(base=_lib.WanSampleConfig(**base), solver=solver)


def test_c_abi_declares_exports_and_binds_the_multistep_symbols():
    from finetrainers_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None, name
    assert lib.ftmi_version() == 101


def test_ms_config_has_the_euler_config_as_its_prefix():
    from finetrainers_amd import _lib

    assert ctypes.sizeof(_lib.WanSampleConfig) == 13 * 4 + 17 * 4, "ftmi_wan_sample_config keeps its size: 13 geometry ints and 17 four-byte fields"
    assert _lib.WanSampleMsConfig.base.offset == 0 and _lib.WanSampleMsConfig.solver.offset == ctypes.sizeof(_lib.WanSampleConfig)
    assert ctypes.sizeof(_lib.WanSampleMsConfig) == ctypes.sizeof(_lib.WanSampleConfig) + 4
    assert [n for n, _ in _lib.WanSampleConfig._fields_][-3:] == ["steps", "guidance", "TI2"]
    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    body = re.search(r"typedef struct ftmi_wan_sample_ms_config \{(.*?)\} ftmi_wan_sample_ms_config;", header, flags=re.S).group(1)
    fields = [l.strip() for l in body.strip().splitlines()]
    assert fields[0].startswith("ftmi_wan_sample_config base;") and fields[1].startswith("int solver;") and len(fields) == 2


def test_ms_workspace_is_the_euler_workspace_plus_three_state_buffers():
    from finetrainers_amd import _lib

    lib = _lib.load()
    ms = lambda **kw: lib.ftmi_wan_sample_ms_workspace_bytes(ctypes.byref(_cfg(**kw)))
    euler = lambda **kw: lib.ftmi_wan_sample_workspace_bytes(ctypes.byref(_cfg(**kw).base))
    S, Kc = 48, 64
    assert euler() > 0 and ms() == euler() + 3 * 4 * 1 * S * Kc
    assert ms(L=1) == ms(L=40) == ms()
    assert ms(guidance=1.0) == euler(guidance=1.0) + 3 * 4 * S * Kc, "the history is the state's size: one row group"
    assert ms(geo=_geo(B=2)) == euler(geo=_geo(B=2)) + 3 * 4 * 2 * S * Kc
    assert ms(steps=50) == ms(steps=3), "nothing is kept per step"
    for kw, code_msg in ((dict(solver=0), "solver"), (dict(solver=2), "solver"), (dict(L=41), "1 .. 40 blocks"), (dict(steps=0), "positive"),
                         (dict(geo=_geo(P=1)), "P is 2"), (dict(geo=_geo(C=8)), "must equal po")):
        assert ms(**kw) == 0 and code_msg in _lib.last_error(), (kw, _lib.last_error())
    assert lib.ftmi_wan_sample_ms_workspace_bytes(None) == 0


def test_ms_entry_points_check_their_arguments_before_any_launch():
    from finetrainers_amd import _lib

    lib = _lib.load()
    p, q, r, s = (ctypes.c_void_p(256 * k) for k in (1, 2, 3, 4))
    step = lambda geo=None, pred=p, x=p, last=q, m1=r, m2=s, coef=p, sigma=p, g=5.0, cols=p: lib.ftmi_wan_sample_step_unipc(
        ctypes.byref(geo or _geo()), pred, x, last, m1, m2, coef, sigma, g, cols, None)
    for kw, code, msg in [(dict(C=15, po=60), _lib.FTMI_ERR_UNSUPPORTED, "multiples of 8"), (dict(po=128), _lib.FTMI_ERR_INVALID, "must equal po"),
                          (dict(W=13), _lib.FTMI_ERR_UNSUPPORTED, "whole patches"), (dict(copies=3), _lib.FTMI_ERR_INVALID, "copies"),
                          (dict(C=24, po=96, Kp=128), _lib.FTMI_ERR_UNSUPPORTED, "divide 2048")]:
        assert step(_geo(**kw)) == code and msg in _lib.last_error(), (kw, _lib.last_error())
    assert step(g=1.0) == _lib.FTMI_ERR_INVALID and "guidance" in _lib.last_error()
    assert step(last=ctypes.c_void_p(260)) == _lib.FTMI_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert step(m2=r) == _lib.FTMI_ERR_INVALID and "four buffers" in _lib.last_error()
    assert step(last=p) == _lib.FTMI_ERR_INVALID and "four buffers" in _lib.last_error()
    for missing in ("pred", "last", "m1", "m2", "coef", "sigma"):
        assert step(**{missing: None}) == _lib.FTMI_ERR_INVALID, missing
    # the loop: the workspace and the weights, as ftmi_wan_sample checks them
    cfg = _cfg()
    need = lib.ftmi_wan_sample_ms_workspace_bytes(ctypes.byref(cfg))
    blocks = (_lib.WanLoraFfnBlockWeights * 2)()
    w = _lib.WanSampleWeights()
    w.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.WanLoraFfnBlockWeights))
    w.patch_w = w.patch_b = w.proj_w = w.proj_b = 256
    call = lambda c, nbytes, coef=p: lib.ftmi_wan_sample_ms(ctypes.byref(c), ctypes.byref(w), p, p, p, p, p, p, None, p, p, coef, p, p, nbytes, None)
    assert call(cfg, need - 1) == _lib.FTMI_ERR_INVALID and "workspace too small" in _lib.last_error()
    assert call(cfg, need) == _lib.FTMI_ERR_INVALID and "block without parameters" in _lib.last_error()
    assert call(cfg, need, coef=None) == _lib.FTMI_ERR_INVALID
    assert call(_cfg(solver=2), need) == _lib.FTMI_ERR_UNSUPPORTED and "solver" in _lib.last_error()


# ---- the checkpoint's scheduler config ----------------------------------------------------------------------------------------------------------------------------------
def test_scheduler_config_is_read_from_the_checkpoint_directory(tmp_path):
    from finetrainers_amd import wire
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, MI355XWanLatentSampler, MI355XWanModelSpecification

    conf = {"_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.33.0.dev0", "flow_shift": 5.0, "num_train_timesteps": 1000, "solver_order": 2,
            "prediction_type": "flow_prediction", "use_flow_sigmas": True, "solver_type": "bh2", "predict_x0": True, "final_sigmas_type": "zero",
            "disable_corrector": [], "lower_order_final": True, "thresholding": False, "solver_p": None}
    os.makedirs(tmp_path / "scheduler")
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(conf, f)
    assert wire.load_scheduler_config(str(tmp_path)) == conf
    with pytest.raises(FileNotFoundError, match="scheduler_config.json"):
        wire.load_scheduler_config(str(tmp_path / "scheduler"))
    for cls in (MI355XWanModelSpecification, MI355XWanControlModelSpecification):
        assert cls(pretrained_model_name_or_path=str(tmp_path)).validation_scheduler_config() == conf
        assert cls(pretrained_model_name_or_path="Wan-AI/Wan2.1-T2V-1.3B-Diffusers").validation_scheduler_config() is None
        assert cls(pretrained_model_name_or_path=None).validation_scheduler_config() is None
    s = MI355XWanLatentSampler(None, wire.load_scheduler_config(str(tmp_path)))
    assert s.unipc and math.isclose(float(s.schedule(4, None, None)[0][0]), 5 * 0.999 / (1 + 4 * 0.999), rel_tol=1e-15)
