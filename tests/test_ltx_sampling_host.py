"""CPU-side tests of the LTX-Video latent sampler: the C ABI carries the new entry points, the sigma schedule has the shape a flow-match sampler
needs, and the loop the GPU tests compose (CFG combine, Euler update, bf16 model input, fp32 state) reproduces a closed form on a toy model."""

import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAMPLING_SYMBOLS = ("ftmi_ltx_cfg_euler_step", "ftmi_ltx_unpack_denorm", "ftmi_ltx_ff_sample", "ftmi_ltx_ff_sample_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from finetrainers_amd import _lib

    if not _lib.lib_available():
        from finetrainers_amd.csrc.build import build

        build()
    return _lib.load()


def torch_sampling_loop(model, x0, sigmas, guidance):
    """The denoising loop, restated in torch: ``model(x_in bf16 [nb, ...], step) -> pred bf16 [nb, ...]`` with nb = 2B rows (unconditional first) or B
    for ``guidance == 1``; the state stays fp32, the model sees its bf16 rounding, v = u + g (c - u), x += (sigma_next - sigma) v."""
    x = x0.float().clone()
    B = x.shape[0]
    for i in range(len(sigmas) - 1):
        xin = x.to(torch.bfloat16)
        if guidance != 1.0:
            pred = model(torch.cat([xin, xin]), i).float()
            u, c = pred[:B], pred[B:]
            v = u + guidance * (c - u)
        else:
            v = model(xin, i).float()
        x = x + (sigmas[i + 1] - sigmas[i]) * v
    return x


def test_sampling_symbols_declared_and_exported(lib):
    from finetrainers_amd import _lib

    header = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", header))
    for name in SAMPLING_SYMBOLS:
        assert name in declared, f"include/ftmi355.h does not declare {name}"
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), f"libftmi355.so does not export {name}"


def test_sample_workspace_is_forward_only(lib):
    """Condition of the forward-only mode: at BASELINE config 2 the sampler's workspace is the checkpoint = 1 layout at batch 2B, within 5 %."""
    from finetrainers_amd import _lib

    def cfg(B, checkpoint):
        return _lib.LtxConfig(B=B, S=2688, T=128, D=2048, H=32, L=28, C_in=128, C_out=128, D_ff=8192, D_cap=4096, r=64, lora_scale=1.0, eps_norm=1e-6,
                              eps_qk=1e-5, gemm_variant=8, checkpoint=checkpoint)

    w = ctypes.byref(_lib.LtxFfWeights())  # (no feed-forward adapters; a planner never dereferences the weights)
    for videos in (1, 2):
        ws_two = lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg(videos, 0)), w, 1)
        ws_one = lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg(videos, 0)), w, 0)
        ref_two = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg(2 * videos, 1)), w)
        ref_one = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg(videos, 1)), w)
        assert ref_two <= ws_two <= 1.05 * ref_two, (ws_two, ref_two)
        assert ref_one <= ws_one <= 1.05 * ref_one, (ws_one, ref_one)
        assert ws_one < 0.6 * ws_two  # guidance == 1 runs B rows only
        assert ws_two < 0.25 * lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg(2 * videos, 0)), w)  # far from a full activation stash


def test_sampling_entry_points_check_arguments(lib):
    from finetrainers_amd import _lib

    assert lib.ftmi_ltx_cfg_euler_step(None, None, None, None, 3.0, None, 1, 64, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_ltx_unpack_denorm(None, None, None, None, 1, 128, 64, None) == _lib.FTMI_ERR_INVALID
    p = ctypes.c_void_p(256)
    assert lib.ftmi_ltx_cfg_euler_step(p, p, p, p, 3.0, p, 1, 60, None) == _lib.FTMI_ERR_UNSUPPORTED and "multiple of 8" in _lib.last_error()
    assert lib.ftmi_ltx_unpack_denorm(p, p, p, p, 1, 126, 64, None) == _lib.FTMI_ERR_UNSUPPORTED
    cfg = _lib.LtxConfig(B=1, S=64, T=128, D=2048, H=32, L=1, C_in=128, C_out=128, D_ff=8192, D_cap=4096, r=0, lora_scale=0.0, eps_norm=1e-6, eps_qk=1e-5,
                         gemm_variant=8)
    w = _lib.LtxFfWeights()
    # guidance != 1 without the unconditional prompt, and a workspace that is too small: refused before any launch
    assert lib.ftmi_ltx_ff_sample(ctypes.byref(cfg), ctypes.byref(w), p, None, None, None, p, p, p, 2, 3.0, p, 1 << 40, None) == _lib.FTMI_ERR_INVALID
    assert lib.ftmi_ltx_ff_sample(ctypes.byref(cfg), ctypes.byref(w), p, p, None, None, p, p, p, 2, 3.0, p, 1024, None) == _lib.FTMI_ERR_INVALID
    assert "workspace too small" in _lib.last_error()
    cfg.B = 5  # 10 model rows
    assert lib.ftmi_ltx_ff_sample(ctypes.byref(cfg), ctypes.byref(w), p, p, None, None, p, p, p, 2, 3.0, p, 1 << 40, None) == _lib.FTMI_ERR_UNSUPPORTED


def test_sampler_refuses_cpu_and_narrow_models():
    from finetrainers_amd import ops
    from finetrainers_amd.ltx_video import MI355XLTXLatentSampler

    with pytest.raises(ValueError):
        ops.ltx_cfg_euler_step(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(1, 64), torch.zeros(1), torch.zeros(1), 3.0)
    with pytest.raises(ValueError):
        ops.ltx_unpack_denorm(torch.zeros(1, 8, 128), torch.zeros(128), torch.ones(128), 2, 2, 2)

    class Narrow:
        _narrow = (32, 8)

    with pytest.raises(NotImplementedError, match="narrow"):
        MI355XLTXLatentSampler(Narrow())


@pytest.mark.parametrize("n", [1, 4, 50])
def test_flow_match_sigmas(n):
    from finetrainers_amd.ltx_video.sampler import LTX_SCHEDULER_CONFIG, flow_match_sigmas

    for seq_len in (32, 2688, 8192):
        s = flow_match_sigmas(n, seq_len, LTX_SCHEDULER_CONFIG)
        assert s.dtype == torch.float32 and s.shape == (n + 1,)
        assert (s[1:] < s[:-1]).all(), s
        assert s[0] <= 1.0 and s[-1] == 0.0
    # no dynamic shifting, shift 1, no terminal stretch: the unshifted linear table
    plain = {"num_train_timesteps": 1000, "shift": 1.0, "use_dynamic_shifting": False}
    want = torch.cat([torch.linspace(1.0, 1.0 / n, n, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)]).float()
    assert torch.equal(flow_match_sigmas(n, 2688, plain), want)
    # more tokens shift the schedule towards high noise; the terminal stretch pins the last non-zero entry
    if n > 1:
        lo, hi = flow_match_sigmas(n, 1024, LTX_SCHEDULER_CONFIG), flow_match_sigmas(n, 4096, LTX_SCHEDULER_CONFIG)
        assert (hi[1:-2] > lo[1:-2]).all()
        assert abs(lo[-2].item() - LTX_SCHEDULER_CONFIG["shift_terminal"]) < 1e-6
    # every constant comes from the config: a dynamic-shifting config without them is refused
    with pytest.raises(ValueError, match="base_shift"):
        flow_match_sigmas(n, 2688, {"use_dynamic_shifting": True, "base_image_seq_len": 1024, "max_image_seq_len": 4096, "max_shift": 2.05})
    # ... and changing one changes the table
    other = dict(LTX_SCHEDULER_CONFIG, max_shift=3.0)
    if n > 1:
        assert not torch.equal(flow_match_sigmas(n, 2688, other), flow_match_sigmas(n, 2688, LTX_SCHEDULER_CONFIG))


@pytest.mark.parametrize("guidance", [1.0, 3.0])
def test_torch_loop_closed_form(guidance):
    """Constant velocity: x_N = x_0 - sigma_0 v exactly (dyadic values: every product and sum below is exact in fp32, and the velocity in bf16)."""
    B, n = 2, 6
    g = torch.Generator().manual_seed(0)
    x0 = torch.randint(-64, 64, (B, 24, 16), generator=g).float() / 8
    v = (torch.randint(-32, 32, (B, 24, 16), generator=g).float() / 16).to(torch.bfloat16)
    assert torch.equal(v.float().to(torch.bfloat16), v)
    sigmas = torch.tensor([1.0, 0.75, 0.5, 0.375, 0.25, 0.125, 0.0])
    assert len(sigmas) == n + 1
    seen = []

    def model(xin, i):
        assert xin.dtype == torch.bfloat16 and xin.shape[0] == (2 * B if guidance != 1.0 else B)
        seen.append(i)
        if guidance != 1.0:
            # unconditional and conditional predictions that combine to v: u + g (c - u) = v with c - u = 1 / 4
            c = v.float() + 0.25 * (1 - guidance)
            u = c - 0.25
            return torch.cat([u, c]).to(torch.bfloat16)
        return v

    xN = torch_sampling_loop(model, x0, sigmas, guidance)
    assert seen == list(range(n))
    assert torch.equal(xN, x0 - sigmas[0] * v.float())
    # a velocity field that depends on the state through its bf16 rounding: the model input is bf16(x), the state is not rounded
    xo = torch.full((1, 8), 1.0 + 2.0**-12)
    out = torch_sampling_loop(lambda xin, i: xin, xo, torch.tensor([1.0, 0.5]), 1.0)
    assert torch.equal(out, xo - 0.5 * xo.to(torch.bfloat16).float()) and not torch.equal(out, xo * 0.5)
