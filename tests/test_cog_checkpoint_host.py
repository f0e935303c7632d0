"""CogVideoX gradient checkpointing (ftmi_cog_config.checkpoint), the parts that need no GPU: the workspace plan -- one block slot, a layer costs its
modulation rows and one hidden state --, the refusal of any value but 0 / 1 before a launch, the ABI table and the model's host interface."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
r256 = lambda n: (n + 255) // 256 * 256  # the Bump allocator's granule (csrc/common.hip.h)


def _cfg(L, **kw):
    from finetrainers_amd import _lib

    base = dict(B=2, T=16, S=48, D=256, H=4, L=L, D_ff=1024, D_temb=512, r=64, lora_scale=1.0, eps_norm=1e-5, eps_qk=1e-6, gemm_variant=8)
    base.update(kw)
    return _lib.CogConfig(**base)


def _bytes(cfg):
    from finetrainers_amd import _lib

    return _lib.load().ftmi_cog_workspace_bytes(ctypes.byref(cfg))


def _slot(B, N, D, H, D_ff, r):
    """One block slot of the training layout (make_layout in csrc/cog_dit.hip): the forward entries, then the backward's stash."""
    M = B * N
    fwd = [M * D * 2, M * 3 * D * 2, M * D * 2, M * D * 2, M * D * 2, B * H * N * 4, M * 9 * r * 2, M * 3 * r * 2, M * D * 2, M * D * 2, M * D_ff * 2]
    stash = [M * 3 * D * 2, M * D * 2, M * 9 * r * 2, M * 3 * r * 2]
    return sum(r256(n) for n in fwd + stash)


def _plan(L, slots, B=2, T=16, S=48, D=256, H=4, D_ff=1024, r=64):
    N, M = T + S, B * (T + S)
    head = [B * L * 2 * 6 * D * 2, L * 2 * 3 * B * 2 * D * 2, max(L - 1, 1) * M * D * 2]
    scratch = [M * D_ff * 2, M * D * 2, M * D_ff * 2] + [M * D * 2] * 7 + [B * H * N * 4]
    return sum(r256(n) for n in head) + r256(_slot(B, N, D, H, D_ff, r) * slots) + sum(r256(n) for n in scratch)


@pytest.mark.parametrize("L", [2, 3, 7, 30])
def test_one_more_layer_costs_its_modulation_rows_and_one_hidden_state(L):
    B, D, M = 2, 256, 2 * 64
    more = (r256(B * (L + 1) * 12 * D * 2) - r256(B * L * 12 * D * 2) + r256((L + 1) * 24 * B * D) - r256(L * 24 * B * D)
            + r256((L + 1 - 1) * M * D * 2) - r256((L - 1) * M * D * 2))
    assert _bytes(_cfg(L + 1, checkpoint=1)) - _bytes(_cfg(L, checkpoint=1)) == more
    assert _bytes(_cfg(L, checkpoint=1)) == _plan(L, 1)


@pytest.mark.parametrize("L", [1, 2, 5, 30])
def test_checkpoint_zero_is_the_layout_with_one_slot_per_block(L):
    named, unnamed = _bytes(_cfg(L, checkpoint=0)), _bytes(_cfg(L))
    assert named == unnamed == _plan(L, L)
    assert _bytes(_cfg(L, checkpoint=1)) == _plan(L, 1) and (_bytes(_cfg(L, checkpoint=1)) < named) == (L > 1)
    assert _bytes(_cfg(L, r=0, checkpoint=1)) == _bytes(_cfg(L, checkpoint=1)), "r = 0 plans the rank-64 entries, as the kept layout does"


def test_config_3_needs_less_than_a_sixth():
    geo = dict(B=1, T=226, S=17550, D=1920, H=30, D_ff=7680, D_temb=512, r=64)
    off, on = _bytes(_cfg(30, **geo)), _bytes(_cfg(30, checkpoint=1, **geo))
    print(f"[cog-ckpt plan] config 3: {off / 1e9:.2f} GB kept, {on / 1e9:.2f} GB checkpointed ({off / on:.1f} x)")
    assert 0 < on < off / 6
    assert off - on == r256(_slot(1, 17776, 1920, 30, 7680, 64) * 30) - r256(_slot(1, 17776, 1920, 30, 7680, 64))


@pytest.mark.parametrize("value", [2, -1])
def test_other_values_are_refused_before_a_launch(value):
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg, w = _cfg(2, checkpoint=value), _lib.CogWeights()
    assert lib.ftmi_cog_blocks_forward(ctypes.byref(cfg), ctypes.byref(w), None, None, None, None, 0, None) == _lib.FTMI_ERR_INVALID
    assert "checkpoint must be 0 or 1" in _lib.last_error()
    assert lib.ftmi_cog_blocks_backward(ctypes.byref(cfg), ctypes.byref(w), None, None, None, None, None, None, 0, 2, 0, 0, None) == _lib.FTMI_ERR_INVALID
    assert "checkpoint must be 0 or 1" in _lib.last_error()
    # with every pointer given the orchestrator's own check answers, still before the workspace is looked at
    p = ctypes.c_void_p(256)
    assert lib.ftmi_cog_blocks_forward(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, 0, None) == _lib.FTMI_ERR_INVALID and "checkpoint" in _lib.last_error()


def test_header_and_binding_agree_on_the_trailing_field():
    from finetrainers_amd import _lib

    text = open(os.path.join(ROOT, "include", "ftmi355.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ftmi_cog_config;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.CogConfig._fields_] and names[-1] == "checkpoint"
    assert _lib.CogConfig().checkpoint == 0
    assert "checkpoint" not in [n for n, _ in _lib.CogSampleConfig._fields_], "sampling plans its own one-slot layout"


def _host_model(**kw):
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXTransformer3DModel

    cfg = CogVideoXTransformerConfig(num_attention_heads=2, num_layers=2, time_embed_dim=64, text_embed_dim=64, max_text_seq_length=16, **kw)
    return MI355XCogVideoXTransformer3DModel(cfg, device=torch.device("cpu"))


def test_model_interface_matches_the_ltx_model():
    from finetrainers_amd.cogvideox import MI355XCogVideoXTransformer3DModel as Cog
    from finetrainers_amd.ltx_video import MI355XLTXVideoTransformer3DModel as Ltx

    for name in ("apply_activation_checkpointing", "enable_gradient_checkpointing", "disable_gradient_checkpointing", "is_gradient_checkpointing"):
        assert hasattr(Cog, name) and type(getattr(Cog, name)) is type(getattr(Ltx, name)), name
    assert isinstance(Cog.is_gradient_checkpointing, property)
    m = _host_model()
    assert m.gradient_checkpointing is False and not m.is_gradient_checkpointing and m._c_config(2, 64).checkpoint == 0
    assert m.apply_activation_checkpointing("full") is m and m.is_gradient_checkpointing and m._c_config(2, 64).checkpoint == 1
    m.disable_gradient_checkpointing()
    assert not m.is_gradient_checkpointing and m._c_config(2, 64).checkpoint == 0
    assert m.enable_gradient_checkpointing() is None and m.is_gradient_checkpointing
    cfg = m._c_config(2, 64)
    assert (cfg.B, cfg.T, cfg.S, cfg.L, cfg.checkpoint) == (2, 16, 48, 2, 1)
    for bad in ("block_skip", "ops", ""):
        m.disable_gradient_checkpointing()
        with pytest.raises(ValueError, match=repr(bad)):
            m.apply_activation_checkpointing(bad)
        assert not m.is_gradient_checkpointing, "a refused type leaves the flag alone"


def test_python_composition_refuses_the_flag():
    m = _host_model()
    m.enable_gradient_checkpointing()
    m.native_blocks = False
    m.proj_out_w_t = torch.zeros(1)  # (stands for "weights loaded": the refusal comes before anything is computed)
    x, text, t = torch.zeros(1, 1, 16, 4, 4), torch.zeros(1, 16, 64), torch.zeros(1)
    with pytest.raises(NotImplementedError, match="native block stack"):
        m(x, text, t)
