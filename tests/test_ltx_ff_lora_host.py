"""LTX-Video feed-forward adapters, host side (no GPU): the ``target_modules`` selection table, the four new parameters and the [A | B | FF] flat layout, the peft
state dict and its safetensors round trip, the C ABI of the ``ftmi_ltx_ff_*`` entries (the only LTX entries that run blocks) against include/ftmi355.h and the
byte plans recorded when the narrow family still stood beside them (tests/ltx_entry_bytes.py), and the refusal on the narrow geometry."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from finetrainers_amd import _lib, wire
from finetrainers_amd.ltx_video.transformer import (CONTROL_TARGET_MODULES, DEFAULT_TARGET_MODULES, LORA_FF_ORDER, LORA_ORDER, LTXTransformerConfig,
                                                    MI355XLTXVideoTransformer3DModel)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ftmi355.h")
# finetrainers/trainer/control_trainer/config.py:60 and trainer/sft_trainer/config.py:24-26, spelled out so that a change of the module's constants shows
CONTROL = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)"
SFT = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0)"
EIGHT = ["attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0"]
D, F = 2048, 8192


def _model(L=2):
    return MI355XLTXVideoTransformer3DModel(LTXTransformerConfig(num_layers=L), device=torch.device("cpu"))


# ---- selection -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_module_constants_are_the_reference_defaults():
    assert DEFAULT_TARGET_MODULES == SFT and CONTROL_TARGET_MODULES == CONTROL
    assert tuple(LORA_ORDER) == tuple(EIGHT) and tuple(LORA_FF_ORDER) == ("ff.net.0.proj", "ff.net.2")


@pytest.mark.parametrize("target,adapters", [
    (None, 8), (SFT, 8), (list(EIGHT), 8), (["to_q", "to_k", "to_v", "to_out.0"], 8),
    (CONTROL, 10), (list(EIGHT) + ["ff.net.0.proj", "ff.net.2"], 10), (["to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2"], 10),
])
def test_selection_table(target, adapters):
    m = _model(1)
    m.add_adapter(r=4, lora_alpha=4, target_modules=target)
    assert m.lora_ff == (adapters == 10)
    assert len(m.lora_state_dict()) == 2 * adapters
    assert (m.lora_ff_A1 is not None) == (adapters == 10)


@pytest.mark.parametrize("target,named", [
    ("ff.net.0.proj", "attn1.to_q"),                      # feed-forward modules alone: raised before this feature and still
    (["ff.net.0.proj", "ff.net.2"], "attn1.to_q"),
    (list(EIGHT) + ["ff.net.2"], "ff.net.0.proj"),        # the eight plus one of the pair
    (list(EIGHT) + ["ff.net.0.proj"], "ff.net.2"),
    (["to_q", "to_k", "to_v"], "attn1.to_out.0"),
])
def test_unserved_selections_raise_naming_the_first_module_they_lack(target, named):
    m = _model(1)
    with pytest.raises(ValueError) as e:
        m.add_adapter(r=4, lora_alpha=4, target_modules=target)
    assert named in str(e.value)
    assert m.lora_A is None and m.lora_flat is None


def test_a_second_add_adapter_raises():
    m = _model(1)
    m.add_adapter(r=4, lora_alpha=4, target_modules=CONTROL)
    with pytest.raises(ValueError):
        m.add_adapter(r=4, lora_alpha=4, target_modules=CONTROL)


# ---- parameters and the flat layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [64, 32])
def test_parameters_shapes_init_and_flat_aliasing(r):
    L = 2
    m = _model(L)
    torch.manual_seed(0)
    m.add_adapter(r=r, lora_alpha=r, target_modules=CONTROL)
    rp = 64
    names = dict(m.named_parameters())
    assert set(names) == {"lora_A", "lora_B", "lora_ff_A1", "lora_ff_B1", "lora_ff_A2", "lora_ff_B2"}
    assert tuple(m.lora_ff_A1.shape) == (L, r, D) and tuple(m.lora_ff_B1.shape) == (L, F, r)
    assert tuple(m.lora_ff_A2.shape) == (L, r, F) and tuple(m.lora_ff_B2.shape) == (L, D, r)
    for p in names.values():
        assert p.dtype == torch.float32 and p.requires_grad
    # peft's init: A ~ kaiming-uniform(a = sqrt(5)) -> |A| <= 1 / sqrt(fan_in), B = 0
    b1, b2 = 1 / math.sqrt(D), 1 / math.sqrt(F)
    assert 0.9 * b1 < m.lora_ff_A1.abs().max().item() <= b1
    assert 0.9 * b2 < m.lora_ff_A2.abs().max().item() <= b2
    assert m.lora_ff_B1.abs().max().item() == 0 and m.lora_ff_B2.abs().max().item() == 0
    # flat layout [A | B | FF], FF per block [A1 | B1 | A2 | B2]
    n = L * 8 * rp * D
    per = 2 * rp * (D + F)
    assert m.lora_flat.numel() == 2 * n + L * per
    base = m.lora_flat.data_ptr()
    assert m.lora_A.data_ptr() == base and m.lora_B.data_ptr() == base + 4 * n
    offs = (0, rp * D, rp * D + F * rp, rp * D + 2 * F * rp)
    sizes = (rp * D, F * rp, rp * F, D * rp)
    for l in range(L):
        at = base + 4 * (2 * n + l * per)
        for p, off, size in zip((m.lora_ff_A1, m.lora_ff_B1, m.lora_ff_A2, m.lora_ff_B2), offs, sizes):
            assert p[l].data_ptr() == at + 4 * off  # contiguous and adjacent: each view starts where the previous one's storage ends
        assert offs[3] + sizes[3] == per and all(offs[i] + sizes[i] == offs[i + 1] for i in range(3))
    m._assert_flat_aliasing()
    if r < rp:  # padded rows / columns are zero
        full = m._ff_views(m._lora_ff_full, padded=True)
        assert full[0][:, r:, :].abs().max() == 0 and full[2][:, r:, :].abs().max() == 0
    # every element of the FF region belongs to exactly one (padded) view
    marks = torch.zeros_like(m._lora_ff_full)
    for v in m._ff_views(marks, padded=True):
        v += 1
    assert bool((marks == 1).all())


def test_the_eight_adapter_model_is_what_it_was():
    L, r = 2, 64
    m = _model(L)
    m.add_adapter(r=r, lora_alpha=r, target_modules=SFT)
    assert set(dict(m.named_parameters())) == {"lora_A", "lora_B"}
    assert m.lora_flat.numel() == 2 * L * 8 * r * D
    assert not m.lora_ff and m._ff_params() == ()
    w = m._c_weights(torch.zeros(1), torch.zeros(1))  # the one weights structure, its feed-forward extension NULL
    assert isinstance(w, _lib.LtxFfWeights) and all(getattr(w, n) is None for n in _lib.LTX_FF_WEIGHT_FIELDS)
    assert w.base.proj_in_w == m.proj_in_w.data_ptr() and w.base.lora_a_sp == m.lora_a_sp.data_ptr()


# ---- state dict and wire ---------------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_round_trip_and_mismatch(tmp_path):
    L, r = 2, 8
    m = _model(L)
    m.add_adapter(r=r, lora_alpha=2 * r, target_modules=CONTROL)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape))
    sd = m.lora_state_dict()
    assert len(sd) == 2 * 10 * L
    for l in range(L):
        for n in list(EIGHT) + ["ff.net.0.proj", "ff.net.2"]:
            assert f"transformer_blocks.{l}.{n}.lora_A.weight" in sd and f"transformer_blocks.{l}.{n}.lora_B.weight" in sd
    assert tuple(sd["transformer_blocks.1.ff.net.0.proj.lora_A.weight"].shape) == (r, D)
    assert tuple(sd["transformer_blocks.1.ff.net.0.proj.lora_B.weight"].shape) == (F, r)
    assert tuple(sd["transformer_blocks.1.ff.net.2.lora_A.weight"].shape) == (r, F)
    assert tuple(sd["transformer_blocks.1.ff.net.2.lora_B.weight"].shape) == (D, r)
    meta = wire.lora_config_metadata(r, 2 * r, m.lora_target_modules)
    path = wire.save_lora_weights(str(tmp_path), {k: v.detach() for k, v in sd.items()}, metadata=meta)
    loaded, cfg = wire.load_lora_weights(path if os.path.isfile(path) else str(tmp_path))
    assert cfg["target_modules"] == CONTROL and m.lora_target_modules == CONTROL
    other = _model(L)
    other.add_adapter(r=cfg["r"], lora_alpha=cfg["lora_alpha"], target_modules=cfg["target_modules"])
    other.load_lora_state_dict(loaded)
    for k, v in other.lora_state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert torch.equal(other.lora_flat, m.lora_flat)
    # the file and the model must agree about the feed-forward adapters, both ways
    eight = _model(L)
    eight.add_adapter(r=r, lora_alpha=2 * r, target_modules=SFT)
    with pytest.raises(ValueError, match="feed-forward"):
        eight.load_lora_state_dict(loaded)
    with pytest.raises(ValueError, match="feed-forward"):
        other.load_lora_state_dict(eight.lora_state_dict())


def test_metadata_carries_the_target_modules_string():
    meta = wire.lora_config_metadata(16, 16, CONTROL)
    blob = json.dumps({k: v for k, v in meta.items()})
    assert "ff.net.0.proj|ff.net.2" in blob


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_fields(struct_name):
    """[(type, name)] of ``typedef struct { ... } struct_name;`` in the header, comments stripped (pointer stars go with the type)."""
    m = re.search(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*" + struct_name + r"\s*;", _header_text())
    assert m, struct_name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head, *rest = [p.strip() for p in decl.split(",")]
        typ, first = head.replace("*", " * ").rsplit(None, 1)
        ptr_type = "*" in typ
        typ = typ.replace("*", "").strip()
        for nm in [first] + rest:
            is_ptr = ptr_type or nm.startswith("*")
            out.append((typ + (" *" if is_ptr else ""), nm.lstrip("* ").strip()))
    return out


def _ctype_of(typ):
    if typ.endswith("*"):
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "float": ctypes.c_float, "ftmi_ltx_weights": _lib.LtxWeights}[typ]


def _rebuilt(struct_name):
    return type("Expected_" + struct_name, (ctypes.Structure,), {"_fields_": [(n, _ctype_of(t)) for t, n in _header_fields(struct_name)]})


def test_base_structures_keep_their_size_and_the_extension_starts_with_the_base():
    cfg, w = _rebuilt("ftmi_ltx_config"), _rebuilt("ftmi_ltx_weights")
    assert ctypes.sizeof(_lib.LtxConfig) == ctypes.sizeof(cfg) == 18 * 4
    assert [n for n, _ in _lib.LtxConfig._fields_] == [n for _, n in _header_fields("ftmi_ltx_config")]
    assert ctypes.sizeof(_lib.LtxWeights) == ctypes.sizeof(w) == 48 * ctypes.sizeof(ctypes.c_void_p)
    assert [n for n, _ in _lib.LtxWeights._fields_] == [n for _, n in _header_fields("ftmi_ltx_weights")]
    ff = _header_fields("ftmi_ltx_ff_weights")
    assert ff[0] == ("ftmi_ltx_weights", "base")
    assert [n for _, n in ff] == [n for n, _ in _lib.LtxFfWeights._fields_]
    assert _lib.LtxFfWeights.base.offset == 0
    assert ctypes.sizeof(_lib.LtxFfWeights) == ctypes.sizeof(_rebuilt("ftmi_ltx_ff_weights")) == ctypes.sizeof(_lib.LtxWeights) + 8 * ctypes.sizeof(ctypes.c_void_p)
    assert len(_lib.LTX_FF_WEIGHT_FIELDS) == 8


NEW_SYMBOLS = ["ftmi_ltx_ff_workspace_bytes", "ftmi_ltx_ff_workspace_offset", "ftmi_ltx_ff_forward", "ftmi_ltx_ff_forward_frames_workspace_bytes",
               "ftmi_ltx_ff_forward_frames", "ftmi_ltx_ff_backward_range", "ftmi_ltx_ff_sample_workspace_bytes", "ftmi_ltx_ff_sample",
               "ftmi_ltx_ff_sample_cond_workspace_bytes", "ftmi_ltx_ff_sample_cond", "ftmi_gelu_from_pre", "ftmi_lora_refresh_rect"]


def test_new_symbols_are_declared_bound_and_exported():
    text = _header_text()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert s in _lib.EXPORTED_SYMBOLS
    if not _lib.lib_available():
        pytest.skip("libftmi355.so is not built")
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert lib.ftmi_version() == 101
    import ltx_entry_bytes

    declared = set(re.findall(r"\b(ftmi_[a-z0-9_]+)\s*\(", text))
    ltx_entry_bytes.assert_only_the_wide_family(lib, declared, set(_lib.EXPORTED_SYMBOLS))  # ... and the narrow family they were twins of is gone


def _cfg(r=64, **kw):
    base = dict(B=2, S=72, T=128, D=2048, H=32, L=2, C_in=128, C_out=128, D_ff=8192, D_cap=4096, r=r, lora_scale=1.0, eps_norm=1e-6, eps_qk=1e-5,
                gemm_variant=8, checkpoint=0, d_valid=0, head_dim_valid=0)
    base.update(kw)
    return _lib.LtxConfig(**base)


def test_workspace_plans_no_device():
    """All eight pointers NULL: the entry plans what the narrow entry planned (the recorded number).  All set: the plan grows by the two kept [M, 3r] buffers
    per block slot and the two scratch ones.  Some set, or any with r = 0: refused (a planner returns 0)."""
    if not _lib.lib_available():
        pytest.skip("libftmi355.so is not built")
    import ltx_entry_bytes

    lib = _lib.load()
    plans = ltx_entry_bytes.recorded()
    for ck in (0, 1):
        cfg = _cfg(checkpoint=ck)
        none = _lib.LtxFfWeights()
        narrow = plans[(cfg.B, cfg.S, 3, cfg.L, cfg.r, ck, 0)]  # (workspace, ..., sample(two_pass = 1), ...) of the narrow family, recorded before it went
        eight = narrow[0]
        assert lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(none)) == eight > 0
        full = _lib.LtxFfWeights()
        for n in _lib.LTX_FF_WEIGHT_FIELDS:
            setattr(full, n, 256)  # (never dereferenced by a planner)
        M, r = cfg.B * cfg.S, cfg.r
        buf = (M * 3 * r * 2 + 255) // 256 * 256
        slots = 1 if ck else cfg.L
        assert lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(full)) == eight + 2 * buf * slots + 2 * buf
        off = ctypes.c_size_t(0)
        assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), ctypes.byref(full), b"xa_ff2", 0, ctypes.byref(off)) == 0
        assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), ctypes.byref(none), b"xa_ff2", 0, ctypes.byref(off)) != 0
        assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), ctypes.byref(none), b"xa_ff1", 0, ctypes.byref(off)) != 0
        # the eight-adapter slot is a prefix of the ten-adapter one
        o8, o10 = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), ctypes.byref(none), b"z", 0, ctypes.byref(o8)) == 0
        assert lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(cfg), ctypes.byref(full), b"z", 0, ctypes.byref(o10)) == 0
        assert o8.value == o10.value
        some = _lib.LtxFfWeights()
        some.ff_a1_sp = 256
        assert lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(cfg), ctypes.byref(some)) == 0
        assert lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(_cfg(r=0, checkpoint=ck)), ctypes.byref(full)) == 0
        assert lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), ctypes.byref(some), 1) == 0
        assert lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), ctypes.byref(none), 1) == narrow[3] > 0
        assert lib.ftmi_ltx_ff_sample_workspace_bytes(ctypes.byref(cfg), ctypes.byref(full), 1) > narrow[3]


def test_the_planners_reproduce_every_recorded_row():
    """Every row recorded through both families at the parent of the fold -- accepted and refused (ff with r = 0, a partial pointer set, frames = 0 for the
    per-frame planners) -- and the offset of every name at layers 0 and L - 1, to the byte."""
    if not _lib.lib_available():
        pytest.skip("libftmi355.so is not built")
    import ltx_entry_bytes

    plans = ltx_entry_bytes.recorded()
    assert len(plans) >= 192 + 32 + 32
    assert sum(1 for v in plans.values() if v == (0,) * 6) >= 64 + 8 and sum(1 for k, v in plans.items() if k[2] == 0 and v[0] > 0 and v[1] == v[4] == v[5] == 0) >= 16
    for key, want in plans.items():
        assert ltx_entry_bytes.planned(*key) == want, (key, want)
    offsets = ltx_entry_bytes.recorded_offsets()
    assert {k[5] for k in offsets} == {0, 1} and len(offsets) == 4
    for key, want in offsets.items():
        assert ltx_entry_bytes.planned_offsets(*key) == want, key


# ---- narrow geometry -------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_narrow_geometry_refuses_the_ten_adapter_selection():
    from finetrainers_amd.ltx_video.narrow import MI355XNarrowLTXVideoTransformer3DModel

    tcfg = LTXTransformerConfig(in_channels=8, out_channels=8, num_attention_heads=4, attention_head_dim=8, cross_attention_dim=32, num_layers=1, caption_channels=32)
    m = MI355XNarrowLTXVideoTransformer3DModel(tcfg, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="narrow"):
        m.add_adapter(r=4, lora_alpha=4, target_modules=CONTROL)
    m.add_adapter(r=4, lora_alpha=4, target_modules=SFT)  # the eight are served as before
