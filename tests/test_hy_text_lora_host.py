"""HunyuanVideo text-stream adapters, host side (no GPU): the ``target_modules`` resolver over the model's module names, and the C ABI of the ``text_adapters``
field -- the struct layouts against include/ftmi355.h, the buffer plans with the flag off (pinned to the plans without the field) and on, and the refusals
that happen before any launch."""
import ctypes
import os
import re

import pytest

RECIPE = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|add_q_proj|add_k_proj|add_v_proj|to_add_out)"
DEFAULT = "(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0)"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ftmi355.h")


# ---- 7. resolver ---------------------------------------------------------------------------------------------------------------------------------------------------
def _cfg(nl=3, ns=2, refiner=2):
    from finetrainers_amd.hunyuan_video.model import HunyuanVideoTransformerConfig

    return HunyuanVideoTransformerConfig(num_attention_heads=2, attention_head_dim=128, num_layers=nl, num_single_layers=ns, num_refiner_layers=refiner,
                                         text_embed_dim=64, pooled_projection_dim=64)


def _per_block(selected):
    dual, single = {}, {}
    for n in selected:
        m = re.match(r"(single_transformer_blocks|transformer_blocks)\.(\d+)\.", n)
        assert m, n
        d = single if m.group(1).startswith("single") else dual
        d[int(m.group(2))] = d.get(int(m.group(2)), 0) + 1
    return dual, single


@pytest.mark.parametrize("full_size", [False, True])
def test_resolver_accepts_exactly_the_recipe_and_the_video_only_selection(full_size):
    from finetrainers_amd.hunyuan_video.model import HunyuanVideoTransformerConfig, linear_module_names, resolve_target_modules
    from finetrainers_amd.wan.model import select_module_names

    cfg = HunyuanVideoTransformerConfig() if full_size else _cfg()
    names = linear_module_names(cfg)
    assert len(names) == len(set(names))
    refiner = [n for n in names if "token_refiner" in n]
    assert f"context_embedder.token_refiner.refiner_blocks.{cfg.num_refiner_layers - 1}.attn.to_q" in refiner
    assert resolve_target_modules(cfg, RECIPE) is True
    assert resolve_target_modules(cfg, DEFAULT) is False
    assert resolve_target_modules(cfg, None) is False
    for target, per_dual in ((RECIPE, 8), (DEFAULT, 4)):
        sel = select_module_names(names, target)
        assert not set(sel) & set(refiner), "the refiner is never selected by an accepted regex"
        dual, single = _per_block(sel)
        assert dual == {i: per_dual for i in range(cfg.num_layers)} and single == {i: 3 for i in range(cfg.num_single_layers)}
        assert len(sel) == per_dual * cfg.num_layers + 3 * cfg.num_single_layers
    if full_size:
        assert len(select_module_names(names, RECIPE)) == 280 and len(select_module_names(names, DEFAULT)) == 200


@pytest.mark.parametrize("target,named", [
    (["to_q", "to_k", "to_v", "to_out.0"], "context_embedder.token_refiner.refiner_blocks.0.attn.to_q"),         # the suffix rule reaches the refiner
    (["to_q", "to_k", "to_v", "to_out.0", "add_q_proj", "add_k_proj", "add_v_proj", "to_add_out"], "context_embedder.token_refiner.refiner_blocks.0.attn.to_q"),
    ("transformer_blocks.*(to_q|to_k|to_v|to_out.0)", "single_transformer_blocks.0.attn.to_q"),                    # a subset: the single blocks left out
    ("(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v)", "transformer_blocks.0.attn.to_out.0"),   # a subset: to_out.0 left out
    ("(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|add_q_proj|add_k_proj|add_v_proj)", "transformer_blocks.0.attn.to_add_out"),
    ("(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|proj_out)", "single_transformer_blocks.0.proj_out"),
    ("(transformer_blocks|single_transformer_blocks).*(to_q|to_k|to_v|to_out.0|ff.net.0.proj|ff.net.2)", "transformer_blocks.0.ff.net.0.proj"),
    (".*(to_q|to_k|to_v|to_out.0)", "context_embedder.token_refiner.refiner_blocks.0.attn.to_q"),
    ("proj_out", "proj_out"),
])
def test_resolver_refuses_every_other_selection_naming_a_module(target, named):
    from finetrainers_amd.hunyuan_video.model import linear_module_names, resolve_target_modules

    cfg = _cfg()
    assert named in linear_module_names(cfg)
    with pytest.raises(NotImplementedError) as e:
        resolve_target_modules(cfg, target)
    assert named in str(e.value), str(e.value)


def test_resolver_shares_the_selection_rule_with_wan():
    """One statement of peft's rule: the Wan model's method and the HunyuanVideo resolver call the same function."""
    import inspect

    from finetrainers_amd.hunyuan_video import model as hy_model
    from finetrainers_amd.wan import model as wan_model

    assert hy_model.select_module_names is wan_model.select_module_names
    assert "select_module_names" in inspect.getsource(wan_model.MI355XWanTransformer3DModel.select_modules)
    assert "fullmatch" not in inspect.getsource(hy_model.resolve_target_modules)
    with pytest.raises(TypeError):
        hy_model.resolve_target_modules(_cfg(), 7)


# ---- 8. ABI --------------------------------------------------------------------------------------------------------------------------------------------------------
def _header_fields(struct_name):
    """[(type, name)] of ``typedef struct [tag] { ... } struct_name;`` in the header, comments stripped."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*" + struct_name + r"\s*;", text)
    assert m, struct_name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, first = decl.split(",")[0].rsplit(None, 1)  # "int T, S" -> type "int", names T, S
        for nm in [first] + decl.split(",")[1:]:
            out.append((typ.strip(), nm.strip()))
    return out


def _ctype_of(typ):
    from finetrainers_amd import _lib

    return {"int": ctypes.c_int, "float": ctypes.c_float, "ftmi_hy_sample_geometry": _lib.HySampleGeometry, "ftmi_hy_sample_config": _lib.HySampleConfig}[typ]


@pytest.mark.parametrize("c_name,py_name", [("ftmi_hy_dual_config", "HyDualConfig"), ("ftmi_hy_sample_text_config", "HySampleTextConfig")])
def test_text_adapters_is_the_last_field_and_the_ctypes_mirror_matches_the_header(c_name, py_name):
    """The dual block's configuration carries the flag as its trailing field.  The sampler's carries it as the trailing field of ftmi_hy_sample_text_config, the
    extension that embeds ftmi_hy_sample_config unchanged: that structure's size is pinned (tests/test_hy_sampling_host.py), so it cannot grow."""
    from finetrainers_amd import _lib

    struct = getattr(_lib, py_name)
    hdr = _header_fields(c_name)
    assert hdr[-1] == ("int", "text_adapters"), hdr[-1]
    assert struct._fields_[-1] == ("text_adapters", ctypes.c_int)
    assert [n for _, n in hdr] == [n for n, _ in struct._fields_]
    assert [_ctype_of(t) for t, _ in hdr] == [t for _, t in struct._fields_]
    expected = type("Expected_" + py_name, (ctypes.Structure,), {"_fields_": [(n, _ctype_of(t)) for t, n in hdr]})
    assert ctypes.sizeof(struct) == ctypes.sizeof(expected)
    assert getattr(struct, "text_adapters").offset == ctypes.sizeof(struct) - ctypes.sizeof(ctypes.c_int)
    if c_name == "ftmi_hy_sample_text_config":  # the embedded structures are themselves mirrors of their header structs, and the base is what it was
        assert hdr[0] == ("ftmi_hy_sample_config", "base") and struct.base.offset == 0
        base = _header_fields("ftmi_hy_sample_config")
        assert [n for _, n in base] == [n for n, _ in _lib.HySampleConfig._fields_] and [_ctype_of(t) for t, _ in base] == [t for _, t in _lib.HySampleConfig._fields_]
        assert "text_adapters" not in [n for _, n in base]
        assert ctypes.sizeof(_lib.HySampleConfig) == ctypes.sizeof(type("ExpectedBase", (ctypes.Structure,), {"_fields_": [(n, _ctype_of(t)) for t, n in base]}))
        geo = _header_fields("ftmi_hy_sample_geometry")
        assert [n for _, n in geo] == [n for n, _ in _lib.HySampleGeometry._fields_] and all(t == "int" for t, _ in geo)
        declared = open(HEADER).read()
        for sym in ("ftmi_hy_sample_text_workspace_bytes", "ftmi_hy_sample_text"):
            assert re.search(r"\b" + sym + r"\s*\(", declared) and sym in _lib.EXPORTED_SYMBOLS and getattr(_lib.load(), sym) is not None
    assert struct().text_adapters == 0  # callers that build the struct by keyword without the field get the old behaviour


def _dual_cfg(**kw):
    from finetrainers_amd import _lib

    base = dict(T=8, S=40, D=256, H=2, mlp=1024, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    base.update(kw)
    return _lib.HyDualConfig(**base)


def _dual_bytes(cfg):
    from finetrainers_amd import _lib

    lib = _lib.load()
    return lib.ftmi_hy_dual_saved_bytes(ctypes.byref(cfg)), lib.ftmi_hy_dual_scratch_bytes(ctypes.byref(cfg))


def _a256(n):
    return (n + 255) & ~255


def _dual_plan_without_the_field(T, S, D, H, mlp, r):
    """The dual block's buffer plan as it stood before the field existed (csrc/hy_dit.hip make_dual_layout: every area rounded up to 256 bytes)."""
    N = S + T
    saved = [2 * 6 * D * 2] * 2 + [S * D * 2, T * D * 2, S * D * 2, S * D * 2, T * D * 2, T * D * 2] + [N * D * 2] * 4 + [H * N * 4, S * D * 2, T * D * 2, S * mlp * 2, T * mlp * 2,
                                                                                                                       4 * S * 3 * r * 2]
    fwd = [S * D * 2, T * D * 2, S * D * 2, T * D * 2, S * mlp * 2, T * mlp * 2, S * D * 2, T * D * 2, 4 * 2 * r * D * 2, 4 * D * 3 * r * 2]
    bwd = [S * D * 2, T * D * 2, S * mlp * 2, T * mlp * 2] + [S * D * 2, T * D * 2] * 3 + [N * D * 2] * 4 + [H * N * 4] + [S * D * 2] * 6 + [T * D * 2] * 6 + [
        S * 3 * r * 2, 4 * 2 * r * D * 2, 4 * D * 3 * r * 2]
    tot = lambda parts: sum(_a256(p) for p in parts)
    return tot(saved), max(tot(fwd), tot(bwd))


@pytest.mark.parametrize("T,S,r", [(8, 40, 64), (72, 40, 64), (16, 150, 0), (256, 32640, 64), (24, 200, 128)])
def test_dual_buffer_plans_with_the_flag_off_are_the_plans_without_the_field(T, S, r):
    from finetrainers_amd import _lib

    assert ("text_adapters", ctypes.c_int) in _lib.HyDualConfig._fields_  # (a ctypes Structure takes an unknown keyword as a plain attribute: no field, no test)
    D, H, mlp = (3072, 24, 12288) if S > 10000 else (256, 2, 1024)
    implicit = _dual_bytes(_dual_cfg(T=T, S=S, D=D, H=H, mlp=mlp, r=r))
    explicit = _dual_bytes(_dual_cfg(T=T, S=S, D=D, H=H, mlp=mlp, r=r, text_adapters=0))
    assert implicit == explicit == _dual_plan_without_the_field(T, S, D, H, mlp, r)


@pytest.mark.parametrize("T,S,r", [(8, 40, 64), (72, 40, 64), (256, 32640, 64), (24, 200, 128)])
def test_dual_buffer_plans_with_the_flag_on_hold_the_text_rows(T, S, r):
    D, H, mlp = (3072, 24, 12288) if S > 10000 else (256, 2, 1024)
    s0, c0 = _dual_bytes(_dual_cfg(T=T, S=S, D=D, H=H, mlp=mlp, r=r))
    s1, c1 = _dual_bytes(_dual_cfg(T=T, S=S, D=D, H=H, mlp=mlp, r=r, text_adapters=1))
    assert s1 - s0 == _a256(4 * T * 3 * r * 2)  # the text rows' down-projections, xa's per-row format, four adapters
    assert c1 > c0
    # eight instead of four operand copies in each direction's area, dxa over max(S, T) rows
    fwd_extra = _a256(8 * 2 * r * D * 2) + _a256(8 * D * 3 * r * 2) - _a256(4 * 2 * r * D * 2) - _a256(4 * D * 3 * r * 2)
    bwd_extra = fwd_extra + _a256(max(S, T) * 3 * r * 2) - _a256(S * 3 * r * 2)
    assert c1 - c0 in (fwd_extra, bwd_extra) and c1 - c0 >= fwd_extra


def test_scratch_with_the_flag_on_grows_with_the_text_rows_beyond_the_video_rows():
    """T > S is legal: the down-projection gradient of the text rows needs T rows, where the plan without the flag holds S."""
    S, r = 8, 64
    sizes = [_dual_bytes(_dual_cfg(T=T, S=S, r=r, text_adapters=1)) for T in (8, 72, 136)]
    off = [_dual_bytes(_dual_cfg(T=T, S=S, r=r)) for T in (8, 72, 136)]
    grow_on = [b[1] - a[1] for a, b in zip(sizes, sizes[1:])]
    grow_off = [b[1] - a[1] for a, b in zip(off, off[1:])]
    assert all(g > 0 for g in grow_on)
    assert all(on - of == _a256(64 * 3 * r * 2) for on, of in zip(grow_on, grow_off))  # 64 more rows of dxa per 64 more text rows, on top of what grows anyway
    assert all(b[0] > a[0] for a, b in zip(sizes, sizes[1:]))


def _refused_dual(cfg):
    """ftmi_hy_dual_forward / _backward on host memory: a refused configuration returns before anything is launched or read."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    w = _lib.HyDualWeights()
    bufs = [ctypes.create_string_buffer(4096) for _ in range(8)]
    p = [ctypes.addressof(b) for b in bufs]
    rc_f = lib.ftmi_hy_dual_forward(ctypes.byref(cfg), ctypes.byref(w), p[0], p[1], p[2], None, None, None, p[3], p[4], p[5], 1 << 40, p[6], 1 << 40, None)
    msg_f = _lib.last_error()
    rc_b = lib.ftmi_hy_dual_backward(ctypes.byref(cfg), ctypes.byref(w), p[0], p[1], p[2], p[3], None, None, None, p[4], p[5], p[6], None, None, p[7], 1 << 40, p[7], 1 << 40,
                                     None)
    msg_b = _lib.last_error()
    return (rc_f, msg_f), (rc_b, msg_b)


@pytest.mark.parametrize("kw,what", [(dict(text_adapters=1, r=0), "need a LoRA rank"), (dict(text_adapters=2), "0 or 1"), (dict(text_adapters=-1), "0 or 1"),
                                     (dict(text_adapters=8), "0 or 1")])
def test_bad_text_adapters_values_are_refused_before_any_launch(kw, what):
    from finetrainers_amd import _lib

    for rc, msg in _refused_dual(_dual_cfg(**kw)):
        assert rc == _lib.FTMI_ERR_INVALID and "hy_dual" in msg and what in msg, (rc, msg)
    assert _dual_bytes(_dual_cfg(**kw)) == (0, 0) and what in _lib.last_error()  # the planners size nothing from a refused flag


def _sample_cfg(**kw):
    from finetrainers_amd import _lib

    geo = _lib.HySampleGeometry(B=1, C=16, F=3, H=8, W=12, p=2, pt=1, P=1)
    base = dict(geo=geo, T=8, D=256, H=2, mlp=1024, Ld=2, Ls=1, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8, steps=2, true_cfg=1.0)
    text = kw.pop("text_adapters", None)
    base.update(kw)
    cfg = _lib.HySampleTextConfig(base=_lib.HySampleConfig(**base))
    if text is not None:
        cfg.text_adapters = text
    return cfg


def test_sample_workspace_follows_the_dual_layout_and_refuses_bad_flags():
    from finetrainers_amd import _lib

    lib = _lib.load()
    import hy_sample_bytes

    ws = lambda cfg: lib.ftmi_hy_sample_text_workspace_bytes(ctypes.byref(cfg))
    off, explicit, on = ws(_sample_cfg()), ws(_sample_cfg(text_adapters=0)), ws(_sample_cfg(text_adapters=1))
    # the field left at its default, the field set to 0, and what the planner over the bare ftmi_hy_sample_config returned before it went
    assert off == explicit == hy_sample_bytes.recorded()[(1, 3, 8, 12, 1, 8, 2, 1, 64, 2, 1, 0)] > 0
    d0 = _dual_bytes(_dual_cfg(T=8, S=72))
    d1 = _dual_bytes(_dual_cfg(T=8, S=72, text_adapters=1))
    single = _lib.HySingleConfig(B=1, T=8, S=72, D=256, H=2, mlp=1024, r=64, lora_scale=1.0, eps=1e-6, gemm_variant=8)
    s = (lib.ftmi_hy_single_saved_bytes(ctypes.byref(single)), lib.ftmi_hy_single_scratch_bytes(ctypes.byref(single)))
    assert on - off == sum(max(a, c) - max(b, c) for a, b, c in zip(d1, d0, s))  # ONE saved slot and ONE scratch area, each the larger of the two blocks' needs
    assert ws(_sample_cfg(Ld=2, Ls=0, text_adapters=1)) - ws(_sample_cfg(Ld=2, Ls=0)) == sum(a - b for a, b in zip(d1, d0)) > 0
    for kw in (dict(text_adapters=1, r=0), dict(text_adapters=2), dict(text_adapters=-1)):
        cfg = _sample_cfg(**kw)
        assert ws(cfg) == 0
        assert "text_adapters" in _lib.last_error()
        w = _lib.HySampleWeights()
        buf = ctypes.create_string_buffer(4096)
        p = ctypes.addressof(buf)
        rc = lib.ftmi_hy_sample_text(ctypes.byref(cfg), ctypes.byref(w), p, p, p, p, p, p, None, p, p, p, p, 1 << 40, None)
        assert rc == _lib.FTMI_ERR_INVALID and "text_adapters" in _lib.last_error()


def test_the_sample_planner_reproduces_every_recorded_row():
    """Every row recorded at the parent of the fold through ftmi_hy_sample_workspace_bytes (text_adapters = 0, where the two planners agreed) and through
    ftmi_hy_sample_text_workspace_bytes, the refused ones (text_adapters = 1 with r = 0, text_adapters = 2) as 0."""
    import hy_sample_bytes

    plans = hy_sample_bytes.recorded()
    assert {k[11] for k in plans} == {0, 1, 2} and any(v > 0 for k, v in plans.items() if k[11] == 1)
    assert all(v == 0 for k, v in plans.items() if k[11] == 2 or (k[11] == 1 and k[8] == 0)) and all(v > 0 for k, v in plans.items() if k[11] == 0)
    for key, want in plans.items():
        assert hy_sample_bytes.planned(*key) == want, (key, want)
