"""The byte plans of the Wan LoRA block as recorded in tests/golden/wan_lora_entry_bytes.txt (from the library when it still had three entry families
that agreed on them) and as the one remaining planner pair, ``ftmi_wan_lora_ffn_block_{saved,scratch}_bytes``, returns them now."""
import ctypes
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wan_lora_entry_bytes.txt")
SURVIVING = ("ftmi_wan_lora_ffn_block_saved_bytes", "ftmi_wan_lora_ffn_block_scratch_bytes", "ftmi_wan_lora_ffn_block_forward", "ftmi_wan_lora_ffn_block_backward")
# the two narrow families folded into the wide one: neither declared nor exported any more, and the names stay unused
DELETED = tuple(f"ftmi_wan_{fam}lora_block_{fn}" for fam in ("", "i2v_") for fn in ("saved_bytes", "scratch_bytes", "forward", "backward"))


def recorded():
    """{(B, S, T, D, H, F, r, TI, ffn): (saved, scratch)}; (0, 0): a configuration the block refuses."""
    rows = [tuple(map(int, ln.split())) for ln in open(GOLDEN) if ln.strip() and not ln.startswith("#")]
    assert all(len(row) == 11 for row in rows)
    plans = {row[:9]: row[9:] for row in rows}
    assert len(plans) == len(rows)
    return plans


def config(B, S, T, D, H, F, r, TI=0, ffn=0):
    from finetrainers_amd import _lib

    return _lib.WanLoraFfnBlockConfig(B=B, S=S, T=T, D=D, H=H, F=F, eps=1e-6, gemm_variant=8, r=r, lora_scale=1.0, TI=TI, ffn=ffn)


def planned(B, S, T, D, H, F, r, TI=0, ffn=0):
    """(saved, scratch) bytes the library plans for this configuration."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    cfg = ctypes.byref(config(B, S, T, D, H, F, r, TI, ffn))
    return lib.ftmi_wan_lora_ffn_block_saved_bytes(cfg), lib.ftmi_wan_lora_ffn_block_scratch_bytes(cfg)


def assert_only_the_wide_family(lib, declared, exported):
    for name in SURVIVING:
        assert name in declared and name in exported and getattr(lib, name) is not None, name
    for name in DELETED:
        assert name not in declared and name not in exported and not hasattr(lib, name), name
