"""The workspace plans of the HunyuanVideo sampler as recorded in tests/golden/hy_sample_bytes.txt (from the library when ``ftmi_hy_sample_workspace_bytes`` still
stood beside ``ftmi_hy_sample_text_workspace_bytes`` and agreed with it at ``text_adapters = 0``) and as the one remaining planner returns them now."""
import ctypes
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hy_sample_bytes.txt")
SURVIVING = ("ftmi_hy_sample_text_workspace_bytes", "ftmi_hy_sample_text")
DELETED = ("ftmi_hy_sample_workspace_bytes", "ftmi_hy_sample")


def recorded():
    """{(B, F, H, W, P, T, Ld, Ls, r, steps, true_cfg, text_adapters): bytes}; 0: refused."""
    rows = [tuple(map(int, ln.split())) for ln in open(GOLDEN) if ln.strip() and not ln.startswith("#")]
    assert rows and all(len(row) == 13 for row in rows)
    plans = {row[:12]: row[12] for row in rows}
    assert len(plans) == len(rows)
    return plans


def config(B, F, H, W, P, T, Ld, Ls, r, steps, true_cfg, text_adapters=0):
    from finetrainers_amd import _lib

    geo = _lib.HySampleGeometry(B=B, C=16, F=F, H=H, W=W, p=2, pt=1, P=P)
    base = _lib.HySampleConfig(geo=geo, T=T, D=256, H=2, mlp=1024, Ld=Ld, Ls=Ls, r=r, lora_scale=1.0, eps=1e-6, gemm_variant=8, steps=steps, true_cfg=float(true_cfg))
    return _lib.HySampleTextConfig(base=base, text_adapters=text_adapters)


def planned(*key):
    from finetrainers_amd import _lib

    return _lib.load().ftmi_hy_sample_text_workspace_bytes(ctypes.byref(config(*key)))


def assert_only_the_text_entries(lib, declared, exported):
    for name in SURVIVING:
        assert name in declared and name in exported and getattr(lib, name) is not None, name
    for name in DELETED:
        assert name not in declared and name not in exported and not hasattr(lib, name), name
