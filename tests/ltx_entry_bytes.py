"""The byte plans of the LTX-Video workspace planners as recorded in tests/golden/ltx_entry_bytes.txt (from the library when it still had two entry families,
the narrow ``ftmi_ltx_*`` over ``ftmi_ltx_weights`` and the wide ``ftmi_ltx_ff_*``, that agreed on them) and as the one remaining family returns them now."""
import ctypes
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ltx_entry_bytes.txt")
SURVIVING = tuple("ftmi_ltx_ff_" + n for n in ("workspace_bytes", "workspace_offset", "forward", "forward_frames_workspace_bytes", "forward_frames", "backward_range",
                                               "sample_workspace_bytes", "sample", "sample_cond_workspace_bytes", "sample_cond"))
# the narrow family folded into the wide one: neither declared nor exported any more, and the names stay unused
DELETED = tuple("ftmi_ltx_" + n for n in ("workspace_bytes", "workspace_offset", "forward", "forward_frames_workspace_bytes", "forward_frames", "backward_range",
                                          "backward", "sample_workspace_bytes", "sample", "sample_cond_workspace_bytes", "sample_cond"))
# every name ftmi_ltx_ff_workspace_offset knows, in the column order of the offset rows
OFFSET_NAMES = ("kv2_all", "k2n_all", "xa_kv2_all", "e", "emb", "temb", "ada", "ada_out", "tsin", "hs", "n1", "qkv", "qrot", "krot", "o1", "lse1", "xa_qkv", "xa_o", "h1",
                "q2raw", "q2n", "o2", "lse2", "xa_q2", "xa_o2", "h2", "z", "xa_ff1", "xa_ff2")


def _rows():
    return [tuple(map(int, ln.split())) for ln in open(GOLDEN) if ln.strip() and not ln.startswith("#")]


def recorded():
    """{(B, S, frames, L, r, checkpoint, ff): (workspace, forward_frames(frames), sample(0), sample(1), sample_cond(0, frames), sample_cond(1, frames))};
    0: the planner refuses the row."""
    rows = [row for row in _rows() if len(row) == 13]
    plans = {row[:7]: row[7:] for row in rows}
    assert len(plans) == len(rows) > 0
    return plans


def recorded_offsets():
    """{(B, S, L, r, checkpoint, ff, layer): one offset per OFFSET_NAMES}; -1: the name is refused."""
    rows = [row for row in _rows() if len(row) != 13]
    assert rows and all(len(row) == 7 + len(OFFSET_NAMES) for row in rows)
    return {row[:7]: row[7:] for row in rows}


def config(B, S, L, r, checkpoint=0, **kw):
    from finetrainers_amd import _lib

    base = dict(B=B, S=S, T=128, D=2048, H=32, L=L, C_in=128, C_out=128, D_ff=8192, D_cap=4096, r=r, lora_scale=1.0, eps_norm=1e-6, eps_qk=1e-5, gemm_variant=8,
                checkpoint=checkpoint, d_valid=0, head_dim_valid=0)
    base.update(kw)
    return _lib.LtxConfig(**base)


def weights(ff=0):
    """``LtxFfWeights`` as the planners read it (never dereferenced).  ff: 0 = NULL extension, 1 = all eight pointers, 2 = the first only, 3 = all but the first."""
    from finetrainers_amd import _lib

    w = _lib.LtxFfWeights()
    for n in {0: [], 1: _lib.LTX_FF_WEIGHT_FIELDS, 2: _lib.LTX_FF_WEIGHT_FIELDS[:1], 3: _lib.LTX_FF_WEIGHT_FIELDS[1:]}[ff]:
        setattr(w, n, 256)
    return w


def planned(B, S, frames, L, r, checkpoint=0, ff=0):
    """The six byte counts the library plans for this row, in the order of ``recorded()``."""
    from finetrainers_amd import _lib

    lib = _lib.load()
    c, w = ctypes.byref(config(B, S, L, r, checkpoint)), ctypes.byref(weights(ff))
    return (lib.ftmi_ltx_ff_workspace_bytes(c, w), lib.ftmi_ltx_ff_forward_frames_workspace_bytes(c, w, frames), lib.ftmi_ltx_ff_sample_workspace_bytes(c, w, 0),
            lib.ftmi_ltx_ff_sample_workspace_bytes(c, w, 1), lib.ftmi_ltx_ff_sample_cond_workspace_bytes(c, w, 0, frames),
            lib.ftmi_ltx_ff_sample_cond_workspace_bytes(c, w, 1, frames))


def planned_offsets(B, S, L, r, checkpoint, ff, layer):
    from finetrainers_amd import _lib

    lib = _lib.load()
    out = []
    for name in OFFSET_NAMES:
        off = ctypes.c_size_t(0)
        rc = lib.ftmi_ltx_ff_workspace_offset(ctypes.byref(config(B, S, L, r, checkpoint)), ctypes.byref(weights(ff)), name.encode(), layer, ctypes.byref(off))
        out.append(off.value if rc == 0 else -1)
    return tuple(out)


def assert_only_the_wide_family(lib, declared, exported):
    for name in SURVIVING:
        assert name in declared and name in exported and getattr(lib, name) is not None, name
    for name in DELETED:
        assert name not in declared and name not in exported and not hasattr(lib, name), name
