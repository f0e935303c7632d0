"""CogVideoX validation sampling with the 5b checkpoints' DPM multistep scheduler, on the GPU: the step kernel per element against fp64 with a bound derived
from its rounding points, the noise packer against the reference's patchify bit for bit, the one-call loop (``ftmi_cog_sample_ms``) against its composition
from ``model.forward`` and ``ops.cog_sample_step_dpm`` bit for bit, the trajectory against the stepwise scheduler of tests/cog_dpm_reference.py over the oracle
model in bf16 and fp32, and the public path."""
import pytest
import torch

import cog_dpm_reference as dref
import cog_sampling_reference as ref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
C = 16
# (F, H, W): at patch_size_t = 2 the first is ONE token of 128 columns (two tokens of 64 at 1); the second has 48 / 24 tokens, runs of 12 elements that start
# off the 16-byte grid, and a tail in the step's only workgroup
GRIDS = [(2, 2, 2), (4, 4, 6)]
NAN = float("nan")
N_STEPS = 4


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _geo(B, P, F_, H, W, pt, drop=0):
    from finetrainers_amd import ops

    return ops.cog_sample_geometry(B, C, F_, H, W, patch=2, patch_t=pt if pt > 1 else None, guidance=P == 2, drop=drop)


def _dims(F_, H, W, pt):
    return (F_ // pt) * (H // 2) * (W // 2), C * pt * 4


def _dpm(zero_snr=True, shift=1.0):
    from finetrainers_amd.cogvideox import COG_DPM_SCHEDULER_CONFIG

    return dict(COG_DPM_SCHEDULER_CONFIG, rescale_betas_zero_snr=zero_snr, snr_shift_scale=shift)


# ---- 1. the step kernel ----------------------------------------------------------------------------------------------------------------------------------------
def _rows(guidance):
    """Four rows of real tables (n = 4, snr shift 3): step 0 with zero terminal SNR (sa = m0 = e1 = 0: x itself drops out of x0 and of x'), step 2 of the same
    table (all six numbers in play), its last row (x' = x0: no history, no noise) and step 1 without the zero-SNR rescale (a full row again, other numbers)."""
    from finetrainers_amd.cogvideox import cog_dpm_tables

    on, off = cog_dpm_tables(4, _dpm(True, 3.0), guidance)[1], cog_dpm_tables(4, _dpm(False, 3.0), guidance)[1]
    rows = {"zero_snr_step0": on[0], "full": on[2], "last": on[3], "plain_step1": off[1]}
    assert on[0, [0, 2, 4]].tolist() == [0, 0, 0] and bool((on[2, :6] != 0).all()) and on[3, 2:6].tolist() == [0, 1, 0, 0] and bool((off[1, :6] != 0).all())
    return rows


def _step_inputs(B, P, S, Kc):
    """pred on the 1 / 16 grid: |u|, |c| < 4.5 are bf16 values (7 significant bits), c - u and g (c - u) + u (g = 6: |v| < 59) are multiples of 1 / 16 below
    2^6, exact in fp32 -- v carries NO rounding.  x, old, z: three different random fp32 tensors, different in every element and token."""
    g = torch.Generator().manual_seed(S + 3 * B + P + Kc)
    tok = torch.arange(B * S, dtype=torch.float32).view(B, S, 1)
    col = torch.arange(Kc, dtype=torch.float32)
    grid = (col % 64 - 31.5) / 8 + (tok % 7) / 16 + (col // 64) / 16
    cond = grid.to(bf16)
    assert torch.equal(cond.float(), grid)
    unc = (torch.randint(-64, 65, (B, S, Kc), generator=g).float() / 16).to(bf16)
    pred = cond if P == 1 else torch.cat([unc, cond])
    bufs = [torch.randn(B, S, Kc, generator=g) * 2 + k for k in (0.5, -1.0, 1.5)]
    return pred, bufs


@pytest.mark.parametrize("form", ["zero_snr_step0", "full", "last", "plain_step1"])
@pytest.mark.parametrize("guidance", [1.0, 6.0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_dpm_step_against_fp64(F_, H, W, pt, B, guidance, form):
    """The bound, from the kernel's rounding points (sample_layout.hip cog_sample_step_dpm_kernel; every mul or fma rounds once, by at most 2^-24 of its result):
      v    exact (the inputs sit on the 1 / 16 grid, see _step_inputs; g = 6 is read from the row)
      x0   = fma(-sb, v, sa x): the product and the fma,                        |dx0| <= 2 eps M,       M = sa |x| + sb |v|
      x'   n_t non-zero terms = one mul and n_t - 1 fmas, each partial sum below A = |m0| |x| + |e0| M + |e1| |old| + |mn| |z|, plus e0 dx0 <= 2 eps A:
                                                                                 |dx'| <= (n_t + 2) eps A
    eps = 2^-24 (1 + 2^-10): the second-order terms sit inside the factor.  The row is the fp32 one the kernel reads, so it adds nothing.  m0 x is computed even
    when m0 = 0 (a product of zero: exact), so n_t counts the non-zero ones.  The buffers differ by O(1) in every element: a swapped buffer or a misplaced
    column moves the result by ~2^20 times the bound.  Buffers whose coefficient is zero hold NaN (noise is not even passed on the last row): nothing of them
    may reach a result."""
    from finetrainers_amd import ops

    dev = _dev()
    P = 2 if guidance != 1.0 else 1
    geo = _geo(B, P, F_, H, W, pt)
    S, Kc = _dims(F_, H, W, pt)
    row = _rows(guidance)[form]
    sa, sb, m0, e0, e1, mn, g, pad = row.tolist()
    assert g == guidance and pad == 0.0
    pred, (x0_, old0, z0) = _step_inputs(B, P, S, Kc)
    want_x, want_old, v = dref.step_ref(pred, x0_, old0, z0, row.double(), guidance)
    M = sa * x0_.double().abs() + sb * v.abs()
    A = abs(m0) * x0_.double().abs() + abs(e0) * M + (abs(e1) * old0.double().abs() if e1 != 0 else 0) + (abs(mn) * z0.double().abs() if mn != 0 else 0)
    n_t = sum(c != 0 for c in (m0, e0, e1, mn))
    eps = 2.0 ** -24 * (1 + 2.0 ** -10)
    sentinel = torch.full((P * B * S, Kc), -7.0, dtype=bf16)
    x = x0_.to(dev, copy=True)
    old = (old0 if e1 != 0 else torch.full_like(old0, NAN)).to(dev, copy=True)
    z = None if form == "last" else (z0 if mn != 0 else torch.full_like(z0, NAN)).to(dev, copy=True)
    cols = sentinel.to(dev, copy=True)
    ops.cog_sample_step_dpm(geo, pred.to(dev), x, old, z, row.to(dev), cols)
    torch.cuda.synchronize()
    x, old, cols = x.cpu(), old.cpu(), cols.cpu()
    for name, got, want, bound in (("old", old, want_old, 2 * eps * M), ("x'", x, want_x, (n_t + 2) * eps * A)):
        assert bool(torch.isfinite(got).all()), name
        frac = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())  # v = 0 at sa = 0 makes M = 0: the error must be 0 there too
        print(f"[cog_sample_step_dpm {form} pt={pt} B={B} S={S} Kc={Kc} g={guidance}] {name}: max error / bound {frac:.3f}")
        assert frac <= 1.0, name
    assert not torch.equal(x, x0_)
    if z is not None:
        assert torch.equal(_bits(z.cpu()), _bits(z0 if mn != 0 else torch.full_like(z0, NAN))), "noise is read only"
    rne = x.to(bf16).view(B * S, Kc)
    for p in range(P):
        assert torch.equal(_bits(cols[p * B * S:(p + 1) * B * S]), _bits(rne)), p
    if form == "last":
        assert torch.equal(_bits(x), _bits(old)), "x' IS x0 on the last row (m0 x = +-0, then fma(1, x0, .))"


def test_dpm_step_without_cols_updates_the_state_alone():
    from finetrainers_amd import ops

    dev = _dev()
    F_, H, W, pt, B = 4, 4, 6, 1, 2
    S, Kc = _dims(F_, H, W, pt)
    row = _rows(6.0)["full"]
    pred, (x0_, old0, z0) = _step_inputs(B, 2, S, Kc)
    got = []
    for with_cols in (True, False):
        x, old = x0_.to(dev, copy=True), old0.to(dev, copy=True)
        cols = torch.zeros(2 * B * S, Kc, dtype=bf16, device=dev) if with_cols else None
        ops.cog_sample_step_dpm(_geo(B, 2, F_, H, W, pt), pred.to(dev), x, old, z0.to(dev), row.to(dev), cols)
        torch.cuda.synchronize()
        got.append((x.cpu(), old.cpu()))
    assert torch.equal(_bits(got[0][0]), _bits(got[1][0])) and torch.equal(_bits(got[0][1]), _bits(got[1][1]))


# ---- 2. the noise packer -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("pt", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_pack_is_patchify_of_every_tensor_bit_for_bit(F_, H, W, pt, B, n):
    from finetrainers_amd import ops

    dev = _dev()
    S, Kc = _dims(F_, H, W, pt)
    lat = torch.randn(n, B, F_, C, H, W, generator=torch.Generator().manual_seed(n + 5 * B + pt))
    out = torch.full((n + 1, B, S, Kc), -7.0, device=dev)
    for P in (1, 2):  # the row groups of the geometry do not matter to pack: it writes no cols
        got = ops.cog_sample_pack(_geo(B, P, F_, H, W, pt), lat.to(dev), out=out)
        torch.cuda.synchronize()
        assert got is out
        for i in range(n):
            assert torch.equal(_bits(out[i].cpu()), _bits(ref.patchify(lat[i], 2, pt))), (P, i)
        assert bool((out[n] == -7.0).all()), "the slice past n is untouched"
    fresh = ops.cog_sample_pack(_geo(B, 2, F_, H, W, pt), lat.to(dev))
    assert fresh.shape == (n, B, S, Kc) and torch.equal(_bits(fresh.cpu()), _bits(out[:n].cpu()))
    x, _ = ops.cog_sample_init(_geo(B, 2, F_, H, W, pt), lat[0].to(dev))
    assert torch.equal(_bits(x.cpu()), _bits(fresh[0].cpu())), "one index map: init's x"


# ---- 3. the loop is its composition --------------------------------------------------------------------------------------------------------------------------------
CLIP = (3, 8, 12)  # 72 video tokens + 16 text tokens: 88 joint keys, ragged


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind):
        if kind not in cache:
            omodel = ref.oracle_model(kind)
            cache[kind] = (omodel, ref.gpu_model(omodel, kind, _dev()))
        return cache[kind]

    return get


def _case(kind, n, B=1, seed=21):
    F_, H, W = CLIP
    pt = 2 if kind == "1.5" else 1
    drop = (pt - F_ % pt) % pt  # 1.5: 3 frames -> 4 drawn, the first dropped after the loop
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(B, F_ + drop, C, H, W, generator=g).to(bf16).float()  # bf16-exact: the bf16 oracle, the fp32 oracle and the kernels start from one state
    text = torch.randn(B, 16, 4096, generator=g).to(bf16)
    neg = torch.randn(B, 16, 4096, generator=g).to(bf16)
    step_noise = torch.randn(n, B, F_ + drop, C, H, W, generator=g).to(bf16).float()  # bf16 draws, as the pipeline's
    return dict(noise=noise, text=text, neg=neg, pt=pt, drop=drop, step_noise=step_noise)


def _tables(sampler, n, guidance, dynamic):
    from finetrainers_amd.cogvideox import cog_dpm_tables

    ts, rows = cog_dpm_tables(n, sampler.scheduler_config, guidance, dynamic)
    k = max([i + 1 for i in range(n) if float(rows[i, 5]) != 0.0], default=0)
    return ts, rows, k


def _one_call(sampler, c, guidance, n=N_STEPS, dynamic=False):
    """``ftmi_cog_sample_ms`` piece by piece as ``MI355XCogVideoXLatentSampler.sample`` prepares it, keeping the fp32 state; the ``old`` buffer behind the DDIM
    workspace starts as all-ones bytes, which are NaN in fp32."""
    from finetrainers_amd import ops

    dev = _dev()
    ts, rows, k = _tables(sampler, n, guidance, dynamic)
    noise = c["noise"].to(dev)
    B, F_, _, H, W = noise.shape
    geo = sampler.geometry(B, F_, H, W, guidance != 1.0, c["drop"])
    text = (c["text"] if guidance == 1.0 else torch.cat([c["neg"], c["text"]])).to(dev)
    temb, shift, onep = sampler.step_tables(ts, geo.P * B)
    cfg, w, keep = sampler.c_arguments(geo, n, guidance)
    x, cols = ops.cog_sample_init(geo, noise)
    z = ops.cog_sample_pack(geo, c["step_noise"][:k].to(dev).contiguous()) if k else None
    need, ddim = ops.cog_sample_ms_workspace_bytes(cfg), ops.cog_sample_workspace_bytes(cfg)
    assert need == ddim + (4 * x.numel() + 255) // 256 * 256
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws[ddim:] = 255
    ops.cog_sample_ms(cfg, w, cols, x, text, temb, shift, onep, rows.to(dev), z, workspace=ws)
    out = ops.cog_sample_finish(geo, x, 1.0 / 1.15258426)
    torch.cuda.synchronize()
    return x, out


def _composition(sampler, c, guidance, n=N_STEPS, dynamic=False):
    """The same loop from the model's training forward (under no_grad) and ``ops.cog_sample_step_dpm``: one Python round trip per launch group.  The noise
    slices come from the reference's patchify, not from the packer."""
    from finetrainers_amd import ops
    from finetrainers_amd.cogvideox.model import rotary_tables

    dev = _dev()
    gmodel = sampler.transformer
    ts, rows, k = _tables(sampler, n, guidance, dynamic)
    rows = rows.to(dev)
    noise = c["noise"].to(dev)
    B, F_, _, H, W = noise.shape
    pt, P = c["pt"], 2 if guidance != 1.0 else 1
    geo = _geo(B, P, F_, H, W, pt, c["drop"])
    text = (c["text"] if P == 1 else torch.cat([c["neg"], c["text"]])).to(dev)
    rope = tuple(t.to(dev) for t in rotary_tables(gmodel.config, H, W, F_)) if gmodel.config.use_rotary_positional_embeddings else None
    x, cols = ops.cog_sample_init(geo, noise)
    old = torch.full_like(x, NAN)
    S = cols.shape[0] // (P * B)
    with torch.no_grad():
        for i, t in enumerate(ts.tolist()):
            inp = ref.unpatchify(cols[:B * S].view(B, S, -1), F_, C, H, W, 2, pt)  # bf16(x), as the pipeline hands the latents to the transformer
            inp = torch.cat([inp] * P)
            vel = gmodel(inp, text, torch.full((P * B,), t, dtype=torch.int64, device=dev), image_rotary_emb=rope)[0]
            z = ref.patchify(c["step_noise"][i], 2, pt).to(dev) if i < k else None
            ops.cog_sample_step_dpm(geo, ref.patchify(vel, 2, pt), x, old, z, rows[i], cols)
    out = ops.cog_sample_finish(geo, x, 1.0 / 1.15258426)
    torch.cuda.synchronize()
    return x, out


def _assert_same(sampler, c, guidance, dynamic=False, tag=""):
    x1, out1 = _one_call(sampler, c, guidance, dynamic=dynamic)
    x2, out2 = _composition(sampler, c, guidance, dynamic=dynamic)
    assert out1.shape == (c["noise"].shape[0], CLIP[0], C, CLIP[1], CLIP[2]), "the padded leading frame is dropped"
    assert bool(torch.isfinite(x1).all())
    diff = int((_bits(x1.cpu()) != _bits(x2.cpu())).sum())
    moved = float((x1.cpu() - ref.patchify(c["noise"], 2, c["pt"])).norm() / c["noise"].norm())
    print(f"[cog_sample_ms vs composition {tag} g={guidance} dynamic={dynamic}] differing state elements: {diff} of {x1.numel()}; moved {moved:.3f}")
    assert diff == 0 and torch.equal(_bits(out1.cpu()), _bits(out2.cpu()))
    assert moved > 0.1, "the loop moved the state"


@pytest.mark.parametrize("guidance", [6.0, 1.0])
@pytest.mark.parametrize("kind", ["sincos", "rotary", "1.5"])
def test_one_call_ms_loop_is_its_composition_bit_for_bit(models, kind, guidance):
    """2 blocks, rank-64 adapters with non-zero B, 4 steps of the checkpoints' table: the smallest run with a first step (no history), a second one whose
    history coefficient is zero (r = inf after the zero-SNR step), a full multistep step and a last step without noise."""
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    _, gmodel = models(kind)
    assert float(gmodel.lora_flat.detach().abs().max()) > 0
    sampler = MI355XCogVideoXLatentSampler(gmodel, _dpm())
    _, rows, k = _tables(sampler, N_STEPS, guidance, False)
    assert [bool(v) for v in rows[:, 4] != 0] == [False, False, True, False] and [bool(v) for v in rows[:, 5] != 0] == [True, True, True, False] and k == 3
    _assert_same(sampler, _case(kind, N_STEPS, B=2 if kind == "sincos" else 1), guidance, tag=kind)


def test_one_call_ms_loop_with_dynamic_cfg(models):
    """A guidance scale per step, read from the rows (5b geometry, no zero-SNR rescale: the history enters at step 1)."""
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler

    _, gmodel = models("rotary")
    sampler = MI355XCogVideoXLatentSampler(gmodel, _dpm(False, 3.0))
    _, rows, _ = _tables(sampler, N_STEPS, 6.0, True)
    assert len(set(rows[:, 6].tolist())) > 1 and [bool(v) for v in rows[:, 4] != 0] == [False, True, True, False]
    _assert_same(sampler, _case("rotary", N_STEPS, seed=5), 6.0, dynamic=True, tag="rotary dpm")


# ---- 4. the trajectory ---------------------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_dpm_trajectory_against_the_oracle(models):
    """The rule of test_gpu_cog_sampling.py::test_trajectory_against_the_oracle with the multistep scheduler: the STEPWISE scheduler of tests/cog_dpm_reference.py
    over ``oracle.cogvideox`` twice -- in bf16 with the state rounded to bf16 after every step, as upstream does, and as an fp32 copy of the same weights -- and
    ``ftmi_cog_sample_ms``, the same initial and per-step noise for all three, 5 steps of the 5b checkpoints' table, guidance 6: d_kernel = rel_l2(kernels,
    fp32) may not exceed 1.5 d_oracle = 1.5 rel_l2(bf16, fp32).  The state must have moved by more than 0.1 relative, so that a loop that does nothing fails.
    Measured on an MI355X: d_oracle 1.268e-2, d_kernel 1.248e-2 (ratio 0.98), the state moved by 1.520."""
    from finetrainers_amd.cogvideox import CogVideoXDDIMTables, MI355XCogVideoXLatentSampler

    n = 5
    omodel, gmodel = models("sincos")
    c = _case("sincos", n, seed=33)
    sched = dref.dpm_schedule(n, CogVideoXDDIMTables(snr_shift_scale=1.0, rescale_betas_zero_snr=True).alphas_cumprod)
    t16 = dref.trajectory(omodel, bf16, c["noise"], c["text"], c["neg"], sched, 6.0, c["step_noise"], round_state=True).float()
    t32 = dref.trajectory(ref.fp32_copy(omodel), torch.float32, c["noise"], c["text"], c["neg"], sched, 6.0, c["step_noise"], round_state=False)
    x, _ = _one_call(MI355XCogVideoXLatentSampler(gmodel, _dpm()), c, 6.0, n=n)
    got = ref.unpatchify(x.cpu(), CLIP[0], C, CLIP[1], CLIP[2])
    d_oracle, d_kernel, moved = _rel(t16, t32), _rel(got, t32), _rel(t32, c["noise"])
    print(f"[cog_sample_ms trajectory n={n} g=6] d_oracle {d_oracle:.3e} d_kernel {d_kernel:.3e} ratio {d_kernel / d_oracle:.2f} moved {moved:.3f}")
    assert moved > 0.1 and _rel(got, c["noise"]) > 0.1
    assert d_kernel <= 1.5 * d_oracle


# ---- 5. the public path --------------------------------------------------------------------------------------------------------------------------------------------
def test_validation_latents_run_the_checkpoints_scheduler(models):
    from finetrainers_amd.cogvideox import MI355XCogVideoXLatentSampler, MI355XCogVideoXModelSpecification, cog_dpm_step_noise
    from finetrainers_amd.cogvideox.sampler import cog_ddim_schedule

    dev = _dev()
    _, gmodel = models("1.5")
    c = _case("1.5", 3, seed=9)
    F_, H, W = CLIP
    text, neg = c["text"].to(dev), c["neg"].to(dev)
    spec = MI355XCogVideoXModelSpecification(pretrained_model_name_or_path=None)
    cfg = spec.validation_scheduler_config(gmodel)
    assert cfg == _dpm()
    gen = lambda: torch.Generator(device=dev).manual_seed(1234)
    via = lambda sc, **kw: spec.validation_latents(gmodel, text, neg, F_, H, W, num_inference_steps=3, generator=gen(), scheduler_config=sc, **kw)
    dpm = via(cfg)
    torch.cuda.synchronize()
    assert dpm.shape == (1, F_, C, H, W) and dpm.dtype == bf16 and bool(torch.isfinite(dpm.float()).all())
    # the direct call, drawing by hand in the pipeline's order: the initial noise (one padded leading frame), then the noise of every step
    g = gen()
    lat = torch.randn((1, F_ + 1, C, H, W), generator=g, device=dev, dtype=torch.float32)
    z = cog_dpm_step_noise(lat.shape, 3, cog_ddim_schedule(3)[1], g, dev)
    sampler = MI355XCogVideoXLatentSampler(gmodel, cfg)
    direct = sampler.sample(lat, text, neg, num_inference_steps=3, drop_frames=1, step_noise=z)
    assert torch.equal(_bits(dpm.cpu()), _bits(direct.cpu())), "one generator: initial noise first, then the steps'"
    g = gen()
    lat2 = torch.randn((1, F_ + 1, C, H, W), generator=g, device=dev, dtype=torch.float32)
    assert torch.equal(_bits(dpm.cpu()), _bits(sampler.sample(lat2, text, neg, num_inference_steps=3, drop_frames=1, generator=g).cpu()))
    assert torch.equal(_bits(dpm.cpu()), _bits(via(cfg).cpu())), "reproducible from the seed"
    ddim = via(None)
    assert torch.equal(_bits(ddim.cpu()), _bits(MI355XCogVideoXLatentSampler(gmodel).sample(lat, text, neg, num_inference_steps=3, drop_frames=1).cpu())), \
        "scheduler_config = None is still ftmi_cog_sample"
    d = _rel(dpm.float().cpu(), ddim.float().cpu())
    print(f"[cog validation_latents 1.5] DPM against DDIM, 3 steps: rel_l2 {d:.3f}")
    assert d > 0.05
    dyn = via(cfg, use_dynamic_cfg=True)
    assert bool(torch.isfinite(dyn.float()).all()) and not torch.equal(_bits(dyn.cpu()), _bits(dpm.cpu())), "a guidance scale per step must show"
    with pytest.raises(NotImplementedError, match="use_dynamic_cfg"):
        via(None, use_dynamic_cfg=True)
    saved = gmodel.lora_flat.clone()
    try:
        with torch.no_grad():
            gmodel.lora_flat[gmodel.lora_flat.numel() // 2:].mul_(3.0)
        moved = via(cfg)
    finally:
        with torch.no_grad():
            gmodel.lora_flat.copy_(saved)
    assert not torch.equal(_bits(dpm.cpu()), _bits(moved.cpu())), "a changed adapter must show"
    assert torch.equal(_bits(dpm.cpu()), _bits(via(cfg).cpu())), "restored adapters, the first result's bits"
