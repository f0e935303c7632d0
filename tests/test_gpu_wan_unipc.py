"""Wan validation sampling with the checkpoint's UniPC multistep scheduler, on the GPU: the step kernel per element against fp64 with a bound derived from
its rounding points, the one-call loop (``ftmi_wan_sample_ms``) against its composition from ``model.forward`` and ``ops.wan_sample_step_unipc`` bit for bit,
the trajectory against the stepwise scheduler of tests/wan_unipc_reference.py over the oracle model in bf16 and fp32, and the public path."""
import copy

import pytest
import torch

import wan_sampling_reference as ref
import wan_unipc_reference as uref

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
C = 16
# (stored patch width Kp, extra channels, copies): text-to-video, image-to-video (144 of 192 columns used), control with the folded adapter ([cols | cols])
LAYOUTS = {"t2v": (64, 0, 1), "i2v": (192, 20, 1), "control": (128, 16, 2)}
GRIDS = [(1, 2, 2), (3, 4, 6)]  # one token; 18 tokens (no multiple of any tile)
UNIPC = {"_class_name": "UniPCMultistepScheduler", "flow_shift": 3.0}
NAN = float("nan")


def _dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def _geo(layout, B, P, F_, H, W):
    from finetrainers_amd import ops

    Kp, Cx, copies = LAYOUTS[layout]
    return ops.wan_sample_geometry(B, C, F_, H, W, Kp, extra_channels=Cx, copies=copies, guidance=P == 2)


# ---- 1. the step kernel ----------------------------------------------------------------------------------------------------------------------------------------
def _rows():
    """Four coefficient rows and their sigmas, taken from real tables: the 5-step shift-3 schedule at order 2 (step 0: no history; step 2: order-2 corrector
    and order-2 predictor, all eight numbers in play; step 4: the last step, corrector and x' = m) and the same schedule at order 1 with every corrector
    disabled (step 2: Euler in another form)."""
    from finetrainers_amd.wan import wan_unipc_schedule, wan_unipc_tables

    sig, _ = wan_unipc_schedule(5, UNIPC)
    full, plain = wan_unipc_tables(sig, 2, ()), wan_unipc_tables(sig, 1, range(5))
    s32 = sig.float()  # the sigma the kernel reads is the fp32 one, like the coefficients
    rows = {"step0": (full[0], s32[0]), "order2": (full[2], s32[2]), "last": (full[4], s32[4]), "order1": (plain[2], s32[2])}
    assert full[0, :5].tolist() == [1, 0, 0, 0, 0] and float(full[0, 7]) == 0 and bool((full[2] != 0).sum() == 7) and full[4, 5:].tolist() == [0, 1, 0]
    assert plain[2, :5].tolist() == [1, 0, 0, 0, 0] and float(plain[2, 7]) == 0
    return rows, sig


def _step_inputs(layout, B, P, F_, H, W):
    """pred on the 1 / 16 grid: |u|, |c| < 4.5 are bf16 values (7 significant bits), c - u and g (c - u) + u (g = 5: |v| < 47) are multiples of 1 / 16 below 2^6,
    exact in fp32 -- v carries NO rounding.  x, last, m1, m2: four different random fp32 tensors, different in every element and token."""
    S = F_ * (H // 2) * (W // 2)
    g = torch.Generator().manual_seed(S + 3 * B + P)
    tok = torch.arange(B * S, dtype=torch.float32).view(B, S, 1)
    cond = ((torch.arange(64, dtype=torch.float32) - 31.5) / 8 + (tok % 7) / 16).to(bf16)
    assert torch.equal(cond.float(), (torch.arange(64, dtype=torch.float32) - 31.5) / 8 + (tok % 7) / 16)
    unc = (torch.randint(-64, 65, (B, S, 64), generator=g).float() / 16).to(bf16)
    pred = cond if P == 1 else torch.cat([unc, cond])
    bufs = [torch.randn(B, S, 64, generator=g) * 2 + k for k in (0.5, -1.0, 1.5, -2.0)]
    return S, pred, bufs


def _fp64_step(pred, bufs, row, sigma, guidance):
    """The step in fp64 from the fp32 coefficients and sigma the kernel reads -> (v, m, x~, x', M, A, Bsum): M = |x| + sigma |v|, A and Bsum the sums of the
    absolute terms of the two linear expressions, which the bound is stated in."""
    x, last, m1, m2 = (b.double() for b in bufs)
    Bn = x.shape[0]
    p = ref.pred_in_state_order(pred.double(), C)
    v = p[:Bn] + guidance * (p[Bn:] - p[:Bn]) if guidance != 1.0 else p
    cx, cl, c1, c2, ct, px, p0, p1 = [float(t) for t in row.double()]
    sg = float(sigma)
    m = x - sg * v
    mabs = x.abs() + sg * v.abs()
    xt = cx * x + cl * last + c1 * m1 + c2 * m2 + ct * m
    A = abs(cx) * x.abs() + abs(cl) * last.abs() + abs(c1) * m1.abs() + abs(c2) * m2.abs() + abs(ct) * mabs
    xn = px * xt + p0 * m + p1 * m1
    Bsum = abs(px) * A + abs(p0) * mabs + abs(p1) * m1.abs()
    return v, m, xt, xn, mabs, A, Bsum


@pytest.mark.parametrize("form", ["step0", "order2", "last", "order1"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("guidance", [1.0, 5.0])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("F_,H,W", GRIDS)
def test_unipc_step_against_fp64(F_, H, W, B, guidance, layout, form):
    """The bound, from the kernel's rounding points (sample_layout.hip wan_sample_step_unipc_kernel; every fma or mul rounds once, by at most 2^-24 of its result):
      v    exact (the inputs sit on the 1 / 16 grid, see _step_inputs)
      m    = fma(-sigma, v, x): one rounding,                                   |dm|  <= 2^-24 (|x| + sigma |v|) =: 2^-24 M
      x~   n_c non-zero terms = one mul and n_c - 1 fmas, each partial sum below A = sum |terms|; its term c_t m carries c_t dm <= 2^-24 A:
                                                                                 |dx~| <= (n_c + 1) 2^-24 A
      x'   n_p terms the same way over Bsum = |p_x| A + |p_0| M + |p_1| |m1|, plus |p_x| dx~ and |p_0| dm, each below its share of Bsum:
                                                                                 |dx'| <= (n_p + n_c + 2) 2^-24 Bsum
    (n_c + n_p <= 8: k <= 10; the second-order terms are 2^-24 of these and sit inside the 1 + 2^-10 factor).  The coefficients and sigma are the fp32 values the
    kernel reads, so they add nothing.  The buffers differ by O(1) in every element: a swapped buffer, a wrong slot or a permuted column moves the result by
    ~2^20 times the bound.  Buffers whose coefficients are all zero hold NaN: nothing of them may reach a result."""
    from finetrainers_amd import ops

    dev = _dev()
    Kp, Cx, copies = LAYOUTS[layout]
    P = 2 if guidance != 1.0 else 1
    geo = _geo(layout, B, P, F_, H, W)
    rows, sig = _rows()
    row, sigma = rows[form]
    S, pred, bufs = _step_inputs(layout, B, P, F_, H, W)
    cx, cl, c1, c2, ct, px, p0, p1 = row.tolist()
    unused = [False, cl == 0, c1 == 0 and p1 == 0, c2 == 0]
    v, m, xt, xn, M, A, Bsum = _fp64_step(pred, [torch.zeros_like(b) if u else b for b, u in zip(bufs, unused)], row, sigma, guidance)
    n_c, n_p = sum(c != 0 for c in (cx, cl, c1, c2, ct)), sum(c != 0 for c in (px, p0, p1))
    eps = 2.0 ** -24 * (1 + 2.0 ** -10)
    sentinel = torch.full((P * B * S, copies * Kp), -7.0, dtype=bf16)
    sig_dev = torch.tensor([float(sigma)], dtype=torch.float32, device=dev)

    def launch(coef):
        x, last, m1, m2 = (torch.full_like(b, NAN).to(dev) if u else b.to(dev, copy=True) for b, u in zip(bufs, unused))
        cols = sentinel.to(dev, copy=True)
        ops.wan_sample_step_unipc(geo, pred.to(dev), x, last, m1, m2, coef.to(dev), sig_dev, guidance, cols)
        torch.cuda.synchronize()
        return x.cpu(), last.cpu(), m1.cpu(), m2.cpu(), cols.cpu()

    x, last, m1, m2, cols = launch(row)
    for name, got, want, bound in (("m", m2, m, eps * M), ("x~", last, xt, (n_c + 1) * eps * A), ("x'", x, xn, (n_p + n_c + 2) * eps * Bsum)):
        assert bool(torch.isfinite(got).all()), name
        frac = float(((got.double() - want).abs() / bound).max())
        print(f"[wan_sample_step_unipc {form} {layout} B={B} S={S} g={guidance}] {name}: max error / bound {frac:.3f}")
        assert frac <= 1.0, name
    assert not torch.equal(x, bufs[0])
    if not unused[2]:
        assert torch.equal(_bits(m1), _bits(bufs[2])), "m1 is read only"
    # x~ and m of the kernel's own arithmetic: the same launch with the predictor (1, 0, 0) hands x~ to x, with (0, 1, 0) it hands m
    as_xt, as_m = row.clone(), row.clone()
    as_xt[5:] = torch.tensor([1.0, 0.0, 0.0])
    as_m[5:] = torch.tensor([0.0, 1.0, 0.0])
    assert torch.equal(_bits(launch(as_xt)[0]), _bits(last)), "last is x~ bit for bit"
    assert torch.equal(_bits(launch(as_m)[0]), _bits(m2)), "the older history buffer is m bit for bit"
    rne = x.to(bf16).view(B * S, 64)
    for p in range(P):
        grp = cols[p * B * S:(p + 1) * B * S]
        for cp in range(copies):
            assert torch.equal(_bits(grp[:, cp * Kp:cp * Kp + 64]), _bits(rne)), (p, cp)
            assert torch.equal(_bits(grp[:, cp * Kp + 64:(cp + 1) * Kp]), _bits(sentinel[:B * S, 64:Kp])), "a constant column was written"
    if form == "step0":
        assert unused == [False, True, True, True] and torch.equal(_bits(last), _bits(bufs[0])), "no corrector: x~ is x"
    if form == "last":  # p = (0, 1, 0): x' IS m, to the bit, and within m's share of this row's bound
        assert torch.equal(_bits(x), _bits(m2)) and bool(((x.double() - m).abs() <= (n_p + n_c + 2) * eps * Bsum).all())
    if form == "order1":
        # the fp64 Euler update x + (sigma_3 - sigma_2) v on the fp64 table.  On top of the kernel's roundings the folded numbers were rounded to fp32 once each:
        # p_x and p_0 move their terms by 2^-24 of them (one share of Bsum together), sigma moves |p_0| sigma |v| by 2^-24 (another share at most)
        euler = bufs[0].double() + (float(sig[3]) - float(sig[2])) * v
        frac = float(((x.double() - euler).abs() / ((n_p + n_c + 2 + 2) * eps * Bsum)).max())
        print(f"[wan_sample_step_unipc order1 {layout} B={B} S={S} g={guidance}] against fp64 Euler: max error / bound {frac:.3f}")
        assert frac <= 1.0


def test_unipc_step_0_ignores_an_uninitialised_history():
    """Step 0 of a run: last, m1 and m2 are whatever the workspace held.  NaN everywhere in them: x, x~, m and cols are finite, m1 is untouched."""
    from finetrainers_amd import ops

    dev = _dev()
    geo = _geo("t2v", 2, 2, 3, 4, 6)
    rows, _ = _rows()
    row, sigma = rows["step0"]
    S, pred, bufs = _step_inputs("t2v", 2, 2, 3, 4, 6)
    x = bufs[0].to(dev)
    last, m1, m2 = (torch.full_like(bufs[0], NAN).to(dev) for _ in range(3))
    cols = torch.zeros(2 * 2 * S, 64, dtype=bf16, device=dev)
    ops.wan_sample_step_unipc(geo, pred.to(dev), x, last, m1, m2, row.to(dev), torch.tensor([float(sigma)], device=dev), 5.0, cols)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in (x, last, m2, cols)) and bool(torch.isnan(m1).all())


# ---- 2. the loop is its composition ------------------------------------------------------------------------------------------------------------------------------
F_, H, W, T = 2, 8, 12, 16  # 48 tokens


def _case(kind, dev, B=1, seed=21):
    g = torch.Generator().manual_seed(seed)
    c = dict(latents=torch.randn(B, C, F_, H, W, generator=g).to(dev), pos=torch.randn(B, T, 64, generator=g).to(bf16).to(dev),
             neg=torch.randn(B, T, 64, generator=g).to(bf16).to(dev), image=None, extra=None)
    if kind == "i2v":
        c["image"] = torch.randn(B, 5, 64, generator=g).to(bf16).to(dev)
        c["extra"] = torch.randn(B, 20, F_, H, W, generator=g).to(bf16).to(dev)
    if kind == "control":
        c["extra"] = torch.randn(B, 16, F_, H, W, generator=g).to(bf16).to(dev)
    return c


def _one_call(sampler, c, steps, guidance):
    """``ftmi_wan_sample_ms`` on the sampler's own schedule, piece by piece as ``MI355XWanLatentSampler.sample`` prepares it; the history buffers
    behind the Euler workspace start as all-ones bytes, which are NaN in fp32."""
    from finetrainers_amd import ops

    tr = sampler.transformer
    dev = tr.device
    B = c["latents"].shape[0]
    sig, ts = sampler.schedule(steps, None, None)
    geo = sampler.geometry(B, F_, H, W, guidance=guidance != 1.0)
    enc = sampler.text_rows(c["pos"], c["neg"] if guidance != 1.0 else None)
    enc_img = None if c["image"] is None else tr._embed_image(torch.cat([c["image"]] * geo.P))
    tproj, shift, scale = sampler.step_tables(ts, geo.P * B)
    x, cols = ops.wan_sample_init(geo, c["latents"], c["extra"])
    cfg, weights, keep = sampler.c_arguments(geo, T, 0 if enc_img is None else enc_img.shape[1], ts.numel(), guidance)
    need, euler = ops.wan_sample_ms_workspace_bytes(cfg), ops.wan_sample_workspace_bytes(cfg)
    assert need == euler + 3 * 4 * x.numel()
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws[euler:] = 255
    ops.wan_sample_ms(cfg, weights, cols, x, tproj, shift, scale, enc, enc_img, tr._rope(F_, H, W), sampler.unipc_tables(sig).to(dev), sig.float().to(dev), workspace=ws)
    torch.cuda.synchronize()
    return x, cols


@torch.no_grad()
def _composition(sampler, kind, c, steps, guidance):
    """The same launches from Python: ``model.forward`` at batch [unconditional, conditional] and ``ops.wan_sample_step_unipc``, the two history buffers swapped
    here after every step."""
    from finetrainers_amd import ops

    tr = sampler.transformer
    dev = tr.device
    B = c["latents"].shape[0]
    sig, ts = sampler.schedule(steps, None, None)
    coef, sig32 = sampler.unipc_tables(sig).to(dev), sig.float().to(dev)
    geo = sampler.geometry(B, F_, H, W, guidance=guidance != 1.0)
    P, S = geo.P, F_ * (H // 2) * (W // 2)
    x, cols = ops.wan_sample_init(geo, c["latents"], c["extra"])
    last, m1, m2 = (torch.full_like(x, NAN) for _ in range(3))
    text = torch.cat([c["neg"], c["pos"]]) if P == 2 else c["pos"]
    kw = {} if c["image"] is None else dict(encoder_hidden_states_image=torch.cat([c["image"]] * P))
    used = tr.config.in_channels * 4
    for i in range(ts.numel()):
        t = torch.full((P * B,), float(ts[i]), dtype=torch.float32, device=dev)
        if kind == "control":
            out = tr(None, t, text, patch_columns=cols, latent_shape=(P * B, F_, H, W))[0]
        else:
            hidden = ref.unpatchify(cols[:, :used].reshape(P * B, S, used), tr.config.in_channels, F_, H, W)
            out = tr(hidden, t, text, **kw)[0]
        pred = ref.pred_tokens(out).contiguous()
        ops.wan_sample_step_unipc(geo, pred, x, last, m1, m2, coef[i], sig32[i:i + 1], guidance, cols)
        m1, m2 = m2, m1
    torch.cuda.synchronize()
    return x, cols


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = ref.gpu_model(kind, _dev(), layers=2)
        return cache[kind]

    return get


def _assert_same(sampler, kind, c, steps, guidance):
    x1, cols1 = _one_call(sampler, c, steps, guidance)
    x2, cols2 = _composition(sampler, kind, c, steps, guidance)
    x0 = ref.patchify(c["latents"].cpu())
    print(f"[wan_sample_ms {kind} g={guidance}] one call vs composition: x {ref.rel_l2(x1, x2):.2e}; moved from the noise by {ref.rel_l2(x1, x0):.3f}")
    assert bool(torch.isfinite(x1).all()) and ref.rel_l2(x1, x0) > 0.05
    assert torch.equal(_bits(x1), _bits(x2)), "final state"
    assert torch.equal(_bits(cols1), _bits(cols2)), "final model input"
    assert torch.equal(_bits(cols1[:48, :64]), _bits(x1.to(bf16).view(48, 64)))


@pytest.mark.parametrize("kind", ["t2v", "i2v", "ten", "control"])
def test_one_call_ms_loop_is_its_composition_bit_for_bit(models, kind):
    """2 blocks, rank-64 adapters with non-zero B, guidance 5, one sample, 4 steps of the shift-3 schedule: the smallest run with an order-2 predictor (steps 1, 2),
    an order-1 corrector (step 1), an order-2 corrector (steps 2, 3) and the order-1 last step."""
    from finetrainers_amd.wan import MI355XWanLatentSampler

    gmodel = models(kind)
    assert float(gmodel.blocks[0].lora_B.detach().abs().max()) > 0
    sampler = MI355XWanLatentSampler(gmodel, UNIPC)
    t = sampler.unipc_tables(sampler.schedule(4, None, None)[0])
    assert [bool(v) for v in t[:, 7] != 0] == [False, True, True, False] and [bool(v) for v in t[:, 3] != 0] == [False, False, True, True]
    _assert_same(sampler, kind, _case(kind, _dev()), 4, 5.0)


def test_one_call_ms_loop_without_guidance_and_with_a_disabled_corrector(models):
    from finetrainers_amd.wan import MI355XWanLatentSampler

    _assert_same(MI355XWanLatentSampler(models("t2v"), UNIPC), "t2v", _case("t2v", _dev(), seed=5), 4, 1.0)
    sampler = MI355XWanLatentSampler(models("t2v"), dict(UNIPC, disable_corrector=[0]))
    assert sampler.unipc_tables(sampler.schedule(4, None, None)[0])[1, :5].tolist() == [1, 0, 0, 0, 0]
    _assert_same(sampler, "t2v", _case("t2v", _dev(), seed=6), 4, 5.0)


# ---- 3. the trajectory ---------------------------------------------------------------------------------------------------------------------------------------------
def test_unipc_trajectory_against_the_oracle():
    """The rule of test_gpu_wan_sampling.py::test_trajectory_against_the_oracle with the multistep scheduler: text-to-video, 2 blocks, rank-64 adapters in both
    models, 5 steps of the shift-3 schedule, guidance 5.  The oracle loops are the STEPWISE scheduler of tests/wan_unipc_reference.py over the oracle model, in bf16
    and as an fp32 copy; d_oracle = rel_l2(bf16 oracle, fp32 oracle), d_kernel = rel_l2(ftmi_wan_sample_ms, fp32 oracle); d_kernel <= 1.5 d_oracle.  Measured on an
    MI355X: see BASELINE.md."""
    from finetrainers_amd.wan import MI355XWanLatentSampler

    dev = _dev()
    omodel, gmodel = ref.t2v_pair(dev)
    c = _case("t2v", dev, seed=33)
    sampler = MI355XWanLatentSampler(gmodel, UNIPC)
    sig, ts = sampler.schedule(5, None, None)
    g = 5.0
    lat, pos, neg = c["latents"].cpu(), c["pos"].cpu(), c["neg"].cpu()
    x_bf = uref.trajectory(omodel, bf16, lat, neg, pos, sig.tolist(), ts.tolist(), g)
    x_32 = uref.trajectory(copy.deepcopy(omodel).float(), torch.float32, lat, neg, pos, sig.tolist(), ts.tolist(), g)
    x_k, _ = _one_call(sampler, c, 5, g)
    d_oracle, d_kernel = ref.rel_l2(x_bf, x_32), ref.rel_l2(x_k, x_32)
    move = ref.rel_l2(x_32, ref.patchify(lat))
    print(f"[wan unipc sampling trajectory] d_oracle (bf16 oracle vs fp32 oracle) {d_oracle:.3e}; d_kernel (ftmi_wan_sample_ms vs fp32 oracle) {d_kernel:.3e}; "
          f"ratio {d_kernel / d_oracle:.2f}; the trajectory moves the state by {move:.3f}")
    assert d_oracle == d_oracle and 0.0 < d_oracle < float("inf")
    assert move > 0.1
    assert d_kernel <= 1.5 * d_oracle


# ---- 4. the public path ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["t2v", "control"])
def test_validation_latents_run_the_checkpoints_scheduler(models, kind):
    from finetrainers_amd.wan import MI355XWanControlModelSpecification, MI355XWanLatentSampler, MI355XWanModelSpecification

    dev = _dev()
    gmodel = models(kind)
    c = _case(kind, dev, seed=9)
    cfg = dict(UNIPC, solver_order=2, num_train_timesteps=1000)
    gen = lambda: torch.Generator(device=dev).manual_seed(1234)
    if kind == "control":
        spec = MI355XWanControlModelSpecification(pretrained_model_name_or_path=None)
        via = lambda sc: spec.validation_latents(gmodel, c["pos"], c["neg"], c["extra"], F_, H, W, torch.zeros(C), torch.ones(C), num_inference_steps=3,
                                                 generator=gen(), scheduler_config=sc)
        extra = dict(control_latents=c["extra"])
    else:
        spec = MI355XWanModelSpecification(pretrained_model_name_or_path=None)
        via = lambda sc: spec.validation_latents(gmodel, c["pos"], c["neg"], F_, H, W, num_inference_steps=3, generator=gen(), scheduler_config=sc)
        extra = {}
    unipc = via(cfg)
    torch.cuda.synchronize()
    assert unipc.shape == (1, C, F_, H, W) and unipc.dtype == bf16 and bool(torch.isfinite(unipc.float()).all())
    direct = MI355XWanLatentSampler(gmodel, cfg).sample(c["pos"], c["neg"], F_, H, W, num_inference_steps=3, generator=gen(), **extra)
    assert torch.equal(_bits(unipc), _bits(direct))
    euler = via(None)
    assert torch.equal(_bits(euler), _bits(MI355XWanLatentSampler(gmodel).sample(c["pos"], c["neg"], F_, H, W, num_inference_steps=3, generator=gen(), **extra)))
    d = ref.rel_l2(unipc.float(), euler.float())
    print(f"[wan validation_latents {kind}] UniPC (shift 3) against Euler (shift 1), 3 steps: rel_l2 {d:.3f}")
    assert d > 0.05
    saved = gmodel.blocks[1].lora_B.detach().clone()
    try:
        with torch.no_grad():
            gmodel.blocks[1].lora_B.mul_(3.0)
        moved = via(cfg)
    finally:
        with torch.no_grad():
            gmodel.blocks[1].lora_B.copy_(saved)
    assert not torch.equal(_bits(unipc), _bits(moved)), "a changed adapter must show"
    assert torch.equal(_bits(unipc), _bits(via(cfg))), "restored adapters, the first result's bits"
