"""Torch restatement of CogVideoX's multistep scheduler for the tests: the STEPWISE scheduler with unfolded fp64 quantities, carrying the previous x0
prediction and taking the noise as an argument, the dynamic-CFG formula, and the pipeline loop the GPU trajectory test drives ``oracle.cogvideox`` with.

[upstream, unpinned] ``CogVideoXDPMScheduler`` + ``CogVideoXPipeline`` (diffusers 0.33, neither is vendored; restated from memory): trailing timesteps,
v-prediction, a second-order multistep SDE solver.  The step is written out literally here (``dpm_step``), NOT through the folded eight-number rows of
finetrainers_amd/cogvideox/sampler.py, so the two check each other.  The layout, the models and the DDIM side are tests/cog_sampling_reference.py's."""
import math

import torch

import cog_sampling_reference as ref

bf16 = torch.bfloat16
INF = float("inf")


def dpm_schedule(n, alphas_cumprod, N=1000):
    """-> [(t, prev, alpha_bar_t, alpha_bar_prev, alpha_bar_back or None)] fp64 for trailing spacing and set_alpha_to_one: ``ref.ddim_schedule`` plus the
    alpha_bar of the PREVIOUS timestep (None at step 0)."""
    ac = alphas_cumprod.double()
    base = ref.ddim_schedule(n, alphas_cumprod, N)
    out = []
    for i, (t, a_t, a_prev) in enumerate(base):
        out.append((t, t - N // n, a_t, a_prev, float(ac[base[i - 1][0]]) if i > 0 else None))
    return out


def _lam(a):
    """log sqrt(a / (1 - a)) with its two limits."""
    if a <= 0.0:
        return -INF
    if a >= 1.0:
        return INF
    return math.log(math.sqrt(a / (1.0 - a)))


def dpm_step(x, v, old, z, prev, a_t, a_prev, a_back):
    """One step as upstream writes it -> (x', x0).  ``old``: the previous step's x0 (None at the first step); ``z``: this step's noise."""
    x0 = a_t ** 0.5 * x - (1 - a_t) ** 0.5 * v
    lam, lam_next = _lam(a_t), _lam(a_prev)
    h = lam_next - lam
    mult0 = ((1 - a_prev) / (1 - a_t)) ** 0.5 * math.exp(-h)
    mult1 = math.expm1(-2 * h) * a_prev ** 0.5
    mn = (1 - a_prev) ** 0.5 * (1 - math.exp(-2 * h)) ** 0.5
    noise = mn * z if mn != 0.0 else 0.0
    if old is None or prev < 0:
        return mult0 * x - mult1 * x0 + noise, x0
    r = (lam - _lam(a_back)) / h
    D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * old
    return mult0 * x - mult1 * D + noise, x0


def dynamic_cfg(g, n, t):
    """``1 + g (1 - cos(pi ((n - t) / n) ** 5.0)) / 2`` with the timestep VALUE t and n inference steps, as upstream has it."""
    return 1 + g * ((1 - math.cos(math.pi * ((n - t) / n) ** 5.0)) / 2)


def step_ref(pred, x, old, z, row, g):
    """fp64, one FOLDED row applied to the kernel's operands: pred bf16 [P B, S, Kc] (P = 2 unless g == 1), x / old / z [B, S, Kc] -> (x', x0, v).  A zero
    coefficient leaves its term out (its buffer may hold NaN)."""
    B = x.shape[0]
    sa, sb, m0, e0, e1, mn = (float(c) for c in row[:6])
    pr = pred.double()
    v = pr if g == 1.0 else pr[:B] + g * (pr[B:] - pr[:B])
    x0 = sa * x.double() - sb * v
    out = m0 * x.double() + e0 * x0
    if e1 != 0.0:
        out = out + e1 * old.double()
    if mn != 0.0:
        out = out + mn * z.double()
    return out, x0, v


def trajectory(fn, dtype, latents, text, negative_text, schedule, guidance, noise, round_state=True, rope=None, dynamic=False):
    """``ref.trajectory`` with the multistep scheduler: ``noise`` [n, B, F, C, H, W] is the draw each step uses.  The step runs in fp32 (fp64 for a fp64 run) on
    the state and the carried x0; with ``round_state`` the state is rounded to ``dtype`` after every step, as upstream does with the prompt dtype."""
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    x = latents.to(dtype if round_state else wide)
    cfg = guidance != 1.0
    enc = (torch.cat([negative_text, text]) if cfg else text).to(dtype)
    old, n = None, len(schedule)
    with torch.no_grad():
        for i, (t, prev, a_t, a_prev, a_back) in enumerate(schedule):
            inp = x.to(dtype)
            inp = torch.cat([inp, inp]) if cfg else inp
            ts = torch.full((inp.shape[0],), t, dtype=torch.int64)
            out = fn(hidden_states=inp, encoder_hidden_states=enc, timestep=ts, image_rotary_emb=rope, return_dict=False)[0]
            if cfg:
                u, c = out.chunk(2)
                out = u + (dynamic_cfg(guidance, n, t) if dynamic else guidance) * (c - u)
            x, old = dpm_step(x.to(wide), out.to(wide), old, noise[i].to(wide), prev, a_t, a_prev, a_back)
            x = x.to(dtype) if round_state else x
    return x
