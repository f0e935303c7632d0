"""Validation sampling in latent space for the MI355X Wan backend: text-to-video, image-to-video and control.

The reference validates by running a diffusers pipeline's denoising loop over the transformer that is being trained (finetrainers/models/wan/
base_specification.py:495-529; control_specification.py:310-377 with the control latents concatenated on the channels).  Here the loop -- DiT forward on the
unconditional + conditional prompt, classifier-free-guidance combine, scheduler update -- is ONE C call (``ftmi_wan_sample`` for flow-match Euler,
``ftmi_wan_sample_ms`` for the UniPC multistep scheduler; no host synchronisation) over this backend's flat-buffer model with its current adapters.

Which scheduler: the reference's trainers call ``load_pipeline`` WITHOUT a scheduler (sft_trainer/trainer.py:777-794), and ``WanModelSpecification.load_pipeline``
drops null components before ``WanPipeline.from_pretrained`` (base_specification.py:332-365), so the validation videos are sampled with the scheduler stored in the
checkpoint's ``scheduler/`` folder -- for the Wan2.1 diffusers checkpoints ``UniPCMultistepScheduler`` with flow sigmas (flow_shift 3.0, 5.0 at 720p, order 2, bh2).
The ``FlowMatchEulerDiscreteScheduler()`` built at base_specification.py:328 serves the TRAINING sigmas only.  A ``scheduler_config`` whose ``_class_name`` is
``UniPCMultistepScheduler`` (``wire.load_scheduler_config`` / ``validation_scheduler_config()`` of the specifications read it from the checkpoint) selects that
solver here; ``None`` and every other config run flow-match Euler (shift 1 by default), as before.  The sampler state stays in the patch embedding's operand layout (csrc/sample_layout.hip), so
nothing is patchified between steps.  Text / image encoding and the VAE stay outside: the sampler takes embeddings and latents and returns denormalised
latents (INTEGRATION.md shows the hand-over to the reference pipeline's VAE decode).

The state and the guidance combine are kept in fp32 -- a deliberate choice, like the LTX sampler's: [upstream, unpinned] ``WanPipeline`` holds the latents in
fp32 as well and casts them to the transformer's dtype per step; its combine runs on the bf16 model output, here on its fp32 values (one rounding less).
"""

from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib, ops
from ..cogvideox.model import timestep_embedding
from .block import _WanLoRABlockNativeFunction
from .model import MI355XWanTransformer3DModel, bf16

# [upstream, unpinned] ``FlowMatchEulerDiscreteScheduler()`` with no arguments: what the reference builds for Wan's TRAINING sigmas (base_specification.py:328).
# It is this sampler's default; the reference's validation pipeline runs the checkpoint's own scheduler (UniPC, see the module docstring and ``wan_unipc_schedule``)
WAN_SCHEDULER_CONFIG: Dict[str, Any] = {"num_train_timesteps": 1000, "shift": 1.0, "use_dynamic_shifting": False}


def wan_flow_match_sigmas(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> torch.Tensor:
    """Sigma table of a sampling run: fp32 [num_inference_steps + 1] on the host, decreasing, ending in 0.

    [upstream, unpinned] restates ``FlowMatchEulerDiscreteScheduler.set_timesteps(n)`` without dynamic shifting.  The constructor builds
    ``sigmas = shift * s / (1 + (shift - 1) * s)`` over ``s = (N, ..., 1) / N`` and keeps ``sigma_max = sigmas[0]`` (= 1) and ``sigma_min = sigmas[-1]`` (the
    shifted ``1 / N``); ``set_timesteps`` takes ``linspace(sigma_max, sigma_min, n)`` and applies the static shift to it -- again, the way the scheduler does
    -- then appends 0.  With shift 1 the table is ``linspace(1, 1 / N, n)``.  The timestep the model sees at step i is ``sigma_i * N``."""
    cfg = dict(WAN_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("wan_flow_match_sigmas: at least one step")
    if cfg.get("use_dynamic_shifting", False):
        raise NotImplementedError("wan_flow_match_sigmas: dynamic shifting is not part of the scheduler the reference builds for Wan")
    N, shift = float(cfg.get("num_train_timesteps", 1000)), float(cfg.get("shift", 1.0))
    apply = lambda s: shift * s / (1.0 + (shift - 1.0) * s)
    sigma_max, sigma_min = apply(1.0), apply(1.0 / N)
    s = apply(torch.linspace(sigma_max, sigma_min, n, dtype=torch.float64))
    return torch.cat([s, s.new_zeros(1)]).to(torch.float32)


UNIPC_CLASS_NAME = "UniPCMultistepScheduler"
# [upstream, unpinned] the ``scheduler/scheduler_config.json`` of the Wan2.1 diffusers checkpoints (flow_shift 5.0 on the 720p ones); missing keys take these values
WAN_UNIPC_CONFIG: Dict[str, Any] = {"num_train_timesteps": 1000, "prediction_type": "flow_prediction", "use_flow_sigmas": True, "flow_shift": 3.0, "solver_order": 2,
                                    "solver_type": "bh2", "predict_x0": True, "lower_order_final": True, "final_sigmas_type": "zero", "disable_corrector": [],
                                    "thresholding": False, "solver_p": None, "use_karras_sigmas": False, "use_exponential_sigmas": False, "use_beta_sigmas": False}
# the columns of a row of ``wan_unipc_tables``
UNIPC_COLUMNS = ("c_x", "c_l", "c_1", "c_2", "c_t", "p_x", "p_0", "p_1")


def is_unipc(scheduler_config: Optional[Dict[str, Any]]) -> bool:
    return scheduler_config is not None and scheduler_config.get("_class_name") == UNIPC_CLASS_NAME


def _unipc_config(scheduler_config: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The config over its defaults, after every refusal: what of ``UniPCMultistepScheduler`` this backend restates is what the Wan checkpoints use."""
    cfg = dict(WAN_UNIPC_CONFIG)
    cfg.update(scheduler_config or {})
    no = lambda key, why: NotImplementedError(f"wan_unipc: {key} = {cfg.get(key)!r} is not covered ({why})")
    if cfg["solver_order"] not in (1, 2):
        raise no("solver_order", "1 or 2")
    if cfg["solver_type"] != "bh2":
        raise no("solver_type", "bh2 only")
    if not cfg["predict_x0"]:
        raise no("predict_x0", "the data-prediction form only")
    if cfg["prediction_type"] != "flow_prediction":
        raise no("prediction_type", "flow_prediction only")
    if not cfg["use_flow_sigmas"]:
        raise no("use_flow_sigmas", "flow sigmas only")
    for key in ("use_karras_sigmas", "use_exponential_sigmas", "use_beta_sigmas"):
        if cfg.get(key):
            raise no(key, "flow sigmas only")
    if cfg.get("thresholding"):
        raise no("thresholding", "latent-space models do not threshold")
    if cfg.get("solver_p") is not None:
        raise no("solver_p", "UniPC's own predictor only")
    if cfg["final_sigmas_type"] != "zero":
        raise no("final_sigmas_type", "zero only")
    if cfg.get("use_dynamic_shifting"):
        raise no("use_dynamic_shifting", "the static flow_shift only")
    return cfg


def wan_unipc_schedule(num_inference_steps: int, scheduler_config: Optional[Dict[str, Any]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (sigmas fp64 [n + 1], timesteps fp64 [n]) on the host.

    [upstream, unpinned] restates ``UniPCMultistepScheduler.set_timesteps(n)`` with ``use_flow_sigmas``: ``sigma_i = f(s_i)`` over
    ``s_i = (1 - 1 / N) (1 - i / n)``, i = 0 .. n - 1 (the scheduler builds ``1 - linspace(1, 1 / N, n + 1)``, shifts it, flips it and drops the trailing 0),
    ``f(s) = shift s / (1 + (shift - 1) s)``, N = num_train_timesteps; ``final_sigmas_type = "zero"`` appends 0.  The
    timestep the model sees at step i is ``sigma_i N`` TRUNCATED: the scheduler stores int64 timesteps (999 at step 0 of shift 3), unlike flow-match Euler's
    fp32 ones."""
    cfg = _unipc_config(scheduler_config)
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError("wan_unipc_schedule: at least one step")
    N, shift = float(cfg["num_train_timesteps"]), float(cfg["flow_shift"])
    # in the scheduler's own operation order (numpy's linspace: start + j * step, the end point exact), so that the truncation falls where it falls there
    alphas = 1.0 + torch.arange(n + 1, dtype=torch.float64) * ((1.0 / N - 1.0) / n)
    alphas[n] = 1.0 / N
    s = torch.flip(1.0 - alphas, dims=(0,))[:-1]
    sig = shift * s / (1.0 + (shift - 1.0) * s)
    return torch.cat([sig, sig.new_zeros(1)]), torch.trunc(sig * N)


def wan_unipc_tables(sigmas, solver_order: int = 2, disable_corrector: Sequence[int] = (), dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The multistep scheduler folded per step: fp32 [n, 8] (``dtype=torch.float64``: the numbers before their one rounding), row i =
    (c_x, c_l, c_1, c_2, c_t, p_x, p_0, p_1) of

        x~     = c_x x + c_l last + c_1 m1 + c_2 m2 + c_t m          (the corrector;  (1, 0, 0, 0, 0): none)
        x_next = p_x x~ + p_0 m + p_1 m1                              (the predictor)

    with x the state the last predictor produced, m = x - sigma_i v its data prediction, last = x~ of the step before, m1 / m2 the data predictions of the
    one / two steps before.  The numbers depend on the sigma table only, so they are computed here in fp64, as ``cog_ddim_tables`` folds DDIM.

    [upstream, unpinned] restates ``UniPCMultistepScheduler.step`` (``multistep_uni_c_bh_update`` then ``multistep_uni_p_bh_update``) with ``predict_x0``, bh2,
    flow sigmas and ``lower_order_final``.  alpha = 1 - sigma, lambda = log alpha - log sigma; order_i = min(solver_order, n - i, i + 1).  With
    h = lambda_t - lambda_s, phi1 = B = expm1(-h):
      corrector at i >= 1 (unless i - 1 is in ``disable_corrector``), p = order_{i-1}, s = sigma_{i-1}, t = sigma_i:
        x~ = (sigma_t / sigma_s) last - alpha_t phi1 m1 - alpha_t B (rho_0 (m2 - m1) / r1 + rho_last (m - m1)),     r1 = (lambda_{i-2} - lambda_{i-1}) / h
        p = 1: rho = [1/2];  p = 2: rho solves [[1, 1], [r1, 1]] rho = [b1, b2],  hh = -h, g1 = phi1 / hh - 1, b1 = g1 / B, g2 = g1 / hh - 1/2, b2 = 2 g2 / B
      predictor at i, p = order_i, s = sigma_i, t = sigma_{i+1}:
        x_next = (sigma_t / sigma_s) x~ - alpha_t phi1 m - alpha_t B (1/2) (m1 - m) / r1,                            r1 = (lambda_{i-1} - lambda_i) / h   (p = 2 only)
      last step: sigma_t = 0, h = +inf; the limits phi1 = -1 and sigma_t / sigma_s = 0 are written out (x_n = m), no inf / inf is evaluated."""
    import math

    sig = [float(v) for v in torch.as_tensor(sigmas, dtype=torch.float64).reshape(-1).tolist()]
    n = len(sig) - 1
    if n < 1:
        raise ValueError("wan_unipc_tables: sigmas must hold n + 1 values")
    if solver_order not in (1, 2):
        raise NotImplementedError(f"wan_unipc: solver_order = {solver_order!r} is not covered (1 or 2)")
    if any(not 0.0 < s < 1.0 for s in sig[:-1]) or sig[-1] != 0.0 or any(b >= a for a, b in zip(sig, sig[1:])):
        raise ValueError("wan_unipc_tables: sigmas must decrease strictly inside (0, 1) and end in 0")
    skip = set(int(i) for i in disable_corrector)
    lam = [math.log1p(-s) - math.log(s) for s in sig[:-1]]
    order = [min(solver_order, n - i, i + 1) for i in range(n)]
    rows = []
    for i in range(n):
        cx, cl, c1, c2, ct = 1.0, 0.0, 0.0, 0.0, 0.0
        if i >= 1 and (i - 1) not in skip:
            s, t = sig[i - 1], sig[i]
            h = lam[i] - lam[i - 1]
            phi1 = bh = math.expm1(-h)
            at = 1.0 - t
            if order[i - 1] == 1:
                rho0, rho_last, r1 = 0.0, 0.5, 1.0
            else:
                r1 = (lam[i - 2] - lam[i - 1]) / h
                hh = -h
                g1 = phi1 / hh - 1.0
                g2 = g1 / hh - 0.5
                b1, b2 = g1 / bh, 2.0 * g2 / bh
                # [[1, 1], [r1, 1]] (rho0, rho_last) = (b1, b2)
                rho0 = (b2 - b1) / (r1 - 1.0)
                rho_last = b1 - rho0
            cx, cl = 0.0, t / s
            c2 = -at * bh * rho0 / r1
            ct = -at * bh * rho_last
            c1 = -at * phi1 - c2 - ct
        if i == n - 1:  # sigma_t = 0: h = +inf, phi1 = -1, sigma_t / sigma_s = 0; order 1
            px, p0, p1 = 0.0, 1.0, 0.0
        else:
            s, t = sig[i], sig[i + 1]
            h = lam[i + 1] - lam[i]
            phi1 = bh = math.expm1(-h)
            at = 1.0 - t
            px, p0, p1 = t / s, -at * phi1, 0.0
            if order[i] == 2:
                r1 = (lam[i - 1] - lam[i]) / h
                p1 = -at * bh * 0.5 / r1
                p0 -= p1
        rows.append([cx, cl, c1, c2, ct, px, p0, p1])
    return torch.tensor(rows, dtype=torch.float64).to(dtype)


class MI355XWanLatentSampler:
    """Denoising loop over a ``MI355XWanTransformer3DModel`` (``ftmi_wan_sample``; ``ftmi_wan_sample_ms`` when ``scheduler_config["_class_name"]`` is
    ``UniPCMultistepScheduler``, the scheduler of the Wan2.1 checkpoints).  The adapters are read at every ``sample``: a sample taken between two optimiser steps
    sees them as they are, the folded patch adapter is folded again at the first step of every call."""

    def __init__(self, transformer: MI355XWanTransformer3DModel, scheduler_config: Optional[Dict[str, Any]] = None):
        self.transformer = transformer
        self.unipc = is_unipc(scheduler_config)
        if self.unipc:
            self.scheduler_config = _unipc_config(scheduler_config)
        else:
            self.scheduler_config = dict(WAN_SCHEDULER_CONFIG if scheduler_config is None else scheduler_config)

    # -- what the model is ---------------------------------------------------------------------------------------------------------------------------
    @property
    def extra_channels(self) -> int:
        """Input channels past the latents: 20 for image-to-video (4 mask + 16 condition), 16 for a control model, 0 for text-to-video."""
        c = self.transformer.config
        return c.in_channels - c.out_channels

    def _check_model(self) -> None:
        tr = self.transformer
        if tr.root.numel() < tr.root_layout.total or tr._root_src is not None or any(b.flat.numel() < b.layout.total or b._param_src is not None for b in tr.blocks):
            raise RuntimeError("MI355XWanLatentSampler: the parameters are sharded over the ranks (FSDP); sample from a model that holds its whole flat buffers")
        first = tr.blocks[0]
        for blk in tr.blocks:
            same = (blk.lora_A is None) == (first.lora_A is None) and (blk.lora_ffn is None) == (first.lora_ffn is None) and blk.lora_scale == first.lora_scale
            if not same or (blk.lora_A is not None and blk.lora_A.shape != first.lora_A.shape):
                raise NotImplementedError("MI355XWanLatentSampler: every block carries the same adapter set, rank and scale")

    # -- the state-independent inputs of the loop ----------------------------------------------------------------------------------------------------
    def _lin(self, t: torch.Tensor, name: str, **kw):
        tr = self.transformer
        return ops.gemm_nt(t.reshape(-1, t.shape[-1]), tr.rparam(f"{name}.weight"), tr.rparam(f"{name}.bias"), **kw)

    def text_rows(self, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor]) -> torch.Tensor:
        """enc bf16 [P B, T, D]: the text embedder on the unconditional rows, then the conditional ones (the launches of the model's forward at batch P B)."""
        dev = self.transformer.device
        text = prompt_embeds if negative_prompt_embeds is None else torch.cat([negative_prompt_embeds.to(prompt_embeds.device), prompt_embeds], dim=0)
        text = text.to(dev, bf16).contiguous()
        act, _ = self._lin(text, "condition_embedder.text_embedder.linear_1", epilogue=1, want_out2=True)
        return self._lin(act, "condition_embedder.text_embedder.linear_2").view(text.shape[0], text.shape[1], -1)

    def step_tables(self, timesteps: torch.Tensor, rows: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (tproj bf16 [n, 6 D], head shift fp32 [n, D], head scale fp32 [n, D]) for the n timesteps of a run.  Every step runs the condition embedder's
        launches at ``rows`` = P B equal timesteps, as the model's forward does, and keeps one row: the rounding points are those of model.py's forward
        (``mod = table + temb`` in bf16, ``shift = float(mod[0])``, ``scale = float(1 + mod[1]) - 1``)."""
        tr = self.transformer
        c, silu = tr.config, torch.nn.functional.silu
        tprojs, shifts, scales = [], [], []
        table = tr.rparam("scale_shift_table")
        for t in timesteps.tolist():
            ts = torch.full((rows,), t, dtype=torch.float32, device=tr.device)
            t_emb = timestep_embedding(ts, c.freq_dim).to(bf16)
            temb = self._lin(silu(self._lin(t_emb, "condition_embedder.time_embedder.linear_1")), "condition_embedder.time_embedder.linear_2")
            tprojs.append(self._lin(silu(temb), "condition_embedder.time_proj")[0])
            mod = table + temb.unsqueeze(1)  # [rows, 2, D] bf16
            shifts.append(mod[0, 0].float())
            scales.append((1 + mod[0, 1]).float() - 1)
        return torch.stack(tprojs).contiguous(), torch.stack(shifts).contiguous(), torch.stack(scales).contiguous()

    def geometry(self, B: int, num_frames: int, height: int, width: int, guidance: bool) -> "_lib.WanSampleGeometry":
        tr = self.transformer
        c = tr.config
        Kp = tr.root_layout.offsets["patch_embedding.weight"][1][1]
        return ops.wan_sample_geometry(B, c.out_channels, num_frames, height, width, Kp, extra_channels=self.extra_channels,
                                       copies=2 if tr.patch_lora_A is not None else 1, guidance=guidance, patch_size=tuple(c.patch_size),
                                       po=tr.root_layout.offsets["proj_out.weight"][1][0])

    def c_arguments(self, geo, T: int, TI: int, steps: int, guidance_scale: float):
        """-> (ftmi_wan_sample_config, ftmi_wan_sample_weights, the objects the two structures point into).  ``TI``: the image tokens of one row of enc_img; of a
        first/last-frame model (``config.pos_embed_seq_len``) both images', whose second half goes into the structures as TI2."""
        tr = self.transformer
        c = tr.config
        TI2 = c.second_image_tokens if TI > 0 else 0
        if TI2 and TI != 2 * TI2:
            raise ValueError(f"sample: a first/last-frame model takes {2 * TI2} image tokens (pos_embed_seq_len), got {TI}")
        TI -= TI2
        S, rows = (geo.F // geo.pt) * (geo.H // geo.ph) * (geo.W // geo.pw), geo.P * geo.B
        L = len(tr.blocks)
        blocks = (_lib.WanLoraFfnBlockWeights * L)()
        img = (ctypes.c_void_p * L)()
        keep: List[Any] = [blocks, img]
        first = tr.blocks[0]
        for i, blk in enumerate(tr.blocks):
            ffn = tuple(blk.lora_ffn) if blk.lora_ffn is not None else None
            _, wf, k = _WanLoRABlockNativeFunction._args(blk, rows, S, T, blk.lora_A, blk.lora_B, backward=False, TI=TI, ffn=ffn)
            blocks[i] = wf
            keep += k
            if TI > 0:
                img[i] = blk._img_params().data_ptr()
        r = 0 if first.lora_A is None else int(first.lora_A.shape[1])
        fold = tr.patch_lora_A is not None
        cfg = _lib.WanSampleConfig(geo=geo, T=T, TI=TI, D=c.inner_dim, heads=c.num_attention_heads, ffn_dim=c.ffn_dim, L=L, eps=float(c.eps), gemm_variant=8, r=r,
                                   lora_scale=float(first.lora_scale), ffn=int(first.lora_ffn is not None), patch_fold=int(fold),
                                   patch_r=int(tr.patch_lora_A.shape[0]) if fold else 0, patch_scale=float(tr.patch_lora_scale) if fold else 0.0, steps=steps,
                                   guidance=float(guidance_scale), TI2=TI2)
        w = _lib.WanSampleWeights()
        w.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.WanLoraFfnBlockWeights))
        w.img_params = ctypes.cast(img, ctypes.POINTER(ctypes.c_void_p)) if TI > 0 else None
        w.patch_w, w.patch_b = tr.rparam("patch_embedding.weight").data_ptr(), tr.rparam("patch_embedding.bias").data_ptr()
        w.proj_w, w.proj_b = tr.rparam("proj_out.weight").data_ptr(), tr.rparam("proj_out.bias").data_ptr()
        if fold:
            la, lb = tr.patch_lora_A.detach().contiguous(), tr.patch_lora_B.detach().contiguous()
            dw, w2, _ = tr._patch_ws
            keep += [la, lb]
            w.patch_lora_a, w.patch_lora_b, w.patch_dw, w.patch_w2 = la.data_ptr(), lb.data_ptr(), dw.data_ptr(), w2.data_ptr()
            tr._patch_fold_key = None  # the call folds the adapter as it is now into the model's workspace: the next training forward folds for itself
        return cfg, w, keep

    def schedule(self, num_inference_steps: int, sigmas, timesteps) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (sigmas [n + 1], timesteps fp32 [n]) on the host.  Flow-match Euler: fp32 sigmas, timesteps ``sigma N``.  UniPC: fp64 sigmas (the folded tables are
        computed from them; the kernel reads their fp32 values), timesteps ``trunc(sigma N)`` -- the scheduler's int64 timesteps."""
        if self.unipc:
            sig = wan_unipc_schedule(num_inference_steps, self.scheduler_config)[0] if sigmas is None else torch.as_tensor(sigmas, dtype=torch.float64).reshape(-1).cpu()
            n = sig.numel() - 1
            if n < 1:
                raise ValueError("sample: sigmas must hold n + 1 values")
            N = float(self.scheduler_config["num_train_timesteps"])
            ts = torch.trunc(sig[:-1] * N).float() if timesteps is None else torch.as_tensor(timesteps, dtype=torch.float32).reshape(-1).cpu()
            if ts.numel() != n:
                raise ValueError("sample: timesteps must hold one value per step")
            return sig, ts
        sig = wan_flow_match_sigmas(num_inference_steps, self.scheduler_config) if sigmas is None else torch.as_tensor(sigmas, dtype=torch.float32).reshape(-1).cpu()
        n = sig.numel() - 1
        if n < 1:
            raise ValueError("sample: sigmas must hold n + 1 values")
        ts = sig[:-1] * float(self.scheduler_config.get("num_train_timesteps", 1000)) if timesteps is None else torch.as_tensor(timesteps, dtype=torch.float32).reshape(-1).cpu()
        if ts.numel() != n:
            raise ValueError("sample: timesteps must hold one value per step")
        return sig, ts

    def unipc_tables(self, sigmas: torch.Tensor) -> torch.Tensor:
        """-> fp32 [n, 8] on the host: ``wan_unipc_tables`` with the config's ``solver_order`` and ``disable_corrector``."""
        return wan_unipc_tables(sigmas, int(self.scheduler_config["solver_order"]), self.scheduler_config.get("disable_corrector") or ())

    def check_inputs(self, prompt_embeds, negative_prompt_embeds, guidance_scale: float, image_embeds, condition_latents, control_latents, B: int, num_frames: int,
                     height: int, width: int) -> Optional[torch.Tensor]:
        """Every refusal of ``sample``, with its reason; -> the extra input channels [B, Cx, F, H, W] bf16 (None for text-to-video)."""
        tr = self.transformer
        c = tr.config
        self._check_model()
        if prompt_embeds.dim() != 3 or prompt_embeds.shape[-1] != c.text_dim:
            raise ValueError(f"sample: prompt_embeds must be [B, T, {c.text_dim}], got {tuple(prompt_embeds.shape)}")
        if float(guidance_scale) != 1.0:
            if negative_prompt_embeds is None:
                raise ValueError("sample: guidance_scale != 1 needs negative_prompt_embeds")
            if tuple(negative_prompt_embeds.shape) != tuple(prompt_embeds.shape):
                raise ValueError("sample: negative_prompt_embeds must be shaped like prompt_embeds (pad both prompts to one length)")
        i2v = c.image_dim is not None
        widened = not i2v and c.in_channels > c.out_channels
        if (image_embeds is not None or condition_latents is not None) and not i2v:
            raise ValueError("sample: image_embeds / condition_latents go with an image-to-video model (config.image_dim); this model has none")
        if i2v and (image_embeds is None or condition_latents is None):
            raise ValueError("sample: an image-to-video model (config.image_dim) needs image_embeds and condition_latents")
        if control_latents is not None and not widened:
            raise ValueError("sample: control_latents go with a model whose patch embedding was widened (expand_patch_embedding); this one takes "
                             f"{c.in_channels} channels for {c.out_channels} latent channels")
        if widened and control_latents is None:
            raise ValueError(f"sample: the patch embedding was widened to {c.in_channels} channels: the model needs control_latents")
        extra = condition_latents if i2v else control_latents
        if extra is None:
            return None
        want = (B, self.extra_channels, num_frames, height, width)
        if tuple(extra.shape) != want:
            raise ValueError(f"sample: {'condition_latents' if i2v else 'control_latents'} must be {list(want)}, got {list(extra.shape)}")
        if i2v and c.pos_embed_seq_len is not None:  # first/last-frame: both layouts of the image embedder, see MI355XWanTransformer3DModel._embed_image
            n = c.pos_embed_seq_len
            if image_embeds.dim() != 3 or tuple(image_embeds.shape) not in ((B, n, c.image_dim), (2 * B, n // 2, c.image_dim)):
                raise ValueError(f"sample: image_embeds of a first/last-frame model must be [{B}, {n}, {c.image_dim}] or [{2 * B}, {n // 2}, {c.image_dim}], "
                                 f"got {tuple(image_embeds.shape)}")
        elif i2v and (image_embeds.dim() != 3 or image_embeds.shape[0] != B or image_embeds.shape[-1] != c.image_dim):
            raise ValueError(f"sample: image_embeds must be [{B}, TI, {c.image_dim}], got {tuple(image_embeds.shape)}")
        return extra.to(tr.device, bf16).contiguous()

    @torch.no_grad()
    def sample(self, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor], num_frames: int, height: int, width: int,
               num_inference_steps: int = 50, guidance_scale: float = 5.0, sigmas: Optional[Sequence[float]] = None, timesteps: Optional[Sequence[float]] = None,
               generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, latents_mean: Optional[torch.Tensor] = None,
               latents_std: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None, condition_latents: Optional[torch.Tensor] = None,
               control_latents: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> denormalised latents [B, C, F, H, W] bf16 (the VAE decoder's input).

        ``num_frames`` / ``height`` / ``width`` are the LATENT grid.  ``sigmas`` [n + 1] / ``timesteps`` [n] override the schedule (default:
        ``wan_flow_match_sigmas`` and ``sigma * num_train_timesteps``; with a UniPC config ``wan_unipc_schedule`` and its truncated timesteps); the rows of one step share one timestep, as in the pipeline.  The initial noise is
        ``torch.randn([B, C, F, H, W], fp32, generator)`` on the transformer's device -- the pipeline's draw order, so one seed gives the same noise -- or
        ``latents``.  ``latents_mean`` / ``latents_std`` ([C]: the VAE's statistics, the standard deviation ITSELF, not the 1 / std of the training
        processors) denormalise the result; without them it stays normalised.

        Image-to-video: ``image_embeds`` [B, TI, image_dim] (the CLIP tokens, sent through the model's image embedder; a first/last-frame model takes
        [B, TI + TI2, image_dim] = [B, pos_embed_seq_len, image_dim], a sample's first image and then its last, or [2B, TI, image_dim]) and ``condition_latents``
        [B, 20, F, H, W] (4 mask + 16 normalised condition channels, what the pipeline concatenates to the latents).  Control: ``control_latents``
        [B, 16, F, H, W], normalised and frame-conditioned (``validation_latents`` of the control specification does both).  These channels are constant over
        the loop: they are written into the model input once."""
        tr = self.transformer
        dev, c = tr.device, tr.config
        B, T = prompt_embeds.shape[0], prompt_embeds.shape[1]
        g = float(guidance_scale)
        extra = self.check_inputs(prompt_embeds, negative_prompt_embeds, g, image_embeds, condition_latents, control_latents, B, num_frames, height, width)
        sig, ts = self.schedule(num_inference_steps, sigmas, timesteps)
        if latents is None:
            latents = torch.randn((B, c.out_channels, num_frames, height, width), generator=generator, device=dev, dtype=torch.float32)
        elif tuple(latents.shape) != (B, c.out_channels, num_frames, height, width):
            raise ValueError(f"sample: latents must be [{B}, {c.out_channels}, {num_frames}, {height}, {width}], got {list(latents.shape)}")
        latents = latents.to(dev, torch.float32).contiguous()

        geo = self.geometry(B, num_frames, height, width, guidance=g != 1.0)
        enc = self.text_rows(prompt_embeds, negative_prompt_embeds if g != 1.0 else None)
        enc_img = None
        if image_embeds is not None:
            if c.pos_embed_seq_len is not None:
                image_embeds = image_embeds.reshape(B, c.pos_embed_seq_len, c.image_dim)
            enc_img = tr._embed_image(torch.cat([image_embeds] * geo.P, dim=0))
        tproj, shift, scale = self.step_tables(ts, geo.P * B)
        cfg, weights, keep = self.c_arguments(geo, T, 0 if enc_img is None else enc_img.shape[1], ts.numel(), g)
        x, cols = ops.wan_sample_init(geo, latents, extra)
        if self.unipc:
            ops.wan_sample_ms(cfg, weights, cols, x, tproj, shift, scale, enc, enc_img, tr._rope(num_frames, height, width), self.unipc_tables(sig).to(dev),
                              sig.float().to(dev))
        else:
            ops.wan_sample(cfg, weights, cols, x, tproj, shift, scale, enc, enc_img, tr._rope(num_frames, height, width), sig.to(dev))
        del keep
        C = c.out_channels
        mean = torch.zeros(C, dtype=torch.float32, device=dev) if latents_mean is None else latents_mean.reshape(-1)[:C].to(dev, torch.float32).contiguous()
        std = torch.ones(C, dtype=torch.float32, device=dev) if latents_std is None else latents_std.reshape(-1)[:C].to(dev, torch.float32).contiguous()
        return ops.wan_sample_finish(geo, x, mean, std)
