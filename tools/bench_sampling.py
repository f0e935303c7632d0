"""LTX-Video latent sampling at BASELINE config 2 size (28 blocks, one 49 x 512 x 768 video = 2 688 tokens, cond + uncond, rank 64): HIP-event time per
denoising step of ftmi_ltx_ff_sample with the text-side work hoisted out of the step loop (the product) and repeated in every step (FTMI_SAMPLE_HOIST=0),
interleaved on one box, beside a plain batch-2 forward of the same model.  --cond-frames K (repeatable) adds ftmi_ltx_ff_sample_cond with the first K latent
frames held to the interleaved rounds (K = 0: per-frame conditioning tables, nothing held).
`python tools/bench_sampling.py [--steps 8] [--rounds 5] [--cond-frames 0 --cond-frames 1] [--out FILE]`"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from finetrainers_amd import _lib, ops  # noqa: E402
from finetrainers_amd.ltx_video import LTXTransformerConfig, MI355XLTXVideoModelSpecification  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=28)
ap.add_argument("--cond-frames", type=int, action="append", default=[], help="also time ftmi_ltx_ff_sample_cond with this many latent frames held (repeatable)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
bf16 = torch.bfloat16
F_, H_, W_, T = 7, 16, 24, 128
S = F_ * H_ * W_
spec = MI355XLTXVideoModelSpecification(transformer_config=LTXTransformerConfig(num_layers=a.layers))
model = spec.load_diffusion_models(device=dev, random_init_seed=0)["transformer"]
model.add_adapter(r=64, lora_alpha=64.0)
g = torch.Generator(device=dev).manual_seed(3)
with torch.no_grad():
    model.lora_flat.copy_(torch.randn(model.lora_flat.shape, generator=g, device=dev) * 0.01)
text_c = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
text_u = torch.randn((1, T, 4096), generator=g, device=dev).to(bf16)
kb_c = torch.zeros((1, T), device=dev)
kb_c[:, 96:] = -10000.0
kb_u = torch.zeros((1, T), device=dev)
kb_u[:, 32:] = -10000.0
x0 = torch.randn((1, S, 128), generator=g, device=dev)
sigmas = torch.linspace(1.0, 0.0, a.steps + 1, device=dev)
timesteps = (sigmas[:-1] * 1000.0).contiguous()
cos, sin = model.rope_tables(F_, H_, W_, [1 / (25 / 8), 32, 32])
model.refresh_lora_copies()
cfg = model._c_config(1, S, T)
weights = model._c_weights(cos, sin)
ws = torch.empty((max([ops.ltx_sample_workspace_bytes(cfg, True, weights)] + [ops.ltx_sample_cond_workspace_bytes(cfg, True, F_, weights) for _ in a.cond_frames]),),
                 dtype=torch.uint8, device=dev)
lib = _lib.load()


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def sample(hoist):
    os.environ["FTMI_SAMPLE_HOIST"] = "1" if hoist else "0"
    lib.ftmi_reload_switches()
    x = x0.clone()
    return event_ms(lambda: ops.ltx_sample(cfg, weights, text_c, text_u, kb_c, kb_u, x, sigmas, timesteps, 3.0, workspace=ws)) / a.steps


def sample_cond(k):
    os.environ["FTMI_SAMPLE_HOIST"] = "1"
    lib.ftmi_reload_switches()
    x = x0.clone()
    return event_ms(lambda: ops.ltx_sample_cond(cfg, weights, text_c, text_u, kb_c, kb_u, x, sigmas, timesteps, 3.0, F_, k, workspace=ws)) / a.steps


# plain forward at batch 2 (what one denoising step would cost through the training forward, activations kept)
fcfg = model._c_config(2, S, T, checkpoint=False)
fws_bytes = lib.ftmi_ltx_ff_workspace_bytes(ctypes.byref(fcfg), ctypes.byref(weights))
fws = torch.empty((fws_bytes,), dtype=torch.uint8, device=dev)
xin = torch.cat([x0, x0]).to(bf16)
text2, kb2 = torch.cat([text_u, text_c]).contiguous(), torch.cat([kb_u, kb_c]).contiguous()
tv = timesteps[:1].expand(2).contiguous()
pred = torch.empty((2, S, 128), dtype=bf16, device=dev)


def forward():
    def run():
        for _ in range(a.steps):
            _lib.check(lib.ftmi_ltx_ff_forward(ctypes.byref(fcfg), ctypes.byref(weights), _lib.ptr(xin), _lib.ptr(text2), _lib.ptr(kb2), _lib.ptr(tv), _lib.ptr(pred),
                                               _lib.ptr(fws), fws_bytes, _lib.stream_ptr()), "ftmi_ltx_ff_forward")
    return event_ms(run) / a.steps


for _ in range(2):  # warm-up
    sample(True), sample(False), forward()
    for k in a.cond_frames:
        sample_cond(k)
rows = {"hoisted": [], "unhoisted": [], "forward_batch2": [], **{f"cond_frames_{k}": [] for k in a.cond_frames}}
for _ in range(a.rounds):  # interleaved
    rows["hoisted"].append(sample(True))
    for k in a.cond_frames:
        rows[f"cond_frames_{k}"].append(sample_cond(k))
    rows["unhoisted"].append(sample(False))
    rows["forward_batch2"].append(forward())
del os.environ["FTMI_SAMPLE_HOIST"]
lib.ftmi_reload_switches()
res = {"what": "ms per denoising step, HIP events around the whole call / steps", "layers": a.layers, "tokens": S, "text_tokens": T, "videos": 1, "guidance": 3.0,
       "steps_per_call": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
       **{k + "_ms_per_step": [round(v, 4) for v in vs] for k, vs in rows.items()},
       **{k + "_median": round(statistics.median(vs), 4) for k, vs in rows.items()}}
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
