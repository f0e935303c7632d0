"""Regenerate tests/golden/wan_control_fixtures.safetensors from the reference tree (what oracle/make_golden.py does for the other functions): the
reference's own ``apply_frame_conditioning_on_latents`` (trainer/control_trainer/data.py) and ``_expand_conv3d_with_zeroed_weights`` (models/utils.py) are
AST-extracted and executed on the CPU; only their inputs and outputs are stored.  Run on the development machine:

    FTMI_REFERENCE=<checkout of the reference> python tools/make_wan_control_golden.py

No test and no GPU path reads the reference: they read the fixture file.

Keys.  ``fc.in.n{Fc}``: control latents [1, 2, Fc, 2, 2] (every element non-zero, so the kept frames can be read off an output).
``fc.{type}.n{Fc}.e{F}.i{index}.s{seed}.out`` / ``.outmask``: the function's result for ``expected_num_frames = F`` without / with ``concatenate_mask``,
after ``random.seed(seed)`` (both calls reseeded).  ``conv.*``: a Conv3d(4 -> 8, kernel = stride = (1, 2, 2)) and its expansion to 8 input channels."""

from __future__ import annotations

import ast
import os
import random
import sys
from enum import Enum
from typing import Optional

import torch
from safetensors.torch import save_file

REF = os.environ.get("FTMI_REFERENCE", "")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "wan_control_fixtures.safetensors")

EXPECTED_FRAMES = 3
CONTROL_FRAMES = (2, 3, 5)  # shorter than, equal to and longer than the latents
SEEDS = (0, 1, 2)
CASES = [("index", 0), ("index", 1), ("index", 7), ("prefix", None), ("random", None), ("first_and_last", None), ("full", None)]


def extract(relpath: str, name: str, ns: dict, kind=ast.FunctionDef):
    path = os.path.join(REF, relpath)
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    node = next(n for n in ast.walk(tree) if isinstance(n, kind) and n.name == name)
    node.decorator_list = []
    mod = ast.Module(body=[node], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = dict(ns)
    exec(compile(mod, path, "exec"), ns)
    obj = ns[name]
    if kind is ast.FunctionDef:
        obj.__globals__.update(ns)
    return obj


def main() -> None:
    if not os.path.isdir(os.path.join(REF, "finetrainers")):
        raise SystemExit("set FTMI_REFERENCE to a checkout of the reference (the directory that holds finetrainers/)")
    base = {"torch": torch, "random": random, "Optional": Optional, "Enum": Enum}
    fct = extract("finetrainers/trainer/control_trainer/config.py", "FrameConditioningType", base, kind=ast.ClassDef)
    apply = extract("finetrainers/trainer/control_trainer/data.py", "apply_frame_conditioning_on_latents", dict(base, FrameConditioningType=fct))
    expand = extract("finetrainers/models/utils.py", "_expand_conv3d_with_zeroed_weights", base)

    out = {}
    g = torch.Generator().manual_seed(20)
    for n in CONTROL_FRAMES:
        x = torch.randn((1, 2, n, 2, 2), generator=g)
        x = (x + torch.sign(x) * 0.25).to(torch.bfloat16)  # away from zero
        assert bool((x != 0).all())
        out[f"fc.in.n{n}"] = x
        for name, index in CASES:
            for seed in (SEEDS if name in ("prefix", "random") else (0,)):
                key = f"fc.{name}.n{n}.e{EXPECTED_FRAMES}.i{index}.s{seed}"
                for suffix, cat in ((".out", False), (".outmask", True)):
                    random.seed(seed)
                    out[key + suffix] = apply(x.clone(), EXPECTED_FRAMES, channel_dim=1, frame_dim=2, frame_conditioning_type=fct(name),
                                              frame_conditioning_index=index, concatenate_mask=cat).contiguous()
    torch.manual_seed(21)
    conv = torch.nn.Conv3d(4, 8, kernel_size=(1, 2, 2), stride=(1, 2, 2)).to(torch.bfloat16)
    with torch.no_grad():
        wide = expand(conv, new_in_channels=8)
    out["conv.weight"], out["conv.bias"] = conv.weight.detach().clone(), conv.bias.detach().clone()
    out["conv.expanded.weight"], out["conv.expanded.bias"] = wide.weight.detach().clone(), wide.bias.detach().clone()
    save_file({k: v.contiguous() for k, v in out.items()}, OUT)
    print(f"{OUT}: {len(out)} tensors, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
