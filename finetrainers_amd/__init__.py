"""finetrainers_amd -- MI355X (gfx950) native backend for the finetrainers LTX-Video LoRA SFT step.

Only what the hot path needs lives here: ``csrc/`` (hand-written HIP kernels + the C ABI of
include/ftmi355.h), the ctypes binding, and the host-side mirrors of the reference's two plugin surfaces
(``ModelSpecification`` and the attention-provider registry) plus the step/DP glue of SFTTrainer._train.
"""

__version__ = "0.1.0"


def __getattr__(name):  # MI355XFp8LoRALinear (fp8_linear.py), resolved on first use: importing the package itself stays free of torch
    if name == "MI355XFp8LoRALinear":
        from .fp8_linear import MI355XFp8LoRALinear

        return MI355XFp8LoRALinear
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
