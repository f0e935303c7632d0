"""The Wan LoRA block without transposed weight twins (use_weight_twins(False): NULL w_*_t, every input gradient through ftmi_gemm_nn) next to the twinned
block on identical inputs, both against the fp32 evaluation of the oracle block tests/test_gpu_wan_ffn_lora.py builds.  Per tensor (dx, d text, every adapter
gradient) r = rel-L2 error against the fp32 oracle / E, E = 2^-8 the bf16 format bound.  ASSERTED: r(no twins) <= r(twins) + MARGIN.
MEASURED on an MI355X over the eight block cases: largest r(no twins) - r(twins) = +5.36e-08 (per case +1.86e-08 .. +5.36e-08); MARGIN = max(1.5 x that,
0.15) = 0.15; the model case: 8.00e-07.  Bit identity with the NT path is not required and not asserted."""

import pytest
import torch

import test_gpu_wan_ffn_lora as ffn

pytestmark = pytest.mark.gpu
E, MARGIN = 2.0**-8, 0.15
GEOM, S, T, RANK = (256, 2, 256), 130, 64, 64


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("adapters", [8, 10])
@pytest.mark.parametrize("ti", [0, 257])
def test_block_without_twins_sits_where_the_twinned_block_sits(ti, adapters, ckpt):
    oblk, gblk = ffn._block_pair(GEOM, RANK, i2v=ti > 0)
    if adapters == 8:  # the eight attention adapters alone: none on the feed-forward here, and a zero up-projection there (it then contributes exactly nothing)
        gblk.lora_ffn = None
        with torch.no_grad():
            for n, p in oblk.ffn.named_parameters():
                if "lora_B" in n:
                    p.zero_()
    gblk.gradient_checkpointing = ckpt
    inp = ffn._inputs(1, S, T, GEOM[0], seed=5, ti=ti)
    rope, freqs = ffn._rope_tables(S, 128, seed=3)
    _, dx32, de32, g32 = ffn._oracle_run(oblk.float(), torch.float32, *inp[:4], freqs, inp[4])
    tw = ffn._run_gpu(gblk, *inp[:4], rope, inp[4])
    assert gblk._transposed is not None
    gblk.use_weight_twins(False)
    nn = ffn._run_gpu(gblk, *inp[:4], rope, inp[4])
    assert gblk._transposed is None, "the twin-less backward built transposed weights"
    ref = {"dx": dx32, "d text": de32, **g32}
    got = [{"dx": r[1], "d text": r[2], **ffn._user_rank(r[3], RANK)} for r in (tw, nn)]
    assert not torch.equal(tw[1], torch.zeros_like(tw[1])) and set(got[1]) <= set(ref) and len(got[1]) == 2 + 2 * adapters
    worst = -1.0
    for k in got[1]:
        r_tw, r_nn = ffn._rel(got[0][k], ref[k]) / E, ffn._rel(got[1][k], ref[k]) / E
        worst = max(worst, r_nn - r_tw)
        assert r_nn <= r_tw + MARGIN, (k, r_nn, r_tw)
    print(f"[wan-nn-dgrad TI={ti} adapters={adapters} ckpt={ckpt}] largest r(no twins) - r(twins) = {worst:+.2e}")


def test_partial_twins_and_the_python_composition_are_refused():
    _, gblk = ffn._block_pair(GEOM, RANK)
    inp, (rope, _) = ffn._inputs(1, S, T, GEOM[0], seed=5), ffn._rope_tables(S, 128, seed=3)
    whole = gblk.transposed
    gblk.transposed = lambda: {**whole(), "w_kv2": None}  # six of the seven twins reach the C call
    with pytest.raises(ValueError, match="transposed weights missing"):
        ffn._run_gpu(gblk, *inp[:4], rope)
    gblk.native = False
    with pytest.raises(ValueError, match="twin-less"):
        gblk.use_weight_twins(False)
    with pytest.raises(ValueError, match="frozen base"):
        type(gblk)(dim=GEOM[0], heads=GEOM[1], ffn_dim=GEOM[2], device=ffn._dev()).use_weight_twins(False)


def test_model_step_without_twins():
    """Two layers, ten adapters, one MI355XWanLoRAStep step (the first of an accumulation window of two, so the step's gradient buffer is read before clip and
    update): finite loss, every adapter gradient within MARGIN E of the twinned model's (rel-L2 per tensor), no transposed tensor afterwards."""
    from finetrainers_amd.wan import MI355XWanLoRAStep

    dev, b, res = ffn._dev(), ffn._batch(), []
    for twins in (True, False):
        _, gmodel = ffn._model_pair(2)
        gmodel.use_weight_twins(twins)
        step = MI355XWanLoRAStep(gmodel, gradient_accumulation_steps=2, lr=1e-3)
        out = step.step(b["moments"].to(dev), b["text"].to(dev), b["mean"].to(dev), b["std"].to(dev), b["sigmas"].to(dev), posterior_noise=b["eps"].to(dev),
                        noise=b["noise"].to(dev))
        torch.cuda.synchronize()
        assert (gmodel._proj_out_t is None) == (not twins) and all((blk._transposed is None) == (not twins) for blk in gmodel.blocks)
        grads = {}
        for i, blk in enumerate(gmodel.blocks):
            for j in range(8):
                grads[f"{i}.A{j}"], grads[f"{i}.B{j}"] = blk._grad_a_view[j].clone(), blk._grad_b_view[j].clone()
            grads.update({f"{i}.ffn{j}": v.clone() for j, v in enumerate(blk._grad_ffn_views)})
        res.append((out["loss"].item(), grads))
    (loss_tw, g_tw), (loss_nn, g_nn) = res
    assert loss_nn == loss_nn and abs(loss_nn) < float("inf") and len(g_nn) == 40
    worst = max(ffn._rel(g_nn[k], g_tw[k]) / E for k in g_nn)
    print(f"[wan-nn-dgrad model] loss {loss_nn:.6f} (twins {loss_tw:.6f}); largest rel-L2 distance of an adapter gradient from the twinned model's / E = {worst:.2e}")
    assert not [k for k in g_nn if not (float(g_tw[k].abs().max()) > 0 and ffn._rel(g_nn[k], g_tw[k]) / E <= MARGIN)]
