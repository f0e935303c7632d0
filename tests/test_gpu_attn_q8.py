"""The int8 / fp8 attention forward (ops.attn_fwd_q8, csrc/attn_q8.hip), its quantising pre-pass and the mi355x_sage provider against fp64 on the CPU.

Bounds.  Quantiser, per element, from the formats: int8 |x - code s| <= s / 2 (1 + 2^-20), for K widened by what the fp32 mean may be off -- any summation
order of Sk terms errs by at most Sk 2^-24 max|k| to first order, division included -- and by the rounding of the subtraction, 2^-24 |x|; e4m3 half an ulp,
2^-4 |v| in the normal range and 2^-10 sv below it.  Single-key weight w of a row with l = sum exp(s - max): (2^-3 + 2^-7) w + (1 + 2^-3) 2^-10 / (448 l) -- half
an e4m3 ulp on P, the same on the normaliser, the bf16 output, and the kernel's documented floor 2^-10 / 448 of the row's largest weight (its header).
Random operands: rms(o - o64) / rms(o64) at most 1.5 x that of emulate(), the scheme in fp64 torch on the CPU.
MEASURED on an MI355X, kernel / emulation per case: BASELINE.md."""

import functools
import math

import pytest
import torch

from finetrainers_amd import ops
from finetrainers_amd.attention_dispatch import AttentionProvider, _key_bias_from_mask, attention_dispatch, attention_provider

pytestmark = pytest.mark.gpu
bf16, f64, NINF = torch.bfloat16, torch.float64, float("-inf")
SHAPES = [(1, 1), (33, 63), (128, 64), (130, 65), (96, 257)]
CASES = pytest.mark.parametrize("d,Sq,Sk", [(d, sq, sk) for d in (64, 128) for sq, sk in SHAPES])
B, H = 1, 3


def gpu(t, strided):
    """[B, H, S, d] on the GPU; strided: the [B, H, S, d] view of a [B, S, H, d + 8] buffer (heads not contiguous, room between the rows)."""
    if not strided:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[2], t.shape[1], t.shape[3] + 8), float("nan"), dtype=t.dtype, device="cuda")
    buf[..., :t.shape[3]] = t.permute(0, 2, 1, 3)
    return buf[..., :t.shape[3]].permute(0, 2, 1, 3)


def ragged_bias(Sk):
    """-inf on a ragged set of keys that includes the whole last 64-key tile (never on key 0)."""
    bias = torch.zeros(B, Sk)
    bias[:, [j for j in range(1, Sk) if j % 7 == 3 or 100 <= j < 131 or j >= 64 * ((Sk - 1) // 64)]] = NINF
    return bias


def attention64(q, k, v, scale, bias=None):
    s = q.to(f64) @ k.to(f64).transpose(-1, -2) * scale + (0.0 if bias is None else bias.to(f64)[:, None, None, :])
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    return (p / l) @ v.to(f64), p / l, l


@functools.lru_cache(maxsize=None)
def random_problem(d, Sq, Sk, qmul=1.0):
    g = torch.Generator().manual_seed(31 * d + 7 * Sq + Sk)
    q, k, v = (torch.randn(B, H, S, d, generator=g).to(bf16) for S in (Sq, Sk, Sk))
    return (q.float() * qmul).to(bf16), k, v


@CASES
@pytest.mark.parametrize("smooth", [True, False])
def test_quantiser(d, Sq, Sk, smooth):
    q, k, v = random_problem(d, Sq, Sk)
    strided = (Sq, Sk) == (130, 65)
    q8, sq, k8, sk, v8, sv = (t.cpu() for t in ops.attn_q8_quantize(gpu(q, strided), gpu(k, strided), gpu(v, strided), None, smooth))
    nt, slack = -(-Sk // 64), 1 + 2.0**-20
    x, code, s = q.to(f64), q8.to(f64), sq.to(f64)[..., None]
    assert (code.abs().amax(-1) == 127).all()
    assert ((x - code * s).abs() <= 0.5 * s * slack).all()
    pad = lambda t: torch.cat([t, t.new_zeros(B, H, nt * 64 - Sk, d)], 2)  # noqa: E731
    x = pad(k.to(f64) - (k.to(f64).mean(2, keepdim=True) if smooth else 0.0)).view(B, H, nt, 64, d)
    code, s = k8.to(f64).view(B, H, nt, 64, d), sk.to(f64)[..., None, None]
    assert ((code.abs().amax((-1, -2)) == 127) | (x.abs().amax((-1, -2)) == 0)).all()  # one key: K minus its mean is all zero
    mean_err = Sk * 2.0**-24 * k.to(f64).abs().amax() if smooth else 0.0
    assert ((x - code * s).abs() <= 0.5 * s * slack + mean_err + 2.0**-24 * x.abs()).all()
    assert (code.view(B, H, nt * 64, d)[:, :, Sk:] == 0).all()
    x, s = pad(v.to(f64)), sv.to(f64)[:, :, None, :]
    assert ((v8.view(torch.uint8) & 0x7F) != 0x7F).all()
    assert ((x - v8.to(f64) * s).abs() <= torch.maximum(2.0**-4 * x.abs(), 2.0**-10 * s) * slack).all()
    assert (v8.view(torch.uint8)[:, :, Sk:] == 0).all()


def exact_problem(d, Sq, Sk, seed):
    """Integer-valued q, k in [-4, 4] whose int8 codes are the values themselves (a 127 marker in a channel where the other operand is 0)."""
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randint(-4, 5, (B, H, S, d), generator=g).to(bf16) for S in (Sq, Sk))
    q[..., 0], q[..., 1], k[..., 0], k[..., 1] = 127, 0, 0, 127
    return q, k


def check_single_key(q, k, scale, bias, keys):
    Sk, d = k.shape[2], k.shape[3]
    _, w, l = attention64(q, k, torch.zeros_like(k), scale, bias)
    qg, kg, bg = q.cuda(), k.cuda(), None if bias is None else bias.cuda()
    for j in keys:
        v = torch.zeros(B, H, Sk, d, dtype=bf16)
        v[:, :, j] = 1
        o = ops.attn_fwd_q8(qg, kg, v.cuda(), bg, scale, smooth_k=False).cpu().to(f64)
        wj = w[..., j:j + 1]
        bound = (2.0**-3 + 2.0**-7) * wj + (1 + 2.0**-3) * 2.0**-10 / (448 * l)
        r = ((o - wj).abs() / bound).amax()
        print(f"d={d} Sq={q.shape[2]} Sk={Sk} key {j}: largest |o - w| / bound {float(r):.3f}")
        assert r <= 1


@pytest.mark.parametrize("d,Sq,Sk,biased", [(d, sq, sk, False) for d in (64, 128) for sq, sk in SHAPES] + [(64, 96, 257, True), (128, 96, 257, True)])
def test_single_key_weights(d, Sq, Sk, biased):
    q, k = exact_problem(d, Sq, Sk, 5 * d + Sq + Sk)
    check_single_key(q, k, 1.0 / math.sqrt(d), ragged_bias(Sk) if biased else None, sorted({min(j, Sk - 1) for j in (0, 63, 64, Sk - 1)}))


@pytest.mark.parametrize("d", [64, 128])
def test_peak_plus_tail(d):
    """One key at logit 12 (log2 domain) over 1023 at 0: a tail weight is 2^-12 of the peak and must survive the e4m3 P (it would not under a max lagging 2^8)."""
    q, k = exact_problem(d, 33, 1024, d)
    q[..., 2:], k[..., 2:] = 0, 0
    q[..., 2], k[:, :, 500, 2] = 4, 3
    check_single_key(q, k, math.log(2.0), None, [500, 7])


def emulate(q, k, v, scale, bias=None):
    """The kernel's scheme in fp64 torch: smoothed K, int8 Q per row and K per 64 keys, e4m3 P at 448 against the row max, e4m3 V per channel, bf16 output."""
    q, k, v = q.to(f64), k.to(f64), v.to(f64)
    Sk, d, nt = k.shape[2], k.shape[3], -(-k.shape[2] // 64)
    fp8 = lambda t: t.float().to(torch.float8_e4m3fn).to(f64)  # noqa: E731
    sq = q.abs().amax(-1, keepdim=True) / 127
    kt = torch.cat([k - k.mean(2, keepdim=True), k.new_zeros(B, H, nt * 64 - Sk, d)], 2).view(B, H, nt, 64, d)
    sk = kt.abs().amax((-1, -2), keepdim=True) / 127
    kq = ((kt / sk.clamp_min(1e-300)).round() * sk).view(B, H, nt * 64, d)[:, :, :Sk]
    s = ((q / sq).round() * sq) @ kq.transpose(-1, -2) * (scale * math.log2(math.e))
    s = s + (0.0 if bias is None else bias.to(f64)[:, None, None, :] * math.log2(math.e))
    p = fp8(torch.exp2(s - s.amax(-1, keepdim=True)) * 448)
    sv = v.abs().amax(2, keepdim=True) / 448
    return ((p @ fp8(v / sv)) * sv / p.sum(-1, keepdim=True)).to(bf16).to(f64)


@pytest.mark.parametrize("d,Sq,Sk,qmul", [(d, sq, sk, 1.0) for d in (64, 128) for sq, sk in SHAPES] + [(64, 128, 64, 4.0), (128, 96, 257, 4.0)])
def test_random_against_fp64(d, Sq, Sk, qmul):
    q, k, v = random_problem(d, Sq, Sk, qmul)
    scale, strided = 1.0 / math.sqrt(d), (Sq, Sk) == (130, 65)
    bias = ragged_bias(Sk) if Sk == 257 else None
    ref = attention64(q, k, v, scale, bias)[0]
    err = lambda o: float(((o - ref) ** 2).mean().sqrt() / (ref**2).mean().sqrt())  # noqa: E731
    e_emul = err(emulate(q, k, v, scale, bias))
    e_kernel = err(ops.attn_fwd_q8(gpu(q, strided), gpu(k, strided), gpu(v, strided), None if bias is None else bias.cuda()).cpu().to(f64))
    print(f"d={d} Sq={Sq} Sk={Sk} q x {qmul:g}: kernel {e_kernel:.3e}  emulation {e_emul:.3e}  ratio {e_kernel / e_emul if e_emul else float('nan'):.3f}")
    assert e_kernel <= 1.5 * e_emul


def test_reference_provider_threshold():
    """The reference's own provider test (tests/models/attention_dispatch.py:57): randn [2, 8, 256, 64], seed 0, max |o - o64| <= 1e-1 for SAGE."""
    torch.manual_seed(0)
    q, k, v = (torch.randn(2, 8, 256, 64).to(bf16) for _ in range(3))
    o = ops.attn_fwd_q8(q.cuda(), k.cuda(), v.cuda()).cpu().to(f64)
    assert (o - attention64(q, k, v, 0.125)[0]).abs().max() <= 1e-1


def test_provider():
    q, k, v = (t.cuda() for t in random_problem(64, 96, 257))
    mask = (ragged_bias(257) == 0).cuda()[:, None, None, :]
    with attention_provider(AttentionProvider.MI355X_SAGE):
        with torch.no_grad():
            out = attention_dispatch(q, k, v, attn_mask=mask)
        assert torch.equal(out, ops.attn_fwd_q8(q, k, v, _key_bias_from_mask(mask, B, H, 257)))
        with pytest.raises(ValueError, match="mi355x_sage"):
            attention_dispatch(q.clone().requires_grad_(), k, v, attn_mask=mask)
        with torch.no_grad():
            assert torch.equal(attention_dispatch(q.clone().requires_grad_(), k, v, attn_mask=mask), out)
