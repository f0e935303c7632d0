"""The collective plumbing of the context-parallel attention path on two CPU processes over gloo: the kernels are replaced by fp32 torch stand-ins with the
same contract (ops.attn_fwd_carry / attn_bwd / accum_bf16), so what is checked is the mesh path itself -- K / V gathered, the chunk walk starting at the own
rank, dK / dV summed onto their owners -- against single-process attention over the whole sequence."""

import os

import torch

B, H, S, D, WORLD = 1, 2, 12, 64, 2
N = S // WORLD  # tokens per rank
LOG2E = 1.4426950408889634


def _inputs():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(B, H, S, D, generator=g) for _ in range(4)]  # q, k, v, dout over the whole sequence


def _worker(rank, port, queue):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(WORLD), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from torch.distributed.device_mesh import init_device_mesh

    from finetrainers_amd import attention_dispatch as ad

    walked = []
    def carry(q, k, v, acc, lse, key_bias=None, scale=None, first=False, last=False, out=None):
        walked.append(float(k[0, 0, 0, 0]))
        s = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
        lse_c = torch.logsumexp(s / LOG2E, -1) * LOG2E
        o_c = torch.exp2(s - lse_c[..., None]) @ v
        new = lse_c if first else torch.logaddexp2(lse, lse_c)
        acc.copy_(o_c if first else acc * torch.exp2(lse - new)[..., None] + o_c * torch.exp2(lse_c - new)[..., None])
        lse.copy_(new)
        return acc.clone() if last else None

    def bwd(q, k, v, out, lse, dout, key_bias=None, scale=None):
        p = torch.exp2((q @ k.transpose(-1, -2)) * (scale * LOG2E) - lse[..., None])
        ds = p * (dout @ v.transpose(-1, -2) - (dout * out).sum(-1, keepdim=True))
        return scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ dout

    def accum(acc, x, last=False):
        acc.add_(x)
        return acc.clone() if last else None

    ad.ops.attn_fwd_carry, ad.ops.attn_bwd, ad.ops.accum_bf16 = carry, bwd, accum
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        q, k, v, dout = (t[:, :, rank * N:(rank + 1) * N].clone().requires_grad_() for t in _inputs())
        with ad.attention_provider(ad.AttentionProvider.MI355X), ad.context_parallel(init_device_mesh("cpu", (WORLD,))):
            out = ad.attention_dispatch(q, k, v, scale=0.2)
        out.backward(dout.detach())
        queue.put((rank, walked, out.detach(), q.grad, k.grad, v.grad))
    finally:
        dist.destroy_process_group()


def test_context_parallel_attention_world_size_2_gloo():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    port = 29250 + (os.getpid() % 100)
    procs = [ctx.Process(target=_worker, args=(r, port, queue)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = sorted(queue.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    q, k, v, dout = (t.requires_grad_() for t in _inputs())
    ref = torch.softmax((q @ k.transpose(-1, -2)) * 0.2, -1) @ v
    ref.backward(dout.detach())
    for rank, walked, out, dq, dk, dv in res:
        own = slice(rank * N, (rank + 1) * N)
        assert walked == [float(k.detach()[0, 0, ((rank + j) % WORLD) * N, 0]) for j in range(WORLD)]  # the walk starts with the rank's own chunk
        for got, want in ((out, ref), (dq, q.grad), (dk, k.grad), (dv, v.grad)):
            torch.testing.assert_close(got, want.detach()[:, :, own], rtol=1e-4, atol=1e-5)
