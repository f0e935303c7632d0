"""The host side the four LoRA step objects share (``finetrainers_amd.lora_step.FlatLoRAStep`` over ``parallel.GradBucketReducer``), on the CPU: the span
bookkeeping of the bucketed gradient exchange against a recording backend, the HunyuanVideo step's bucket schedule, and the path of a backward that raises
after its first bucket -- on two gloo ranks, for the shared wrapper alone and through it for the Wan and the HunyuanVideo step."""
import os

import pytest
import torch
import torch.multiprocessing as mp

SMALL_WAN = dict(num_attention_heads=2, attention_head_dim=128, ffn_dim=512, text_dim=64)


class _RecordingParallel:
    """Stands in for the data-parallel backend, with nothing more than the step objects and the reducer (native=False) may touch."""
    active, world_size, rank = True, 1, 0

    def __init__(self):
        self.slices = []

    def broadcast_(self, t, src=0):
        pass

    def all_reduce_mean_async(self, t):
        self.slices.append((t.data_ptr(), t.numel()))
        return None


def test_span_bookkeeping_issues_contiguous_buckets_last_blocks_first():
    from finetrainers_amd.parallel import GradBucketReducer

    n, par = 12, _RecordingParallel()
    gflat = torch.zeros(5 * n)
    red = GradBucketReducer(par, native=False, gflat=gflat, bucket_blocks=2)
    for exchange in (1, 2):
        red.begin()
        for i in reversed(range(5)):
            red.span_done((i * n, (i + 1) * n))
        assert red.bucket_log == [(3 * n, 5 * n), (n, 3 * n), (0, n)]  # {4, 3}, {2, 1}, {0}: the span that starts at element 0 closes its bucket alone
        red.finish()
        assert red.bucket_log == [(3 * n, 5 * n), (n, 3 * n), (0, n)] and not red._ready and not red._pending
        assert par.slices[-3:] == [(gflat.data_ptr() + 4 * lo, hi - lo) for lo, hi in red.bucket_log] and len(par.slices) == 3 * exchange
        assert red.exchange_buckets == 3 and red.buckets_issued == 3 * exchange  # per exchange / cumulative


def test_a_front_span_reported_after_block_0_closes_the_last_bucket():
    from finetrainers_amd.parallel import GradBucketReducer

    n, p, par = 12, 7, _RecordingParallel()
    gflat = torch.zeros(p + 3 * n)
    red = GradBucketReducer(par, native=False, gflat=gflat, bucket_blocks=2)
    red.begin()
    for i in reversed(range(3)):
        red.span_done((p + i * n, p + (i + 1) * n))
    assert red.bucket_log == [(p + n, p + 3 * n)] and red._ready == [(p, p + n)]  # block 0 no longer starts at element 0: it waits
    red.span_done((0, p))
    assert red.bucket_log == [(p + n, p + 3 * n), (0, p + n)] and not red._ready
    red.finish()
    assert par.slices == [(gflat.data_ptr() + 4 * lo, hi - lo) for lo, hi in red.bucket_log] and red.exchange_buckets == 2
    # what is still ready when the backward ends goes out with finish()
    red.begin()
    red.span_done((p + 2 * n, p + 3 * n))
    assert red.bucket_log == []
    red.finish()
    assert red.bucket_log == [(p + 2 * n, p + 3 * n)] and par.slices[-1] == (gflat.data_ptr() + 4 * (p + 2 * n), n)


def test_spans_that_do_not_form_one_slice_trip_the_assertion():
    from finetrainers_amd.parallel import GradBucketReducer

    n, par = 12, _RecordingParallel()
    red = GradBucketReducer(par, native=False, gflat=torch.zeros(5 * n), bucket_blocks=2)
    red.begin()
    red.span_done((4 * n, 5 * n))
    with pytest.raises(AssertionError, match="finished blocks must form one contiguous slice of the flat gradient"):
        red.span_done((2 * n, 3 * n))
    assert par.slices == []
    red.abort()
    assert not red._ready and not red._pending


def _hunyuan_model(nl=1, ns=1):
    from finetrainers_amd.hunyuan_video import HunyuanVideoTransformerConfig, MI355XHunyuanVideoTransformer3DModel

    cfg = HunyuanVideoTransformerConfig(num_attention_heads=2, num_layers=nl, num_single_layers=ns, num_refiner_layers=1, text_embed_dim=64, pooled_projection_dim=64)
    model = MI355XHunyuanVideoTransformer3DModel(cfg, device=torch.device("cpu"))
    model.add_adapter(r=64, lora_alpha=32.0)
    return model, list(model.transformer_blocks) + list(model.single_transformer_blocks)


def test_hunyuan_step_bucket_schedule_on_cpu():
    """The exchange as the blocks' backward drives it (single-stream blocks first, each reporting itself through ``_grad_hook``)."""
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoSFTStep

    model, blocks = _hunyuan_model()
    par = _RecordingParallel()
    step = MI355XHunyuanVideoSFTStep(model, parallel=par, grad_bucket_blocks=1)
    assert step.buckets_issued == 0 and step.grad_bucket_blocks == 1
    step._begin_exchange(True)
    for blk in reversed(blocks):
        blk._grad_hook(blk)
    step._finish_exchange()
    log, n = step.reducer.bucket_log, step.gflat.numel()
    assert len(log) == 2 == step.buckets_issued
    assert log[0][1] == n and log[1][1] == log[0][0] and log[1][0] == 0 and sum(hi - lo for lo, hi in log) == n  # contiguous, cover the buffer once
    assert log == [step._spans[id(blk)] for blk in reversed(blocks)]
    assert par.slices == [(step.gflat.data_ptr() + 4 * lo, hi - lo) for lo, hi in log]
    assert all(blk._grad_hook is None for blk in blocks)
    step._begin_exchange(False)  # a backward that does not exchange: no hooks, nothing counted
    assert all(blk._grad_hook is None for blk in blocks)
    step._finish_exchange()
    assert step.buckets_issued == 0 and len(par.slices) == 2


def test_cogvideox_step_counts_buckets_not_slices_on_cpu():
    """Both CogVideoX hooks hand over a bucket as its (A, B) slices: two collectives, one bucket."""
    from finetrainers_amd.cogvideox import CogVideoXTransformerConfig, MI355XCogVideoXSFTStep, MI355XCogVideoXTransformer3DModel

    kw = dict(num_layers=3, sample_width=12, sample_height=8, sample_frames=9, max_text_seq_length=16)
    model = MI355XCogVideoXTransformer3DModel(CogVideoXTransformerConfig(**kw), device=torch.device("cpu"))
    model.add_adapter(r=64, lora_alpha=64.0)
    par = _RecordingParallel()
    step = MI355XCogVideoXSFTStep(model, parallel=par, grad_bucket_blocks=2)
    assert step.flat is model.lora_flat and step.gflat is model.lora_grad_flat and step.buckets_issued == 0
    n = model.lora_flat.numel() // 2
    ga, gb = step.gflat[:n].view(3, -1), step.gflat[n:].view(3, -1)
    step._begin_exchange(True)
    assert model.grad_bucket_blocks == 2
    for lo, hi in ((1, 3), (0, 1)):  # the native block stack: ranges of grad_bucket_blocks blocks
        model._grad_bucket_hook(lo, hi, ga[lo:hi], gb[lo:hi])
    step._finish_exchange()
    assert step.buckets_issued == 2 and par.slices == [(t.data_ptr(), t.numel()) for lo, hi in ((1, 3), (0, 1)) for t in (ga[lo:hi], gb[lo:hi])]
    assert model._grad_bucket_hook is None and all(blk._grad_hook is None for blk in model.transformer_blocks)
    step._begin_exchange(True)
    for i in reversed(range(3)):  # the per-block composition: one bucket per block
        model.transformer_blocks[i]._grad_hook(ga[i], gb[i])
    step._finish_exchange()
    assert step.buckets_issued == 3 and len(par.slices) == 4 + 6


# ---- a backward that raises after its first bucket, on two gloo ranks ------------------------------------------------------------------------------
class _Block:
    _grad_hook = None


def _bare_step(par):
    """The shared wrapper with nothing of a model family: four blocks of 6 gradient elements each in buckets of 2."""
    from finetrainers_amd.lora_step import FlatLoRAStep

    class Bare(FlatLoRAStep):
        def __init__(self):
            self.blocks, self.grad_bucket_blocks = [_Block() for _ in range(4)], 2
            self.flat, self.gflat = torch.zeros(24), torch.zeros(24)
            self._spans = {id(b): (6 * i, 6 * i + 6) for i, b in enumerate(self.blocks)}
            self._init_exchange(par, self.flat, self.gflat)

        def _install_hooks(self, reducer):
            for b in self.blocks:
                b._grad_hook = None if reducer is None else self._block_done

        def _clear_hooks(self):
            for b in self.blocks:
                b._grad_hook = None

    step = Bare()
    return step, step.blocks, lambda: True


def _wan_step(par):
    from finetrainers_amd.wan import MI355XWanLoRAStep, MI355XWanTransformer3DModel, WanTransformerConfig

    model = MI355XWanTransformer3DModel(WanTransformerConfig(num_layers=4, **SMALL_WAN), device=torch.device("cpu"))
    model.add_adapter(32, 32.0)
    return MI355XWanLoRAStep(model, parallel=par, grad_bucket_blocks=2), list(model.blocks), lambda: model._patch_grad_hook is None


def _hunyuan_step(par):
    from finetrainers_amd.hunyuan_video import MI355XHunyuanVideoSFTStep

    model, blocks = _hunyuan_model(2, 2)
    return MI355XHunyuanVideoSFTStep(model, parallel=par, grad_bucket_blocks=2), blocks, lambda: True


def _fail_then_clean(rank, step, blocks, other_hooks_cleared, per_bucket=2):
    """-> None, or what went wrong.  Four blocks in buckets of two; block i's gradient is (rank + 1)(i + 1) on every element: the mean over the two ranks is 1.5 (i + 1), exactly."""
    red, gflat, spans = step.reducer, step.gflat, [step._spans[id(b)] for b in blocks]
    n_buckets = -(-len(blocks) // per_bucket)

    def backward(fail):
        for k, i in enumerate(reversed(range(len(blocks)))):
            gflat[spans[i][0]:spans[i][1]] = float(rank + 1) * (i + 1)
            blocks[i]._grad_hook(blocks[i])
            if fail and k + 1 == per_bucket + 1:  # the first bucket is on the wire, one more block is ready but not issued
                raise RuntimeError("backward failed")
        return "done"

    def value(i):
        return gflat[spans[i][0]:spans[i][1]]

    gflat.zero_()
    try:
        step._backward_exchanging(lambda: backward(True), True)
        return "the failure did not propagate"
    except RuntimeError as e:
        if str(e) != "backward failed":
            raise
    if red._pending or red._ready or step._exchange is not None:
        return f"after the failure: pending {red._pending} ready {red._ready} exchange {step._exchange}"
    if not (all(b._grad_hook is None for b in blocks) and other_hooks_cleared()):
        return "after the failure: hooks are still installed"
    issued = list(reversed(range(len(blocks))))[:per_bucket]
    if red.bucket_log != [(spans[issued[-1]][0], spans[issued[0]][1])]:
        return f"after the failure: bucket log {red.bucket_log}"
    for i in range(len(blocks)):  # the slice that went out was averaged exactly once; nothing else was touched
        want = 1.5 * (i + 1) if i in issued else (float(rank + 1) * (i + 1) if i == issued[-1] - 1 else 0.0)
        if not torch.equal(value(i), torch.full_like(value(i), want)):
            return f"after the failure: block {i} holds {value(i)[0].item()}, not {want}"
    for attempt in range(2):  # a clean exchange on the same object, twice: the full schedule, every element averaged exactly once
        gflat.zero_()
        if step._backward_exchanging(lambda: backward(False), True) != "done":
            return "the wrapper lost the backward's return value"
        log = red.bucket_log
        if len(log) != n_buckets or step.buckets_issued != n_buckets or red._pending or red._ready:
            return f"clean exchange {attempt}: log {log} buckets {step.buckets_issued} pending {red._pending} ready {red._ready}"
        if not (log[0][1] == gflat.numel() and log[-1][0] == 0 and all(log[j][0] == log[j + 1][1] for j in range(len(log) - 1))):
            return f"clean exchange {attempt}: the buckets {log} do not cover the buffer once"
        for i in range(len(blocks)):
            if not torch.equal(value(i), torch.full_like(value(i), 1.5 * (i + 1))):
                return f"clean exchange {attempt}: block {i} holds {value(i)[0].item()}, not {1.5 * (i + 1)}"
        if not (all(b._grad_hook is None for b in blocks) and other_hooks_cleared()):
            return f"clean exchange {attempt}: hooks are still installed"
    return None


def _failure_worker(rank, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from finetrainers_amd.parallel import DataParallelBackend

    par = DataParallelBackend(backend="gloo", device=torch.device("cpu"))
    try:
        out = {}
        for name, make in (("wrapper", _bare_step), ("wan", _wan_step), ("hunyuan", _hunyuan_step)):
            torch.manual_seed(100 + rank)
            step, blocks, other_hooks_cleared = make(par)
            out[name] = _fail_then_clean(rank, step, blocks, other_hooks_cleared)
        q.put((rank, out))
    finally:
        par.destroy()


def test_a_backward_that_raises_after_the_first_bucket_world2_gloo():
    """No pending handles, no ready spans and no installed hooks on either rank; the slice already issued has been averaged exactly once; the following clean
    exchanges on the same object issue the full schedule and average every element exactly once (gloo: SUM + one divide)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29650 + os.getpid() % 97
    procs = [ctx.Process(target=_failure_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(r, {"wrapper": None, "wan": None, "hunyuan": None}) for r in range(2)]
