"""-m gpu: the launches of ONE vaek_train_steps / vaek_train_steps_gen call of more than 64 steps are chained -- a launch leaves
its last batch to the next launch's reducers and its last two to the next launch's updater, batch n of a call lives in workspace
slot n % 66 (csrc/linear_moments.hip: lin_windows) -- which changes WHEN a batch is reduced and updated, never what is computed.
A call of <= 64 steps is one launch whose three roles take the same batches, as before.  So one call of n steps must end BITWISE
where the same batches end when they are given as consecutive calls of <= 64 steps: parameters, Adam moments, the gradient buffer
with its loss slots, the step counter, the loss ring."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

CHUNK = 50                                            # the unchained side: calls of at most this many steps (one launch each)
LONG = [65, 66, 128, 130, 200]
SHAPES = [(12, 20, 3000),                             # three feature blocks, 12 tiles of 256 rows, the last one ragged
          (20, 20, 3000)]                             # four blocks (D = L = 20: tiles of 192 rows, the last one ragged)


def _engine(D, L, B, **kw):
    from vae_training_amd.engine import Engine
    return Engine(B, D, L, (), (), -1.0, True, False, **kw)


def _batches(D, L, B, n, distinct=7, seed=3):
    """n batches out of `distinct` different ones (a long call walks them round: the order is what the slots must keep)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mix = torch.randn(D, D, generator=g, device="cuda") / D ** 0.5
    pool = [((torch.randn(B, D, generator=g, device="cuda") @ mix).contiguous(), torch.randn(B, L, generator=g, device="cuda"),
             torch.randn(B, D, generator=g, device="cuda")) for _ in range(distinct)]
    return [pool[(i * 3) % distinct] for i in range(n)]


def _state(eng, ring_len, seed=0):
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    return [(torch.randn(eng.P, generator=g, device="cuda") * 0.3).contiguous(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(),
            torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(ring_len, dtype=torch.float32, device="cuda")]


def _run(eng, st, calls, lr=1e-3):
    """calls: lists of batches, one vaek_train_steps call each"""
    eng.set_loss_history(st[5])
    for batches in calls:
        eng.train_steps(*st[:5], batches, lr)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    return st


def _chunks(seq, k=CHUNK):
    return [seq[i:i + k] for i in range(0, len(seq), k)]


def _assert_same(got, want, n_total):
    assert int(got[4].item()) == int(want[4].item()) == n_total
    for a, b, what in zip(got, want, ("params", "grads and loss slots", "m", "v", "step", "loss ring")):
        assert torch.equal(a, b), what
    assert bool(torch.isfinite(got[5][:n_total]).all()) and bool((got[5][:n_total] != 0).all())


@pytest.mark.parametrize("D,L,B", SHAPES)
@pytest.mark.parametrize("n", LONG)
def test_one_long_call_equals_consecutive_short_calls(D, L, B, n):
    eng = _engine(D, L, B)
    assert eng.supports_train_steps()
    seq = _batches(D, L, B, n)
    want = _run(eng, _state(eng, n + 8), _chunks(seq))
    got = _run(eng, _state(eng, n + 8), [seq])
    _assert_same(got, want, n)


@pytest.mark.parametrize("D,L,B", SHAPES)
def test_a_second_long_call_finds_the_counters_zero(D, L, B):
    """Two long calls back to back on one workspace (the second starts in slot 0 again, on the counters the first one left), then
    a short one: the chained result every time."""
    eng = _engine(D, L, B)
    n1, n2, n3 = 130, 67, 5
    seq = _batches(D, L, B, n1 + n2 + n3)
    calls = [seq[:n1], seq[n1:n1 + n2], seq[n1 + n2:]]
    want = _run(eng, _state(eng, len(seq) + 8), _chunks(seq))
    got = _run(eng, _state(eng, len(seq) + 8), calls)
    _assert_same(got, want, len(seq))


def test_the_metric_shape_chains_its_launches():
    """B = 65 536, D = 12, L = 20: the kernel instantiation the headline number is measured on (228 tiles of 288 rows)."""
    D, L, B, n = 12, 20, 65536, 130
    eng = _engine(D, L, B)
    seq = _batches(D, L, B, n, distinct=5)
    want = _run(eng, _state(eng, n + 8), _chunks(seq, 64))
    got = _run(eng, _state(eng, n + 8), [seq])
    _assert_same(got, want, n)


@pytest.mark.parametrize("D,L,B", SHAPES)
@pytest.mark.parametrize("n", LONG)
def test_one_long_drawing_call_equals_make_batch_plus_short_calls(D, L, B, n):
    """vaek_train_steps_gen(n): the streamers of a later launch run two batches ahead of the step counter they read -- the batch
    of the step that takes the Adam counter from t to t + 1 must still be make_batch(step = t)'s, bit for bit."""
    eng = _engine(D, L, B)
    kind, dd, did, var, seed, tag, row0 = 0, 3, 3, 0.25, 77, 5, 1000
    assert eng.supports_train_steps_gen(kind)
    A = torch.randn(dd, did, generator=torch.Generator().manual_seed(11)).cuda().contiguous()
    got = _state(eng, n + 8)
    eng.set_loss_history(got[5])
    eng.train_steps_gen(*got[:5], n, 1e-3, kind, A, dd, did, D - dd, var, seed, tag=tag, row0=row0)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    seq = [eng.make_batch(kind, A, dd, did, D - dd, var, B, seed, step=t, tag=tag, row0=row0) for t in range(n)]
    want = _run(eng, _state(eng, n + 8), _chunks(seq))
    _assert_same(got, want, n)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _p2p_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from vae_training_amd.engine import Engine
        from vae_training_amd.parallel import GradExchange, shard_rows
        D, L, B, n = 12, 20, 1536, 130
        lo, hi = shard_rows(B, world, rank)
        eng = Engine(hi - lo, D, L, (), (), -1.0, True, False, world=world, rank=rank, global_batch=B)
        ex = GradExchange(eng, dist, mode="p2p")
        assert ex.in_library and eng.supports_train_steps()
        seq = [tuple(t[lo:hi].contiguous() for t in b) for b in _batches(D, L, B, n)]       # every rank draws the same global batches
        want = _run(eng, _state(eng, n + 8), _chunks(seq))
        dist.barrier()
        got = _run(eng, _state(eng, n + 8), [seq])
        same = all(torch.equal(a, b) for a, b in zip(got, want)) and int(got[4].item()) == n
        digest = torch.tensor(got[0].cpu().numpy().view(np.int32).astype(np.int64).sum().reshape(1))
        allg = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(allg, digest)
        q.put((rank, same, all(int(a) == int(allg[0]) for a in allg), ex.timed_out(), None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:            # report instead of hanging the parent
        import traceback
        q.put((rank, False, False, True, traceback.format_exc()))


def test_chained_launches_exchange_their_moments_across_ranks():
    """Two ranks rehearsed on one GPU, 130 steps in one call: the exchange epoch of a batch is its Adam step whichever launch
    reduces it -- replicas end bitwise equal, and equal to the same steps given 50 at a time."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_p2p_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, same, replicas_equal, timed_out, tb in res:
        assert tb is None, tb
        assert same and replicas_equal and not timed_out, (rank, same, replicas_equal, timed_out)
