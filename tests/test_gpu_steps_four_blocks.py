"""-m gpu: the persistent form of vaek_train_steps and its in-launch draw for linear VAEs of 49 .. 64 features (four 16-feature
blocks: the D = 20 rows of seed_linpadding_expts.sh, L <= 32) -- routing, the float64 oracle at the script's shapes, agreement
with the launch-per-step form, the in-launch draw bit for bit, hipGraph capture, data parallelism over the P2P communicator,
and run.py's default loop."""
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests.gpu_util import dev, engine_for, host
from tests.test_gpu_loop import _spec
from tests.test_gpu_p2p import _free_port
from tests.test_gpu_steps import _leafwise_grads_of_the_first_step, _problem, _run_pipelined

pytestmark = pytest.mark.gpu


def _lin(D, L, tdv=True, eps=-1.0):
    return O.Config(D, L, (), (), eps, tdv, "linear_gaussian")


def _labels(eng, call):
    eng.profile_begin(256)
    call()
    torch.cuda.synchronize()
    return set(eng.profile_report())


@pytest.mark.parametrize("D,L", [(20, 20), (20, 10), (16, 20), (24, 15), (31, 1)])
def test_four_block_shapes_take_the_persistent_form(D, L):
    cfg = _lin(D, L)
    B = 1000
    eng = engine_for(cfg, B)
    assert L + 2 * D + 1 > 48 and eng.supports_train_steps()
    assert eng.supports_train_steps_gen(0) and eng.supports_train_steps_gen(2)
    p, batches = _problem(cfg, dict(name="linear_gaussian", seed=2, dd=3, did=3, pad=D - 3), B, 2)
    params = dev(O.flatten(cfg, p)); grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    seen = _labels(eng, lambda: eng.train_steps(params, grads, m, v, step, [tuple(dev(a) for a in b) for b in batches], 1e-3))
    assert "lin_moments_persistent" in seen and "lin_moments_step" not in seen, sorted(seen)
    assert not eng.train_steps_gave_up() and int(step.item()) == 2


def test_shapes_past_the_four_block_updater_stay_where_they_were():
    assert not engine_for(_lin(22, 20), 64).supports_train_steps_gen(0)          # 65 features: no moment form at all
    # L > 32: launch-per-step form only -- its streamers and its updater are held to the float64 reference at (10, 40) and (1, 61) by
    # tests/test_gpu_lin_moments.py (test_stream_and_reduce, test_launch_per_step_updater)
    eng = engine_for(_lin(10, 40), 256)
    assert eng.supports_train_steps() and not eng.supports_train_steps_gen(0) and not eng.supports_train_steps_gen(2)


@pytest.mark.parametrize("L,tdv", [(20, True), (10, False)])
def test_script_shapes_against_the_oracle(L, tdv):
    """D = 20 (seed_linpadding_expts.sh: -dd 3 --padding_dim 17) at the metric's batch, four steps against the float64 oracle."""
    cfg = O.Config(20, L, (), (), -1.0, tdv, "linear_gaussian")
    B, n, lr = 65536, 4, 1e-3
    p, batches = _problem(cfg, dict(name="linear_gaussian", seed=2, dd=3, did=3, pad=17), B, n)
    eng = engine_for(cfg, B)
    assert eng.supports_train_steps_gen(0)
    _leafwise_grads_of_the_first_step(cfg, eng, p, batches[0], lr)
    params, grads, m, v, step, losses = _run_pipelined(eng, cfg, p, batches, lr)
    st = O.adam_init(p)
    for i, (x, z1, z2) in enumerate(batches):
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, lr)
        assert abs(losses[i] - loss) <= 1e-5 * abs(loss), (i, losses[i], loss)
    assert step == n
    assert np.max(np.abs(host(params) - O.flatten(cfg, p))) <= 0.02 * lr * n


def test_persistent_and_launch_per_step_forms_agree_at_D20(monkeypatch):
    """70 steps at B = 3000 (two full persistent launches and a short one) in each form, each in a subprocess (the choice is read
    once per process): the bounds of test_gpu_steps.test_persistent_and_launch_per_step_forms_agree."""
    import json, subprocess, sys
    code = r"""
import sys, json, numpy as np, torch
sys.path.insert(0, %r)
from oracle import elbo_oracle as O
from tests.gpu_util import engine_for
from tests.test_gpu_steps import _problem, _run_pipelined
cfg = O.Config(20, 20, (), (), -1.0, True, "linear_gaussian")
p, batches = _problem(cfg, dict(name="linear_gaussian", seed=2, dd=3, did=3, pad=17), 3000, 70)
eng = engine_for(cfg, 3000)
params, grads, m, v, step, losses = _run_pipelined(eng, cfg, p, batches, 1e-3)
print(json.dumps({"p": params.cpu().numpy().astype(np.float64).tolist(), "m": m.cpu().numpy().astype(np.float64).tolist(), "l": np.asarray(losses, np.float64).tolist()}))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for persist in ("1", "0"):
        env = dict(os.environ, VAEK_LIN_PERSIST=persist)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append({k: np.asarray(v) for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()})
    a, b = outs
    assert np.max(np.abs(a["l"] - b["l"]) / np.abs(b["l"])) <= 2e-6
    assert np.max(np.abs(a["p"] - b["p"])) <= 2e-6
    assert np.max(np.abs(a["m"] - b["m"])) <= 1e-5 * np.max(np.abs(b["m"]))


@pytest.mark.parametrize("kind,D,L,dd,pad,B,n", [
    (0, 20, 20, 3, 17, 65536, 3),           # M20: its compile-time instantiation
    (0, 20, 10, 9, 11, 100, 70),            # run.py's batch, two persistent launches
    (2, 21, 16, 5, 16, 300, 4),             # sphere dataset
    (0, 19, 13, 4, 15, 1001, 3),            # odd D, ragged batch
])
def test_in_launch_draw_equals_make_batch_plus_train_steps_four_blocks(kind, D, L, dd, pad, B, n):
    from vae_training_amd.engine import Engine
    eng = Engine(B, D, L, (), (), -1.0, True, False)
    assert eng.supports_train_steps_gen(kind)
    A = _spec(kind, dd, dd)
    torch.manual_seed(0)
    p0 = (torch.randn(eng.P, device="cuda") * 0.3).contiguous()
    seed, tag, row0 = 77, 5, 1000

    def state():
        return [p0.clone(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(), torch.zeros(1, dtype=torch.int32, device="cuda")]
    a, b = state(), state()
    ring_a = torch.zeros(n + 4, dtype=torch.float32, device="cuda"); ring_b = torch.zeros_like(ring_a)
    eng.set_loss_history(ring_a)
    eng.train_steps_gen(*a, n, 1e-3, kind, A, dd, dd, pad, 0.0, seed, tag=tag, row0=row0)
    torch.cuda.synchronize()
    assert not eng.train_steps_gave_up()
    batches = [eng.make_batch(kind, A, dd, dd, pad, 0.0, B, seed, step=t, tag=tag, row0=row0) for t in range(n)]
    eng.set_loss_history(ring_b)
    eng.train_steps(*b, batches, 1e-3)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up()
    assert int(a[4].item()) == n == int(b[4].item())
    for x, y, what in zip(a[:4], b[:4], ("params", "grads", "m", "v")):
        assert torch.equal(x, y), what
    assert torch.equal(ring_a[:n], ring_b[:n]) and bool(torch.isfinite(ring_a[:n]).all())


def test_graph_replay_at_D20_equals_the_eager_call():
    cfg = _lin(20, 20)
    B, n, lr = 20000, 70, 1e-3
    p, batches = _problem(cfg, dict(name="linear_gaussian", seed=2, dd=3, did=3, pad=17), B, 5)
    dbat = [tuple(dev(a) for a in b) for b in batches]
    seq = [dbat[i % len(dbat)] for i in range(n)]
    eng = engine_for(cfg, B)

    def fresh():
        return (dev(O.flatten(cfg, p)), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(),
                torch.zeros(1, dtype=torch.int32, device="cuda"))
    pe, ge, me, ve, se = fresh()
    eng.train_steps(pe, ge, me, ve, se, seq, lr)
    torch.cuda.synchronize()
    assert not eng.train_steps_gave_up()
    pg, gg, mg, vg, sg = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.train_steps(pg, gg, mg, vg, sg, seq, lr)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert not eng.train_steps_gave_up()
    assert int(sg.item()) == int(se.item()) == n
    assert torch.equal(pg, pe) and torch.equal(mg, me) and torch.equal(vg, ve) and torch.equal(gg, ge)


@pytest.mark.parametrize("seed", range(8))
def test_random_four_block_shapes(seed):
    rng = np.random.default_rng(4000 + seed)
    while True:
        D, L = int(rng.integers(1, 32)), int(rng.integers(1, 33))
        if 49 <= L + 2 * D + 1 <= 64:
            break
    B = [7, 100, 191, 193, 4097, 70001, 1000, 2500][seed]
    if B * min(D, L) < 8:
        B = 8
    tdv = bool(rng.integers(0, 2))
    cfg = _lin(D, L, tdv, float(rng.uniform(-3.0, 0.5)))
    r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    p = {k: r32(v) for k, v in O.init_params(cfg, seed=seed).items()}
    for k in p:
        if not k.endswith("kernel"):
            p[k] = r32(p[k] + 0.2 * rng.standard_normal(p[k].shape))
    n, lr = 3, 1e-3
    A = rng.standard_normal((D, D)) / np.sqrt(D)
    batches = [(r32(rng.standard_normal((B, D)) @ A), r32(rng.standard_normal((B, L))), r32(rng.standard_normal((B, D)))) for _ in range(n)]
    eng = engine_for(cfg, B)
    assert eng.supports_train_steps_gen(0), (D, L, B)
    params = dev(O.flatten(cfg, p)); grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ring = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    eng.set_loss_history(ring)
    seen = _labels(eng, lambda: eng.train_steps(params, grads, m, v, step, [tuple(dev(a) for a in b) for b in batches], lr))
    eng.set_loss_history(None)
    assert "lin_moments_persistent" in seen and "lin_moments_step" not in seen, sorted(seen)
    assert not eng.train_steps_gave_up() and int(step.item()) == n
    losses = host(ring)[:n]
    st = O.adam_init(p)
    for i, (x, z1, z2) in enumerate(batches):
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, lr)
        assert abs(losses[i] - loss) <= 1e-5 * abs(loss) + 1e-6, (D, L, B, tdv, i, losses[i], loss)
    assert np.max(np.abs(host(params) - O.flatten(cfg, p))) <= 0.02 * lr * n, (D, L, B, tdv)


def _dp_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from vae_training_amd.engine import Engine
        from vae_training_amd.parallel import GradExchange, shard_rows
        D, L = 20, 20
        cfg = _lin(D, L)
        B, lr, steps = 1536, 1e-3, 7
        rng = np.random.default_rng(0)
        r32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
        p = {k: r32(v) for k, v in O.init_params(cfg, seed=0).items()}
        lo, hi = shard_rows(B, world, rank)
        eng = Engine(hi - lo, D, L, (), (), -1.0, True, False, world=world, rank=rank, global_batch=B)
        ex = GradExchange(eng, dist, mode="p2p")
        assert ex.in_library and eng.supports_train_steps()
        params = dev(O.flatten(cfg, p)); grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
        step = torch.zeros(1, dtype=torch.int32, device="cuda")
        ring = torch.zeros(steps + 4, dtype=torch.float32, device="cuda")
        eng.set_loss_history(ring)
        st, want, batches = O.adam_init(p), [], []
        for s in range(steps):
            x = r32(rng.standard_normal((B, D)))
            z1, z2 = O.split_latents(r32(rng.standard_normal((B, L + D))), L)
            p, st, loss_ref = O.train_step(cfg, p, st, x, z1, z2, lr)
            want.append(loss_ref)
            batches.append((dev(x[lo:hi]), dev(z1[lo:hi]), dev(z2[lo:hi])))
        seen = _labels(eng, lambda: (eng.train_steps(params, grads, m, v, step, batches[:4], lr),
                                     eng.train_steps(params, grads, m, v, step, batches[4:], lr)))
        got = ring.cpu().numpy()[:steps].astype(np.float64)
        worst = float(np.max(np.abs(got - np.array(want)) / np.abs(want)))
        digest = torch.tensor(params.cpu().numpy().view(np.int32).astype(np.int64).sum().reshape(1))
        allg = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(allg, digest)
        bad = eng.train_steps_gave_up() or int(step.item()) != steps or ex.timed_out() or "lin_moments_persistent" not in seen
        q.put((rank, worst, all(int(a) == int(allg[0]) for a in allg), bad, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, 1.0, False, True, traceback.format_exc()))


def test_data_parallel_four_blocks_over_the_p2p_communicator():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, lerr, same, bad, tb in res:
        assert tb is None, tb
        assert lerr <= 1e-5 and same and not bad, (rank, lerr, same, bad)


def test_run_py_default_loop_at_D20(tmp_path, monkeypatch, capsys):
    """A D = 20 line of seed_linpadding_expts.sh with no loop flag: the moment loop (GraphLoop(moments=True)) by itself, and the
    same losses as the per-sample fast loop from the same seeds."""
    from vae_training_amd import run, utils
    from vae_training_amd.trainer import GraphLoop
    monkeypatch.setattr(utils, "DATA_DIR", str(tmp_path) + "/")
    made = []
    orig = GraphLoop.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(GraphLoop, "__init__", spy)
    base = ["--dataset", "linear_gaussian", "--encoder_layer_sizes", "", "--layer_sizes", "", "-ow", "--latent_dim", "20", "--padding_dim", "17",
            "-dd", "3", "--num_batches", "40", "--batch_size", "512", "--epsilon", "-1", "-tdv", "-ds", "2", "-lr", "1e-3"]
    assert run.main(run.parse_arguments(["auto"] + base)) == 0
    capsys.readouterr()
    assert len(made) == 1 and made[0].moments
    z = np.load(os.path.join(str(tmp_path), "auto", "losses.npz"), allow_pickle=True)
    fast = np.asarray(z["VAE Loss"], dtype=np.float64)
    monkeypatch.setattr(GraphLoop, "__init__", lambda self, *a, **kw: (orig(self, *a, **dict(kw, moments=False)), made.append(self))[0])
    assert run.main(run.parse_arguments(["slow"] + base + ["--fast_loop"])) == 0
    capsys.readouterr()
    assert len(made) == 2 and not made[1].moments
    z2 = np.load(os.path.join(str(tmp_path), "slow", "losses.npz"), allow_pickle=True)
    slow = np.asarray(z2["VAE Loss"], dtype=np.float64)
    assert fast.shape == slow.shape and fast.size >= 40 and np.isfinite(fast).all()
    assert np.max(np.abs(fast - slow) / np.abs(slow)) <= 1e-5
