"""-m gpu: the whole-network step for three-hidden-layer MLP VAEs at small batch (csrc/fused_mlp3.hip: the chain kernel, then
gradients + tail + Adam) -- the shapes of sphere_vae_padding_expts.sh -- against the float64 oracle leaf by leaf, against the
layer-by-layer kernels on the same inputs, through vaek_train_step_gen, a captured graph, trainer.GraphLoop and run.py; and the
fence around the predicate (neighbouring shapes stay on the layer-by-layer kernels and still match the oracle).  Tolerances are
those of tests/test_gpu_parity.py / test_gpu_mlp1.py; every input is proven kink-free by tests/test_mlp3_inputs.py."""
import os

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests.gpu_util import dev, engine_for, host, random_problem, rel_err
from tests.mlp3_cases import CASES, FENCE, MAX_BATCH, case_id, sphere

pytestmark = pytest.mark.gpu

LAYER_LABELS = ("gemm", "elbo", "finalize", "bulk_finalize")


def _grads(eng, cfg, p, x, z1, z2):
    grads = eng.new_flat(eng.grad_len)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.profile_begin(64)
    params = dev(O.flatten(cfg, p))
    before = params.clone()
    eng.grads_only(params, grads, step, dev(x), dev(z1), dev(z2))
    torch.cuda.synchronize()
    assert int(step) == 1 and torch.equal(params, before)          # gradients only: the parameters are untouched
    return host(grads), eng.profile_report()


def _check_against_oracle(eng, cfg, got, loss, g, terms=None):
    print(f"loss rel err {abs(got[eng.P] - loss) / abs(loss):.3g}")
    assert abs(got[eng.P] - loss) <= 1e-5 * abs(loss), (got[eng.P], loss)
    want = O.flatten(cfg, g)
    print(f"flat gradient rel err {rel_err(got[:eng.P], want):.3g}")
    assert rel_err(got[:eng.P], want) <= 2e-5
    if terms is not None:            # grads[P + 1], [P + 2]: mean Dkl, mean mse (bounds of tests/test_gpu_parity.py: relative to the loss)
        assert abs(got[eng.P + 1] - terms[0]) <= 1e-5 * abs(loss) and abs(got[eng.P + 2] - terms[1]) <= 1e-5 * abs(loss), (got[eng.P:], terms)
    for name, (off, shape) in eng.leaves.items():
        n = int(np.prod(shape))
        err = np.max(np.abs(got[off:off + n] - want[off:off + n])) / (np.max(np.abs(want[off:off + n])) + 1e-30)
        assert err <= 1e-4, (name, err)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mlp3_every_gradient_leaf_matches_the_oracle(case):
    cfg, dk, B, seed, kw = case
    p, x, z1, z2 = random_problem(cfg, dk, B, seed=seed)
    loss, g = O.loss_and_grad(cfg, p, x, z1, z2)
    eng = engine_for(cfg, B, **kw)
    assert eng.fused and eng.step_path == "mlp3"
    got, rep = _grads(eng, cfg, p, x, z1, z2)
    assert any(k.startswith("fused_mlp3_") for k in rep) and len(rep) <= 3, sorted(rep)
    assert not any(k.startswith(LAYER_LABELS) for k in rep), sorted(rep)
    _check_against_oracle(eng, cfg, got, loss, g, O.loss_eval(cfg, p, x, z1, z2)[1:3])
    assert got[eng.P + 3] == 0.0
    # and the layer-by-layer kernels on the same inputs
    gen_eng = engine_for(cfg, B, force_generic=True)
    assert gen_eng.step_path == "layers" and not gen_eng.fused
    gen, rep2 = _grads(gen_eng, cfg, p, x, z1, z2)
    assert not any(k.startswith("fused_mlp3_") for k in rep2)
    assert rel_err(got[:eng.P], gen[:eng.P]) <= 2e-5 and np.max(np.abs(got[eng.P:eng.P + 3] - gen[eng.P:eng.P + 3])) <= 2e-5 * abs(loss)


def test_mlp3_train_steps_follow_the_oracle_and_are_repeatable():
    cfg, dk = sphere(3, 3, 6)
    B, lr = 100, 1e-4
    p, x, z1, z2 = random_problem(cfg, dk, B)
    eng = engine_for(cfg, B)
    assert eng.step_path == "mlp3"
    runs = []
    for _ in range(2):
        params = dev(O.flatten(cfg, p)); grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
        step = torch.zeros(1, dtype=torch.int32, device="cuda")
        q, st = dict(p), O.adam_init(p)
        for k in range(3):
            q, st, loss = O.train_step(cfg, q, st, x, z1, z2, lr)
            eng.train_step(params, grads, m, v, step, dev(x), dev(z1), dev(z2), lr)
            assert abs(float(grads[eng.P]) - loss) <= 1e-5 * abs(loss), (k, float(grads[eng.P]), loss)
        assert int(step) == 3
        assert np.max(np.abs(host(params) - O.flatten(cfg, q))) <= 0.02 * lr * 3
        wm = O.flatten(cfg, st["m"])
        assert np.max(np.abs(host(m) - wm)) <= 5e-5 * np.max(np.abs(wm))
        runs.append((params.clone(), grads.clone(), m.clone(), v.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))            # fixed summation order everywhere: bitwise


def test_mlp3_shards_sum_to_the_full_batch():
    """data parallel: two half-batch contexts dividing by the GLOBAL batch sum to the full-batch gradient."""
    cfg, dk = sphere(3, 3, 6)
    B = 100
    p, x, z1, z2 = random_problem(cfg, dk, B)
    full, _ = _grads(engine_for(cfg, B), cfg, p, x, z1, z2)
    parts = []
    for r in range(2):
        sl = slice(r * B // 2, (r + 1) * B // 2)
        e = engine_for(cfg, B // 2, world=2, rank=r, global_batch=B)
        assert e.fused and e.step_path == "mlp3"
        parts.append(_grads(e, cfg, p, x[sl], z1[sl], z2[sl])[0])
    tot = parts[0] + parts[1]
    assert rel_err(tot[:e.P], full[:e.P]) <= 2e-6
    assert abs(tot[e.P] - full[e.P]) <= 2e-6 * abs(full[e.P])


def test_mlp3_bucketed_gradients_are_one_bucket_with_the_same_bits():
    cfg, dk = sphere(3, 13, 8)
    B = 100
    p, x, z1, z2 = random_problem(cfg, dk, B)
    eng = engine_for(cfg, B)
    assert eng.step_path == "mlp3" and eng.buckets() == [(0, eng.grad_len)]
    want, _ = _grads(eng, cfg, p, x, z1, z2)
    grads = eng.new_flat(eng.grad_len)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event()]
    ev[0].record()                   # created on this device
    eng.grads_bucketed(dev(O.flatten(cfg, p)), grads, step, dev(x), dev(z1), dev(z2), ev)
    ev[0].synchronize()
    assert np.array_equal(host(grads), want) and int(step) == 1


def test_mlp3_train_step_gen_is_make_batch_plus_train_step_also_from_a_graph():
    """vaek_train_step_gen (the next batch drawn by spare workgroups of the second launch) == vaek_make_batch + vaek_train_step,
    bit for bit, over five steps; the same five calls captured into a graph and replayed give the same bits again."""
    from vae_training_amd.engine import Engine
    B, D, L, dd, pad, k = 100, 6, 6, 3, 3, 2
    A = torch.randn(3, device="cuda")
    eng = Engine(B, D, L, (200, 200, 200), (200, 200, 200), -1.0, True, False)
    assert eng.fused and eng.step_path == "mlp3"
    torch.manual_seed(0)
    p0 = torch.randn(eng.P, device="cuda") * 0.1

    def state():
        return [p0.clone(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(), torch.zeros(1, dtype=torch.int32, device="cuda")]
    seed, var = 77, 0.25
    rings = [torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(3)]       # the loss of step t lands in ring[t - 1]
    sa = state()
    eng.set_loss_history(rings[0])
    for n in range(5):
        x, z1, z2 = eng.make_batch(k, A, dd, 3, pad, var, B, seed, step=n, tag=1, row0=10)
        eng.train_step(*sa, x, z1, z2, 1e-3)
        assert float(rings[0][n]) == float(sa[1][eng.P])

    def gen_steps(s, bufs, counter):
        for n in range(5):
            eng.train_step_gen(*s, bufs[n % 2], 1e-3, k, A, dd, 3, pad, var, bufs[(n + 1) % 2], seed, counter, (n + 1) % 2, tag=1, row0=10)

    sb = state()
    counter = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    bufs = [eng.make_batch(k, A, dd, 3, pad, var, B, seed, counter=counter, which=0, tag=1, row0=10),
            tuple(torch.empty_like(t) for t in (x, z1, z2))]
    eng.set_loss_history(rings[1])
    eng.profile_begin(64)
    gen_steps(sb, bufs, counter)
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert set(rep) == {"fused_mlp3_chain", "fused_mlp3_grads_adam_gen"} and all(r["count"] == 5 for r in rep.values()), rep
    assert counter.tolist() == [6, 5] and int(sb[4]) == 5
    assert torch.equal(rings[0], rings[1]) and bool(torch.isfinite(rings[0][:5]).all()) and float(rings[0][4]) != 0.0
    for ta, tb in zip(sa[:4], sb[:4]):
        assert torch.equal(ta, tb)
    # the same five calls from a captured graph: nothing allocated, nothing read back, no host state per step
    sc = state()
    counter_c = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    bufs_c = [eng.make_batch(k, A, dd, 3, pad, var, B, seed, counter=counter_c, which=0, tag=1, row0=10),
              tuple(torch.empty_like(t) for t in (x, z1, z2))]
    keep = [t.clone() for t in sc] + [counter_c.clone()] + [t.clone() for t in bufs_c[0]]
    eng.set_loss_history(rings[2])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            gen_steps(sc, bufs_c, counter_c)
    torch.cuda.current_stream().wait_stream(side)
    for t, k0 in zip(sc + [counter_c] + list(bufs_c[0]), keep):      # capture does not execute; start from the initial state anyway
        t.copy_(k0)
    g.replay()
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert counter_c.tolist() == [6, 5] and int(sc[4]) == 5 and torch.equal(rings[0], rings[2])
    for ta, tc in zip(sa[:4], sc[:4]):
        assert torch.equal(ta, tc)


def _sphere_model(tmp_path, name, B=100):
    """line 1 of sphere_vae_padding_expts.sh as run.py builds it"""
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([name, "--dataset", "sphere", "--padding_dim", "3", "-dd", "3"])
    ds = get_dataset("sphere", args.dataset_seed, 3, B, args)
    return VAEModel(dirname=str(tmp_path), num_batches=10, num_epochs=1, batch_size=B, learning_rate=args.learning_rate,
                    layer_sizes="200|200|200", encoder_layer_sizes="200|200|200", state_dict=None, data_fn=None, epsilon=-3.0,
                    tqdm=False, dataset=ds, latent_dimension=6, tunable_decoder_var=True, dataset_name="sphere", fast_loop=True)


def test_mlp3_graph_loop_trains_and_is_repeatable(tmp_path):
    from vae_training_amd.trainer import GraphLoop
    out = []
    for name in ("a", "b"):
        m = _sphere_model(tmp_path, name)
        loop = GraphLoop(m, seed=9)
        assert loop.eng.step_path == "mlp3" and loop.pipeline and not loop.moments
        loop.run(400)
        torch.cuda.synchronize()
        assert loop.graph is not None and m.optimizer.state.step == 400 == int(m.optimizer.state.step_dev.item())
        out.append((loop.losses().clone(), m.model.flat.clone()))
    losses = out[0][0].double()
    assert losses.numel() == 400 and bool(torch.isfinite(losses).all())
    assert float(losses[-20:].mean()) < float(losses[:20].mean())
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("case", FENCE, ids=case_id)
def test_mlp3_fence_neighbours_stay_layer_by_layer_and_match_the_oracle(case):
    cfg, dk, B, seed, kw = case
    p, x, z1, z2 = random_problem(cfg, dk, B, seed=seed)
    loss, g = O.loss_and_grad(cfg, p, x, z1, z2)
    eng = engine_for(cfg, B, **kw)
    assert eng.step_path == "layers" and not eng.fused
    got, rep = _grads(eng, cfg, p, x, z1, z2)
    assert not any(k.startswith("fused_mlp3_") for k in rep), sorted(rep)
    _check_against_oracle(eng, cfg, got, loss, g)


def test_mlp3_bf16_stays_layer_by_layer():
    cfg, _ = sphere(3, 3, 6, (192, 192, 192))
    assert engine_for(cfg, 100, dtype="bf16").step_path == "layers"
    assert engine_for(cfg, 100).step_path == "mlp3"
    assert engine_for(sphere(3, 3, 6)[0], MAX_BATCH).step_path == "mlp3"


def test_step_path_names_the_other_forms():
    from vae_training_amd.engine import Engine
    assert Engine(512, 12, 20).step_path == "linear"
    assert Engine(300, 7, 6, (64,), (64,), -3.0, True, True).step_path == "mlp1"
    assert Engine(256, 4096, 16).step_path == "linear_wide"
    assert Engine(128, 6, 6, (40, 40, 40), (40, 40, 40)).step_path == "layers"


def test_run_py_on_the_sphere_script_line(tmp_path, monkeypatch, capsys):
    """`python run.py sphere_dd3_pd3_ld_6_eps-3 ...` (line 1 of the script, 300 batches) with --fast_loop: the graph loop on the new kernels."""
    from vae_training_amd import run, utils
    from vae_training_amd.trainer import GraphLoop
    monkeypatch.setattr(utils, "DATA_DIR", str(tmp_path) + "/")
    made = []
    orig = GraphLoop.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(GraphLoop, "__init__", spy)
    line = ["sphere_dd3_pd3_ld_6_eps-3", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes", "200|200|200", "-ow",
            "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--num_batches", "300", "--epsilon", "-3", "-tdv"]
    assert run.main(run.parse_arguments(line + ["--fast_loop"])) == 0
    out = capsys.readouterr().out
    assert "Train step: mlp3 kernels" in out, out[:2000]
    assert len(made) == 1 and made[0].eng.step_path == "mlp3" and made[0].pipeline
    z = np.load(os.path.join(str(tmp_path), "sphere_dd3_pd3_ld_6_eps-3", "losses.npz"), allow_pickle=True)
    losses = np.asarray(z["VAE Loss"], dtype=np.float64)
    assert losses.size >= 300 and np.isfinite(losses).all()
    # without the flag the reference's own loop (one library call per step) runs on the same kernels
    assert run.main(run.parse_arguments(line)) == 0
    assert "Train step: mlp3 kernels" in capsys.readouterr().out and len(made) == 1
