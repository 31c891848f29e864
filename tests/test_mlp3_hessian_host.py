"""The MLP sampled-ELBO Hessian (csrc/mlp3_hessian.hip) from the host, no GPU: the float64 restatement tools/mlp3_hessian_reference.py
against torch autograd of an independent statement of f_K and against the oracle the training kernels are held to, both under the bound
the GPU tests use; trainer.ReplicaSampledElboHessianMlp3, the table row, run.py's flags, refusals and banners on a stub engine; the
constants, the workspace formula and the description guards of the two entry points."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import mlp3_hessian_cases as K
from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["Sampled ELBO Hessian Ritz Values", "Sampled ELBO Hessian Ritz Residuals", "Sampled Sharpness", "Sampled ELBO Hessian Min Ritz",
        "Sampled ELBO Gradient Norm"]
ENTRIES = ("vaek_mlp3_sampled_elbo_hvp_replicas", "vaek_mlp3_sampled_elbo_hessian_lanczos_replicas")
NEW = {"vaek_supports_mlp3_sampled_elbo_hessian": 3, "vaek_mlp3_sampled_elbo_hessian_max_columns": 0,
       "vaek_mlp3_sampled_elbo_hessian_workspace_bytes": 5, "vaek_mlp3_sampled_elbo_hvp_replicas": 13,
       "vaek_mlp3_sampled_elbo_hessian_lanczos_replicas": 13}


# ---- 1. the restatement against torch autograd, under the bound of the GPU tests ---------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_the_restatement_matches_autograd_within_the_value_bound(case):
    name = case[0]
    m, mg = K.model(case), K.model(case, mag=True)
    V = K.directions(name)
    assert m.P == K.param_count(name) == K.ref().param_count(*K.model_args(name)[:4], K.SHAPES[name]["tdv"]) and V.shape == (3, m.P)
    assert np.count_nonzero(V[1]) == 1 and np.count_nonzero(V[2]) == K.SHAPES[name]["L"] + (1 if K.SHAPES[name]["tdv"] else 0)
    f, g, hv = K.ref().autograd(K.make_theta(name), K.make_rows(case), K.make_samples(case), *K.model_args(name), V=V)
    ratios = (K.worst_ratio(m.f() - f, K.value_bound(case, mg.f())), K.worst_ratio(m.grad() - g, K.value_bound(case, mg.grad())),
              K.worst_ratio(m.hvp(V) - hv, K.value_bound(case, mg.hvp(V))))
    print(f"{case}: |restatement - autograd| / bound: f {ratios[0]:.3e}  gradient {ratios[1]:.3e}  H v {ratios[2]:.3e}")
    assert max(ratios) <= 1.0
    assert np.all(mg.hvp(V) >= np.abs(m.hvp(V)) * (1.0 - 1e-12)) and mg.f() >= abs(m.f()) and np.all(mg.grad() >= np.abs(m.grad()) * (1.0 - 1e-12))
    assert np.linalg.norm(hv[2]) > 0 and (case[1] < 37 or np.linalg.norm(hv[1]) > 0)      # with 74 columns the unit vector's unit is live somewhere


# ---- 2. with K = 1 the gradient is the oracle's: the function is the loss the training kernels differentiate ------------------------------
@pytest.mark.parametrize("case", [c for c in K.CASES if c[2] == 1], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_with_one_sample_the_gradient_is_the_oracles(case):
    name = case[0]
    cfg = K.oracle_cfg(name)
    m, mg = K.model(case), K.model(case, mag=True)
    x, xi = K.make_rows(case), K.make_samples(case)
    loss, g = O.loss_and_grad(cfg, O.unflatten(cfg, K.make_theta(name)), x, xi[:, 0], np.zeros_like(x))
    ratios = (K.worst_ratio(m.f() - loss, K.value_bound(case, mg.f())), K.worst_ratio(m.grad() - O.flatten(cfg, g), K.value_bound(case, mg.grad())))
    print(f"{case}: |restatement - oracle| / bound: loss {ratios[0]:.3e}  gradient {ratios[1]:.3e}")
    assert max(ratios) <= 1.0


def test_the_cases_are_the_issues():
    assert {n: (s["enc"], s["dec"], s["D"], s["L"]) for n, s in K.SHAPES.items() if n != "narrow_notdv"} == {
        "narrow": ((64, 64, 64), (64, 64, 64), 7, 6), "mixed": ((64, 256, 100), (130, 72, 200), 9, 5),
        "odd": ((66, 201, 130), (66, 201, 130), 12, 20), "script1": ((200, 200, 200), (200, 200, 200), 6, 6),
        "wide": ((256, 256, 256), (256, 256, 256), 32, 32)}
    assert K.SHAPES["narrow_notdv"]["tdv"] is False and K.param_count("narrow_notdv") == K.param_count("narrow") - 1
    assert K.ROWS_K == ((1, 1), (5, 3), (37, 2), (9, 1)) and K.R == 3 and K.param_count("wide") == 296545
    assert 2 ** 32 - 1 in K.X_STEPS and 2 ** 32 - 1 in K.Z_STEPS and len(set(K.X_SEEDS)) == len(set(K.Z_SEEDS)) == 3
    assert [(c, s) for c, s in K.LANCZOS_CASES] == [(("narrow", 37, 2), 32), (("script1", 37, 1), 32), (("odd", 5, 3), 7), (("wide", 5, 1), 8)]
    big, small = ("odd", 37, 2), ("odd", 5, 3)
    assert np.array_equal(K.make_rows(big)[:5], K.make_rows(small)) and np.array_equal(K.make_samples(big)[:5], K.make_samples(small)[:, :2])
    assert K.value_bound(("script1", 37, 2), 1.0) == 64.0 * (2 * 74 + 2 * (6 + 200 + 400 + 400 + 200 + 6) + 12 + 12) * 2.0 ** -53
    # a column costs 2 sum (n_in + n_out) doubles of workspace (and 40 / 8 of its tile's partials): 39 KB at the script shape, 51 KB at the widest
    per_col = lambda name: 8 * (K.workspace_doubles(name, 16, 1) - K.workspace_doubles(name, 8, 1)) // 8
    assert per_col("script1") == 8 * (2 * 2424 + 5) == 38824 and per_col("wide") == 8 * (2 * 3200 + 5) == 51240


# ---- 4. trainer.ReplicaSampledElboHessianMlp3, the table row and run.py on a stub engine ------------------------------------------------
class _StubEngine:
    """What ReplicaSampledElboHessianMlp3 asks of an engine, on the CPU."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    elbo_hessian_max_steps = 32
    sampled_elbo_hessian_record_len = 142
    sampled_elbo_hessian_max_columns = 1 << 22
    mlp3_sampled_elbo_hessian_max_columns = 1 << 14
    step_path = "stub"

    def __init__(self, mlp3=True, linear=False, D=7, L=6, world=1, off=0.0, k=3):
        self.mlp3, self.linear, self.D, self.L, self.world, self.off, self.k = mlp3, linear, D, L, world, off, k
        self.calls, self.linear_calls, self.fills, self.ws = [], [], [], []

    def supports_mlp3_sampled_elbo_hessian(self, kind):
        return self.mlp3

    def supports_sampled_elbo_hessian(self, kind):
        return self.linear

    supports_log_likelihood = supports_sampled_elbo_hessian

    def mlp3_sampled_elbo_hessian_workspace(self, n, rows, samples):
        self.ws.append((n, rows, samples))
        return 64 * n

    def rng_fill(self, n, seed, step=0, tag=0, bits=False):
        self.fills.append((n, seed % 2 ** 64, step, tag))
        return torch.full((n,), float(step), dtype=torch.float32)

    def sampled_elbo_hessian_lanczos_replicas(self, *a, **kw):
        self.linear_calls.append(kw)

    def mlp3_sampled_elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, workspace, **kw):
        R, P = params.shape
        assert out.dtype == v0.dtype == basis.dtype == torch.float64 and out.shape == (R, 142) and workspace.dtype == torch.uint8
        assert v0.shape == (R, P) and basis.shape == (R, steps, P) and workspace.numel() == 64 * R
        self.calls.append(dict(n=R, rows=rows, steps=steps, samples=kw["samples"], x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(),
                               z_seeds=kw["z_seeds"].tolist(), z_steps=kw["z_steps"].tolist(), v0=v0.clone(), kw=kw))
        for r in range(R):
            out[r] = 1000.0 * r + torch.arange(142, dtype=torch.float64)
            out[r, 2], out[r, 5], out[r, 6] = self.k, self.off, 1.0


def _model(eng, P=4, kind=2, seed=1, B=100, key=(3, 4), dd=3, rows=1000, **flags):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, None, dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb=None: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=rows, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 _loglik_draws=4, _jacobian_draws=6, dirname="run_dir", compute_stats=lambda: {"VAE Loss": 1.0, "mse": 2.0},
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))), **flags)


def test_the_event_makes_one_call_under_its_own_counter_and_tags():
    from vae_training_amd import events
    from vae_training_amd.trainer import ReplicaSampledElboHessian, ReplicaSampledElboHessianMlp3 as Ev
    assert Ev is events.ReplicaSampledElboHessianMlp3 and issubclass(Ev, ReplicaSampledElboHessian) and list(Ev.KEYS) == KEYS
    assert (Ev.X_TAG, Ev.Z_TAG, Ev.V_TAG) == (14, 15, 16) == (K.X_TAG, K.Z_TAG, K.V_TAG) and Ev.COUNTER == "_mlp_hessian_draws"
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257), (48, (5, 2 ** 64 - 1), 65536)]
    ms = [_model(e, seed=s, key=k, B=B) for s, k, B in spec]
    hs = Ev(ms, steps=8, samples=2)
    assert hs.R == 3 and hs.rows == 1000 and hs.steps == 8 and hs.samples == 2 and hs.basis.shape == (3, 8, 4) and hs.out.shape == (3, 142)
    assert e.ws == [(3, 1000, 2)] and hs.workspace.numel() == 192
    d = Ev([_model(e)])
    assert (d.steps, d.samples) == (32, 1)                               # K = 1: the training loss's own estimator
    want_seeds = [(s ^ 2) % 2 ** 64 for s, _, _ in spec]
    for event in range(2):
        stats = hs.event_after({"mlp_log_likelihood_samples": [{}] * 3})  # what already ran does not couple
        assert len(e.calls) == event + 1 and e.linear_calls == []
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["steps"] == 8 and c["samples"] == 2 and c["kw"]["kind"] == 2 and c["kw"]["A"] is None
        assert c["kw"]["x_tag"] == 14 and c["kw"]["z_tag"] == 15
        assert [s % 2 ** 64 for s in c["x_seeds"]] == [s % 2 ** 64 for s in c["z_seeds"]] == want_seeds
        assert c["x_steps"] == c["z_steps"] == [event + 1] * 3
        assert e.fills[-3:] == [(4, s, event + 1, 16) for s in want_seeds]
        assert torch.equal(c["v0"], torch.full((3, 4), float(event + 1), dtype=torch.float64))
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):    # none of the run's state is touched
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 4 and m._jacobian_draws == 6
            assert m._mlp_hessian_draws == event + 1 and not hasattr(m, "_sampled_hessian_draws")
            assert list(st) == KEYS and all(isinstance(st[k_], float) for k_ in KEYS[2:])
            assert st[KEYS[0]].tolist() == [1000.0 * r + 12 + j for j in range(3)] and st[KEYS[1]].tolist() == [1000.0 * r + 44 + j for j in range(3)]
            assert [st[k_] for k_ in KEYS[2:]] == [1000.0 * r + 9, 1000.0 * r + 10, 1000.0 * r + 1]


def test_the_event_refusals():
    from vae_training_amd.trainer import ReplicaSampledElboHessianMlp3 as Ev
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):
        Ev([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="ReplicaSampledElboHessianMlp3: vaek_mlp3_sampled_elbo_hessian_lanczos_replicas does not cover.*three "
                                           "hidden layers.*step path: stub"):
        Ev([_model(_StubEngine(mlp3=False, linear=True))])
    with pytest.raises(RuntimeError, match="world"):
        Ev([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="-dd / -did <= 16"):
        Ev([_model(e, dd=17)])
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match="rows"):
            Ev([_model(e)], rows=rows)
    for steps in (0, 33):
        with pytest.raises(RuntimeError, match="Lanczos steps, need 1 .. 32"):
            Ev([_model(e)], steps=steps)
    for samples in (0, 1025):
        with pytest.raises(RuntimeError, match="samples per row, need 1 .. 1024"):
            Ev([_model(e)], samples=samples)
    Ev([_model(e)], samples=8)                                            # 8000 columns: the last K that fits one model of 1000 rows
    with pytest.raises(RuntimeError, match=r"1 models x 1000 rows x 9 samples = 9000 columns, at most 16384 fit one call and 8192 one model "
                                           r"\(vaek_mlp3_sampled_elbo_hessian_max_columns\)"):
        Ev([_model(e)], samples=9)                                        # rows x K above 2^13
    Ev([_model(e) for _ in range(16)])                                    # 16000 columns
    with pytest.raises(RuntimeError, match=r"17 models x 1000 rows x 1 samples = 17000 columns"):
        Ev([_model(e) for _ in range(17)])                                # models x rows x K above 2^14
    assert e.calls == [] and e.fills == []
    with pytest.raises(RuntimeError, match=r"ReplicaSampledElboHessianMlp3: model 0 \(run_dir\).*off_F"):
        Ev([_model(_StubEngine(off=2.0 ** -39))]).event()
    for k in (1, 0):
        st = Ev([_model(_StubEngine(k=k))]).event()[0]
        assert st[KEYS[0]].shape == st[KEYS[1]].shape == (k,)


def test_the_table_row_stands_behind_sampled_elbo_hessian_and_the_pinned_tuples_are_unchanged():
    from vae_training_amd import observables
    from vae_training_amd.model import GenerativeModel
    assert [ob.name for ob in observables.OBSERVABLES] == ["log_likelihood_samples", "mlp_log_likelihood_samples", "exact_log_likelihood",
                                                          "elbo_hessian", "eigenvalues", "decoder_jacobian"]
    assert [after for after, _ in observables.LATER_OBSERVABLES] == ["elbo_hessian"] and len(observables.TABLE) == len(observables.OBSERVABLES) + 1
    assert [ob.name for ob in observables.TABLE if ob.name.startswith("mlp_sampled")] == []
    names = [ob.name for ob in observables.ALL_OBSERVABLES]
    assert names[names.index("sampled_elbo_hessian") + 1] == "mlp_sampled_elbo_hessian" and len(names) == len(observables.TABLE) + 1
    assert [n for n in names if n != "mlp_sampled_elbo_hessian"] == [ob.name for ob in observables.TABLE]
    ob, fl = observables.FLAGS["mlp_sampled_elbo_hessian"]
    assert fl.flag == "--mlp_sampled_elbo_hessian" and fl.linear_hint.endswith("use --sampled_elbo_hessian")
    assert ob.events == (("mlp_sampled_elbo_hessian", "_mlp_sampled_hessian", "ReplicaSampledElboHessianMlp3"),)
    assert observables.array_keys("mlp_sampled_elbo_hessian") == tuple(KEYS[:2]) == observables.array_keys("sampled_elbo_hessian")
    assert set(observables.stats_line_rules(observables.ALL_OBSERVABLES)) >= set(KEYS[:2])
    e = _StubEngine()
    m = _model(e)
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == []      # opt-in
    m.mlp_sampled_elbo_hessian, m.mlp_sampled_elbo_hessian_samples = 8, 2
    st = GenerativeModel._stats_event(m)
    assert list(st) == ["VAE Loss", "mse"] + KEYS and e.calls[-1]["steps"] == 8 and e.calls[-1]["samples"] == 2
    assert e.calls[-1]["x_steps"] == [1] and e.calls[-1]["kw"]["x_tag"] == 14
    lines = []
    w = types.SimpleNamespace(batchnum=0, stats={k: [] for k in KEYS}, _write=lines.append)
    GenerativeModel.write_stats(w, {KEYS[0]: np.array([2.5]), KEYS[1]: np.array([0.5]), KEYS[2]: 2.5, KEYS[3]: 2.5, KEYS[4]: 0.25})
    assert isinstance(w.stats[KEYS[0]][0], np.ndarray) and w.stats[KEYS[2]] == [2.5]
    assert lines == ["Batch | 0 | Sampled Sharpness | 2.500 | Sampled ELBO Hessian Min Ritz | 2.500 | Sampled ELBO Gradient Norm | 0.250"]


def test_run_py_flags_refusals_and_banners(monkeypatch):
    from vae_training_amd import observables, run
    base = ["sph", "--dataset", "sphere"]
    a = run.parse_arguments(base)
    assert a.mlp_sampled_elbo_hessian is None and a.mlp_sampled_elbo_hessian_samples is None      # opt-in
    assert run.parse_arguments(base + ["--mlp_sampled_elbo_hessian"]).mlp_sampled_elbo_hessian == 32
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--mlp_sampled_elbo_hessian", "8", "--mlp_sampled_elbo_hessian_samples", "4",
                                    "--mlp_log_likelihood_samples", "16", "--decoder_jacobian", "prior", "--mlp_fused_stats"])
    assert a.mlp_sampled_elbo_hessian == 8 and a.mlp_sampled_elbo_hessian_samples == 4
    for bad in ("0", "33", "x"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--mlp_sampled_elbo_hessian", bad])
    with pytest.raises(SystemExit):
        run.parse_arguments(base + ["--mlp_sampled_elbo_hessian_samples", "0"])
    with pytest.raises(RuntimeError, match="--mlp_sampled_elbo_hessian_samples sets the samples per row of --mlp_sampled_elbo_hessian"):
        run.main(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian_samples", "4"]))
    assert run.MLP_SAMPLED_ELBO_HESSIAN_NEEDS == observables.FLAGS["mlp_sampled_elbo_hessian"][1].needs
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian needs .*three hidden layers.*; this is a linear VAE: use "
                                           r"--sampled_elbo_hessian \(this model's step path: stub\)"):
        run.check_mlp_sampled_elbo_hessian_model(_model(_StubEngine(mlp3=False, linear=True)))
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian needs .*three hidden layers.*step path: stub, world 1"):
        run.check_mlp_sampled_elbo_hessian_model(_model(_StubEngine(mlp3=False)))          # another MLP
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian needs .*world 2"):
        run.check_mlp_sampled_elbo_hessian_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian needs"):
        run.check_mlp_sampled_elbo_hessian_model(_model(_StubEngine(), dd=17))
    run.check_mlp_sampled_elbo_hessian_model(_model(_StubEngine()))
    e = _StubEngine()
    m = _model(e)
    fl, = observables.attach(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian"]), [m], m, build=False)
    assert (m.mlp_sampled_elbo_hessian, m.mlp_sampled_elbo_hessian_samples) == (32, 1)
    assert fl.banner_one(m) == ("Sampled ELBO Hessian events: 32 Lanczos steps on 1000 rows x 1 samples "
                                "(vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)")
    sweep, ms = types.SimpleNamespace(), [_model(e, seed=s) for s in (69, 24)]
    fl, = observables.attach(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian", "4", "--mlp_sampled_elbo_hessian_samples", "3"]), ms, sweep,
                             build=True)
    (ob, ev), = observables.active(ms, sweep)
    assert fl.banner_sweep(ev, 2, sweep) == ("Sampled ELBO Hessian events: 4 Lanczos steps on 1000 rows x 3 samples per model, one call for 2 "
                                             "models (vaek_mlp3_sampled_elbo_hessian_lanczos_replicas)")
    assert [list(x) for x in observables.run_events(ms, sweep)] == [KEYS, KEYS] and len(e.calls) == 1 and e.calls[0]["n"] == 2
    # the linear flag on an mlp3 model is still refused with its own message
    with pytest.raises(RuntimeError, match=r"^--sampled_elbo_hessian needs .*one or two decoders.*step path: stub"):
        list(observables.attach(run.parse_arguments(base + ["--sampled_elbo_hessian"]), [m], m, build=False))
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian_samples 2000: at most 1024 samples per row"):
        list(observables.attach(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian", "--mlp_sampled_elbo_hessian_samples", "2000"]), [m], m,
                                build=False))
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian_samples 9: 1 models x 1000 rows x 9 samples = 9000 columns, at most 16384 "
                                           r"fit one call and 8192 one model"):
        list(observables.attach(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian", "--mlp_sampled_elbo_hessian_samples", "9"]), [m], m,
                                build=False))
    with pytest.raises(RuntimeError, match=r"--mlp_sampled_elbo_hessian_samples 8: 3 models x 1000 rows x 8 samples = 24000 columns"):
        list(observables.attach(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian", "--mlp_sampled_elbo_hessian_samples", "8"]),
                                [_model(e) for _ in range(3)], types.SimpleNamespace(), build=False))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^--mlp_sampled_elbo_hessian needs .*does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--mlp_sampled_elbo_hessian"]))


# ---- 5 / 6. the ABI: declarations, constants, the refusals without a context, the description guards ------------------------------------------
def test_the_declarations_the_constants_and_the_null_refusals():
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    for name, nargs in NEW.items():
        assert _c_args(hdr, name) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES[ENTRIES[0]][1][2]._type_ is _lib.VaekSampledElboHvp            # the existing descriptions, unchanged
    assert _lib.SIGNATURES[ENTRIES[1]][1][2]._type_ is _lib.VaekSampledElboHessian
    assert "definition of \"live\" of vaek_mlp3_decoder_jacobian_replicas does not apply here" in hdr and "LAUNCHES: 3 + 2 nvec" in hdr and "LAUNCHES: 6 + 6 steps" in hdr
    lib = _lib.load()
    assert lib.vaek_mlp3_sampled_elbo_hessian_max_columns() == 1 << 14 and lib.vaek_sampled_elbo_hessian_record_len() == 142 == K.ref().RECORD_LEN
    yes = C.c_int32(7)
    assert lib.vaek_supports_mlp3_sampled_elbo_hessian(None, 2, C.byref(yes)) == -1 and yes.value == 7
    assert b"vaek_supports_mlp3_sampled_elbo_hessian" in lib.vaek_last_error()
    n = C.c_size_t(7)
    assert lib.vaek_mlp3_sampled_elbo_hessian_workspace_bytes(None, 1, 10, 8, C.byref(n)) == -1 and n.value == 7
    assert lib.vaek_last_error().decode() == "vaek_mlp3_sampled_elbo_hessian_workspace_bytes: null argument"


@pytest.mark.parametrize("name", ENTRIES)
def test_the_description_is_checked_before_the_context(name):
    """check_eval's order, as tests/test_eval_descriptions_host.py holds the other entries to it: a NULL description, then a struct_size
    of another header (both sizes in the message), then the NULL context -- each with the entry's name."""
    from vae_training_amd import _lib
    check_description_guard(_lib.load(), name)
