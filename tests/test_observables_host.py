"""The stats-event observables as ONE table (vae_training_amd/observables.py), no GPU: what GenerativeModel._stats_event and the sweep's
event runner return on stub engines with every flag of a linear model and of an mlp3 model set -- the keys and their order, the rows
the combined events share, the key filter of --subspace alone -- and the consistency of the table with run.py's parser, its refusals,
the event classes' KEYS and model.py's array-key constants."""
import types

import pytest
import torch

# compute_stats' keys, then the keys every event adds, in the order of losses.npz
LINEAR_KEYS = ["VAE Loss", "mse",
               "Average Log Likelihood", "ELBO estimate", "Effective Sample Size",
               "Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning", "IWAE Gap",
               "ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm",
               "learnt eigenvalue", "ground truth eigenvalue", "Principal Angles", "Subspace Distance"]
MLP3_KEYS = ["VAE Loss", "mse",
             "Average Log Likelihood", "ELBO estimate", "Effective Sample Size",
             "Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"]
SUBSPACE_ALONE_KEYS = ["VAE Loss", "mse", "Principal Angles", "Subspace Distance"]
LINEAR_FLAGS = dict(log_likelihood_samples=8, exact_log_likelihood=True, elbo_hessian=4, eigenvalues=True, subspace=True)
MLP3_FLAGS = dict(mlp_log_likelihood_samples=8, decoder_jacobian="prior")


class _StubEngine:
    """What the seven event classes ask of an engine, on the CPU: every evaluation call logs (name, row steps, row tag) and fills
    records that pass the solve checks."""
    rank, world = 0, 1
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = stats_event_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    mlp3_log_likelihood_max_columns = mlp3_decoder_jacobian_max_columns = 1 << 22
    elbo_hessian_max_steps = 32
    elbo_hessian_record_len = 140
    step_path = "stub"

    def __init__(self, linear=True, D=3, L=6):
        self.linear, self.D, self.L = linear, D, L
        self.log = []
        self.exact_log_likelihood_record_len = 10 + D
        self.cov_spectrum_record_len = D * D + 2 * D + 4
        self.cov_eigen_record_len = self.cov_spectrum_record_len + D * D
        self.decoder_jacobian_record_len = 2 * L + 8

    def supports_log_likelihood(self, kind):
        return self.linear

    supports_exact_log_likelihood = supports_elbo_hessian = supports_spectrum_event = supports_log_likelihood

    def supports_mlp3_log_likelihood(self, kind):
        return not self.linear

    def supports_mlp3_decoder_jacobian(self):
        return not self.linear

    def supports_cov_spectrum(self):
        return True

    def log_likelihood_workspace(self, n, rows):
        return 32 * n

    def mlp3_log_likelihood_workspace(self, n, rows, samples):
        return 32 * n

    def mlp3_decoder_jacobian_workspace(self, n, rows):
        return 32 * n

    def subspace_record_len(self, kb):
        return kb + 4

    def rng_fill(self, n, seed, step=0, tag=0, bits=False):
        return torch.zeros(n, dtype=torch.float32)

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.log.append(("iwae", kw["x_steps"].tolist(), kw["x_tag"]))
        out.zero_()

    def mlp3_log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.log.append(("iwae_mlp3", kw["x_steps"].tolist(), kw["x_tag"]))
        out.zero_()

    def exact_log_likelihood_replicas(self, params, rows, out, **kw):
        self.log.append(("exact", kw["x_steps"].tolist(), kw["x_tag"]))
        out.zero_()
        out[:, 7] = 1.0

    def elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, **kw):
        self.log.append(("hessian", kw["x_steps"].tolist(), kw["x_tag"]))
        out.zero_()
        out[:, 2], out[:, 6] = 3, 1.0

    def _eigen(self, out, name, x_steps, kw):
        self.log.append((name, x_steps.tolist(), kw["x_tag"]))
        out.zero_()
        out.view(-1, out.shape[1] // 2)[:, 2 * self.D + self.D * self.D + 2] = 1.0           # |C|_F

    def spectrum_event_replicas(self, params, rows, kind, A, dd, did, pad, var, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        self._eigen(out, "spectrum", x_steps, kw)

    def eigen_event_replicas(self, params, rows, kind, A, dd, did, pad, var, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        self._eigen(out, "eigen", x_steps, kw)

    def subspace_angles(self, a, b, ka, kb, out, n=None, a_stride=None, b_stride=None):
        out.zero_()
        out[:, :kb] = 0.25

    def mlp3_decoder_jacobian_replicas(self, params, rows, out, workspace, **kw):
        self.log.append(("jacobian", kw["z_steps"].tolist(), kw["z_tag"]))
        out.zero_()


def _model(eng, seed=1, **flags):
    P, kind = 4, 0 if eng.linear else 2
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=100, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    A = torch.full((3,), float(seed)) if eng.linear else None
    ds = types.SimpleNamespace(device_spec=lambda: (kind, A, 3, 3, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb=None: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=100, optimizer=opt, key=(3, 4), num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], gt_eigen=[],
                                 ht_eigen=[], _latent_draws=9, _loglik_draws=4, _exact_loglik_draws=6, dirname="run_dir",
                                 compute_stats=lambda: {"VAE Loss": 1.0, "mse": 2.0},
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))), **flags)


def _check_linear_log(log, steps):
    """One call per event in the table's order; the exact event on the IWAE event's rows, the Hessian on the exact event's."""
    assert [name for name, _, _ in log] == ["iwae", "exact", "hessian", "eigen"]
    by = {name: (x_steps, tag) for name, x_steps, tag in log}
    assert by["iwae"] == (steps, 3) and by["exact"] == by["iwae"] and by["hessian"] == by["exact"] and by["eigen"][1] == 5


def test_stats_event_of_a_linear_model_with_every_flag():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e, **LINEAR_FLAGS)
    for event in range(2):
        del e.log[:]
        assert list(GenerativeModel._stats_event(m)) == LINEAR_KEYS
        _check_linear_log(e.log, [5 + event])                             # _loglik_draws: 4, incremented before use
    assert m._exact_loglik_draws == 6 and m._elbo_hessian_draws == 2 and m._spectrum_draws == 2
    # the event objects are built on first use and kept under these names
    assert all(getattr(m, name, None) is not None for name in ("_loglik", "_exact_loglik", "_elbo_hessian", "_subspace"))
    assert not hasattr(m, "_spectrum") and not hasattr(m, "_jacobian") and not hasattr(m, "_loglik_mlp3")


def test_stats_event_of_an_mlp3_model_with_every_flag():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine(linear=False)
    m = _model(e, **MLP3_FLAGS)
    assert list(GenerativeModel._stats_event(m)) == MLP3_KEYS
    assert e.log == [("iwae_mlp3", [5], 3), ("jacobian", [1], 8)]
    assert getattr(m, "_loglik_mlp3", None) is not None and getattr(m, "_jacobian", None) is not None and not hasattr(m, "_loglik")


def test_subspace_alone_leaves_the_eigenvalue_keys_out():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    st = GenerativeModel._stats_event(_model(e, subspace=True))
    assert list(st) == SUBSPACE_ALONE_KEYS and "learnt eigenvalue" not in st and "ground truth eigenvalue" not in st
    assert [name for name, _, _ in e.log] == ["eigen"]
    assert list(GenerativeModel._stats_event(_model(e, eigenvalues=True))) == ["VAE Loss", "mse", "learnt eigenvalue", "ground truth eigenvalue"]
    assert e.log[-1][0] == "spectrum"
    assert GenerativeModel._stats_event(_model(e)) == {"VAE Loss": 1.0, "mse": 2.0} and len(e.log) == 2


# ---- the sweep's event runner: the same table, the same keys, the same shared rows -------------------------------------------------------
def _sweep(eng, argv, seeds=(69, 24)):
    """What run.main_sweep does before any step: the flags checked on model 0, their attributes on the sweep's settings, the events built."""
    from vae_training_amd import observables, run
    args = run.parse_arguments(["name", "--dataset", "linear_gaussian", "--sweep_dataset_seeds", ",".join(map(str, seeds))] + argv)
    ms = [_model(eng, seed=s) for s in seeds]
    sweep = types.SimpleNamespace()
    flags = [fl.flag for fl in observables.attach(args, ms, sweep, build=True)]
    return ms, sweep, args, flags


def test_the_sweep_runner_gives_the_single_model_keys_in_one_call_per_event():
    from vae_training_amd import observables
    e = _StubEngine()
    ms, sweep, args, flags = _sweep(e, ["--log_likelihood_samples", "8", "--exact_log_likelihood", "--elbo_hessian", "4", "--eigenvalues",
                                        "--subspace", "auto"])
    assert flags == ["--log_likelihood_samples", "--exact_log_likelihood", "--elbo_hessian", "--eigenvalues", "--subspace"]
    assert e.log == [] and sweep._subspace.k == 3 and sweep.subspace_k is None and not hasattr(sweep, "_spectrum")      # built before any step
    ms[1]._loglik_draws = 11
    extra = observables.run_events(ms, sweep)
    assert len(extra) == 2 and all(["VAE Loss", "mse"] + list(x) == LINEAR_KEYS for x in extra)
    _check_linear_log(e.log, [5, 12])                                     # ONE call per event for both models, each on its own step
    banners = [fl.banner_sweep(ev, 2, sweep) for ob, ev in observables.active(ms, sweep) for fl in ob.flags if fl.value(args) is not None]
    assert banners == ["Log-likelihood events: 8 samples × 1000 rows (vaek_log_likelihood_replicas)",
                       "Exact log-likelihood events: 1000 rows per model, one launch for 2 models (vaek_exact_log_likelihood_replicas)",
                       "ELBO Hessian events: 4 Lanczos steps on 1000 rows per model, one launch for 2 models (vaek_elbo_hessian_lanczos_replicas)",
                       "Eigenvalue events: 1000 generated and 1000 real rows per model (vaek_eigen_event_replicas)",
                       "Subspace events: the 3 leading eigenvectors of 1000 generated and 1000 real rows per model (vaek_eigen_event_replicas, "
                       "vaek_subspace_angles)"]


def test_the_sweep_runner_on_mlp3_models_and_with_subspace_alone():
    from vae_training_amd import observables
    e = _StubEngine(linear=False)
    ms, sweep, _, flags = _sweep(e, ["--mlp_log_likelihood_samples", "8", "--decoder_jacobian", "prior"])
    assert flags == ["--mlp_log_likelihood_samples", "--decoder_jacobian"] and sweep.decoder_jacobian_tol == 1e-4
    assert all(["VAE Loss", "mse"] + list(x) == MLP3_KEYS for x in observables.run_events(ms, sweep))
    assert e.log == [("iwae_mlp3", [5, 5], 3), ("jacobian", [1, 1], 8)]
    e = _StubEngine()
    ms, sweep, _, _ = _sweep(e, ["--subspace", "2"])
    assert all(["VAE Loss", "mse"] + list(x) == SUBSPACE_ALONE_KEYS for x in observables.run_events(ms, sweep)) and sweep.subspace_k == 2
    assert observables.run_events(ms, types.SimpleNamespace()) == [{}, {}]


# ---- the table against the parser, the refusals, the event classes and model.py -----------------------------------------------------------
def _flags():
    from vae_training_amd import observables
    return [(ob, fl) for ob in observables.OBSERVABLES for fl in ob.flags]


EXAMPLE = {"log_likelihood_samples": ["8"], "mlp_log_likelihood_samples": ["8"], "exact_log_likelihood": [], "elbo_hessian": ["4"],
           "eigenvalues": [], "subspace": ["auto"], "decoder_jacobian": ["prior"]}


def test_the_table_lists_every_observable_flag_once_in_the_order_of_the_stats_line():
    assert [fl.dest for _, fl in _flags()] == list(EXAMPLE)
    assert [fl.flag for _, fl in _flags()] == ["--" + dest for dest in EXAMPLE]


@pytest.mark.parametrize("dest", list(EXAMPLE))
def test_every_entry_is_consistent_with_the_parser_the_refusals_and_its_event_class(dest, monkeypatch):
    from vae_training_amd import events, observables, run
    from vae_training_amd.model import GenerativeModel
    ob, fl = observables.FLAGS[dest]
    base = ["name", "--dataset", "linear_gaussian"]
    assert fl.value(run.parse_arguments(base)) is None                    # opt-in
    args = run.parse_arguments(base + [fl.flag] + EXAMPLE[dest])
    assert fl.value(args) is not None and fl.dest == dest and getattr(run, {"log_likelihood_samples": "LOGLIK_NEEDS",
        "mlp_log_likelihood_samples": "MLP_LOGLIK_NEEDS", "exact_log_likelihood": "EXACT_LOGLIK_NEEDS", "elbo_hessian": "ELBO_HESSIAN_NEEDS",
        "eigenvalues": "EIGEN_NEEDS", "subspace": "SUBSPACE_NEEDS", "decoder_jacobian": "JACOBIAN_NEEDS"}[dest]) == fl.needs
    # its dest is the attribute _stats_event reads: set on a model the event covers, the event runs and is kept under the row's cache name
    e = _StubEngine(linear=not dest.startswith(("mlp", "decoder")))
    m = _model(e)
    for name, v in ({dest: fl.value(args)} if fl.attrs is None else fl.attrs(args, fl.value(args), None)).items():
        setattr(m, name, v)
    row = next(r for r in ob.events if r[0] == dest)
    assert len(GenerativeModel._stats_event(m)) > 2 and len(e.log) == 1 and isinstance(getattr(m, row[1]), getattr(events, row[2]))
    # its array keys are keys of its event class
    for r, (_, _, cls) in enumerate(ob.events):
        assert set(ob.array_keys(ob.event_class(r))) <= set(getattr(events, cls).KEYS)
    assert ob.line is None or ob.line[0] in ob.array_keys(ob.event_class())
    # data parallelism: refused by main() before a process group exists
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match=f"^{fl.flag} needs .* does not combine with data parallelism"):
        run.main(args)


def test_the_array_keys_of_model_py_are_the_tables():
    from vae_training_amd import events, model, observables
    assert model.HESSIAN_ARRAY_KEYS == observables.array_keys("elbo_hessian") == events.ReplicaElboHessian.KEYS[:2]
    assert model.JACOBIAN_KEYS == observables.array_keys("decoder_jacobian") == events.ReplicaJacobianMlp3.KEYS
    assert observables.stats_line_rules() == {"ELBO Hessian Ritz Values": None, "ELBO Hessian Ritz Residuals": None,
                                              "Decoder Jacobian Spectrum": None, "Decoder Jacobian Rank": "Decoder Jacobian Rank (mean)",
                                              "Latent Sensitivity": None}
