"""Host side of the decoder Jacobian of linear VAEs, no GPU: the ABI surface of vaek_linear_decoder_jacobian_replicas, the table entry of
--linear_decoder_jacobian, trainer.ReplicaJacobianLinear around a stub engine, run.py's parser, refusals and banners, and the stats
line."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"]
NEW = {"vaek_supports_linear_decoder_jacobian": 2, "vaek_linear_decoder_jacobian_max_rows": 0,
       "vaek_linear_decoder_jacobian_workspace_bytes": 4, "vaek_linear_decoder_jacobian_replicas": 6}


def test_abi_surface_of_the_linear_decoder_jacobian():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols; the cap; argument checks that need no device."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.vaek_linear_decoder_jacobian_max_rows() == 2 ** 20
    # the description is the MLP call's, unchanged
    assert _lib.SIGNATURES["vaek_linear_decoder_jacobian_replicas"][1] == _lib.SIGNATURES["vaek_mlp3_decoder_jacobian_replicas"][1]
    csrc = os.path.join(ROOT, "vae_training_amd", "csrc")
    assert "linear_jacobian.hip" in open(os.path.join(csrc, "Makefile")).read()
    # one text of the solve and of the finalize launch: both units call the header's functions and neither restates them
    shared = open(os.path.join(csrc, "jacobian_dev.h")).read()
    assert "jacobi_solve<false>" in shared and "tree_sum256" in shared
    for unit in ("mlp3_jacobian.hip", "linear_jacobian.hip"):
        text = open(os.path.join(csrc, unit)).read()
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        assert '#include "jacobian_dev.h"' in code and "jacobian_solve_row<" in code and "jacobian_finalize_replica(" in code, unit
        assert "jacobi_solve<" not in code and "tree_sum256" not in code and "atomic" not in code, unit
    yes = C.c_int32(7)
    assert lib.vaek_supports_linear_decoder_jacobian(None, C.byref(yes)) == -1 and yes.value == 7
    assert b"vaek_supports_linear_decoder_jacobian" in lib.vaek_last_error()
    b = C.c_size_t(7)
    assert lib.vaek_linear_decoder_jacobian_workspace_bytes(None, 1, 1, C.byref(b)) == -1 and b.value == 7
    assert b"vaek_linear_decoder_jacobian_workspace_bytes" in lib.vaek_last_error()


def test_the_description_is_checked_before_the_context():
    from vae_training_amd import _lib
    check_description_guard(_lib.load(), "vaek_linear_decoder_jacobian_replicas")


def test_the_table_entry_stands_behind_decoder_jacobian_and_the_pinned_tables_are_unchanged():
    from vae_training_amd import model, observables, run
    assert [ob.name for ob in observables.OBSERVABLES] == ["log_likelihood_samples", "mlp_log_likelihood_samples", "exact_log_likelihood",
                                                           "elbo_hessian", "eigenvalues", "decoder_jacobian"]
    assert len(observables.TABLE) == len(observables.OBSERVABLES) + 1 and len(observables.ALL_OBSERVABLES) == len(observables.TABLE) + 1
    assert [after for after, _ in observables.LINEAR_OBSERVABLES] == ["decoder_jacobian"]
    names = [ob.name for ob in observables.EVERY_OBSERVABLE]
    assert names[names.index("decoder_jacobian") + 1] == "linear_decoder_jacobian" and len(names) == len(observables.ALL_OBSERVABLES) + 1
    assert [n for n in names if n != "linear_decoder_jacobian"] == [ob.name for ob in observables.ALL_OBSERVABLES]
    ob, fl = observables.FLAGS["linear_decoder_jacobian"]
    assert fl.flag == "--linear_decoder_jacobian" and ob.events == (("linear_decoder_jacobian", "_linear_jacobian", "ReplicaJacobianLinear"),)
    assert ob.line == ("Decoder Jacobian Rank", "(mean)") and list(ob.array_keys(ob.event_class())) == KEYS
    assert run.LINEAR_JACOBIAN_NEEDS == fl.needs and "--decoder_jacobian" in fl.needs
    assert set(observables.FLAGS) == {f.dest for o in observables.EVERY_OBSERVABLE for f in o.flags}
    # the default of stats_line_rules is the pinned tuple; model.py reads the whole
    assert observables.stats_line_rules() == observables.stats_line_rules(observables.OBSERVABLES)
    assert model._ARRAY_KEY_LINES == observables.stats_line_rules(observables.EVERY_OBSERVABLE)
    assert model._ARRAY_KEY_LINES["Decoder Jacobian Rank"] == "Decoder Jacobian Rank (mean)"


class _StubEngine:
    """What ReplicaJacobianLinear asks of an engine, on the CPU; records the library calls in order and fills the records."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    stats_event_max_rows = 4096
    linear_decoder_jacobian_max_rows = 2 ** 20
    mlp3_decoder_jacobian_max_columns = 2 ** 20
    step_path = "stub"

    def __init__(self, linear=True, mlp3=False, D=7, L=6, world=1):
        self._linear, self._mlp3, self.D, self.L, self.world, self.calls, self.ws, self.log = linear, mlp3, D, L, world, [], [], []

    decoder_jacobian_record_len = property(lambda self: 2 * self.L + 8)
    decoder_jacobian_row_record_len = property(lambda self: 2 * self.L + 4)

    def supports_linear_decoder_jacobian(self):
        return self._linear

    def supports_mlp3_decoder_jacobian(self):
        return self._mlp3

    def supports_log_likelihood(self, kind):
        return self._linear

    def supports_train_loop_gen(self, kind):
        raise AssertionError("the decoder Jacobian does not ask a train loop's predicate: it has no batch-size condition")

    supports_stats_event = supports_train_step_replicas = supports_mlp3_log_likelihood = supports_train_loop_gen

    def linear_decoder_jacobian_workspace(self, n, rows):
        self.ws.append((n, rows))
        return 64 * n * rows

    def make_batch(self, kind, A, dd, did, pad, var, rows, seed, **kw):
        self.log.append(("make_batch", seed % 2 ** 64, kw["step"], kw["tag"], rows))
        return torch.full((rows, self.D), 1.0), torch.zeros(rows, self.L), torch.zeros(rows, self.D)

    def forward(self, params, x, z1, z2, sampling=False, want_mu=True, **kw):
        assert not sampling and want_mu
        self.log.append(("forward", float(params[0]), x.shape[0]))
        return None, torch.full((x.shape[0], self.L), float(params[0]))      # mu: the model's mark

    def linear_decoder_jacobian_replicas(self, params, rows, out, workspace, **kw):
        self.log.append(("jacobian",))
        z = kw.get("z")
        self.calls.append(dict(n=params.shape[0], rows=rows, params=params.clone(), ws=workspace.numel(), kw=kw,
                               z=None if z is None else z.clone(),
                               z_seeds=None if kw.get("z_seeds") is None else kw["z_seeds"].tolist(),
                               z_steps=None if kw.get("z_steps") is None else kw["z_steps"].tolist()))
        for r in range(params.shape[0]):                 # record r: 100 r + slot; slot [6] is the solve's ratio
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float64)
            out[r, 6] = self.ratio if hasattr(self, "ratio") else 2.0 ** -50

    def mlp3_decoder_jacobian_replicas(self, *a, **kw):
        raise AssertionError("a linear model's Jacobian is not the MLP call's")

    stats_event_replicas = mlp3_log_likelihood_replicas = mlp3_decoder_jacobian_workspace = mlp3_decoder_jacobian_replicas


def _model(eng, P=4, kind=2, seed=1, B=100, key=(3, 4), dd=3):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    A = None if kind == 2 else torch.full((3,), float(seed))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, A, dd, 3, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb=None: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 _loglik_draws=2, _spectrum_draws=3, dirname="stub",
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def _untouched(m, s, k):
    return (m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m.dataset.key == (s, 2) and m._loglik_draws == 2 and
            m._spectrum_draws == 3 and m.vae_losses == [] and m.var_enc == [] and m.current_epsilon == -3.0)


def test_the_two_events_share_one_spine():
    from vae_training_amd import trainer
    J, M, Lin = trainer.ReplicaJacobian, trainer.ReplicaJacobianMlp3, trainer.ReplicaJacobianLinear
    assert issubclass(M, J) and issubclass(Lin, J) and issubclass(J, trainer.ReplicaEvent)
    for name in ("event", "_allocate", "__init__", "KEYS", "COUNTER", "X_TAG", "Z_TAG", "MODES"):      # stated once
        assert name not in vars(M) and name not in vars(Lin) and name in vars(J), name
    assert Lin.KEYS == tuple(KEYS) and (Lin.X_TAG, Lin.Z_TAG, Lin.COUNTER) == (7, 8, "_jacobian_draws")
    assert (M.ENTRY, Lin.ENTRY) == ("mlp3_decoder_jacobian", "linear_decoder_jacobian")


def test_replica_jacobian_linear_prior_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaJacobianLinear
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 256), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B, kind=1) for s, k, B in spec]
    jac = ReplicaJacobianLinear(ms)
    assert jac.R == 3 and jac.rows == 1000 and jac.at == "prior" and jac.rank_tol == 1e-4 and jac.params.shape == (3, 4)
    assert jac.out.shape == (3, 20) and jac.out.dtype == torch.float64 and e.ws == [(3, 1000)] and jac.workspace.numel() == 64 * 3 * 1000
    for event in range(2):
        stats = jac.event()
        assert len(e.calls) == event + 1 and e.log == [("jacobian",)] * (event + 1)      # ONE library call for R models, nothing else
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["z"] is None and c["kw"]["z_tag"] == 8 and c["kw"]["rank_tol"] == 1e-4
        assert [s % 2 ** 64 for s in c["z_seeds"]] == [(s ^ 2) % 2 ** 64 for s, _, _ in spec]      # dataset.key[0] ^ dataset.key[1]
        assert c["z_steps"] == [event + 1] * 3                                                # its own counter, incremented before use
        assert c["params"][:, 0].tolist() == [float(s) for s, _, _ in spec] and c["ws"] == jac.workspace.numel()
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):
            assert _untouched(m, s, k) and m._jacobian_draws == event + 1
            assert list(st) == KEYS
            assert st[KEYS[0]].tolist() == [100.0 * r + 8 + j for j in range(6)] and st[KEYS[2]].tolist() == [100.0 * r + 14 + j for j in range(6)]
            assert st[KEYS[1]].tolist() == [100.0 * r + 1, 100.0 * r + 2, 100.0 * r + 3]
            assert len(m.jacobian_spectra) == len(m.jacobian_ranks) == len(m.latent_sensitivities) == event + 1
    # the solve figures: a record whose largest off_F / |G|_F exceeds 2^-40 is refused, with the model's number
    e.ratio = 2.0 ** -39
    with pytest.raises(RuntimeError, match=r"ReplicaJacobianLinear: model 0 .*solve of J\^T J.*2\^-40"):
        jac.event()
    del e.ratio
    # rows and threshold are the caller's; the cap itself is legal
    ReplicaJacobianLinear([_model(e) for _ in range(256)], rows=4096, rank_tol=0.0)       # 256 x 4096 = 2^20 rows
    ReplicaJacobianLinear([_model(e)], rows=37, rank_tol=0.25).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["kw"]["rank_tol"] == 0.25


def test_replica_jacobian_linear_posterior_draws_encodes_and_passes_explicit_rows():
    from vae_training_amd.trainer import ReplicaJacobianLinear
    e = _StubEngine()
    spec = [(69, (3, 4)), (24, (7, 8))]
    ms = [_model(e, seed=s, key=k) for s, k in spec]
    jac = ReplicaJacobianLinear(ms, rows=5, at="posterior", rank_tol=1e-3)
    for event in range(2):
        e.log.clear()
        jac.event()
        # per model make_batch -> forward(sampling=False) under the class's row tag and counter, then ONE explicit call
        assert e.log == [("make_batch", 69 ^ 2, event + 1, 7, 5), ("forward", 69.0, 5), ("make_batch", 24 ^ 2, event + 1, 7, 5),
                         ("forward", 24.0, 5), ("jacobian",)]
        c = e.calls[-1]
        assert c["z_seeds"] is None and c["z_steps"] is None and c["z"].shape == (2, 5, 6) and c["kw"]["rank_tol"] == 1e-3
        assert (c["z"][0] == 69.0).all() and (c["z"][1] == 24.0).all()                      # mu of the library's own forward
        assert all(_untouched(m, s, k) and m._jacobian_draws == event + 1 for m, (s, k) in zip(ms, spec))
    assert len(e.calls) == 2


def test_replica_jacobian_linear_refusals():
    from vae_training_amd.trainer import ReplicaJacobianLinear, ReplicaJacobianMlp3
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaJacobianLinear([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaJacobianLinear([_model(e), _model(_StubEngine(D=9))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianLinear: vaek_linear_decoder_jacobian_replicas does not cover.*"
                                           r"ReplicaJacobianMlp3 \(--decoder_jacobian\).*step path: stub"):
        ReplicaJacobianLinear([_model(_StubEngine(linear=False, mlp3=True))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianLinear.*world"):
        ReplicaJacobianLinear([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianLinear draws.*-dd / -did <= 16"):
        ReplicaJacobianLinear([_model(e, dd=17)])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaJacobianLinear([_model(e) for _ in range(1025)], rows=1)
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match="rows"):
            ReplicaJacobianLinear([_model(e)], rows=rows)
    with pytest.raises(RuntimeError, match=r"257 models x 4096 rows = 1052672 rows, at most 1048576.*vaek_linear_decoder_jacobian_max_rows"):
        ReplicaJacobianLinear([_model(e) for _ in range(257)], rows=4096)
    with pytest.raises(RuntimeError, match="at="):
        ReplicaJacobianLinear([_model(e)], at="encoder")
    for tol in (-0.1, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match="rank_tol"):
            ReplicaJacobianLinear([_model(e)], rank_tol=tol)
    with pytest.raises(RuntimeError):
        ReplicaJacobianLinear([])
    assert e.calls == [] and e.ws == []
    # the sibling's refusal of a linear model keeps its sentence and now names the class and flag that take it
    with pytest.raises(RuntimeError, match=r"ReplicaJacobianMlp3: vaek_mlp3_decoder_jacobian_replicas does not cover.*K\^T K.*"
                                           r"ReplicaJacobianLinear \(--linear_decoder_jacobian\).*step path: stub"):
        ReplicaJacobianMlp3([_model(_StubEngine(linear=True, mlp3=False))])


def test_the_stats_helper_adds_the_jacobian_only_when_asked_and_the_line_shows_the_mean_rank(capsys):
    """GenerativeModel._stats_event: compute_stats() alone without the attribute; with it, the three keys behind compute_stats' own, from
    ONE event object for the run; write_stats keeps the arrays (L = 1 included) and prints the mean rank."""
    import collections

    from vae_training_amd.model import GenerativeModel
    e = _StubEngine(L=1)
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_jacobian_draws")
    m.linear_decoder_jacobian, m.linear_decoder_jacobian_tol = "prior", 1e-3
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["n"] == 1
        assert e.calls[-1]["z_steps"] == [event + 1] and e.calls[-1]["kw"]["rank_tol"] == 1e-3
        assert _untouched(m, 1, (3, 4))
    assert e.ws == [(1, 1000)]                            # one ReplicaJacobianLinear for the run, not one per event
    assert type(m._linear_jacobian).__name__ == "ReplicaJacobianLinear" and getattr(m, "_jacobian", None) is None
    m.stats, m.batchnum, m.tqdm, m.rank = collections.defaultdict(list), 0, False, 0
    m._write = lambda msg: GenerativeModel._write(m, msg)
    GenerativeModel.write_stats(m, st)
    line = capsys.readouterr().out
    assert "| Decoder Jacobian Rank (mean) | 1.000" in line and "VAE Loss | 1.000" in line
    assert [np.asarray(m.stats[k][0]).shape for k in KEYS] == [(1,), (3,), (1,)]


def test_attach_sets_the_attributes_builds_one_event_and_prints_the_banners():
    from vae_training_amd import observables, run
    base = ["sig", "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", ""]
    e = _StubEngine()
    ms = [_model(e, seed=s) for s in (69, 24)]
    args = run.parse_arguments(base + ["--linear_decoder_jacobian", "posterior", "--linear_decoder_jacobian_tol", "1e-3"])
    sweep = types.SimpleNamespace()
    flags = list(observables.attach(args, ms, sweep, build=True))
    assert [f.dest for f in flags] == ["linear_decoder_jacobian"]
    assert sweep.linear_decoder_jacobian == "posterior" and sweep.linear_decoder_jacobian_tol == 1e-3
    ev = sweep._linear_jacobian
    assert type(ev).__name__ == "ReplicaJacobianLinear" and (ev.R, ev.at, ev.rank_tol, ev.rows) == (2, "posterior", 1e-3, 1000)
    assert [(ob.name, x) for ob, x in observables.active(ms, sweep)] == [("linear_decoder_jacobian", ev)] and e.ws == [(2, 1000)]
    assert flags[0].banner_sweep(ev, 2, sweep) == ("Decoder Jacobian events: 1000 posterior latent rows per model, rank threshold 0.001, one "
                                                   "call for 2 models (vaek_linear_decoder_jacobian_replicas)")
    m = _model(e)
    args = run.parse_arguments(base + ["--linear_decoder_jacobian", "prior"])
    assert [f.dest for f in observables.attach(args, [m], m, build=False)] == ["linear_decoder_jacobian"]
    assert m.linear_decoder_jacobian == "prior" and m.linear_decoder_jacobian_tol == 1e-4 and not hasattr(m, "_linear_jacobian")
    assert flags[0].banner_one(m) == ("Decoder Jacobian events: 1000 prior latent rows, rank threshold 0.0001 "
                                      "(vaek_linear_decoder_jacobian_replicas)")
    out = observables.run_events([m], m)
    assert list(out[0]) == KEYS and len(e.calls) == 1


def test_run_py_parses_and_refuses_the_linear_decoder_jacobian_flags(monkeypatch):
    from vae_training_amd import run
    base = ["sig", "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", ""]
    a = run.parse_arguments(base)
    assert a.linear_decoder_jacobian is None and a.linear_decoder_jacobian_tol is None       # opt-in: without the flag nothing changes
    a = run.parse_arguments(base + ["--linear_decoder_jacobian", "prior"])
    assert a.linear_decoder_jacobian == "prior" and run.observables.linear_decoder_jacobian_tol(a) == 1e-4
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--linear_decoder_jacobian", "posterior", "--linear_decoder_jacobian_tol",
                                    "1e-3", "--fused_stats", "--log_likelihood_samples", "8", "--sampled_elbo_hessian", "--eigenvalues"])
    assert a.linear_decoder_jacobian == "posterior" and run.observables.linear_decoder_jacobian_tol(a) == 1e-3 and a.fused_stats
    assert a.log_likelihood_samples == 8 and a.eigenvalues
    for bad in (["--linear_decoder_jacobian", "encoder"], ["--linear_decoder_jacobian"],
                ["--linear_decoder_jacobian", "prior", "--linear_decoder_jacobian_tol", "1"],
                ["--linear_decoder_jacobian", "prior", "--linear_decoder_jacobian_tol", "-1e-3"]):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + bad)
    # the model check: an MLP model (with the hint), an uncovered model, data parallelism, -dd / -did above the generator's, the cap
    with pytest.raises(RuntimeError, match=r"--linear_decoder_jacobian needs .*MLP model takes --decoder_jacobian.*step path: stub"):
        run.check_linear_decoder_jacobian_model(_model(_StubEngine(linear=False, mlp3=True)))
    with pytest.raises(RuntimeError, match=r"--linear_decoder_jacobian needs .*step path: stub"):
        run.check_linear_decoder_jacobian_model(_model(_StubEngine(linear=False)))
    with pytest.raises(RuntimeError, match=r"--linear_decoder_jacobian needs .*world 2"):
        run.check_linear_decoder_jacobian_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match="--linear_decoder_jacobian needs .*-dd / -did <= 16"):
        run.check_linear_decoder_jacobian_model(_model(_StubEngine(), dd=17))
    with pytest.raises(RuntimeError, match=r"1049 models x 1000 rows = 1049000 rows, at most 1048576.*vaek_linear_decoder_jacobian_max_rows.*"
                                           "step path: stub"):
        run.check_linear_decoder_jacobian_model(_model(_StubEngine()), 1049)
    run.check_linear_decoder_jacobian_model(_model(_StubEngine()), 1048)
    run.check_linear_decoder_jacobian_model(_model(_StubEngine(L=32, D=28)))
    # the old refusal of --decoder_jacobian on a linear model: its old pattern, and now the new flag
    with pytest.raises(RuntimeError, match=r"--decoder_jacobian needs .*use --exact_log_likelihood.*K\^T K.*step path: stub") as ei:
        run.check_decoder_jacobian_model(_model(_StubEngine(linear=True, mlp3=False)))
    assert "two-decoder models" in str(ei.value) and "--linear_decoder_jacobian" in str(ei.value)
    # the threshold without its flag, both Jacobian flags, and data parallelism: main() refuses before a process group or a directory exists
    for extra in ([], ["--sweep_dataset_seeds", "1,2"]):
        with pytest.raises(RuntimeError, match="--linear_decoder_jacobian_tol sets the rank threshold of --linear_decoder_jacobian"):
            run.main(run.parse_arguments(base + ["--linear_decoder_jacobian_tol", "1e-3"] + extra))
        with pytest.raises(RuntimeError, match="--decoder_jacobian .* and --linear_decoder_jacobian .* cover disjoint models"):
            run.main(run.parse_arguments(base + ["--linear_decoder_jacobian", "prior", "--decoder_jacobian", "prior"] + extra))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--linear_decoder_jacobian needs .*does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--linear_decoder_jacobian", "prior"]))
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--linear_decoder_jacobian", "prior", "--sweep_dataset_seeds", "1,2"]))
