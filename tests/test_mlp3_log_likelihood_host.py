"""Host side of vaek_mlp3_log_likelihood_replicas, no GPU: the C ABI surface of the four entry points (declared, bound, exported, the
caps, refusals that need no device), trainer.ReplicaLogLikMlp3 on a stub engine (one library call for R models, its own seeds, steps
and tags, the run's RNG state untouched, what it refuses, ReplicaLogLik's behaviour on the same stub unchanged), the stats-event helper
of model.py and run.py's --mlp_log_likelihood_samples flag."""
import ctypes as C
import os
import types

import pytest
import torch

from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_mlp3_log_likelihood", "vaek_mlp3_log_likelihood_max_columns", "vaek_mlp3_log_likelihood_workspace_bytes",
       "vaek_mlp3_log_likelihood_replicas")
KEYS = ["Average Log Likelihood", "ELBO estimate", "Effective Sample Size"]


def test_abi_surface_of_the_mlp3_log_likelihood():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols; the cap; argument checks that need no device."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_mlp3_log_likelihood_replicas") == 13 == _c_args(hdr, "vaek_log_likelihood_replicas")
    assert _lib.SIGNATURES["vaek_mlp3_log_likelihood_replicas"] == _lib.SIGNATURES["vaek_log_likelihood_replicas"]      # one description
    assert _c_args(hdr, "vaek_mlp3_log_likelihood_workspace_bytes") == 5
    assert lib.vaek_mlp3_log_likelihood_max_columns() == 4194304 == 2 ** 22
    # the description's checks are the linear call's, as behaviour: refused by its size, before the context, with this entry's name
    check_description_guard(lib, "vaek_mlp3_log_likelihood_replicas")
    assert "mlp3_loglik.hip" in open(os.path.join(ROOT, "vae_training_amd", "csrc", "Makefile")).read()
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_mlp3_log_likelihood(None, 2, C.byref(yes)) == -1 and yes.value == 7
    b = C.c_size_t(7)
    assert lib.vaek_mlp3_log_likelihood_workspace_bytes(None, 1, 1, 1, C.byref(b)) == -1 and b.value == 7
    ll = _lib.VaekLogLikelihood()
    ll.struct_size = C.sizeof(_lib.VaekLogLikelihood)
    assert lib.vaek_mlp3_log_likelihood_replicas(None, None, C.byref(ll), 2, None, 3, 3, 3, 0.0, 3, 4, None, None) == -1
    assert b"vaek_mlp3_log_likelihood_replicas" in lib.vaek_last_error()


class _StubEngine:
    """What ReplicaLogLikMlp3 (and ReplicaLogLik) ask of an engine, on the CPU; records the library calls and fills the records."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    mlp3_log_likelihood_max_columns = 2 ** 22
    step_path = "stub"

    def __init__(self, mlp3=True, linear=False, D=6, L=6, world=1):
        self._mlp3, self._linear, self.D, self.L, self.world, self.calls, self.ws, self.lin_calls = mlp3, linear, D, L, world, [], [], []

    def supports_mlp3_log_likelihood(self, kind):
        return self._mlp3

    def supports_log_likelihood(self, kind):
        return self._linear

    def supports_train_loop_gen(self, kind):
        raise AssertionError("the log-likelihood does not ask a train loop's predicate: it has no batch-size condition")

    supports_stats_event = supports_train_step_replicas = supports_train_loop_gen

    def mlp3_log_likelihood_workspace(self, n, rows, samples):
        self.ws.append((n, rows, samples))
        return 16 * n * rows * samples

    def log_likelihood_workspace(self, n, rows):
        return 32 * n * ((rows + 255) // 256)

    def mlp3_log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.calls.append(dict(n=params.shape[0], rows=rows, samples=samples, z_seeds=z_seeds.tolist(), z_steps=z_steps.tolist(),
                               x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(), params=params.clone(),
                               A=None if kw["A"] is None else kw["A"].clone(), ws=workspace.numel(), kw=kw))
        for r in range(params.shape[0]):                 # record r: 100 r + slot
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float32)

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.lin_calls.append((params.shape[0], rows, samples))
        out.zero_()

    def loss_eval(self, *a, **kw):
        raise AssertionError("one log-likelihood call for all models, nothing else")

    forward = make_batch = stats_event_replicas = loss_eval


def _model(eng, P=4, kind=2, seed=1, B=100, key=(3, 4), dd=3):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    A = None if kind == 2 else torch.full((3,), float(seed))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, A, dd, 3, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def test_replica_loglik_mlp3_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaLogLik, ReplicaLogLikMlp3
    assert issubclass(ReplicaLogLikMlp3, ReplicaLogLik) and ReplicaLogLikMlp3.KEYS == ReplicaLogLik.KEYS == tuple(KEYS)
    assert (ReplicaLogLikMlp3.X_TAG, ReplicaLogLikMlp3.Z_TAG) == (3, 4)
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 256), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B, kind=1) for s, k, B in spec]
    ll = ReplicaLogLikMlp3(ms, 8)
    assert ll.R == 3 and ll.rows == 1000 and ll.samples == 8 and ll.params.shape == (3, 4) and ll.out.shape == (3, 4) and ll.a_stride == 3
    assert e.ws == [(3, 1000, 8)] and ll.workspace.numel() == 16 * 3 * 1000 * 8
    for event in range(2):
        stats = ll.event()
        assert len(e.calls) == event + 1 and e.lin_calls == []            # ONE library call for R models, and it is the mlp3 one
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["samples"] == 8 and c["kw"]["kind"] == 1 and c["kw"]["a_stride"] == 3
        assert c["kw"]["x_tag"] == 3 and c["kw"]["z_tag"] == 4
        want = [(s ^ 2) % 2 ** 64 for s, _, _ in spec]                    # dataset.key[0] ^ dataset.key[1]
        assert [s % 2 ** 64 for s in c["x_seeds"]] == want == [s % 2 ** 64 for s in c["z_seeds"]]
        assert c["x_steps"] == c["z_steps"] == [event + 1] * 3           # its own counter, incremented before use
        assert c["params"][:, 0].tolist() == [float(s) for s, _, _ in spec] and c["A"].shape == (3, 3)
        assert c["ws"] == ll.workspace.numel()
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m.dataset.key == (s, 2)      # the run is not perturbed
            assert m._loglik_draws == event + 1
            assert list(st) == KEYS
            assert [float(v) for v in st.values()] == [100.0 * r + j for j in (0, 1, 2)]
            assert len(m.average_log_likelihoods) == event + 1 and float(m.average_log_likelihoods[-1]) == 100.0 * r
            assert m.vae_losses == [] and m.var_enc == [] and m.var_dec == [] and m.current_epsilon == -3.0
    # a sphere model has no matrix; rows and samples are the caller's; the caps themselves are legal
    m = _model(e)
    ReplicaLogLikMlp3([m], 1024, rows=37).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["samples"] == 1024 and e.calls[-1]["A"] is None and e.calls[-1]["kw"]["a_stride"] == 0
    ReplicaLogLikMlp3([_model(e) for _ in range(4)], 1024, rows=1024)      # 4 x 1024 x 1024 = 2^22 columns


def test_replica_loglik_mlp3_refusals_and_the_linear_class_is_what_it_was():
    from vae_training_amd.trainer import ReplicaLogLik, ReplicaLogLikMlp3
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaLogLikMlp3([_model(e), _model(e, P=5)], 8)
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaLogLikMlp3([_model(e, kind=1), _model(e, kind=0)], 8)
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaLogLikMlp3([_model(e), _model(_StubEngine(D=9))], 8)
    with pytest.raises(RuntimeError, match="ReplicaLogLikMlp3: vaek_mlp3_log_likelihood_replicas does not cover.*step path: stub"):
        ReplicaLogLikMlp3([_model(_StubEngine(mlp3=False, linear=True))], 8)
    with pytest.raises(RuntimeError, match="ReplicaLogLikMlp3.*world"):
        ReplicaLogLikMlp3([_model(_StubEngine(world=2))], 8)
    with pytest.raises(RuntimeError, match="ReplicaLogLikMlp3 draws.*-dd / -did <= 16"):
        ReplicaLogLikMlp3([_model(e, dd=17)], 8)
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaLogLikMlp3([_model(e) for _ in range(1025)], 1, rows=1)
    with pytest.raises(RuntimeError, match="samples"):
        ReplicaLogLikMlp3([_model(e)], 1025)
    with pytest.raises(RuntimeError, match="samples"):
        ReplicaLogLikMlp3([_model(e)], 0)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaLogLikMlp3([_model(e)], 8, rows=4097)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaLogLikMlp3([_model(e)], 8, rows=0)
    with pytest.raises(RuntimeError, match=r"5 models x 1000 rows x 1024 samples = 5120000 columns, at most 4194304"):
        ReplicaLogLikMlp3([_model(e) for _ in range(5)], 1024)
    with pytest.raises(RuntimeError):
        ReplicaLogLikMlp3([], 8)
    assert e.calls == [] and e.ws == []
    # ReplicaLogLik on the same stub: its own predicate, its own call, its own messages, no column cap
    with pytest.raises(RuntimeError, match="ReplicaLogLik: vaek_log_likelihood_replicas does not cover.*step path: stub"):
        ReplicaLogLik([_model(e)], 8)
    lin = _StubEngine(mlp3=False, linear=True)
    ReplicaLogLik([_model(lin) for _ in range(5)], 1024).event()
    assert lin.lin_calls == [(5, 1000, 1024)] and lin.calls == [] and lin.ws == []


def test_the_stats_helper_adds_the_mlp3_log_likelihood_only_when_asked():
    """GenerativeModel._stats_event: compute_stats() alone without the attribute; with it, the three keys behind compute_stats' own."""
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_loglik_draws")
    m.mlp_log_likelihood_samples = 5
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["samples"] == 5 and e.calls[-1]["n"] == 1
        assert e.calls[-1]["z_steps"] == [event + 1] and len(m.average_log_likelihoods) == event + 1
    assert e.ws == [(1, 1000, 5)] and e.lin_calls == []                 # one ReplicaLogLikMlp3 for the run, not one per event


def test_run_py_parses_the_mlp_log_likelihood_flag(monkeypatch):
    from vae_training_amd import run
    base = ["sph", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes", "200|200|200"]
    assert run.parse_arguments(base).mlp_log_likelihood_samples is None      # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--mlp_log_likelihood_samples", "8"]).mlp_log_likelihood_samples == 8
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--mlp_log_likelihood_samples", "64"])
    assert a.mlp_log_likelihood_samples == 64 and a.sweep_dataset_seeds == [69, 24] and a.log_likelihood_samples is None
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--mlp_log_likelihood_samples", bad])
    # the model check: a model the predicate does not cover, a linear model, data parallelism, -dd above the generator's, the caps
    with pytest.raises(RuntimeError, match=r"--mlp_log_likelihood_samples needs .*step path: stub"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine(mlp3=False)), 8)
    with pytest.raises(RuntimeError, match=r"--mlp_log_likelihood_samples needs .*use --log_likelihood_samples.*step path: stub"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine(mlp3=False, linear=True)), 8)
    with pytest.raises(RuntimeError, match=r"--mlp_log_likelihood_samples needs .*world 2"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine(world=2)), 8)
    with pytest.raises(RuntimeError, match="--mlp_log_likelihood_samples needs"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine(), dd=17), 8)
    with pytest.raises(RuntimeError, match="at most 1024 samples.*step path: stub"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine()), 1025)
    with pytest.raises(RuntimeError, match=r"5 models x 1000 rows x 1024 samples = 5120000 columns, at most 4194304.*step path: stub"):
        run.check_mlp_log_likelihood_model(_model(_StubEngine()), 1024, 5)
    run.check_mlp_log_likelihood_model(_model(_StubEngine()), 1024, 4)
    run.check_mlp_log_likelihood_model(_model(_StubEngine()), 1024)
    # both flags together, and data parallelism: main() refuses before a process group or a directory exists
    with pytest.raises(RuntimeError, match="disjoint models"):
        run.main(run.parse_arguments(base + ["--mlp_log_likelihood_samples", "8", "--log_likelihood_samples", "8"]))
    with pytest.raises(RuntimeError, match="disjoint models"):
        run.main(run.parse_arguments(base + ["--mlp_log_likelihood_samples", "8", "--log_likelihood_samples", "8", "--sweep_dataset_seeds", "1,2"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--mlp_log_likelihood_samples", "8"]))
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--mlp_log_likelihood_samples", "8", "--sweep_dataset_seeds", "1,2"]))
