"""Host side of vaek_mlp3_decoder_jacobian_replicas, no GPU: the C ABI surface of the six entry points (declared, bound, exported,
argument counts, the cap, refusals that need no device), trainer.ReplicaJacobianMlp3 on a stub engine (one library call for R models,
its own seeds, steps and tags, the run's RNG state untouched, posterior mode's make_batch -> forward -> explicit call, what it refuses),
the stats-event helper and stats line of model.py and run.py's --decoder_jacobian / --decoder_jacobian_tol flags."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vaek_supports_mlp3_decoder_jacobian": 2, "vaek_decoder_jacobian_record_len": 2, "vaek_decoder_jacobian_row_record_len": 2,
       "vaek_mlp3_decoder_jacobian_max_columns": 0, "vaek_mlp3_decoder_jacobian_workspace_bytes": 4, "vaek_mlp3_decoder_jacobian_replicas": 6}
KEYS = ["Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"]


def test_abi_surface_of_the_decoder_jacobian():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols; the cap; argument checks that need no device."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name, nargs in NEW.items():
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.vaek_mlp3_decoder_jacobian_max_columns() == 1048576 == 2 ** 20
    # the ctypes struct is the header's: the same fields in the same order, doubles and pointers 8 bytes wide
    body = re.search(r"typedef struct vaek_decoder_jacobian \{(.*?)\} vaek_decoder_jacobian;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);\s*/\*", body)
    assert fields == [f for f, _ in _lib.VaekDecoderJacobian._fields_], fields
    assert C.sizeof(_lib.VaekDecoderJacobian) == 16 + 8 * 10
    csrc = os.path.join(ROOT, "vae_training_amd", "csrc")
    assert "mlp3_jacobian.hip" in open(os.path.join(csrc, "Makefile")).read()
    unit = open(os.path.join(csrc, "mlp3_jacobian.hip")).read()
    assert '#include "mlp3_dev.h"' in unit and '#include "eigen_dev.h"' in unit and "jacobi_solve<false>" in unit and "ml_dense<" in unit
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_mlp3_decoder_jacobian(None, C.byref(yes)) == -1 and yes.value == 7
    assert b"vaek_supports_mlp3_decoder_jacobian" in lib.vaek_last_error()
    n = C.c_int64(7)
    for fn in (lib.vaek_decoder_jacobian_record_len, lib.vaek_decoder_jacobian_row_record_len):
        assert fn(None, C.byref(n)) == -1 and n.value == 7
    b = C.c_size_t(7)
    assert lib.vaek_mlp3_decoder_jacobian_workspace_bytes(None, 1, 1, C.byref(b)) == -1 and b.value == 7
    assert b"vaek_mlp3_decoder_jacobian_workspace_bytes" in lib.vaek_last_error()
    dj = _lib.VaekDecoderJacobian()
    dj.struct_size = C.sizeof(_lib.VaekDecoderJacobian)
    assert lib.vaek_mlp3_decoder_jacobian_replicas(None, None, C.byref(dj), 8, None, None) == -1
    assert b"vaek_mlp3_decoder_jacobian_replicas: null context" in lib.vaek_last_error()
    dj.struct_size -= 8                                  # another header's description: refused by its size, before the context is read
    assert lib.vaek_mlp3_decoder_jacobian_replicas(None, None, C.byref(dj), 8, None, None) == -1
    err = lib.vaek_last_error()
    assert b"vaek_mlp3_decoder_jacobian_replicas" in err and b"struct_size 88 != 96" in err, err
    assert lib.vaek_mlp3_decoder_jacobian_replicas(None, None, None, 8, None, None) == -1
    assert b"vaek_mlp3_decoder_jacobian_replicas: null description" in lib.vaek_last_error()


class _StubEngine:
    """What ReplicaJacobianMlp3 asks of an engine, on the CPU; records the library calls in order and fills the records."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    stats_event_max_rows = 4096
    mlp3_decoder_jacobian_max_columns = 2 ** 20
    step_path = "stub"

    def __init__(self, mlp3=True, linear=False, D=6, L=6, world=1):
        self._mlp3, self._linear, self.D, self.L, self.world, self.calls, self.ws, self.log = mlp3, linear, D, L, world, [], [], []

    decoder_jacobian_record_len = property(lambda self: 2 * self.L + 8)
    decoder_jacobian_row_record_len = property(lambda self: 2 * self.L + 4)

    def supports_mlp3_decoder_jacobian(self):
        return self._mlp3

    def supports_log_likelihood(self, kind):
        return self._linear

    def supports_train_loop_gen(self, kind):
        raise AssertionError("the decoder Jacobian does not ask a train loop's predicate: it has no batch-size condition")

    supports_stats_event = supports_train_step_replicas = supports_mlp3_log_likelihood = supports_train_loop_gen

    def mlp3_decoder_jacobian_workspace(self, n, rows):
        self.ws.append((n, rows))
        return 64 * n * rows

    def make_batch(self, kind, A, dd, did, pad, var, rows, seed, **kw):
        self.log.append(("make_batch", seed % 2 ** 64, kw["step"], kw["tag"], rows))
        return torch.full((rows, self.D), 1.0), torch.zeros(rows, self.L), torch.zeros(rows, self.D)

    def forward(self, params, x, z1, z2, sampling=False, want_mu=True, **kw):
        assert not sampling and want_mu
        self.log.append(("forward", float(params[0]), x.shape[0]))
        return None, torch.full((x.shape[0], self.L), float(params[0]))      # mu: the model's mark

    def mlp3_decoder_jacobian_replicas(self, params, rows, out, workspace, **kw):
        self.log.append(("jacobian",))
        z = kw.get("z")
        self.calls.append(dict(n=params.shape[0], rows=rows, params=params.clone(), ws=workspace.numel(), kw=kw,
                               z=None if z is None else z.clone(),
                               z_seeds=None if kw.get("z_seeds") is None else kw["z_seeds"].tolist(),
                               z_steps=None if kw.get("z_steps") is None else kw["z_steps"].tolist()))
        for r in range(params.shape[0]):                 # record r: 100 r + slot; slot [6] is the solve's ratio
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float64)
            out[r, 6] = self.ratio if hasattr(self, "ratio") else 2.0 ** -50

    def loss_eval(self, *a, **kw):
        raise AssertionError("one decoder-Jacobian call for all models, nothing else")

    stats_event_replicas = mlp3_log_likelihood_replicas = loss_eval


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


def test_replica_jacobian_prior_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaJacobianMlp3
    assert ReplicaJacobianMlp3.KEYS == tuple(KEYS) and (ReplicaJacobianMlp3.X_TAG, ReplicaJacobianMlp3.Z_TAG) == (7, 8)
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 256), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B, kind=1) for s, k, B in spec]
    jac = ReplicaJacobianMlp3(ms)
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
    with pytest.raises(RuntimeError, match=r"ReplicaJacobianMlp3: model 0 .*solve of J\^T J"):
        jac.event()
    del e.ratio
    # rows and threshold are the caller's; the cap itself is legal
    e2 = _StubEngine(L=32)
    ReplicaJacobianMlp3([_model(e2) for _ in range(8)], rows=4096, rank_tol=0.0)        # 8 x 4096 x 32 = 2^20 columns
    ReplicaJacobianMlp3([_model(e)], rows=37, rank_tol=0.25).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["kw"]["rank_tol"] == 0.25


def test_replica_jacobian_posterior_draws_encodes_and_passes_explicit_rows():
    from vae_training_amd.trainer import ReplicaJacobianMlp3
    e = _StubEngine()
    spec = [(69, (3, 4)), (24, (7, 8))]
    ms = [_model(e, seed=s, key=k) for s, k in spec]
    jac = ReplicaJacobianMlp3(ms, rows=5, at="posterior", rank_tol=1e-3)
    for event in range(2):
        e.log.clear()
        jac.event()
        # per model make_batch -> forward under the class's row tag and counter, then ONE explicit call
        assert e.log == [("make_batch", 69 ^ 2, event + 1, 7, 5), ("forward", 69.0, 5), ("make_batch", 24 ^ 2, event + 1, 7, 5),
                         ("forward", 24.0, 5), ("jacobian",)]
        c = e.calls[-1]
        assert c["z_seeds"] is None and c["z_steps"] is None and c["z"].shape == (2, 5, 6) and c["kw"]["rank_tol"] == 1e-3
        assert (c["z"][0] == 69.0).all() and (c["z"][1] == 24.0).all()                      # mu of the library's own forward
        assert all(_untouched(m, s, k) and m._jacobian_draws == event + 1 for m, (s, k) in zip(ms, spec))
    assert len(e.calls) == 2


def test_replica_jacobian_refusals():
    from vae_training_amd.trainer import ReplicaJacobianMlp3
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaJacobianMlp3([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaJacobianMlp3([_model(e, kind=1), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaJacobianMlp3([_model(e), _model(_StubEngine(D=9))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianMlp3: vaek_mlp3_decoder_jacobian_replicas does not cover.*step path: stub"):
        ReplicaJacobianMlp3([_model(_StubEngine(mlp3=False, linear=True))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianMlp3.*world"):
        ReplicaJacobianMlp3([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="ReplicaJacobianMlp3 draws.*-dd / -did <= 16"):
        ReplicaJacobianMlp3([_model(e, dd=17)])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaJacobianMlp3([_model(e) for _ in range(1025)], rows=1)
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match="rows"):
            ReplicaJacobianMlp3([_model(e)], rows=rows)
    with pytest.raises(RuntimeError, match=r"44 models x 4096 rows x 6 latents = 1081344 columns, at most 1048576"):
        ReplicaJacobianMlp3([_model(e) for _ in range(44)], rows=4096)
    with pytest.raises(RuntimeError, match="at="):
        ReplicaJacobianMlp3([_model(e)], at="encoder")
    for tol in (-0.1, 1.0, float("nan")):
        with pytest.raises(RuntimeError, match="rank_tol"):
            ReplicaJacobianMlp3([_model(e)], rank_tol=tol)
    with pytest.raises(RuntimeError):
        ReplicaJacobianMlp3([])
    assert e.calls == [] and e.ws == []


def test_the_stats_helper_adds_the_jacobian_only_when_asked_and_the_line_shows_the_mean_rank(capsys):
    """GenerativeModel._stats_event: compute_stats() alone without the attribute; with it, the three keys behind compute_stats' own;
    write_stats keeps the arrays (L = 1 included) and prints the mean rank."""
    import collections

    from vae_training_amd.model import JACOBIAN_KEYS, GenerativeModel
    assert list(JACOBIAN_KEYS) == KEYS
    e = _StubEngine(L=1)
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_jacobian_draws")
    m.decoder_jacobian, m.decoder_jacobian_tol = "prior", 1e-3
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["n"] == 1
        assert e.calls[-1]["z_steps"] == [event + 1] and e.calls[-1]["kw"]["rank_tol"] == 1e-3
    assert e.ws == [(1, 1000)]                            # one ReplicaJacobianMlp3 for the run, not one per event
    m.stats, m.batchnum, m.tqdm, m.rank = collections.defaultdict(list), 0, False, 0
    m._write = lambda msg: GenerativeModel._write(m, msg)
    GenerativeModel.write_stats(m, st)
    line = capsys.readouterr().out
    assert "| Decoder Jacobian Rank (mean) | 1.000" in line and "VAE Loss | 1.000" in line
    assert [np.asarray(m.stats[k][0]).shape for k in KEYS] == [(1,), (3,), (1,)]


def test_run_py_parses_the_decoder_jacobian_flags(monkeypatch):
    from vae_training_amd import run
    base = ["sph", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes", "200|200|200"]
    a = run.parse_arguments(base)
    assert a.decoder_jacobian is None and a.decoder_jacobian_tol is None       # opt-in: without the flag nothing changes
    a = run.parse_arguments(base + ["--decoder_jacobian", "prior"])
    assert a.decoder_jacobian == "prior" and run.decoder_jacobian_tol(a) == 1e-4
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--decoder_jacobian", "posterior", "--decoder_jacobian_tol", "1e-3",
                                    "--mlp_fused_stats", "--mlp_log_likelihood_samples", "8"])
    assert a.decoder_jacobian == "posterior" and run.decoder_jacobian_tol(a) == 1e-3 and a.mlp_fused_stats and a.mlp_log_likelihood_samples == 8
    for bad in (["--decoder_jacobian", "encoder"], ["--decoder_jacobian"], ["--decoder_jacobian", "prior", "--decoder_jacobian_tol", "1"],
                ["--decoder_jacobian", "prior", "--decoder_jacobian_tol", "-1e-3"], ["--decoder_jacobian", "prior", "--decoder_jacobian_tol", "x"]):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + bad)
    # the model check: a model the predicate does not cover, a linear model, data parallelism, -dd above the generator's, the cap
    with pytest.raises(RuntimeError, match=r"--decoder_jacobian needs .*step path: stub"):
        run.check_decoder_jacobian_model(_model(_StubEngine(mlp3=False)))
    with pytest.raises(RuntimeError, match=r"--decoder_jacobian needs .*use --exact_log_likelihood.*K\^T K.*step path: stub"):
        run.check_decoder_jacobian_model(_model(_StubEngine(mlp3=False, linear=True)))
    with pytest.raises(RuntimeError, match=r"--decoder_jacobian needs .*world 2"):
        run.check_decoder_jacobian_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match="--decoder_jacobian needs"):
        run.check_decoder_jacobian_model(_model(_StubEngine(), dd=17))
    with pytest.raises(RuntimeError, match=r"33 models x 1000 rows x 32 latents = 1056000 columns, at most 1048576.*step path: stub"):
        run.check_decoder_jacobian_model(_model(_StubEngine(L=32)), 33)
    run.check_decoder_jacobian_model(_model(_StubEngine(L=32)), 32)
    run.check_decoder_jacobian_model(_model(_StubEngine()))
    # the threshold without the flag, and data parallelism: main() refuses before a process group or a directory exists
    for extra in ([], ["--sweep_dataset_seeds", "1,2"]):
        with pytest.raises(RuntimeError, match="--decoder_jacobian_tol sets the rank threshold of --decoder_jacobian"):
            run.main(run.parse_arguments(base + ["--decoder_jacobian_tol", "1e-3"] + extra))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--decoder_jacobian", "prior"]))
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--decoder_jacobian", "prior", "--sweep_dataset_seeds", "1,2"]))
