"""Host side of vaek_exact_log_likelihood_replicas, no GPU: the float64 restatement (tools/exact_log_likelihood_reference.py) against
an independent 60-digit evaluation on every case of tests/exact_loglik_cases.py, per row and within the bounds stated there; the C ABI
surface of the three entry points; trainer.ReplicaExactLogLik on a stub engine (one library call, its own counter, row tag 3, step=
honoured, the run untouched, what it refuses); the stats-event helper of model.py and run.py's --exact_log_likelihood flag.

The 60-digit evaluation costs about a millisecond per row and matrix side, so a case is checked on the first HOST_ROWS rows of its
set: a row's values do not depend on the row count (tests/test_gpu_exact_log_likelihood.py walks the row counts on the device)."""
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import exact_loglik_cases as K
from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ROWS = 32
NEW = ("vaek_supports_exact_log_likelihood", "vaek_exact_log_likelihood_record_len", "vaek_exact_log_likelihood_replicas")
FIELDS = ["struct_size", "n", "rows", "reserved", "state_stride", "x_seeds", "x_steps", "a_stride", "out", "out_stride", "x", "x_stride",
          "row_out", "row_stride"]
KEYS = ["Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning"]


@functools.lru_cache(maxsize=None)
def _ref():
    spec = importlib.util.spec_from_file_location("exact_log_likelihood_reference", os.path.join(ROOT, "tools", "exact_log_likelihood_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _evaluated(name, D, L, eps_cli):
    """(eps, the restatement's dict, the 60-digit log p, ELBO, gap and logdet) of a case's first HOST_ROWS rows; computed once."""
    X = _ref()
    p, _, _, eps = K.make_model(D, L, eps_cli)
    x = K.make_rows(p, eps, HOST_ROWS)
    return eps, X.evaluate(p, eps, x), X.high_precision(p, eps, x)


CASES = K.all_cases() + K.all_cases(ill=True)


@pytest.mark.parametrize("name,D,L,eps_cli", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_the_high_precision_evaluation(name, D, L, eps_cli):
    """Per row: |d log p| within the conditioning bound, |d ELBO| <= 2^-40 M, gap >= -(the two bounds); logdet within its bound."""
    if _ref().mp is None and eps_cli < -8.0:
        pytest.skip("mpmath is absent and scipy's float64 logpdf is only trusted for eps >= -8")
    eps, r, (lp, el, gap, ld) = _evaluated(name, D, L, eps_cli)
    b1 = K.logp_bound(D, r["quad"], r["logdet"], r["off"], r["norm"], eps)
    b2 = K.elbo_bound(r["M"])
    e1, e2 = np.abs(r["logp"] - lp), np.abs(r["elbo"] - el)
    print(f"{name}: sweeps {r['sweeps']} conditioning {r['cond']:.3e}; raw |d log p| {e1.max():.3e} = {np.max(e1 / b1):.5f} of its bound; "
          f"raw |d ELBO| {e2.max():.3e} = {np.max(e2 / b2):.5f} of 2^-40 M; min gap {r['gap'].min():.6e} (60-digit: {gap.min():.6e})")
    assert r["off"] <= 2.0 ** -43 * r["norm"] and r["sweeps"] < 32
    assert np.all(e1 <= b1), (e1 / b1).max()
    assert np.all(e2 <= b2), (e2 / b2).max()
    assert np.all(r["gap"] >= -(b1 + b2))
    assert abs(r["logdet"] - ld) <= K.logdet_bound(D, r["logdet"], r["off"], r["norm"], eps)
    assert np.all(gap >= 0.0)                                             # the truth is a KL divergence


def test_exact_posterior_model_has_no_gap():
    """An orthogonal-row decoder with the encoder set to its posterior: gap within the two bounds of 0 -- of the gap the model really
    has, which is not exactly 0 because its leaves are rounded to float32 (the 60-digit evaluation gives it; it is printed)."""
    X = _ref()
    p, _, _, eps = K.exact_posterior_model()
    x = K.make_rows(p, eps, HOST_ROWS)
    r = X.evaluate(p, eps, x)
    lp, el, gap, _ = X.high_precision(p, eps, x)
    D = x.shape[1]
    b = K.logp_bound(D, r["quad"], r["logdet"], r["off"], r["norm"], eps) + K.elbo_bound(r["M"])
    print(f"exact posterior: max |gap| {np.abs(r['gap']).max():.3e}, bounds from {b.min():.3e}, the float32 leaves' own gap {gap.max():.3e}")
    assert np.all(gap >= 0.0) and gap.max() <= 1e-12
    assert np.all(np.abs(r["gap"] - gap) <= b)
    assert np.all(np.abs(r["gap"]) <= b + gap)
    assert np.all(np.abs(r["logp"] - lp) <= b) and np.all(np.abs(r["elbo"] - el) <= b)


def test_record_layout_of_the_restatement():
    X = _ref()
    p, _, _, eps = K.make_model(7, 7, -0.8)
    x = K.make_rows(p, eps, 5)
    rec, r = X.record(p, eps, x), X.evaluate(p, eps, x)
    assert rec.shape == (10 + 7,) and rec[9] == 5 and rec[3] == eps and rec[5] == r["sweeps"]
    assert rec[0] == r["logp"].mean() and rec[1] == r["elbo"].mean() and rec[2] == r["gap"].mean()
    assert rec[8] == (rec[6] + 64 * 7 * 2.0 ** -53 * rec[7]) * np.exp(-eps)
    assert np.all(np.diff(rec[10:]) >= 0)
    g = p[K.KD].T @ p[K.KD]
    assert np.max(np.abs(rec[10:] - np.linalg.eigvalsh(g))) <= K.eig_bound(7, rec[6], rec[7])
    # G = 0: no sweep, logdet = D eps
    p0 = dict(p)
    p0[K.KD] = np.zeros_like(p[K.KD])
    r0 = X.evaluate(p0, eps, x)
    assert r0["sweeps"] == 0 and r0["off"] == 0.0 and abs(r0["logdet"] - 7 * eps) <= 1e-14


# ---- the C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_surface_of_the_exact_log_likelihood():
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct vaek_exact_log_likelihood \{(.*?)\} vaek_exact_log_likelihood;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekExactLogLikelihood._fields_] == FIELDS, fields
    assert _lib.EXACT_LOGLIK_RECORD_HEAD == 10
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_exact_log_likelihood(None, 1, C.byref(yes)) == -1 and yes.value == 7
    n = C.c_int64(7)
    assert lib.vaek_exact_log_likelihood_record_len(None, C.byref(n)) == -1 and n.value == 7
    ll = _lib.VaekExactLogLikelihood()
    ll.struct_size = C.sizeof(_lib.VaekExactLogLikelihood)
    assert lib.vaek_exact_log_likelihood_replicas(None, None, C.byref(ll), 1, None, 3, 1, 3, 0.0, 3, None) == -1
    assert b"vaek_exact_log_likelihood_replicas" in lib.vaek_last_error()


def test_struct_layout_matches_a_c_compiled_probe(tmp_path):
    from vae_training_amd import _lib
    probe = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vaek_exact_log_likelihood, {f}));' for f in FIELDS)
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaek.h"\nint main(void) {\n'
                     '    printf("sizeof %zu\\n", sizeof(vaek_exact_log_likelihood));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(_lib.VaekExactLogLikelihood) == 96
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_lib.VaekExactLogLikelihood, f).offset for f in FIELDS}


# ---- trainer.ReplicaExactLogLik on a stub engine ----------------------------------------------------------------------------------------
class _StubEngine:
    """What ReplicaExactLogLik (and ReplicaLogLik, for the combined event) asks of an engine, on the CPU; records the library calls."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    step_path = "stub"

    def __init__(self, covered=True, D=7, L=6, world=1, off=0.0):
        self._covered, self.D, self.L, self.world, self.off, self.calls, self.iwae = covered, D, L, world, off, [], []
        self.exact_log_likelihood_record_len = 10 + D

    def supports_exact_log_likelihood(self, kind):
        return self._covered

    def supports_log_likelihood(self, kind):
        return True

    def log_likelihood_workspace(self, n, rows):
        return 32 * n

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.iwae.append(dict(x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(), x_tag=kw["x_tag"], rows=rows))
        for r in range(params.shape[0]):
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float32)

    def exact_log_likelihood_replicas(self, params, rows, out, **kw):
        assert out.dtype == torch.float64 and out.shape == (params.shape[0], 10 + self.D)
        self.calls.append(dict(n=params.shape[0], rows=rows, x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(),
                               params=params.clone(), A=None if kw["A"] is None else kw["A"].clone(), kw=kw))
        for r in range(params.shape[0]):                 # record r: 1000 r + slot; off_F and |G|_F as the test asks
            out[r] = 1000.0 * r + torch.arange(out.shape[1], dtype=torch.float64)
            out[r, 6], out[r, 7] = self.off, 1.0

    def loss_eval(self, *a, **kw):
        raise AssertionError("one exact call for all models, nothing else")

    forward = make_batch = stats_event_replicas = supports_train_loop_gen = supports_stats_event = loss_eval


def _model(eng, P=4, kind=0, seed=1, B=100, key=(3, 4), dd=3):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 _loglik_draws=4, dirname="run_dir", model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def test_replica_exact_loglik_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaExactLogLik
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B) for s, k, B in spec]
    ex = ReplicaExactLogLik(ms)
    assert ex.R == 3 and ex.rows == 1000 and ex.params.shape == (3, 4) and ex.out.shape == (3, 17) and ex.out.dtype == torch.float64
    want_seeds = [(s ^ 2) % 2 ** 64 for s, _, _ in spec]                  # dataset.key[0] ^ dataset.key[1]
    for event in range(2):
        stats = ex.event()
        assert len(e.calls) == event + 1                                  # ONE library call for R models
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["kw"]["kind"] == 0 and c["kw"]["a_stride"] == 3
        assert c["kw"]["x_tag"] == 3                                      # ReplicaLogLik's row tag
        assert [s % 2 ** 64 for s in c["x_seeds"]] == want_seeds
        assert c["x_steps"] == [event + 1] * 3                            # its own counter, incremented before use
        assert c["params"][:, 0].tolist() == [float(s) for s, _, _ in spec] and c["A"].shape == (3, 3)
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 4 and m.dataset.key == (s, 2)
            assert m._exact_loglik_draws == event + 1
            assert list(st) == KEYS and all(isinstance(v, float) for v in st.values())
            assert list(st.values()) == [1000.0 * r + j for j in (0, 1, 2, 8)]
            assert m.average_log_likelihoods == [] and m.vae_losses == [] and m.current_epsilon == -3.0
    # step= draws under that step and leaves the counter alone; one step per model is accepted too
    ex.event(step=41)
    assert e.calls[-1]["x_steps"] == [41] * 3 and all(m._exact_loglik_draws == 2 for m in ms)
    ex.event(step=[7, 2 ** 31 + 8, 9])
    assert [s % 2 ** 32 for s in e.calls[-1]["x_steps"]] == [7, 2 ** 31 + 8, 9] and all(m._exact_loglik_draws == 2 for m in ms)
    with pytest.raises(RuntimeError, match="2 steps for 3 models"):
        ex.event(step=[1, 2])
    # rows are the caller's
    ReplicaExactLogLik([_model(e)], rows=37).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["n"] == 1


def test_replica_exact_loglik_with_the_iwae_event_scores_the_same_rows():
    from vae_training_amd.trainer import ReplicaExactLogLik, ReplicaLogLik
    e = _StubEngine()
    ms = [_model(e, seed=s) for s in (69, 24)]
    ll, ex = ReplicaLogLik(ms, 8), ReplicaExactLogLik(ms)
    ms[1]._loglik_draws = 11                                              # the two counters need not agree between models
    iw = ll.event()
    st = ex.event_after(iw)
    assert e.calls[-1]["x_steps"] == e.iwae[-1]["x_steps"] == [5, 12] and e.calls[-1]["x_seeds"] == e.iwae[-1]["x_seeds"]
    assert e.calls[-1]["kw"]["x_tag"] == e.iwae[-1]["x_tag"] == 3 and e.calls[-1]["rows"] == e.iwae[-1]["rows"]
    assert all(not hasattr(m, "_exact_loglik_draws") for m in ms)         # the step was given: the counter is not touched
    for r in range(2):
        assert list(st[r]) == KEYS + ["IWAE Gap"]
        assert st[r]["IWAE Gap"] == st[r]["Exact Log Likelihood"] - float(iw[r]["Average Log Likelihood"]) == 1000.0 * r - 100.0 * r
    assert list(ex.event_after(None)[0]) == KEYS and ms[0]._exact_loglik_draws == 1


def test_replica_exact_loglik_refusals():
    from vae_training_amd.trainer import ReplicaExactLogLik
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaExactLogLik([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaExactLogLik([_model(e), _model(e, kind=2)])
    with pytest.raises(RuntimeError, match="vaek_exact_log_likelihood_replicas does not cover.*ONE decoder.*step path: stub"):
        ReplicaExactLogLik([_model(_StubEngine(covered=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaExactLogLik([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="-dd / -did <= 16"):
        ReplicaExactLogLik([_model(e, dd=17)])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaExactLogLik([_model(e) for _ in range(1025)])
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match="rows"):
            ReplicaExactLogLik([_model(e)], rows=rows)
    with pytest.raises(RuntimeError):
        ReplicaExactLogLik([])
    assert e.calls == []
    # a solve that ended above 2^-40 of its norm names the model
    bad = _StubEngine(off=2.0 ** -39)
    with pytest.raises(RuntimeError, match=r"ReplicaExactLogLik: model 0 \(run_dir\).*off_F"):
        ReplicaExactLogLik([_model(bad)]).event()
    ReplicaExactLogLik([_model(_StubEngine(off=2.0 ** -41))]).event()


def test_the_stats_helper_adds_the_exact_keys_only_when_asked():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_exact_loglik_draws")
    m.exact_log_likelihood = True
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["x_steps"] == [event + 1]
    assert e.iwae == [] and m._loglik_draws == 4
    m.log_likelihood_samples = 8                                          # with the IWAE event: the same rows, and the gap between the two
    st = GenerativeModel._stats_event(m)
    assert list(st) == ["VAE Loss", "mse", "Average Log Likelihood", "ELBO estimate", "Effective Sample Size"] + KEYS + ["IWAE Gap"]
    assert e.calls[-1]["x_steps"] == e.iwae[-1]["x_steps"] == [5] and m._exact_loglik_draws == 2


def test_run_py_parses_the_exact_flag(monkeypatch):
    from vae_training_amd import run
    base = ["lin", "--dataset", "linear_gaussian"]
    assert run.parse_arguments(base).exact_log_likelihood is False       # opt-in: without the flag nothing changes
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--exact_log_likelihood", "--log_likelihood_samples", "64"])
    assert a.exact_log_likelihood is True and a.log_likelihood_samples == 64 and a.sweep_dataset_seeds == [69, 24]
    with pytest.raises(RuntimeError, match=r"--exact_log_likelihood needs .*ONE decoder.*step path: stub"):
        run.check_exact_log_likelihood_model(_model(_StubEngine(covered=False)))
    with pytest.raises(RuntimeError, match=r"--exact_log_likelihood needs .*world 2"):
        run.check_exact_log_likelihood_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match="--exact_log_likelihood needs"):
        run.check_exact_log_likelihood_model(_model(_StubEngine(), dd=17))
    run.check_exact_log_likelihood_model(_model(_StubEngine()))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--exact_log_likelihood needs .*does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--exact_log_likelihood"]))
