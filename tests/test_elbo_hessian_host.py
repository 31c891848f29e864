"""Host side of vaek_elbo_hvp_replicas and vaek_elbo_hessian_lanczos_replicas, no GPU: the float64 restatement
(tools/elbo_hessian_reference.py) against torch float64 autograd of f written row by row, on every case of tests/elbo_hessian_cases.py
-- f, the gradient, H v and the bound property of its Lanczos run against eigvalsh of the autograd Hessian; the C ABI surface of the
eight entry points and the layout of the two structs against a C-compiled probe; trainer.ReplicaElboHessian on a stub engine (one
library call, its own counter and tags, the run untouched, the exact event's rows, what it refuses); the stats-event helper of
model.py and run.py's --elbo_hessian flag."""
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

from tests import elbo_hessian_cases as K
from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_elbo_hessian", "vaek_elbo_hvp_max_vectors", "vaek_elbo_hvp_record_len", "vaek_elbo_hessian_max_steps",
       "vaek_elbo_hessian_record_len", "vaek_elbo_hessian_basis_doubles", "vaek_elbo_hvp_replicas", "vaek_elbo_hessian_lanczos_replicas")
ROWS_FIELDS = ["state_stride", "x_seeds", "x_steps", "a_stride", "x", "x_stride"]
HVP_FIELDS = ["struct_size", "n", "rows", "nvec"] + ROWS_FIELDS + ["v", "v_stride", "hv", "hv_stride", "grad", "grad_stride", "out", "out_stride"]
HESS_FIELDS = ["struct_size", "n", "rows", "steps"] + ROWS_FIELDS + ["v0", "v0_stride", "basis", "basis_stride", "out", "out_stride"]
KEYS = ["ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm"]


@functools.lru_cache(maxsize=None)
def _ref():
    spec = importlib.util.spec_from_file_location("elbo_hessian_reference", os.path.join(ROOT, "tools", "elbo_hessian_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _evaluated(name, rows):
    """(the restatement, its magnitude image, autograd's f, gradient, Hessian, its eigenvalues) of a case; computed once."""
    X, c = _ref(), K.BY_NAME[name]
    theta, x = K.make_theta(c), K.make_rows(c, rows)
    a = (theta, x, c.D, c.L, c.eps_cli, c.tdv)
    f, g, H = X.autograd(*a)
    return X.Model(*a), X.Model(*a, mag=True), f, g, H, np.linalg.eigvalsh(H)


CASE_ROWS = [(c.name, rows) for c in K.CASES for rows in c.rows]


@pytest.mark.parametrize("name,rows", CASE_ROWS, ids=[f"{n}_rows{r}" for n, r in CASE_ROWS])
def test_restatement_against_autograd(name, rows):
    """f, every element of the gradient and of H v on the GPU test's directions: within the GPU test's own bound of autograd."""
    c = K.BY_NAME[name]
    m, mg, f, g, H, _ = _evaluated(name, rows)
    V = K.directions(c)
    assert sorted(set(np.flatnonzero(V[3:].sum(axis=0)))) == sorted(K.first_elements(c)), "a unit vector per leaf"
    err, bound = np.abs(m.hvp(V) - V @ H), K.value_bound(c, rows, mg.hvp(V))
    gerr, gbound = np.abs(m.grad() - g), K.value_bound(c, rows, mg.grad())
    print(f"{name} rows {rows}: max|Hv - H_autograd v| / max|H v| {err.max() / np.max(np.abs(V @ H)):.2e}; worst share of the bound: Hv "
          f"{np.max(err[bound > 0] / bound[bound > 0]):.4f}, gradient {np.max(gerr[gbound > 0] / gbound[gbound > 0]):.4f}")
    assert np.all(err <= bound) and np.all(gerr <= gbound)
    assert abs(m.f() - f) <= K.value_bound(c, rows, mg.f())
    assert np.all(mg.hvp(V) >= np.abs(m.hvp(V))) and np.all(mg.grad() >= np.abs(m.grad())) and mg.f() >= abs(m.f())
    one = m.hvp(V[1])
    assert one.shape == (m.P,) and np.array_equal(one, m.hvp(V[1:2])[0])


@pytest.mark.parametrize("name,rows,steps", [(c.name, c.rows[0], s) for c in K.CASES for s in c.steps],
                         ids=[f"{c.name}_steps{s}" for c in K.CASES for s in c.steps])
def test_lanczos_of_the_restatement_has_the_bound_property(name, rows, steps):
    """Every Ritz value within rho_i + (64 P u + k omega) |H|_2 of an eigenvalue of the AUTOGRAD Hessian; omega <= 2^-40; T's
    eigenvalues are the Ritz values; the extremes inside the spectrum; on the two large cases the top Ritz value has converged."""
    X, c = _ref(), K.BY_NAME[name]
    m, _, _, _, H, lam = _evaluated(name, rows)
    P = m.P
    run = X.lanczos(m.hvp, K.start_vector(c), steps)
    k, th, rho = run["k"], run["theta"], run["rho"]
    norm_h = max(abs(lam[0]), abs(lam[-1]))
    assert 1 <= k <= min(steps, P) and run["omega"] <= K.OMEGA_MAX
    slack = K.ritz_slack(P, k, run["omega"], norm_h)
    gap = np.array([np.min(np.abs(lam - t)) for t in th])
    print(f"{name} steps {steps}: k {k}, omega {run['omega']:.2e}, theta_max {th[-1]:.6e} (rho {rho[-1]:.1e}), theta_min {th[0]:.6e}, "
          f"worst (gap - rho) / |H| {np.max(gap - rho) / norm_h:.2e}")
    assert np.all(gap <= rho + slack)
    assert th[-1] <= lam[-1] + slack and th[0] >= lam[0] - slack
    assert np.max(np.abs(np.linalg.eigvalsh(X.tridiagonal(run["alpha"], run["beta"])) - th)) <= 2.0 ** -40 * run["norm_t"]
    if name in ("D12_L20", "D32_L32"):
        assert rho[-1] <= 1e-8 * abs(th[-1])
    if name == "D2_L1":                                                   # the run spans the whole space: every Ritz value IS an eigenvalue
        assert k <= 8 and np.all(gap <= slack)
    if name == "D3_L2" and steps == 32:
        assert k < P, "this case ends by breakdown"
    rec = X.record(m, run)
    assert rec.shape == (140,) and rec[2] == k and rec[9] == th[-1] and rec[10] == th[0] and rec[7] == rows and rec[8] == c.eps_cli
    assert np.all(rec[12 + k:44] == 0) and np.array_equal(rec[12:12 + k], th) and np.array_equal(rec[108:108 + k], run["beta"])


def test_lanczos_edges_of_the_restatement():
    X, c = _ref(), K.BY_NAME["D3_L2"]
    m = _evaluated("D3_L2", 7)[0]
    run = X.lanczos(m.hvp, np.zeros(m.P), 5)
    assert run["k"] == 0 and run["theta"].size == 0 and np.all(X.record(m, run)[2:7] == 0) and np.all(X.record(m, run)[9:] == 0)
    one = X.lanczos(m.hvp, K.start_vector(c), 1)
    v = K.start_vector(c) / np.linalg.norm(K.start_vector(c))
    assert one["k"] == 1 and abs(one["theta"][0] - v @ m.hvp(v)) <= 1e-12 * abs(one["theta"][0]) and one["rho"][0] == one["beta"][0]


# ---- the C ABI surface ------------------------------------------------------------------------------------------------------------------
def test_abi_surface_of_the_elbo_hessian():
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    for struct, cls, want in (("vaek_elbo_hvp", _lib.VaekElboHvp, HVP_FIELDS), ("vaek_elbo_hessian", _lib.VaekElboHessian, HESS_FIELDS)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, flags=re.S).group(1)
        fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f[0] for f in cls._fields_] == want, fields
    assert lib.vaek_elbo_hvp_max_vectors() == 64 and lib.vaek_elbo_hvp_record_len() == 4
    assert lib.vaek_elbo_hessian_max_steps() == 32 == _lib.ELBO_HESSIAN_MAX_STEPS
    assert lib.vaek_elbo_hessian_record_len() == 140 == _lib.ELBO_HESSIAN_RECORD_HEAD + 4 * _lib.ELBO_HESSIAN_MAX_STEPS
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_elbo_hessian(None, 1, C.byref(yes)) == -1 and yes.value == 7
    n = C.c_int64(7)
    assert lib.vaek_elbo_hessian_basis_doubles(None, 4, C.byref(n)) == -1 and n.value == 7
    hp = _lib.VaekElboHvp()
    hp.struct_size = C.sizeof(_lib.VaekElboHvp)
    assert lib.vaek_elbo_hvp_replicas(None, None, C.byref(hp), 1, None, 3, 1, 3, 0.0, 3, None) == -1
    assert b"vaek_elbo_hvp_replicas" in lib.vaek_last_error()
    hs = _lib.VaekElboHessian()
    hs.struct_size = C.sizeof(_lib.VaekElboHessian)
    assert lib.vaek_elbo_hessian_lanczos_replicas(None, None, C.byref(hs), 1, None, 3, 1, 3, 0.0, 3, None) == -1
    assert b"vaek_elbo_hessian_lanczos_replicas" in lib.vaek_last_error()
    assert lib.vaek_elbo_hessian_lanczos_replicas(None, None, None, 1, None, 3, 1, 3, 0.0, 3, None) == -1


def test_struct_layouts_match_a_c_compiled_probe(tmp_path):
    from vae_training_amd import _lib
    lines = []
    for struct, fields in (("vaek_elbo_hvp", HVP_FIELDS), ("vaek_elbo_hessian", HESS_FIELDS)):
        lines.append(f'    printf("{struct}.sizeof %zu\\n", sizeof({struct}));')
        lines += [f'    printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaek.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for struct, cls, fields, size in (("vaek_elbo_hvp", _lib.VaekElboHvp, HVP_FIELDS, 128), ("vaek_elbo_hessian", _lib.VaekElboHessian, HESS_FIELDS, 112)):
        assert int(out[f"{struct}.sizeof"]) == C.sizeof(cls) == size
        assert {f: int(out[f"{struct}.{f}"]) for f in fields} == {f: getattr(cls, f).offset for f in fields}


# ---- trainer.ReplicaElboHessian on a stub engine ----------------------------------------------------------------------------------------
class _StubEngine:
    """What ReplicaElboHessian (and ReplicaExactLogLik / ReplicaLogLik, for the combined events) asks of an engine, on the CPU."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    elbo_hessian_max_steps = 32
    elbo_hessian_record_len = 140
    step_path = "stub"

    def __init__(self, covered=True, D=7, L=6, world=1, off=0.0, k=3):
        self._covered, self.D, self.L, self.world, self.off, self.k = covered, D, L, world, off, k
        self.calls, self.exact, self.iwae, self.fills = [], [], [], []
        self.exact_log_likelihood_record_len = 10 + D

    def supports_elbo_hessian(self, kind):
        return self._covered

    supports_exact_log_likelihood = supports_elbo_hessian

    def supports_log_likelihood(self, kind):
        return True

    def log_likelihood_workspace(self, n, rows):
        return 32 * n

    def rng_fill(self, n, seed, step=0, tag=0, bits=False):
        self.fills.append((n, seed % 2 ** 64, step, tag))
        return torch.full((n,), float(step), dtype=torch.float32)

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.iwae.append(dict(x_steps=kw["x_steps"].tolist(), x_tag=kw["x_tag"]))
        out.zero_()

    def exact_log_likelihood_replicas(self, params, rows, out, **kw):
        self.exact.append(dict(x_steps=kw["x_steps"].tolist(), x_seeds=kw["x_seeds"].tolist(), x_tag=kw["x_tag"], rows=rows))
        out.zero_()
        out[:, 7] = 1.0

    def elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, **kw):
        R, P = params.shape
        assert out.dtype == v0.dtype == basis.dtype == torch.float64 and out.shape == (R, 140)
        assert v0.shape == (R, P) and basis.shape == (R, steps, P)
        self.calls.append(dict(n=R, rows=rows, steps=steps, x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(), v0=v0.clone(),
                               params=params.clone(), A=None if kw["A"] is None else kw["A"].clone(), kw=kw))
        for r in range(R):                               # record r: 1000 r + slot; k Ritz values; off_F and |T|_F as the test asks
            out[r] = 1000.0 * r + torch.arange(140, dtype=torch.float64)
            out[r, 2], out[r, 5], out[r, 6] = self.k, self.off, 1.0

    def loss_eval(self, *a, **kw):
        raise AssertionError("one Lanczos call for all models, nothing else")

    forward = make_batch = stats_event_replicas = supports_train_loop_gen = supports_stats_event = loss_eval


def _model(eng, P=4, kind=0, seed=1, B=100, key=(3, 4), dd=3):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 _loglik_draws=4, _exact_loglik_draws=6, dirname="run_dir",
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def test_replica_elbo_hessian_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaElboHessian
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B) for s, k, B in spec]
    hs = ReplicaElboHessian(ms, steps=8)
    assert hs.R == 3 and hs.rows == 1000 and hs.steps == 8 and hs.params.shape == (3, 4) and hs.basis.shape == (3, 8, 4)
    assert hs.out.shape == (3, 140) and hs.out.dtype == hs.v0.dtype == torch.float64
    assert ReplicaElboHessian([_model(e)]).steps == 32
    want_seeds = [(s ^ 2) % 2 ** 64 for s, _, _ in spec]                  # dataset.key[0] ^ dataset.key[1]
    for event in range(2):
        stats = hs.event()
        assert len(e.calls) == event + 1                                  # ONE Lanczos call for R models
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["steps"] == 8 and c["kw"]["kind"] == 0 and c["kw"]["a_stride"] == 3
        assert c["kw"]["x_tag"] == 9                                      # its own row tag
        assert [s % 2 ** 64 for s in c["x_seeds"]] == want_seeds
        assert c["x_steps"] == [event + 1] * 3                            # its own counter, incremented before use
        assert e.fills[-3:] == [(4, s, event + 1, 10) for s in want_seeds]      # v0: vaek_rng_fill under that counter and tag 10 ...
        assert torch.equal(c["v0"], torch.full((3, 4), float(event + 1), dtype=torch.float64))      # ... widened
        assert c["params"][:, 0].tolist() == [float(s) for s, _, _ in spec] and c["A"].shape == (3, 3)
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 4 and m.dataset.key == (s, 2)
            assert m._exact_loglik_draws == 6 and m._elbo_hessian_draws == event + 1
            assert list(st) == KEYS and all(isinstance(st[k_], float) for k_ in KEYS[2:])
            assert st[KEYS[0]].tolist() == [1000.0 * r + 12 + j for j in range(3)] and st[KEYS[1]].tolist() == [1000.0 * r + 44 + j for j in range(3)]
            assert [st[k_] for k_ in KEYS[2:]] == [1000.0 * r + 9, 1000.0 * r + 10, 1000.0 * r + 1]
            assert m.average_log_likelihoods == [] and m.vae_losses == [] and m.current_epsilon == -3.0
    # step= draws the ROWS under that step and the exact event's row tag; the start vector stays under the own counter
    hs.event(step=41)
    assert e.calls[-1]["x_steps"] == [41] * 3 and e.calls[-1]["kw"]["x_tag"] == 3 and e.fills[-1][2:] == (3, 10)
    hs.event(step=[7, 2 ** 31 + 8, 9])
    assert [s % 2 ** 32 for s in e.calls[-1]["x_steps"]] == [7, 2 ** 31 + 8, 9]
    with pytest.raises(RuntimeError, match="2 steps for 3 models"):
        hs.event(step=[1, 2])
    ReplicaElboHessian([_model(e)], steps=1, rows=37).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["n"] == 1 and e.calls[-1]["steps"] == 1


def test_replica_elbo_hessian_after_the_exact_event_scores_the_same_rows():
    from vae_training_amd.trainer import ReplicaElboHessian, ReplicaExactLogLik, ReplicaLogLik
    e = _StubEngine()
    ms = [_model(e, seed=s) for s in (69, 24)]
    ex, hs = ReplicaExactLogLik(ms), ReplicaElboHessian(ms, 4)
    ex.event_after(None)
    hs.event_after(exact=True)
    assert e.calls[-1]["x_steps"] == e.exact[-1]["x_steps"] == [7, 7] and e.calls[-1]["x_seeds"] == e.exact[-1]["x_seeds"]
    assert e.calls[-1]["kw"]["x_tag"] == e.exact[-1]["x_tag"] == 3 and e.calls[-1]["rows"] == e.exact[-1]["rows"]
    ms[1]._loglik_draws = 11
    iw = ReplicaLogLik(ms, 8).event()
    ex.event_after(iw)
    hs.event_after(exact=True, iwae=True)
    assert e.calls[-1]["x_steps"] == e.exact[-1]["x_steps"] == e.iwae[-1]["x_steps"] == [5, 12]
    hs.event_after()
    assert e.calls[-1]["x_steps"] == [3, 3] and e.calls[-1]["kw"]["x_tag"] == 9 and all(m._elbo_hessian_draws == 3 for m in ms)


def test_replica_elbo_hessian_refusals():
    from vae_training_amd.trainer import ReplicaElboHessian
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaElboHessian([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaElboHessian([_model(e), _model(e, kind=2)])
    with pytest.raises(RuntimeError, match="vaek_elbo_hessian_lanczos_replicas does not cover.*ONE decoder.*step path: stub"):
        ReplicaElboHessian([_model(_StubEngine(covered=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaElboHessian([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="-dd / -did <= 16"):
        ReplicaElboHessian([_model(e, dd=17)])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaElboHessian([_model(e) for _ in range(1025)])
    for rows in (0, 4097):
        with pytest.raises(RuntimeError, match="rows"):
            ReplicaElboHessian([_model(e)], rows=rows)
    for steps in (0, 33):
        with pytest.raises(RuntimeError, match="Lanczos steps, need 1 .. 32"):
            ReplicaElboHessian([_model(e)], steps=steps)
    with pytest.raises(RuntimeError):
        ReplicaElboHessian([])
    assert e.calls == [] and e.fills == []
    # a solve that ended above 2^-40 of its norm names the model
    with pytest.raises(RuntimeError, match=r"ReplicaElboHessian: model 0 \(run_dir\).*off_F"):
        ReplicaElboHessian([_model(_StubEngine(off=2.0 ** -39))]).event()
    ReplicaElboHessian([_model(_StubEngine(off=2.0 ** -41))]).event()
    # k = 1 still gives arrays; k = 0 empty ones
    for k in (1, 0):
        st = ReplicaElboHessian([_model(_StubEngine(k=k))]).event()[0]
        assert st[KEYS[0]].shape == st[KEYS[1]].shape == (k,)


def test_the_stats_helper_adds_the_hessian_keys_only_when_asked():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_elbo_hessian_draws")
    m.elbo_hessian = 8
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1
        assert e.calls[-1]["x_steps"] == [event + 1] and e.calls[-1]["steps"] == 8 and e.calls[-1]["kw"]["x_tag"] == 9
    assert e.exact == [] and m._exact_loglik_draws == 6
    m.exact_log_likelihood = True                                         # with the exact event: the same rows
    st = GenerativeModel._stats_event(m)
    assert list(st)[:2] == ["VAE Loss", "mse"] and list(st)[-5:] == KEYS and "Exact ELBO" in st
    assert e.calls[-1]["x_steps"] == e.exact[-1]["x_steps"] == [7] and e.calls[-1]["kw"]["x_tag"] == 3 and m._elbo_hessian_draws == 3
    # write_stats keeps the two arrays as arrays whatever k is and puts the three floats on the line
    lines = []
    w = types.SimpleNamespace(batchnum=0, stats={k: [] for k in KEYS}, _write=lines.append)
    GenerativeModel.write_stats(w, {KEYS[0]: np.array([2.5]), KEYS[1]: np.array([0.5]), KEYS[2]: 2.5, KEYS[3]: 2.5, KEYS[4]: 0.25})
    assert isinstance(w.stats[KEYS[0]][0], np.ndarray) and w.stats[KEYS[2]] == [2.5]
    assert lines == ["Batch | 0 | Sharpness | 2.500 | ELBO Hessian Min Ritz | 2.500 | ELBO Gradient Norm | 0.250"]


def test_run_py_parses_the_hessian_flag(monkeypatch):
    from vae_training_amd import run
    base = ["lin", "--dataset", "linear_gaussian"]
    assert run.parse_arguments(base).elbo_hessian is None                 # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--elbo_hessian"]).elbo_hessian == 32
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--elbo_hessian", "8", "--exact_log_likelihood"])
    assert a.elbo_hessian == 8 and a.exact_log_likelihood is True and a.sweep_dataset_seeds == [69, 24]
    for bad in ("0", "33", "x"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--elbo_hessian", bad])
    with pytest.raises(RuntimeError, match=r"--elbo_hessian needs .*ONE decoder.*step path: stub"):
        run.check_elbo_hessian_model(_model(_StubEngine(covered=False)))
    with pytest.raises(RuntimeError, match=r"--elbo_hessian needs .*world 2"):
        run.check_elbo_hessian_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match="--elbo_hessian needs"):
        run.check_elbo_hessian_model(_model(_StubEngine(), dd=17))
    run.check_elbo_hessian_model(_model(_StubEngine()))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--elbo_hessian needs .*does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--elbo_hessian"]))
