"""The sampled-ELBO Hessian (csrc/sampled_hessian.hip) from the host, no GPU: the float64 restatement
tools/sampled_hessian_reference.py against torch autograd of an independent statement of f_K under the bound the GPU tests use, against
the exact restatement on the sigma-point cases, the symmetry of its dense Hessian; trainer.ReplicaSampledElboHessian, the table row,
run.py's flags, refusals and banners on a stub engine; the ABI mirrors and the description guards of the two entry points."""
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

from tests import sampled_hessian_cases as K
from tests.abi_util import check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["Sampled ELBO Hessian Ritz Values", "Sampled ELBO Hessian Ritz Residuals", "Sampled Sharpness", "Sampled ELBO Hessian Min Ritz",
        "Sampled ELBO Gradient Norm"]
EXTRA_FIELDS = ["samples", "reserved", "z_seeds", "z_steps", "xi", "xi_stride"]
ENTRIES = ("vaek_sampled_elbo_hvp_replicas", "vaek_sampled_elbo_hessian_lanczos_replicas")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _ref():
    return _tool("sampled_hessian_reference")


@functools.lru_cache(maxsize=None)
def _models(name, rows):
    c = K.BY_NAME[name]
    a = (K.make_theta(c), K.make_rows(c, rows), K.make_samples(c, rows), c.D, c.L, c.eps_cli, c.tdv, c.sig)
    return _ref().Model(*a), _ref().Model(*a, mag=True), a


CASE_ROWS = [(c.name, rows) for c in K.CASES for rows in c.rows]


# ---- 1. the restatement against torch autograd, under the bound of the GPU tests ---------------------------------------------------------
@pytest.mark.parametrize("name,rows", CASE_ROWS)
def test_the_restatement_matches_autograd_within_the_value_bound(name, rows):
    c = K.BY_NAME[name]
    m, mg, a = _models(name, rows)
    V = K.directions(c)
    assert m.P == K.param_count(c) == _ref().param_count(c.D, c.L, c.tdv, c.sig) and V.shape == (3 + len(K.first_elements(c)), m.P)
    f, g, hv, _ = _ref().autograd(*a, V=V)
    ratios = (K.worst_ratio(m.f() - f, K.value_bound(c, rows, mg.f())), K.worst_ratio(m.grad() - g, K.value_bound(c, rows, mg.grad())),
              K.worst_ratio(m.hvp(V) - hv, K.value_bound(c, rows, mg.hvp(V))))
    print(f"{name} rows {rows}: |restatement - autograd| / bound: f {ratios[0]:.3e}  gradient {ratios[1]:.3e}  H v {ratios[2]:.3e}")
    assert max(ratios) <= 1.0 / 8.0                                       # the bound has 8x room over honest float64 in another order
    assert np.all(mg.hvp(V) >= np.abs(m.hvp(V)) * (1.0 - 1e-12)) and mg.f() >= abs(m.f()) and np.all(mg.grad() >= np.abs(m.grad()) * (1.0 - 1e-12))


# ---- 2. sigma points: f_K is the exact f, identically in theta ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in K.SIGMA_CASES])
def test_sigma_points_reproduce_the_exact_restatement(name):
    c = K.BY_NAME[name]
    rows = c.rows[0]
    m, mg, a = _models(name, rows)
    ex = _tool("elbo_hessian_reference")
    b = (a[0], a[1], c.D, c.L, c.eps_cli, c.tdv)
    e, eg = ex.Model(*b), ex.Model(*b, mag=True)
    V = K.directions(c)
    both = lambda s, x: K.value_bound(c, rows, s) + K.exact_value_bound(c, rows, x)
    ratios = (K.worst_ratio(m.f() - e.f(), both(mg.f(), eg.f())), K.worst_ratio(m.grad() - e.grad(), both(mg.grad(), eg.grad())),
              K.worst_ratio(m.hvp(V) - e.hvp(V), both(mg.hvp(V), eg.hvp(V))))
    print(f"{name}: |sampled - exact| / (sum of the bounds): f {ratios[0]:.3e}  gradient {ratios[1]:.3e}  H v {ratios[2]:.3e}")
    assert max(ratios) <= 1.0


# ---- 3. the dense Hessian is symmetric -------------------------------------------------------------------------------------------------------
def test_the_dense_hessian_is_symmetric():
    c = K.BY_NAME["D4_L2s"]
    for rows in c.rows:
        m, mg, _ = _models(c.name, rows)
        H, M = m.hessian(), mg.hessian()
        assert H.shape == (37, 37)
        assert K.worst_ratio(H - H.T, K.value_bound(c, rows, M) + K.value_bound(c, rows, M.T)) <= 1.0
        lam = np.linalg.eigvalsh(0.5 * (H + H.T))
        assert lam[0] < 0.0 < lam[-1]                                     # a random point is a saddle: the spectrum tests see both signs


def test_the_cases_are_the_issues():
    assert [(c.name, c.D, c.L, c.sig, c.rows, c.K, c.steps) for c in K.CASES] == [
        ("D2_L1", 2, 1, False, (5,), 2, (32,)), ("D4_L2s", 4, 2, True, (7, 1), 3, (5, 32)), ("D5_L4", 5, 4, False, (7,), 8, (32,)),
        ("D13_L5s", 13, 5, True, (300,), 5, (32,)), ("D32_L16", 32, 16, False, (40,), 32, (32,)), ("D28_L32s", 28, 32, True, (64,), 8, (32,)),
        ("D28_L24s", 28, 24, True, (1000,), 8, (32,))]
    assert [c.name for c in K.SIGMA_CASES] == ["D2_L1", "D5_L4", "D32_L16"] and K.param_count(K.BY_NAME["D28_L32s"]) == 2809
    for c in K.SIGMA_CASES:
        xi = K.make_samples(c, 3)
        assert np.allclose(xi.mean(axis=1), 0.0) and np.array_equal(np.einsum("rkl,rkm->rlm", xi, xi) / c.K, np.broadcast_to(np.eye(c.L), (3, c.L, c.L)))
    c = K.BY_NAME["D13_L5s"]
    assert np.array_equal(K.make_rows(c, 300)[:7], K.make_rows(c, 7)) and np.array_equal(K.make_samples(c, 300)[:7], K.make_samples(c, 7))
    assert K.value_bound(c, 300, 1.0) == 64.0 * (1500 + 26 + 10) * 2.0 ** -53


# ---- 4. trainer.ReplicaSampledElboHessian, the table row and run.py on a stub engine ----------------------------------------------------
class _StubEngine:
    """What ReplicaSampledElboHessian (and the events it couples with) asks of an engine, on the CPU."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    elbo_hessian_max_steps = 32
    elbo_hessian_record_len = 140
    sampled_elbo_hessian_record_len = 142
    sampled_elbo_hessian_max_columns = 1 << 22
    step_path = "stub"

    def __init__(self, covered=True, one_decoder=True, D=7, L=6, world=1, off=0.0, k=3):
        self._covered, self.one, self.D, self.L, self.world, self.off, self.k = covered, one_decoder, D, L, world, off, k
        self.calls, self.exact_h, self.exact, self.fills, self.ws = [], [], [], [], []
        self.exact_log_likelihood_record_len = 10 + D

    def supports_sampled_elbo_hessian(self, kind):
        return self._covered

    supports_log_likelihood = supports_sampled_elbo_hessian

    def supports_elbo_hessian(self, kind):
        return self._covered and self.one

    supports_exact_log_likelihood = supports_elbo_hessian

    def sampled_elbo_hessian_workspace(self, n, rows, samples):
        self.ws.append((n, rows, samples))
        return 64 * n

    def rng_fill(self, n, seed, step=0, tag=0, bits=False):
        self.fills.append((n, seed % 2 ** 64, step, tag))
        return torch.full((n,), float(step), dtype=torch.float32)

    def exact_log_likelihood_replicas(self, params, rows, out, **kw):
        self.exact.append(dict(x_steps=kw["x_steps"].tolist(), x_tag=kw["x_tag"]))
        out.zero_()
        out[:, 7] = 1.0

    def elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, **kw):
        self.exact_h.append(dict(x_steps=kw["x_steps"].tolist(), x_seeds=kw["x_seeds"].tolist(), x_tag=kw["x_tag"], rows=rows))
        out.zero_()
        out[:, 2], out[:, 6], out[:, 9] = 3, 1.0, 100.0

    def sampled_elbo_hessian_lanczos_replicas(self, params, rows, steps, v0, basis, out, workspace, **kw):
        R, P = params.shape
        assert out.dtype == v0.dtype == basis.dtype == torch.float64 and out.shape == (R, 142) and workspace.dtype == torch.uint8
        assert v0.shape == (R, P) and basis.shape == (R, steps, P) and workspace.numel() == 64 * R
        self.calls.append(dict(n=R, rows=rows, steps=steps, samples=kw["samples"], x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(),
                               z_seeds=kw["z_seeds"].tolist(), z_steps=kw["z_steps"].tolist(), v0=v0.clone(), params=params.clone(), kw=kw))
        for r in range(R):                               # record r: 1000 r + slot; k Ritz values; off_F and |T|_F as the test asks
            out[r] = 1000.0 * r + torch.arange(142, dtype=torch.float64)
            out[r, 2], out[r, 5], out[r, 6] = self.k, self.off, 1.0


def _model(eng, P=4, kind=0, seed=1, B=100, key=(3, 4), dd=3, rows=1000, **flags):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb=None: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=rows, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 _loglik_draws=4, _exact_loglik_draws=6, dirname="run_dir", compute_stats=lambda: {"VAE Loss": 1.0, "mse": 2.0},
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))), **flags)


def test_the_event_makes_one_call_under_its_own_counter_and_tags():
    from vae_training_amd import events
    from vae_training_amd.trainer import ReplicaSampledElboHessian
    assert ReplicaSampledElboHessian is events.ReplicaSampledElboHessian and list(ReplicaSampledElboHessian.KEYS) == KEYS
    assert (ReplicaSampledElboHessian.X_TAG, ReplicaSampledElboHessian.Z_TAG, ReplicaSampledElboHessian.V_TAG) == (11, 12, 13)
    assert ReplicaSampledElboHessian.COUNTER == "_sampled_hessian_draws"
    e = _StubEngine(one_decoder=False)
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257), (48, (5, 2 ** 64 - 1), 65536)]
    ms = [_model(e, seed=s, key=k, B=B) for s, k, B in spec]
    hs = ReplicaSampledElboHessian(ms, steps=8, samples=5)
    assert hs.R == 3 and hs.rows == 1000 and hs.steps == 8 and hs.samples == 5 and hs.basis.shape == (3, 8, 4) and hs.out.shape == (3, 142)
    assert e.ws == [(3, 1000, 5)] and hs.workspace.numel() == 192
    d = ReplicaSampledElboHessian([_model(e)])
    assert (d.steps, d.samples) == (32, 8)
    want_seeds = [(s ^ 2) % 2 ** 64 for s, _, _ in spec]
    for event in range(2):
        stats = hs.event()
        assert len(e.calls) == event + 1
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["steps"] == 8 and c["samples"] == 5 and c["kw"]["kind"] == 0 and c["kw"]["a_stride"] == 3
        assert c["kw"]["x_tag"] == 11 and c["kw"]["z_tag"] == 12
        assert [s % 2 ** 64 for s in c["x_seeds"]] == [s % 2 ** 64 for s in c["z_seeds"]] == want_seeds
        assert c["x_steps"] == c["z_steps"] == [event + 1] * 3
        assert e.fills[-3:] == [(4, s, event + 1, 13) for s in want_seeds]
        assert torch.equal(c["v0"], torch.full((3, 4), float(event + 1), dtype=torch.float64))
        for r, (m, (s, k, _), st) in enumerate(zip(ms, spec, stats)):
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 4 and m._exact_loglik_draws == 6
            assert m._sampled_hessian_draws == event + 1 and not hasattr(m, "_elbo_hessian_draws")
            assert list(st) == KEYS and all(isinstance(st[k_], float) for k_ in KEYS[2:])
            assert st[KEYS[0]].tolist() == [1000.0 * r + 12 + j for j in range(3)] and st[KEYS[1]].tolist() == [1000.0 * r + 44 + j for j in range(3)]
            assert [st[k_] for k_ in KEYS[2:]] == [1000.0 * r + 9, 1000.0 * r + 10, 1000.0 * r + 1]
    # step= draws the ROWS under that step and the exact event's row tag; samples and start vector stay under the own counter
    hs.event(step=41)
    c = e.calls[-1]
    assert c["x_steps"] == [41] * 3 and c["kw"]["x_tag"] == 3 and c["z_steps"] == [3] * 3 and e.fills[-1][2:] == (3, 13)
    with pytest.raises(RuntimeError, match="2 steps for 3 models"):
        hs.event(step=[1, 2])


def test_the_event_refusals():
    from vae_training_amd.trainer import ReplicaSampledElboHessian as Ev
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):
        Ev([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="vaek_sampled_elbo_hessian_lanczos_replicas does not cover.*one or two decoders.*step path: stub"):
        Ev([_model(_StubEngine(covered=False))])
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
    with pytest.raises(RuntimeError, match=r"1 models x 1000 rows x 66 samples = 66000 columns.*vaek_sampled_elbo_hessian_max_columns"):
        Ev([_model(e)], samples=66)                                       # rows x K above 2^16
    with pytest.raises(RuntimeError, match=r"100 models x 1000 rows x 64 samples = 6400000 columns"):
        Ev([_model(e) for _ in range(100)], samples=64)                   # models x rows x K above 2^22
    assert e.calls == [] and e.fills == []
    with pytest.raises(RuntimeError, match=r"ReplicaSampledElboHessian: model 0 \(run_dir\).*off_F"):
        Ev([_model(_StubEngine(off=2.0 ** -39))]).event()
    for k in (1, 0):
        st = Ev([_model(_StubEngine(k=k))]).event()[0]
        assert st[KEYS[0]].shape == st[KEYS[1]].shape == (k,)


def test_the_table_row_the_coupling_and_the_stats_line():
    from vae_training_amd import observables
    from vae_training_amd.model import GenerativeModel
    names = [ob.name for ob in observables.TABLE]
    assert names[names.index("elbo_hessian") + 1] == "sampled_elbo_hessian" and len(names) == len(observables.OBSERVABLES) + 1
    ob, fl = observables.FLAGS["sampled_elbo_hessian"]
    assert fl.flag == "--sampled_elbo_hessian" and ob.events == (("sampled_elbo_hessian", "_sampled_hessian", "ReplicaSampledElboHessian"),)
    assert observables.array_keys("sampled_elbo_hessian") == tuple(KEYS[:2])
    e = _StubEngine()
    m = _model(e)
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == []      # opt-in
    m.sampled_elbo_hessian, m.sampled_elbo_hessian_samples = 8, 5
    st = GenerativeModel._stats_event(m)
    assert list(st) == ["VAE Loss", "mse"] + KEYS and e.calls[-1]["steps"] == 8 and e.calls[-1]["samples"] == 5
    assert e.calls[-1]["x_steps"] == [1] and e.calls[-1]["kw"]["x_tag"] == 11
    # with --elbo_hessian: the exact Hessian's rows (its own counter and tag 9), and the gap
    m.elbo_hessian = 4
    st = GenerativeModel._stats_event(m)
    assert list(st)[-6:] == KEYS + ["Sharpness Sampling Gap"] and "Sharpness" in st
    assert e.calls[-1]["x_steps"] == e.exact_h[-1]["x_steps"] == [1] and e.calls[-1]["kw"]["x_tag"] == e.exact_h[-1]["x_tag"] == 9
    assert e.calls[-1]["x_seeds"] == e.exact_h[-1]["x_seeds"] and e.calls[-1]["rows"] == e.exact_h[-1]["rows"]
    assert e.calls[-1]["z_steps"] == [2] and st["Sharpness Sampling Gap"] == st["Sampled Sharpness"] - st["Sharpness"] == 9.0 - 100.0
    # ... which are the exact log-likelihood event's where that ran too
    m.exact_log_likelihood = True
    GenerativeModel._stats_event(m)
    assert e.calls[-1]["x_steps"] == e.exact_h[-1]["x_steps"] == e.exact[-1]["x_steps"] == [7] and e.calls[-1]["kw"]["x_tag"] == 3
    # write_stats keeps the two arrays as arrays whatever k is and puts the floats on the line
    lines = []
    w = types.SimpleNamespace(batchnum=0, stats={k: [] for k in KEYS}, _write=lines.append)
    GenerativeModel.write_stats(w, {KEYS[0]: np.array([2.5]), KEYS[1]: np.array([0.5]), KEYS[2]: 2.5, KEYS[3]: 2.5, KEYS[4]: 0.25})
    assert isinstance(w.stats[KEYS[0]][0], np.ndarray) and w.stats[KEYS[2]] == [2.5]
    assert lines == ["Batch | 0 | Sampled Sharpness | 2.500 | Sampled ELBO Hessian Min Ritz | 2.500 | Sampled ELBO Gradient Norm | 0.250"]


def test_run_py_flags_refusals_and_banners(monkeypatch):
    from vae_training_amd import observables, run
    base = ["sig", "--dataset", "sigmoid"]
    a = run.parse_arguments(base)
    assert a.sampled_elbo_hessian is None and a.sampled_elbo_hessian_samples is None      # opt-in
    assert run.parse_arguments(base + ["--sampled_elbo_hessian"]).sampled_elbo_hessian == 32
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--sampled_elbo_hessian", "8", "--sampled_elbo_hessian_samples", "16"])
    assert a.sampled_elbo_hessian == 8 and a.sampled_elbo_hessian_samples == 16
    for bad in ("0", "33", "x"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--sampled_elbo_hessian", bad])
    with pytest.raises(SystemExit):
        run.parse_arguments(base + ["--sampled_elbo_hessian_samples", "0"])
    with pytest.raises(RuntimeError, match="--sampled_elbo_hessian_samples sets the samples per row of --sampled_elbo_hessian"):
        run.main(run.parse_arguments(base + ["--sampled_elbo_hessian_samples", "4"]))
    assert run.SAMPLED_ELBO_HESSIAN_NEEDS == observables.FLAGS["sampled_elbo_hessian"][1].needs
    with pytest.raises(RuntimeError, match=r"--sampled_elbo_hessian needs .*one or two decoders.*step path: stub"):
        run.check_sampled_elbo_hessian_model(_model(_StubEngine(covered=False)))
    with pytest.raises(RuntimeError, match=r"--sampled_elbo_hessian needs .*world 2"):
        run.check_sampled_elbo_hessian_model(_model(_StubEngine(world=2)))
    run.check_sampled_elbo_hessian_model(_model(_StubEngine()))
    # attach: the attributes, the banners, the caps -- a two-decoder model, where --elbo_hessian is still refused with its old message
    e = _StubEngine(one_decoder=False)
    m = _model(e)
    fl, = observables.attach(run.parse_arguments(base + ["--sampled_elbo_hessian"]), [m], m, build=False)
    assert (m.sampled_elbo_hessian, m.sampled_elbo_hessian_samples) == (32, 8)
    assert fl.banner_one(m) == ("Sampled ELBO Hessian events: 32 Lanczos steps on 1000 rows x 8 samples "
                                "(vaek_sampled_elbo_hessian_lanczos_replicas)")
    sweep, ms = types.SimpleNamespace(), [_model(e, seed=s) for s in (69, 24)]
    fl, = observables.attach(run.parse_arguments(base + ["--sampled_elbo_hessian", "4", "--sampled_elbo_hessian_samples", "3"]), ms, sweep, build=True)
    (ob, ev), = observables.active(ms, sweep)
    assert fl.banner_sweep(ev, 2, sweep) == ("Sampled ELBO Hessian events: 4 Lanczos steps on 1000 rows x 3 samples per model, one call for 2 "
                                             "models (vaek_sampled_elbo_hessian_lanczos_replicas)")
    assert [list(x) for x in observables.run_events(ms, sweep)] == [KEYS, KEYS] and len(e.calls) == 1 and e.calls[0]["n"] == 2
    with pytest.raises(RuntimeError, match=r"^--elbo_hessian needs .*ONE decoder.*step path: stub"):
        list(observables.attach(run.parse_arguments(base + ["--elbo_hessian"]), [m], m, build=False))
    with pytest.raises(RuntimeError, match=r"--sampled_elbo_hessian_samples 2000: at most 1024 samples per row"):
        list(observables.attach(run.parse_arguments(base + ["--sampled_elbo_hessian", "--sampled_elbo_hessian_samples", "2000"]), [m], m, build=False))
    with pytest.raises(RuntimeError, match=r"--sampled_elbo_hessian_samples 66: 1 models x 1000 rows x 66 samples = 66000 columns"):
        list(observables.attach(run.parse_arguments(base + ["--sampled_elbo_hessian", "--sampled_elbo_hessian_samples", "66"]), [m], m, build=False))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="^--sampled_elbo_hessian needs .*does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--sampled_elbo_hessian"]))


# ---- 5. the ABI: mirrors, constants, the description guards ----------------------------------------------------------------------------------
def test_the_mirrors_match_the_header_and_a_c_compiled_probe(tmp_path):
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    pairs = (("vaek_sampled_elbo_hvp", _lib.VaekSampledElboHvp, _lib.VaekElboHvp, 168), ("vaek_sampled_elbo_hessian", _lib.VaekSampledElboHessian,
                                                                                         _lib.VaekElboHessian, 152))
    lines = []
    for struct, cls, base, size in pairs:
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, flags=re.S).group(1)
        fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f[0] for f in cls._fields_] == [f[0] for f in base._fields_] + EXTRA_FIELDS, fields
        lines.append(f'    printf("{struct}.sizeof %zu\\n", sizeof({struct}));')
        lines += [f'    printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaek.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for struct, cls, _, size in pairs:
        assert int(out[f"{struct}.sizeof"]) == C.sizeof(cls) == size
        assert all(int(out[f"{struct}.{f}"]) == getattr(cls, f).offset for f, _ in cls._fields_)


def test_the_constants_and_the_null_refusals():
    from vae_training_amd import _lib
    lib = _lib.load()
    assert lib.vaek_sampled_elbo_hessian_max_columns() == 1 << 22 and lib.vaek_sampled_elbo_hessian_record_len() == 142 == _ref().RECORD_LEN
    yes = C.c_int32(7)
    assert lib.vaek_supports_sampled_elbo_hessian(None, 1, C.byref(yes)) == -1 and yes.value == 7
    assert b"vaek_supports_sampled_elbo_hessian" in lib.vaek_last_error()
    n = C.c_size_t(7)
    assert lib.vaek_sampled_elbo_hessian_workspace_bytes(None, 1, 10, 8, C.byref(n)) == -1 and n.value == 7
    assert b"vaek_sampled_elbo_hessian_workspace_bytes" in lib.vaek_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_the_description_is_checked_before_the_context(name):
    """check_eval's order, as tests/test_eval_descriptions_host.py holds the other ten entries to it: a NULL description, then a
    struct_size of another header (both sizes in the message), then the NULL context -- each with the entry's name."""
    from vae_training_amd import _lib
    check_description_guard(_lib.load(), name)
