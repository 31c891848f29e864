"""Host side of the covariance spectra (csrc/cov_spectrum.hip), no GPU: the float64 restatement of the kernel's algorithm
(tools/cov_spectrum_reference.py) on EVERY input set of tests/test_gpu_cov_spectrum.py -- it converges below the sweep cap and agrees
with numpy.linalg.eigvalsh within T2 -- the C ABI surface of the seven entry points, trainer.ReplicaSpectrum on a stub engine (both
routes, tags 5 and 6, its own counter, the run's RNG state untouched, what it refuses), run.py's --eigenvalues flag and its refusals,
and that losses.npz has no EigenValues key without the flag."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import cov_spectrum_cases as K
from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_cov_spectrum", "vaek_cov_spectrum_record_len", "vaek_cov_spectrum_max_sets", "vaek_cov_spectrum_max_sweeps",
       "vaek_cov_spectrum_rows", "vaek_supports_spectrum_event", "vaek_spectrum_event_replicas")
FIELDS = ["struct_size", "n", "rows", "reserved", "state_stride", "x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps", "a_stride", "out",
          "out_stride"]
KEYS = ["learnt eigenvalue", "ground truth eigenvalue"]


def _reference():
    spec = importlib.util.spec_from_file_location("cov_spectrum_reference", os.path.join(ROOT, "tools", "cov_spectrum_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_restatement_converges_and_meets_t2_on_every_input_set():
    """The same ordering, rotation, stop rule and cap as the kernel, in NumPy float64: every set of the GPU file converges below the
    cap and its eigenvalues agree with LAPACK's within T2.  A case that fails here is changed here, never the cap on the GPU."""
    ref = _reference()
    assert ref.MAX_SWEEPS == K.MAX_SWEEPS == 32 and ref.TOL == K.STOP == 2.0 ** -43
    most, n = 0, 0
    for name, x in K.all_host_sets():
        r = ref.record(x)
        K.check_t1(name, r, x)
        sweeps, _ = K.check_t2(name, r)
        most, n = max(most, sweeps), n + 1
    assert n == len(K.DIMS) * len(K.ROWS) * len(K.VARIANTS) + len(K.PADDED) * len(K.PADDED_ROWS)
    print(f"most sweeps: {most} of {K.MAX_SWEEPS}")


def test_the_restatement_on_the_degenerate_matrices():
    """Rotations that must be skipped or taken with t = 1 / (2 theta): an exactly diagonal matrix (0 sweeps), a zero matrix, a_pq tiny
    against a_qq - a_pp (theta overflows), equal diagonal elements (theta = 0: 45 degrees), and the round-robin pairs themselves."""
    ref = _reference()
    eig, sweeps, off, norm = ref.jacobi_eigenvalues(np.diag([3.0, 1.0, 2.0]))
    assert eig.tolist() == [1.0, 2.0, 3.0] and sweeps == 0 and off == 0.0
    eig, sweeps, off, norm = ref.jacobi_eigenvalues(np.zeros((4, 4)))
    assert eig.tolist() == [0.0] * 4 and sweeps == 0 and norm == 0.0
    c = np.array([[1e150, 1e-160], [1e-160, -1e150]])
    eig, sweeps, off, norm = ref.jacobi_eigenvalues(c)
    assert np.isfinite(eig).all() and eig.tolist() == [-1e150, 1e150]
    assert ref.rotation(1.0, 1.0, 0.0) == (1.0, 0.0)
    co, si = ref.rotation(2.0, 2.0, 0.5)
    assert abs(co - np.sqrt(0.5)) < 1e-15 and abs(si - np.sqrt(0.5)) < 1e-15
    for de in (2, 4, 8, 22, 32):
        seen = set()
        for rnd in range(de - 1):
            pairs = ref.round_pairs(de, rnd)
            assert sorted(i for p in pairs for i in p) == list(range(de))           # de / 2 DISJOINT rotations
            seen |= {tuple(sorted(p)) for p in pairs}
        assert len(seen) == de * (de - 1) // 2                                        # every pair once per sweep


def test_abi_surface_of_the_spectrum_calls():
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_cov_spectrum_rows") == 8 and _c_args(hdr, "vaek_spectrum_event_replicas") == 12
    assert lib.vaek_cov_spectrum_max_sweeps() == 32
    assert lib.vaek_cov_spectrum_max_sets() == 2 * lib.vaek_train_loop_max_replicas()
    body = re.search(r"typedef struct vaek_spectrum_event \{(.*?)\} vaek_spectrum_event;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekSpectrumEvent._fields_] == FIELDS == [f[0] for f in _lib.VaekStatsEvent._fields_], fields
    assert "double* out;" in re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert "cov_spectrum.hip" in open(os.path.join(ROOT, "vae_training_amd", "csrc", "Makefile")).read()
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_cov_spectrum(None, C.byref(yes)) == -1 and yes.value == 7
    assert lib.vaek_supports_spectrum_event(None, 1, C.byref(yes)) == -1 and yes.value == 7
    n = C.c_int64(7)
    assert lib.vaek_cov_spectrum_record_len(None, C.byref(n)) == -1 and n.value == 7
    assert lib.vaek_cov_spectrum_rows(None, None, 1, 5, 0, None, 0, None) == -1
    assert b"vaek_cov_spectrum_rows" in lib.vaek_last_error()
    ev = _lib.VaekSpectrumEvent()
    ev.struct_size = C.sizeof(_lib.VaekSpectrumEvent)
    assert lib.vaek_spectrum_event_replicas(None, None, C.byref(ev), 1, None, 3, 1, 3, 0.0, 5, 6, None) == -1
    assert b"vaek_spectrum_event_replicas" in lib.vaek_last_error()


def test_struct_layout_matches_a_c_compiled_probe(tmp_path):
    from vae_training_amd import _lib
    probe = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vaek_spectrum_event, {f}));' for f in FIELDS)
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaek.h"\nint main(void) {\n'
                     '    printf("sizeof %zu\\n", sizeof(vaek_spectrum_event));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(_lib.VaekSpectrumEvent) == C.sizeof(_lib.VaekStatsEvent)
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_lib.VaekSpectrumEvent, f).offset for f in FIELDS}


class _StubEngine:
    """What ReplicaSpectrum asks of an engine, on the CPU; records the library calls event() makes and fills the records."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    stats_event_max_rows = 4096
    step_path = "stub"

    def __init__(self, fused=True, D=3, L=6, world=1, covered=True, off=0.0):
        self._fused, self.D, self.L, self.world, self._covered, self._off = fused, D, L, world, covered, off
        self.calls, self.batches, self.forwards = [], [], []
        self.cov_spectrum_record_len = D * D + 2 * D + 4

    def supports_cov_spectrum(self):
        return self._covered

    def supports_spectrum_event(self, kind):
        return self._fused

    def supports_train_loop_gen(self, kind):
        raise AssertionError("the spectrum does not ask the resident loop's predicate: it has no batch-size condition")

    supports_stats_event = supports_train_loop_gen

    def _fill(self, out2d):
        D = self.D
        for s in range(out2d.shape[0]):                      # record s: eigenvalues 100 s + k, |C|_F = 1, off_F as configured
            out2d[s, :D] = 100.0 * s + torch.arange(D, dtype=torch.float64)
            out2d[s, 2 * D + D * D:] = torch.tensor([3.0, self._off, 1.0, 1000.0], dtype=torch.float64)

    def spectrum_event_replicas(self, params, rows, kind, A, dd, did, pad, var, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        self.calls.append(dict(route="fused", n=params.shape[0], rows=rows, kind=kind, x_seeds=x_seeds.tolist(), x_steps=x_steps.tolist(),
                               z_seeds=z_seeds.tolist(), z_steps=z_steps.tolist(), sample_eps=sample_eps.tolist(), params=params.clone(), kw=kw))
        assert out.shape == (params.shape[0], 2 * self.cov_spectrum_record_len) and out.dtype == torch.float64
        self._fill(out.view(-1, self.cov_spectrum_record_len))

    def make_batch(self, kind, A, dd, did, pad, var, rows, seed, step=0, tag=0, want_x=True, want_z=True, out=None):
        self.batches.append(dict(rows=rows, seed=seed, step=step, tag=tag, want_x=want_x and out is None or out is not None and out[0] is not None))
        if out is not None:
            out[0].fill_(float(tag))
            return out
        return None, torch.full((rows, self.L), 1.0), torch.full((rows, self.D), 2.0)

    def forward(self, params, x, z1, z2, sampling=False, eps=0.0, want_mu=True):
        assert sampling and x is None and not want_mu
        self.forwards.append(dict(eps=eps, p0=float(params[0])))
        return torch.full((z1.shape[0], self.D), 7.0), None

    def cov_spectrum_rows(self, x, rows, out):
        self.calls.append(dict(route="rows", n=x.shape[0], rows=rows, x=x.clone()))
        self._fill(out)

    def loss_eval(self, *a, **kw):
        raise AssertionError("one spectrum call for all models, nothing else")

    stats_event_replicas = log_likelihood_replicas = loss_eval


def _model(eng, P=4, kind=1, seed=1, B=100, key=(3, 4), dd=3, eps=-3.0):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb=0: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=eps, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 gt_eigen=[], ht_eigen=[], dirname="data/stub", _loglik_draws=2,
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "host_route"])
def test_replica_spectrum_makes_one_call_and_leaves_the_run_alone(fused):
    from vae_training_amd.trainer import ReplicaSpectrum
    e = _StubEngine(fused=fused)
    spec = [(69, (3, 4), 100, -3.0), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257, torch.tensor([-1.5])), (48, (5, 2 ** 64 - 1), 65536, -0.25)]
    ms = [_model(e, seed=s, key=k, B=B, eps=eps) for s, k, B, eps in spec]
    sp = ReplicaSpectrum(ms)
    assert sp.R == 3 and sp.rows == 1000 and sp.fused == fused and sp.out.shape == (6, 3 * 3 + 2 * 3 + 4) and sp.out.dtype == torch.float64
    for event in range(2):
        stats = sp.event()
        assert len(e.calls) == event + 1                                  # ONE spectrum call for R models
        c = e.calls[-1]
        want = [(s ^ 2) % 2 ** 64 for s, _, _, _ in spec]                 # dataset.key[0] ^ dataset.key[1]
        if fused:
            assert c["route"] == "fused" and c["n"] == 3 and c["rows"] == 1000 and c["kind"] == 1 and c["kw"]["a_stride"] == 3
            assert c["kw"]["x_tag"] == 5 and c["kw"]["z_tag"] == 6       # 0 .. 4 are taken
            assert [s % 2 ** 64 for s in c["x_seeds"]] == want == [s % 2 ** 64 for s in c["z_seeds"]]
            assert c["x_steps"] == c["z_steps"] == [event + 1] * 3       # its own counter, incremented before use
            assert c["sample_eps"] == [-3.0, -1.5, -0.25]                 # current_epsilon
            assert c["params"][:, 0].tolist() == [float(s) for s, _, _, _ in spec]
            assert e.batches == [] and e.forwards == []
        else:
            assert c["route"] == "rows" and c["n"] == 6 and c["rows"] == 1000 and c["x"].shape == (6, 1000, 3)
            b = e.batches[-6:]
            assert [d["tag"] for d in b] == [5, 6] * 3 and [d["want_x"] for d in b] == [True, False] * 3
            assert [d["seed"] % 2 ** 64 for d in b] == [w for w in want for _ in range(2)]
            assert all(d["step"] == event + 1 and d["rows"] == 1000 for d in b)
            assert [f["eps"] for f in e.forwards[-3:]] == [-3.0, -1.5, -0.25]
            assert [f["p0"] for f in e.forwards[-3:]] == [float(s) for s, _, _, _ in spec]
            assert bool((c["x"][0::2] == 7.0).all()) and bool((c["x"][1::2] == 5.0).all())      # fake rows, then real rows (tag 5's)
        for r, (m, (s, k, _, eps), st) in enumerate(zip(ms, spec, stats)):
            assert m.key == k and m.dataset._draws == 5 and m._latent_draws == 9 and m._loglik_draws == 2 and m.dataset.key == (s, 2)
            assert m._spectrum_draws == event + 1
            assert list(st) == KEYS
            assert st[KEYS[0]].tolist() == [200.0 * r + j for j in range(3)] and st[KEYS[1]].tolist() == [200.0 * r + 100 + j for j in range(3)]
            assert len(m.ht_eigen) == len(m.gt_eigen) == event + 1
            assert m.ht_eigen[-1].tolist() == st[KEYS[0]].tolist() and m.gt_eigen[-1].tolist() == st[KEYS[1]].tolist()
            assert m.vae_losses == [] and m.var_enc == [] and m.var_dec == [] and m.average_log_likelihoods == []
    ReplicaSpectrum([_model(e)], rows=37).event()
    assert e.calls[-1]["rows"] == 37


def test_replica_spectrum_refusals():
    from vae_training_amd.trainer import ReplicaSpectrum
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaSpectrum([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaSpectrum([_model(e), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match="data_dim <= 32.*data_dim: 33"):
        ReplicaSpectrum([_model(_StubEngine(covered=False, D=33))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaSpectrum([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="-dd / -did <= 16"):
        ReplicaSpectrum([_model(e, dd=17)])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaSpectrum([_model(e) for _ in range(1025)])
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaSpectrum([_model(e)], rows=4097)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaSpectrum([_model(e)], rows=1)                             # one row has no covariance
    with pytest.raises(RuntimeError):
        ReplicaSpectrum([])
    assert e.calls == []
    # a solve that stopped at the cap without converging names the model
    bad = _StubEngine(off=2.0 ** -39)
    m = _model(bad)
    with pytest.raises(RuntimeError, match=r"model 0 \(data/stub\).*learnt eigenvalue.*off_F"):
        ReplicaSpectrum([m]).event()
    assert m.ht_eigen == [] and m.gt_eigen == []
    ok = _StubEngine(off=2.0 ** -41)
    ReplicaSpectrum([_model(ok)]).event()


def test_the_stats_helper_adds_the_spectra_only_when_asked():
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_spectrum_draws")
    m.eigenvalues = True
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["n"] == 1
        assert e.calls[-1]["z_steps"] == [event + 1] and len(m.ht_eigen) == event + 1


def test_losses_have_no_eigenvalues_key_without_the_flag():
    """model_save_data writes "EigenValues": (ht_eigen, gt_eigen) with the flag and only with it."""
    from vae_training_amd.vae import VAEModel
    m = types.SimpleNamespace(vae_losses=[1.0], var_dec=[0.5], var_enc=[0.25], correlation_ratios=[], ht_eigen=[np.arange(3.0)],
                              gt_eigen=[np.arange(3.0) + 1])
    plain = VAEModel.model_save_data(m, final=True)
    assert "EigenValues" not in plain and list(plain) == ["VAE Loss", "Decoder Variance", "Encoder Variance", "Correlation Ratio"]
    m.eigenvalues = True
    flagged = VAEModel.model_save_data(m, final=True)
    assert [k for k in flagged if k not in plain] == ["EigenValues"]
    assert flagged["EigenValues"][0] is m.ht_eigen and flagged["EigenValues"][1] is m.gt_eigen
    assert {k: flagged[k] for k in plain} == plain


def test_run_py_parses_the_eigenvalues_flag_and_refuses(monkeypatch):
    from vae_training_amd import run
    base = ["sig", "--dataset", "sigmoid"]
    assert run.parse_arguments(base).eigenvalues is False                # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--eigenvalues"]).eigenvalues is True
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--fused_stats", "--log_likelihood_samples", "64", "--eigenvalues"])
    assert a.eigenvalues is True and a.log_likelihood_samples == 64 and a.sweep_dataset_seeds == [69, 24] and a.fused_stats is True
    with pytest.raises(SystemExit):
        run.parse_arguments(base + ["--mlp_eigenvalues"])               # one flag, no --mlp_ twin
    with pytest.raises(RuntimeError, match=r"--eigenvalues needs data_dim <= 32.*data_dim: 33"):
        run.check_eigenvalues_model(_model(_StubEngine(covered=False, D=33)))
    with pytest.raises(RuntimeError, match=r"--eigenvalues needs .*world 2"):
        run.check_eigenvalues_model(_model(_StubEngine(world=2)))
    with pytest.raises(RuntimeError, match="--eigenvalues needs"):
        run.check_eigenvalues_model(_model(_StubEngine(), dd=17))
    run.check_eigenvalues_model(_model(_StubEngine()))
    run.check_eigenvalues_model(_model(_StubEngine(fused=False)))        # any architecture: the host route
    # under data parallelism main() refuses before a process group or a directory exists
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--eigenvalues needs .* does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--eigenvalues"]))
