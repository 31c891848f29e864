"""Host side of vaek_log_likelihood_replicas, no GPU: the C ABI surface of the six entry points (declared, bound, exported; the
description's size and field offsets against a C-compiled probe), trainer.ReplicaLogLik on a stub engine (one library call for R
models, its own seeds, steps and tags, the run's RNG state untouched, what it refuses), the stats-event helper of model.py and run.py's
--log_likelihood_samples flag."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest
import torch

from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_log_likelihood", "vaek_log_likelihood_record_len", "vaek_log_likelihood_max_rows", "vaek_log_likelihood_max_samples",
       "vaek_log_likelihood_workspace_bytes", "vaek_log_likelihood_replicas")
FIELDS = ["struct_size", "n", "rows", "samples", "state_stride", "x_seeds", "x_steps", "z_seeds", "z_steps", "a_stride", "out", "out_stride",
          "x", "x_stride"]
KEYS = ["Average Log Likelihood", "ELBO estimate", "Effective Sample Size"]


def test_abi_surface_of_the_log_likelihood():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols; the caps; argument checks that need no device."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_log_likelihood_replicas") == 13
    assert lib.vaek_log_likelihood_record_len() == 4
    assert lib.vaek_log_likelihood_max_rows() == 4096 == lib.vaek_stats_event_max_rows()
    assert lib.vaek_log_likelihood_max_samples() == 1024
    body = re.search(r"typedef struct vaek_log_likelihood \{(.*?)\} vaek_log_likelihood;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekLogLikelihood._fields_] == FIELDS, fields
    check_description_guard(lib, "vaek_log_likelihood_replicas")        # the guard as behaviour: refused by its size, before the context
    assert "linear_loglik.hip" in open(os.path.join(ROOT, "vae_training_amd", "csrc", "Makefile")).read()
    # a NULL context is refused before anything is touched, and the message names the entry point
    yes = C.c_int32(7)
    assert lib.vaek_supports_log_likelihood(None, 1, C.byref(yes)) == -1 and yes.value == 7
    b = C.c_size_t(7)
    assert lib.vaek_log_likelihood_workspace_bytes(None, 1, 1, C.byref(b)) == -1 and b.value == 7
    ll = _lib.VaekLogLikelihood()
    ll.struct_size = C.sizeof(_lib.VaekLogLikelihood)
    assert lib.vaek_log_likelihood_replicas(None, None, C.byref(ll), 1, None, 3, 1, 3, 0.0, 3, 4, None, None) == -1
    assert b"vaek_log_likelihood_replicas" in lib.vaek_last_error()


def test_struct_layout_matches_a_c_compiled_probe(tmp_path):
    """sizeof and every offsetof of vaek_log_likelihood as a C compiler lays the header's struct out = the ctypes mirror's."""
    from vae_training_amd import _lib
    probe = tmp_path / "probe.c"
    lines = "\n".join(f'    printf("{f} %zu\\n", offsetof(vaek_log_likelihood, {f}));' for f in FIELDS)
    probe.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vaek.h"\nint main(void) {\n'
                     '    printf("sizeof %zu\\n", sizeof(vaek_log_likelihood));\n' + lines + "\n    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(_lib.VaekLogLikelihood) == 96
    assert {k: int(v) for k, v in out.items()} == {f: getattr(_lib.VaekLogLikelihood, f).offset for f in FIELDS}


class _StubEngine:
    """What ReplicaLogLik asks of an engine, on the CPU; records the library calls event() makes and fills the records."""
    rank = 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    log_likelihood_max_rows = 4096
    log_likelihood_max_samples = 1024
    log_likelihood_record_len = 4
    step_path = "stub"

    def __init__(self, covered=True, D=7, L=6, world=1):
        self._covered, self.D, self.L, self.world, self.calls, self.ws = covered, D, L, world, [], []

    def supports_log_likelihood(self, kind):
        return self._covered

    def supports_train_loop_gen(self, kind):
        raise AssertionError("the log-likelihood does not ask the resident loop's predicate: it has no batch-size condition")

    supports_stats_event = supports_train_loop_gen

    def log_likelihood_workspace(self, n, rows):
        self.ws.append((n, rows))
        return 32 * n * ((rows + 255) // 256)

    def log_likelihood_replicas(self, params, rows, samples, z_seeds, z_steps, out, workspace, **kw):
        self.calls.append(dict(n=params.shape[0], rows=rows, samples=samples, z_seeds=z_seeds.tolist(), z_steps=z_steps.tolist(),
                               x_seeds=kw["x_seeds"].tolist(), x_steps=kw["x_steps"].tolist(), params=params.clone(),
                               A=None if kw["A"] is None else kw["A"].clone(), ws=workspace.numel(), kw=kw))
        for r in range(params.shape[0]):                 # record r: 100 r + slot
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float32)

    def loss_eval(self, *a, **kw):
        raise AssertionError("one log-likelihood call for all models, nothing else")

    forward = make_batch = stats_event_replicas = loss_eval


def _model(eng, P=4, kind=1, seed=1, B=100, key=(3, 4), dd=3):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 1, 3, 0.0), key=(seed, 2), _draws=5)
    module = types.SimpleNamespace(engine=lambda B_, gb: eng, tunable_decoder_var=True)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=-3.0,
                                 current_epsilon=-3.0, vae_losses=[], var_enc=[], var_dec=[], average_log_likelihoods=[], _latent_draws=9,
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def test_replica_loglik_makes_one_call_and_leaves_the_run_alone():
    from vae_training_amd.trainer import ReplicaLogLik
    e = _StubEngine()
    spec = [(69, (3, 4), 100), (2 ** 63 + 24, (2 ** 63 + 11, 9), 257), (48, (5, 2 ** 64 - 1), 65536)]      # any batch size, also mixed
    ms = [_model(e, seed=s, key=k, B=B) for s, k, B in spec]
    ll = ReplicaLogLik(ms, 8)
    assert ll.R == 3 and ll.rows == 1000 and ll.samples == 8 and ll.params.shape == (3, 4) and ll.out.shape == (3, 4) and ll.a_stride == 3
    assert e.ws == [(3, 1000)] and ll.workspace.numel() == 32 * 3 * 4
    for event in range(2):
        stats = ll.event()
        assert len(e.calls) == event + 1                                  # ONE library call for R models
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["samples"] == 8 and c["kw"]["kind"] == 1 and c["kw"]["a_stride"] == 3
        assert c["kw"]["x_tag"] == 3 and c["kw"]["z_tag"] == 4           # 0, 1 and 2 are the train loop's, the dataset's and the latents'
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
    # rows and samples are the caller's
    m = _model(e)
    ReplicaLogLik([m], 1024, rows=37).event()
    assert e.calls[-1]["rows"] == 37 and e.calls[-1]["samples"] == 1024 and e.calls[-1]["ws"] == 32


def test_replica_loglik_refusals():
    from vae_training_amd.trainer import ReplicaLogLik
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaLogLik([_model(e), _model(e, P=5)], 8)
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaLogLik([_model(e), _model(e, kind=0)], 8)
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaLogLik([_model(e), _model(_StubEngine(D=9))], 8)
    with pytest.raises(RuntimeError, match="vaek_log_likelihood_replicas does not cover.*step path: stub"):
        ReplicaLogLik([_model(_StubEngine(covered=False))], 8)
    with pytest.raises(RuntimeError, match="world"):
        ReplicaLogLik([_model(_StubEngine(world=2))], 8)
    with pytest.raises(RuntimeError, match="-dd / -did <= 16"):
        ReplicaLogLik([_model(e, dd=17)], 8)
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaLogLik([_model(e) for _ in range(1025)], 8)
    with pytest.raises(RuntimeError, match="samples"):
        ReplicaLogLik([_model(e)], 1025)
    with pytest.raises(RuntimeError, match="samples"):
        ReplicaLogLik([_model(e)], 0)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaLogLik([_model(e)], 8, rows=4097)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaLogLik([_model(e)], 8, rows=0)
    with pytest.raises(RuntimeError):
        ReplicaLogLik([], 8)
    assert e.calls == []


def test_the_stats_helper_adds_the_log_likelihood_only_when_asked():
    """GenerativeModel._stats_event: compute_stats() alone without the attribute; with it, the three keys behind compute_stats' own."""
    from vae_training_amd.model import GenerativeModel
    e = _StubEngine()
    m = _model(e)
    m.compute_stats = lambda: {"VAE Loss": 1.0, "mse": 2.0}
    assert GenerativeModel._stats_event(m) == {"VAE Loss": 1.0, "mse": 2.0} and e.calls == [] and not hasattr(m, "_loglik_draws")
    m.log_likelihood_samples = 5
    for event in range(2):
        st = GenerativeModel._stats_event(m)
        assert list(st) == ["VAE Loss", "mse"] + KEYS and len(e.calls) == event + 1 and e.calls[-1]["samples"] == 5 and e.calls[-1]["n"] == 1
        assert e.calls[-1]["z_steps"] == [event + 1] and len(m.average_log_likelihoods) == event + 1
    assert e.ws == [(1, 1000)]                                         # one ReplicaLogLik for the run, not one per event


def test_run_py_parses_the_log_likelihood_flag(monkeypatch):
    from vae_training_amd import run
    base = ["sig", "--dataset", "sigmoid"]
    assert run.parse_arguments(base).log_likelihood_samples is None      # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--log_likelihood_samples", "8"]).log_likelihood_samples == 8
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--fused_stats", "--log_likelihood_samples", "64"])
    assert a.log_likelihood_samples == 64 and a.sweep_dataset_seeds == [69, 24] and a.fused_stats is True
    for bad in ("0", "-3", "many"):
        with pytest.raises(SystemExit):
            run.parse_arguments(base + ["--log_likelihood_samples", bad])
    # the model check: a model the predicate does not cover, data parallelism, -dd above the generator's, K above the cap
    e = _StubEngine(covered=False)
    with pytest.raises(RuntimeError, match=r"--log_likelihood_samples needs .*step path: stub"):
        run.check_log_likelihood_model(_model(e), 8)
    with pytest.raises(RuntimeError, match=r"--log_likelihood_samples needs .*world 2"):
        run.check_log_likelihood_model(_model(_StubEngine(world=2)), 8)
    with pytest.raises(RuntimeError, match="--log_likelihood_samples needs"):
        run.check_log_likelihood_model(_model(_StubEngine(), dd=17), 8)
    with pytest.raises(RuntimeError, match="at most 1024 samples"):
        run.check_log_likelihood_model(_model(_StubEngine()), 1025)
    run.check_log_likelihood_model(_model(_StubEngine()), 1024)
    # under data parallelism main() refuses before a process group or a directory exists
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="does not combine with data parallelism"):
        run.main(run.parse_arguments(base + ["--log_likelihood_samples", "8"]))
