"""Host side of vaek_stats_event_replicas, no GPU: the C ABI surface of the four entry points, trainer.ReplicaStats on a stub engine
(one library call for R models, the seeds and steps compute_stats would use, the host RNG bookkeeping of a twin model run through
the host event, what it refuses) and run.py's --fused_stats flag."""
import os
import re
import types

import pytest
import torch

from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_stats_event", "vaek_stats_record_len", "vaek_stats_event_max_rows", "vaek_stats_event_replicas")
STATS_KEYS = ["VAE Loss", "KL divergence", "mse", "Squared Norm of Padding Dimensions", "Squared Norm of Manifold Dimension"]


def test_abi_surface_of_the_stats_event():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols: declared, bound with as many arguments, exported;
    the event description is struct_size-guarded and the ctypes mirror has the header's fields in the header's order."""
    import ctypes as C

    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_stats_event_replicas") == 12
    assert lib.vaek_stats_event_max_rows() == 4096
    body = re.search(r"typedef struct vaek_stats_event \{(.*?)\} vaek_stats_event;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekStatsEvent._fields_], fields
    assert fields == ["struct_size", "n", "rows", "reserved", "state_stride", "x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps",
                      "a_stride", "out", "out_stride"]
    assert C.sizeof(_lib.VaekStatsEvent) == 88
    check_description_guard(lib, "vaek_stats_event_replicas")          # the guard as behaviour: refused by its size, before the context
    # argument checks that need no device: a NULL context is refused before anything is touched, and the message names the entry point
    n = C.c_int64(7)
    assert lib.vaek_stats_record_len(None, C.byref(n)) == -1 and n.value == 7
    yes = C.c_int32(7)
    assert lib.vaek_supports_stats_event(None, 1, C.byref(yes)) == -1 and yes.value == 7
    ev = _lib.VaekStatsEvent()
    ev.struct_size = C.sizeof(_lib.VaekStatsEvent)
    assert lib.vaek_stats_event_replicas(None, None, C.byref(ev), 1, None, 3, 1, 3, 0.0, 1, 2, None) == -1
    assert b"vaek_stats_event_replicas" in lib.vaek_last_error()


class _StubEngine:
    """What ReplicaStats asks of an engine, on the CPU; records the library calls event() makes and fills the records."""
    world, rank = 1, 0
    device = torch.device("cpu")
    train_loop_max_replicas = 1024
    stats_event_max_rows = 4096

    def __init__(self, covered=True, D=7, L=6, world=1):
        self._covered, self.D, self.L, self.world, self.calls = covered, D, L, world, []

    @property
    def stats_record_len(self):
        return 8 + self.L

    def supports_stats_event(self, kind):
        return self._covered

    def supports_train_loop_gen(self, kind):
        return self._covered

    def stats_event_replicas(self, params, rows, kind, A, dd, did, pad, var_added, x_seeds, x_steps, z_seeds, z_steps, sample_eps, out, **kw):
        self.calls.append(dict(n=params.shape[0], rows=rows, kind=kind, x_seeds=x_seeds.tolist(), x_steps=x_steps.tolist(),
                               z_seeds=z_seeds.tolist(), z_steps=z_steps.tolist(), sample_eps=sample_eps.tolist(), params=params.clone(),
                               A=None if A is None else A.clone(), kw=kw))
        for r in range(params.shape[0]):                 # record r: 100 r + slot
            out[r] = 100.0 * r + torch.arange(out.shape[1], dtype=torch.float32)

    def loss_eval(self, *a, **kw):
        raise AssertionError("one fused call for all models, not the host event")

    forward = make_batch = loss_eval


def _model(eng, P=4, kind=1, seed=1, B=100, tdv=True, eps=-3.0, key=(3, 4)):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), 3, 1, 3, 0.0), key=(seed, 2), _draws=0)
    module = types.SimpleNamespace(engine=lambda B_, gb: eng, tunable_decoder_var=tdv)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=key, num_batches=16, print_batch_size=1000, epsilon=eps,
                                 current_epsilon=eps, vae_losses=[], var_enc=[], var_dec=[],
                                 model=types.SimpleNamespace(module=module, flat=torch.full((P,), float(seed))))


def _host_event_bookkeeping(m):
    """The host RNG bookkeeping of GenerativeModel.compute_stats on a twin: model.py's key split, datasets._device_batch's counter and
    seed (tag 1), vae._latent_pair's counter and seed (tag 2).  Returns (x_seed, x_step, z_seed, z_step)."""
    from vae_training_amd import random as vrandom
    key, m.key = vrandom.split(m.key)
    m.dataset._draws += 1
    x = (m.dataset.key[0] ^ m.dataset.key[1], m.dataset._draws)
    m._latent_draws = getattr(m, "_latent_draws", 0) + 1
    return x + (key[0] ^ key[1], m._latent_draws)


def _u64(v):
    return [s % 2 ** 64 for s in v]


def test_replica_stats_makes_one_call_and_keeps_the_host_bookkeeping():
    from vae_training_amd.trainer import ReplicaLoop, ReplicaStats
    e = _StubEngine()
    spec = [(69, (3, 4)), (24, (2 ** 63 + 11, 9)), (48, (5, 2 ** 64 - 1))]
    ms = [_model(e, seed=s, key=k) for s, k in spec]
    twins = [_model(e, seed=s, key=k) for s, k in spec]
    rs = ReplicaStats(ms)
    assert rs.R == 3 and rs.rows == 1000 and rs.params.shape == (3, 4) and rs.out.shape == (3, 14) and rs.a_stride == 3
    for event in range(2):
        stats = rs.event()
        want = [_host_event_bookkeeping(t) for t in twins]
        assert len(e.calls) == event + 1                                  # ONE library call for R models
        c = e.calls[-1]
        assert c["n"] == 3 and c["rows"] == 1000 and c["kind"] == 1 and c["kw"]["x_tag"] == 1 and c["kw"]["z_tag"] == 2 and c["kw"]["a_stride"] == 3
        assert _u64(c["x_seeds"]) == [w[0] % 2 ** 64 for w in want] and c["x_steps"] == [w[1] for w in want] == [event + 1] * 3
        assert _u64(c["z_seeds"]) == [w[2] % 2 ** 64 for w in want] and c["z_steps"] == [w[3] for w in want] == [event + 1] * 3
        assert c["params"][:, 0].tolist() == [69.0, 24.0, 48.0] and c["A"][:, 0].tolist() == [69.0, 24.0, 48.0]
        # the sampling pass takes the PREVIOUS event's eps: the CLI eps first, then slot [3] of the last record
        assert c["sample_eps"] == ([-3.0] * 3 if event == 0 else [3.0, 103.0, 203.0])
        for r, (m, t, st) in enumerate(zip(ms, twins, stats)):
            assert m.key == t.key and m._latent_draws == t._latent_draws == event + 1 and m.dataset._draws == t.dataset._draws == event + 1
            assert list(st) == STATS_KEYS                                # compute_stats' keys in its order
            assert [float(v) for v in st.values()] == [100.0 * r + k for k in (0, 1, 2, 4, 5)]
            assert len(m.vae_losses) == len(m.var_enc) == len(m.var_dec) == event + 1
            assert float(m.vae_losses[-1]) == 100.0 * r and m.var_enc[-1].tolist() == [100.0 * r + 8 + l for l in range(6)]
            assert m.var_dec[-1].tolist() == [100.0 * r + 3] == m.current_epsilon.tolist() and m.current_epsilon.shape == (1,)
    # without -tdv eps stays the CLI float, as VAE.loss returns it
    m = _model(e, tdv=False, eps=-1.0)
    ReplicaStats([m], rows=37).event()
    assert e.calls[-1]["rows"] == 37 and m.current_epsilon == -1.0 and m.var_dec == [-1.0]
    # ReplicaLoop.stats_event is a thin wrapper over the same object
    e2 = _StubEngine()
    e2.train_loop_replicas_workspace = lambda n: 0
    lp = ReplicaLoop([_model(e2, seed=s) for s in (69, 24)], loss_capacity=4)
    out = lp.stats_event()
    assert len(out) == 2 and list(out[0]) == STATS_KEYS and len(e2.calls) == 1 and lp.stats_event() and len(e2.calls) == 2
    assert e2.calls[-1]["x_steps"] == [2, 2]


def test_replica_stats_refusals():
    from vae_training_amd.trainer import ReplicaStats
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaStats([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaStats([_model(e), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaStats([_model(e), _model(_StubEngine(D=9))])
    with pytest.raises(RuntimeError, match="vaek_stats_event_replicas does not cover"):
        ReplicaStats([_model(_StubEngine(covered=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaStats([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaStats([_model(e) for _ in range(1025)])
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaStats([_model(e)], rows=4097)
    with pytest.raises(RuntimeError, match="rows"):
        ReplicaStats([_model(e)], rows=0)
    with pytest.raises(RuntimeError):
        ReplicaStats([])
    assert e.calls == []


def test_run_py_parses_the_fused_stats_flag():
    from vae_training_amd.run import main, parse_arguments
    base = ["sig", "--dataset", "sigmoid"]
    assert parse_arguments(base).fused_stats is False                    # opt-in: without the flag nothing changes
    assert parse_arguments(base + ["--sweep_dataset_seeds", "69,24"]).fused_stats is False
    a = parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--fused_stats"])
    assert a.fused_stats is True and a.sweep_dataset_seeds == [69, 24]
    # without the sweep flag it is refused before anything is created, with a message that says why
    with pytest.raises(RuntimeError, match="--fused_stats needs --sweep_dataset_seeds"):
        main(parse_arguments(base + ["--fused_stats"]))
