"""Host side of vaek_mlp3_stats_event_replicas, no GPU: the C ABI surface of the three entry points, trainer.ReplicaStatsMlp3 on a stub
engine (one library call and one read-back per event, the bookkeeping of ReplicaStats on the same stub, what it refuses), ReplicaStats'
own messages unchanged, and run.py's --mlp_fused_stats flag with its three refusals."""
import ctypes as C
import os
import types

import pytest
import torch

from tests import test_stats_event_host as SE
from tests.abi_util import _c_args, check_description_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_mlp3_stats_event", "vaek_mlp3_stats_event_workspace_bytes", "vaek_mlp3_stats_event_replicas")
SPHERE_KEYS = ["VAE Loss", "KL divergence", "mse", "Sphere Error", "Padding Error"]


def test_abi_surface_of_the_mlp3_stats_event():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the three symbols: declared, bound with as many arguments, exported; the
    description is vaek_stats_event as it is; NULL arguments are refused with the entry's name and leave the outputs alone."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_mlp3_stats_event_replicas") == _c_args(hdr, "vaek_stats_event_replicas") + 1 == 13      # + workspace
    assert _c_args(hdr, "vaek_mlp3_stats_event_workspace_bytes") == 4 and _c_args(hdr, "vaek_supports_mlp3_stats_event") == 3
    assert _lib.SIGNATURES["vaek_mlp3_stats_event_replicas"][1][2]._type_ is _lib.VaekStatsEvent
    assert C.sizeof(_lib.VaekStatsEvent) == 88
    check_description_guard(lib, "vaek_mlp3_stats_event_replicas")      # the guard as behaviour: refused by its size, before the context
    assert "mlp3_stats.hip" in open(os.path.join(ROOT, "vae_training_amd", "csrc", "Makefile")).read()
    yes = C.c_int32(7)
    assert lib.vaek_supports_mlp3_stats_event(None, 2, C.byref(yes)) == -1 and yes.value == 7
    assert b"vaek_supports_mlp3_stats_event" in lib.vaek_last_error()
    b = C.c_size_t(7)
    assert lib.vaek_mlp3_stats_event_workspace_bytes(None, 1, 37, C.byref(b)) == -1 and b.value == 7
    assert b"vaek_mlp3_stats_event_workspace_bytes" in lib.vaek_last_error()
    ev = _lib.VaekStatsEvent()
    ev.struct_size = C.sizeof(_lib.VaekStatsEvent)
    assert lib.vaek_mlp3_stats_event_replicas(None, None, C.byref(ev), 2, None, 3, 3, 3, 0.0, 1, 2, None, None) == -1
    assert b"vaek_mlp3_stats_event_replicas" in lib.vaek_last_error()


def test_the_workspace_query_refuses_n_and_rows_out_of_range():
    """The ranges belong to no context, so the query checks them first: without a device (no context can be made) every n or rows
    outside 1 .. vaek_train_loop_max_replicas() / 1 .. vaek_stats_event_max_rows() is refused with the ranges in the message and
    *bytes left alone; arguments inside them reach the context check."""
    from vae_training_amd import _lib
    lib = _lib.load()
    cap = lib.vaek_train_loop_max_replicas()
    b = C.c_size_t(7)
    for n, rows in ((0, 37), (cap + 1, 37), (1, 0), (1, 4097), (-1, 37), (1, -5), (0, 0)):
        assert lib.vaek_mlp3_stats_event_workspace_bytes(None, n, rows, C.byref(b)) == -1 and b.value == 7, (n, rows)
        msg = lib.vaek_last_error().decode()
        assert msg.startswith("vaek_mlp3_stats_event_workspace_bytes: ") and f"1 .. {cap} replicas" in msg and "1 .. 4096 rows" in msg, msg
    for n, rows in ((1, 1), (cap, 4096), (3, 1000)):
        assert lib.vaek_mlp3_stats_event_workspace_bytes(None, n, rows, C.byref(b)) == -1 and b.value == 7
        assert lib.vaek_last_error().decode() == "vaek_mlp3_stats_event_workspace_bytes: null argument"
    assert lib.vaek_mlp3_stats_event_workspace_bytes(None, 1, 1, None) == -1


class _StubMlp3(SE._StubEngine):
    """The stub of the linear host test plus what ReplicaStatsMlp3 asks: the predicate, the workspace query and the call; the linear
    predicate is false, as it is on an mlp3 context."""
    step_path = "mlp3"

    def __init__(self, covered=True, D=6, L=6, world=1):
        super().__init__(False, D, L, world)
        self._mlp3, self.ws_queries = covered, []

    def supports_mlp3_stats_event(self, kind):
        return self._mlp3

    def mlp3_stats_event_workspace(self, n, rows):
        self.ws_queries.append((n, rows))
        return 64 * n * ((rows + 31) // 32)

    def stats_event_replicas(self, *a, **kw):
        raise AssertionError("the linear call on an mlp3 sweep")

    def mlp3_stats_event_replicas(self, *a, workspace=None, **kw):
        assert workspace is not None and workspace.dtype == torch.uint8
        SE._StubEngine.stats_event_replicas(self, *a, **kw)
        self.calls[-1]["workspace"] = workspace


def _model(eng, **kw):
    kw.setdefault("kind", 2)
    return SE._model(eng, **kw)


def test_replica_stats_mlp3_makes_one_call_and_keeps_replica_stats_bookkeeping(monkeypatch):
    from vae_training_amd.trainer import ReplicaGraphLoop, ReplicaStats, ReplicaStatsMlp3
    assert issubclass(ReplicaStatsMlp3, ReplicaStats)
    # only small methods are replaced: the predicate and its message, the workspace, the library call
    assert set(k for k in vars(ReplicaStatsMlp3) if not k.startswith("__")) == {"NAME", "_check_covered", "_make_workspace", "_call"}
    e, lin = _StubMlp3(), SE._StubEngine(L=6)
    spec = [(69, (3, 4)), (24, (2 ** 63 + 11, 9)), (48, (5, 2 ** 64 - 1))]
    ms = [_model(e, seed=s, key=k) for s, k in spec]
    twins = [_model(lin, seed=s, key=k) for s, k in spec]                # ReplicaStats on the linear stub: the same bookkeeping
    rs, base = ReplicaStatsMlp3(ms), ReplicaStats(twins)
    assert rs.R == 3 and rs.rows == 1000 and rs.params.shape == (3, 4) and rs.out.shape == (3, 14) and rs.a_stride == 3
    assert e.ws_queries == [(3, 1000)] and rs.workspace.numel() == 64 * 3 * 32
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **kw: (copies.append(tuple(t.shape)), real_cpu(t, *a, **kw))[1])
    for event in range(2):
        copies.clear()
        stats, want = rs.event(), base.event()
        assert copies == [(3, 14), (3, 14)]                               # ONE read-back each: the records
        assert len(e.calls) == event + 1 == len(lin.calls)                # ONE library call for R models
        c, w = e.calls[-1], lin.calls[-1]
        assert c["workspace"] is rs.workspace
        for k in ("n", "rows", "x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps", "kw"):
            assert c[k] == w[k], k
        assert c["kind"] == 2 and c["kw"] == dict(a_stride=3, x_tag=1, z_tag=2)
        assert torch.equal(c["params"], w["params"]) and torch.equal(c["A"], w["A"])
        for r, (m, t, st, sw) in enumerate(zip(ms, twins, stats, want)):
            assert list(st) == SPHERE_KEYS and [float(v) for v in st.values()] == [float(v) for v in sw.values()]
            assert m.key == t.key and m._latent_draws == t._latent_draws == event + 1 and m.dataset._draws == t.dataset._draws == event + 1
            assert len(m.vae_losses) == len(m.var_enc) == len(m.var_dec) == event + 1
            assert float(m.vae_losses[-1]) == float(t.vae_losses[-1]) and m.var_enc[-1].tolist() == t.var_enc[-1].tolist()
            assert m.var_dec[-1].tolist() == t.var_dec[-1].tolist() == m.current_epsilon.tolist() == t.current_epsilon.tolist()
    monkeypatch.undo()
    m = _model(e, tdv=False, eps=-1.0)
    ReplicaStatsMlp3([m], rows=37).event()
    assert e.calls[-1]["rows"] == 37 and m.current_epsilon == -1.0 and m.var_dec == [-1.0]
    # ReplicaGraphLoop.stats_event is a thin wrapper over the same object
    lp = types.SimpleNamespace(ms=[_model(e, seed=s) for s in (69, 24)])
    n = len(e.calls)
    out = ReplicaGraphLoop.stats_event(lp)
    assert len(out) == 2 and list(out[0]) == SPHERE_KEYS and len(e.calls) == n + 1 and isinstance(lp._stats, ReplicaStatsMlp3)
    first = lp._stats
    assert ReplicaGraphLoop.stats_event(lp) and lp._stats is first and e.calls[-1]["x_steps"] == [2, 2]
    assert ReplicaGraphLoop.stats_event(lp, rows=37) and lp._stats is not first and e.calls[-1]["rows"] == 37


def test_replica_stats_mlp3_refusals_and_replica_stats_messages():
    from vae_training_amd.trainer import ReplicaStats, ReplicaStatsMlp3
    e = _StubMlp3()
    with pytest.raises(RuntimeError, match="ReplicaStatsMlp3: .*shape"):
        ReplicaStatsMlp3([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):
        ReplicaStatsMlp3([_model(e), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match=r"ReplicaStatsMlp3: vaek_mlp3_stats_event_replicas does not cover .*three hidden layers.*"
                                           r"a linear VAE is ReplicaStats'.*step path: mlp3"):
        ReplicaStatsMlp3([_model(_StubMlp3(covered=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaStatsMlp3([_model(_StubMlp3(world=2))])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaStatsMlp3([_model(e) for _ in range(1025)])
    for rows in (4097, 0):
        with pytest.raises(RuntimeError, match=rf"ReplicaStatsMlp3: {rows} rows per event, need 1 \.\. 4096 \(vaek_stats_event_max_rows\)"):
            ReplicaStatsMlp3([_model(e)], rows=rows)
    with pytest.raises(RuntimeError):
        ReplicaStatsMlp3([])
    assert e.calls == [] and e.ws_queries == []
    # ReplicaStats says what it said, and refuses the mlp3 stub (whose linear predicate is false) without asking for anything new
    with pytest.raises(RuntimeError) as ei:
        ReplicaStats([_model(e)])
    assert str(ei.value) == ("ReplicaStats: vaek_stats_event_replicas does not cover this model / dataset (it needs what the resident loop needs: "
                             "a float32 linear VAE with one or two decoders, D, L <= 32 and a train batch of at most 256 rows)")
    with pytest.raises(RuntimeError) as ei:
        ReplicaStats([_model(SE._StubEngine())], rows=4097)
    assert str(ei.value) == "ReplicaStats: 4097 rows per event, need 1 .. 4096 (vaek_stats_event_max_rows)"


def test_run_py_parses_the_mlp_fused_stats_flag_and_refuses():
    from vae_training_amd import run
    from vae_training_amd.trainer import ReplicaLoop
    base = ["sph", "--dataset", "sphere"]
    assert run.parse_arguments(base).mlp_fused_stats is False              # opt-in: without the flag nothing changes
    assert run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24"]).mlp_fused_stats is False
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--mlp_fused_stats", "--mlp_log_likelihood_samples", "8"])
    assert a.mlp_fused_stats is True and a.fused_stats is False and a.sweep_dataset_seeds == [69, 24] and a.mlp_log_likelihood_samples == 8
    a = run.parse_arguments(base + ["--sweep_dataset_seeds", "69,24", "--fused_stats"])
    assert a.fused_stats is True and a.mlp_fused_stats is False           # --fused_stats as before ...
    with pytest.raises(RuntimeError, match="--fused_stats needs --sweep_dataset_seeds"):
        run.main(run.parse_arguments(base + ["--fused_stats"]))           # ... its refusal included
    # 1. without --sweep_dataset_seeds
    with pytest.raises(RuntimeError, match=r"--mlp_fused_stats needs --sweep_dataset_seeds .*step path: mlp3"):
        run.refuse_mlp_fused_stats_single("mlp3")
    # 2. a sweep ReplicaLoop takes: pointed to --fused_stats
    lin = object.__new__(ReplicaLoop)
    lin.eng, lin.kind = types.SimpleNamespace(step_path="linear"), 1
    with pytest.raises(RuntimeError, match=r"--mlp_fused_stats needs .*step path is 'linear'.*use --fused_stats"):
        run.check_mlp_fused_stats_loop(lin)
    # 3. both flags together
    mlp = types.SimpleNamespace(eng=_StubMlp3(), kind=2)
    with pytest.raises(RuntimeError, match=r"--fused_stats .* and --mlp_fused_stats .*disjoint sweeps.*'mlp3'"):
        run.check_mlp_fused_stats_loop(mlp, fused_stats=True)
    run.check_mlp_fused_stats_loop(mlp)                                    # the sweep it is for
    with pytest.raises(RuntimeError, match="vaek_supports_mlp3_stats_event does not cover"):
        run.check_mlp_fused_stats_loop(types.SimpleNamespace(eng=_StubMlp3(covered=False), kind=2))
