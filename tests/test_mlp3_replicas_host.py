"""Host side of vaek_train_step_gen_replicas, no GPU: the C ABI surface of the new entry points, trainer.ReplicaGraphLoop on a stub
engine (which library calls run() makes, its stacks, seeds and copies, what it refuses) and run.py's choice between the two
replica loops."""
import os
import re
import types

import pytest
import torch

from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_supports_train_step_replicas", "vaek_train_step_max_replicas", "vaek_train_step_replicas_workspace_bytes",
       "vaek_train_step_gen_replicas")


def test_abi_surface_of_the_replica_step():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols: declared, bound with as many arguments, exported;
    vaek_replicas is reused as it is; a NULL context is refused before anything is touched."""
    import ctypes as C

    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_train_step_gen_replicas") == 26
    sig = _lib.SIGNATURES["vaek_train_step_gen_replicas"][1]
    assert sig[6] == C.POINTER(_lib.VaekReplicas) and sig[10] == C.c_float and sig[21] == C.c_int64 and sig[24] == C.c_uint32
    assert C.sizeof(_lib.VaekReplicas) == 64 and len(re.findall(r"typedef struct vaek_replicas", hdr)) == 1
    assert lib.vaek_train_step_max_replicas() == 256
    b, f = C.c_size_t(7), C.c_int32(7)
    assert lib.vaek_train_step_replicas_workspace_bytes(None, 4, C.byref(b)) == -1 and b.value == 7
    assert lib.vaek_supports_train_step_replicas(None, C.byref(f)) == -1 and f.value == 7
    assert lib.vaek_train_step_gen_replicas(None, None, None, None, None, None, None, None, None, None, 1e-3, None, 2, None, 3, 3, 3, 0.0,
                                            None, None, None, 0, None, 0, 0, None) == -1
    assert b"vaek_train_step_gen_replicas" in lib.vaek_last_error()


class _StubEngine:
    """What the two replica loops ask of an engine, on the CPU; records the library calls run() makes."""
    world, rank = 1, 0
    device = torch.device("cpu")
    train_loop_steps_per_launch = 1024
    train_loop_max_replicas = 1024
    train_step_max_replicas = 256
    step_path = "stub"

    def __init__(self, resident=False, mlp3=True, D=6, L=6, world=1):
        self._resident, self._mlp3, self.D, self.L, self.world, self.calls = resident, mlp3, D, L, world, []

    def supports_train_loop_gen(self, kind):
        return self._resident

    def supports_train_step_replicas(self):
        return self._mlp3

    def train_loop_replicas_workspace(self, n):
        return 0

    def train_step_replicas_workspace(self, n):
        return 64 * n

    def make_batch(self, kind, A, dd, did, pad, var, rows, seed, tag=0, row0=0, out=None, counter=None, which=0):
        self.calls.append(("make_batch", seed, None if A is None else float(A[0]), int(counter[which]), which))
        counter[which ^ 1] = counter[which] + 1
        for t in out:
            t.fill_(float(seed))

    def train_step_gen_replicas(self, params, grads, m, v, step_dev, cur, lr, kind, A, dd, did, pad, var, nxt, seeds, counter, which, **kw):
        assert cur[0].data_ptr() != nxt[0].data_ptr() and kw["workspace"].numel() == 64 * params.shape[0]
        self.calls.append(("train_step_gen_replicas", params.shape[0], which))
        counter[:, which ^ 1] = counter[:, which] + 1
        step_dev += 1                    # what the chain launch leaves in step_dev[r]
        params[:, :4] += 1.0

    def set_loss_history(self, buf):
        raise AssertionError("a replica loop must not touch the context-level ring")

    def train_step_gen(self, *a, **kw):
        raise AssertionError("one call for all replicas, not one per model")

    def train_loop_gen_replicas(self, params, grads, m, v, step_dev, n_steps, *a, **kw):
        self.calls.append(("train_loop_gen_replicas", n_steps, params.shape[0]))


def _model(eng, P=5, kind=0, seed=1, lr=1e-3, B=100):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=lr))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((9,), float(seed)), 3, 3, 3, 0.0), key=(seed, 2))
    module = types.SimpleNamespace(engine=lambda B_, gb: eng)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=(3, 4), num_batches=16,
                                 model=types.SimpleNamespace(module=module, flat=torch.zeros(P)))


def test_replica_graph_loop_makes_one_call_per_step():
    from vae_training_amd.trainer import ReplicaGraphLoop
    e = _StubEngine()
    ms = [_model(e, seed=s, lr=lr) for s, lr in ((69, 1e-3), (24, 2e-3), (48, 3e-3))]
    lp = ReplicaGraphLoop(ms, steps_per_graph=7, loss_capacity=8)
    # stacks of stride roundup4(P); an even graph length; GraphLoop's seed, model by model; every model's own lr and dataset matrix
    assert lp.R == 3 and lp.G == 8 and lp.stride == 8 and lp.params.shape == (3, 8) == lp.m.shape == lp.v.shape
    assert lp.grads.shape == (3, 9) and lp.rings.shape == (3, 8) and lp.counter.shape == (3, 2) and lp.workspace.numel() == 192
    assert [tuple(t.shape) for t in lp.bufs[0]] == [(3, 100, 6), (3, 100, 6), (3, 100, 6)] == [tuple(t.shape) for t in lp.bufs[1]]
    assert lp.seeds.tolist() == [s ^ 2 ^ 4 for s in (69, 24, 48)]
    assert lp.lrs.tolist() == pytest.approx([1e-3, 2e-3, 3e-3]) and lp.a_stride == 9 and lp.A[:, 0].tolist() == [69.0, 24.0, 48.0]
    ms[1].model.flat.fill_(5.0)
    lp.run(5); lp.run(0); lp.run(3)              # fewer than G + 1 steps per run: no capture (a hipGraph needs the GPU)
    lp.check()
    prime = [("make_batch", s ^ 2 ^ 4, float(s), 0, 0) for s in (69, 24, 48)]
    steps = [("train_step_gen_replicas", 3, (k + 1) % 2) for k in range(8)]
    assert e.calls == prime + steps, e.calls      # one draw per model before the first step, then ONE library call per step
    for r, m in enumerate(ms):
        # the host mirror, the device counter and the parameters all came back to the model's own tensors
        assert m.optimizer.state.step == 8 and int(m.optimizer.state.step_dev) == 8
        assert m.model.flat.tolist() == [(5.0 if r == 1 else 0.0) + 8.0] * 4 + [5.0 if r == 1 else 0.0]
    assert "3 replicas" in lp.describe() and lp.describe().startswith("hipGraph of 8 steps")
    assert lp.losses(1).numel() == 8 and lp.view(2).losses().numel() == 8
    assert ReplicaGraphLoop(ms).rings.shape == (3, 16) and ReplicaGraphLoop(ms).G == 200
    # a model whose step counter was changed between two runs has the batch buffers drawn afresh, from its new step
    del e.calls[:]
    ms[2].optimizer.state.step = 3
    ms[2].optimizer.state.step_dev.fill_(3)
    lp.run(1)
    assert [c[0] for c in e.calls] == ["make_batch"] * 3 + ["train_step_gen_replicas"] and [c[3] for c in e.calls[:3]] == [8, 8, 3]
    assert [m.optimizer.state.step for m in ms] == [9, 9, 4]


def test_replica_graph_loop_refusals():
    """The validation of ReplicaLoop, error for error."""
    from vae_training_amd.trainer import ReplicaGraphLoop
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaGraphLoop([_model(e), _model(e, P=6)])
    with pytest.raises(RuntimeError, match="shape"):                    # another batch size
        ReplicaGraphLoop([_model(e), _model(e, B=50)])
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaGraphLoop([_model(e), _model(e, kind=2)])
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaGraphLoop([_model(e), _model(_StubEngine(D=9))])
    with pytest.raises(RuntimeError, match="vaek_train_step_gen_replicas does not cover"):
        ReplicaGraphLoop([_model(_StubEngine(mlp3=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaGraphLoop([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="257 models"):
        ReplicaGraphLoop([_model(e) for _ in range(257)], loss_capacity=1)
    with pytest.raises(RuntimeError):
        ReplicaGraphLoop([])
    assert e.calls == []


def test_run_py_chooses_between_the_two_replica_loops():
    from vae_training_amd.run import build_parser, sweep_loop
    from vae_training_amd.trainer import ReplicaGraphLoop, ReplicaLoop
    both = _StubEngine(resident=True, mlp3=True)
    assert type(sweep_loop([_model(both), _model(both, seed=2)])) is ReplicaLoop            # today's behaviour where the resident loop covers
    only_mlp3 = _StubEngine(resident=False, mlp3=True)
    lp = sweep_loop([_model(only_mlp3), _model(only_mlp3, seed=2)])
    assert type(lp) is ReplicaGraphLoop and lp.R == 2 and only_mlp3.calls == []
    neither = _StubEngine(resident=False, mlp3=False)
    with pytest.raises(RuntimeError) as ei:
        sweep_loop([_model(neither)])
    assert "ReplicaLoop" in str(ei.value) and "ReplicaGraphLoop" in str(ei.value) and neither.calls == []
    with pytest.raises(RuntimeError, match="world"):                     # data parallelism: ReplicaLoop's own refusal, unchanged
        sweep_loop([_model(_StubEngine(resident=False, mlp3=True, world=2))])
    helptext = " ".join(build_parser().format_help().split())
    assert "ReplicaGraphLoop" in helptext and "ReplicaLoop" in helptext
