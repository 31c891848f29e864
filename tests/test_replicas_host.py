"""Host side of vaek_train_loop_gen_replicas, no GPU: the C ABI surface of the three entry points, trainer.ReplicaLoop on a stub
engine (which library calls run() makes, what it refuses) and run.py's --sweep_dataset_seeds flag."""
import os
import re
import types

import pytest
import torch

from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_train_loop_gen_replicas", "vaek_train_loop_max_replicas", "vaek_train_loop_replicas_workspace_bytes")


def test_abi_surface_of_the_replica_loop():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols: declared, bound with as many arguments, exported;
    the replica description is struct_size-guarded and the ctypes mirror has the header's fields in the header's order."""
    import ctypes as C

    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert _c_args(hdr, "vaek_train_loop_gen_replicas") == 19
    assert lib.vaek_train_loop_max_replicas() == 1024
    body = re.search(r"typedef struct vaek_replicas \{(.*?)\} vaek_replicas;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekReplicas._fields_], fields
    assert fields[0] == "struct_size" and set(fields) >= {"n", "state_stride", "grads_stride", "seeds", "lrs", "a_stride", "loss_hist",
                                                           "loss_hist_cap"}
    assert C.sizeof(_lib.VaekReplicas) == 64
    # argument checks that need no device: a NULL context is refused before anything is touched
    b = C.c_size_t(7)
    assert lib.vaek_train_loop_replicas_workspace_bytes(None, 4, C.byref(b)) == -1 and b.value == 7
    assert lib.vaek_train_loop_gen_replicas(None, None, None, None, None, None, None, 1, None, 3, 3, 3, 0.0, 0, 0, 1, 1e-3, None, None) == -1
    assert b"vaek_train_loop_gen_replicas" in lib.vaek_last_error()


class _StubEngine:
    """What ReplicaLoop asks of an engine, on the CPU; records the library calls run() makes."""
    world, rank = 1, 0
    device = torch.device("cpu")
    train_loop_steps_per_launch = 1024
    train_loop_max_replicas = 1024

    def __init__(self, resident=True, D=7, L=6, world=1):
        self._resident, self.D, self.L, self.world, self.calls = resident, D, L, world, []

    def supports_train_loop_gen(self, kind):
        return self._resident

    def train_loop_replicas_workspace(self, n):
        return 0

    def train_loop_gen_replicas(self, params, grads, m, v, step_dev, n_steps, *a, **kw):
        self.calls.append(("train_loop_gen_replicas", n_steps, params.shape[0]))
        step_dev += n_steps              # what the kernel leaves in step_dev[r]
        params += 1.0

    def set_loss_history(self, buf):
        raise AssertionError("the replica loop must not touch the context-level ring")

    def train_loop_gen(self, *a, **kw):
        raise AssertionError("one call for all replicas, not one per model")


def _model(eng, P=4, kind=1, seed=1, lr=1e-3, B=100):
    state = types.SimpleNamespace(step=0, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P), step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=lr))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), 3, 1, 3, 0.0), key=(seed, 2))
    module = types.SimpleNamespace(engine=lambda B_, gb: eng)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=(3, 4), num_batches=16,
                                 model=types.SimpleNamespace(module=module, flat=torch.zeros(P)))


def test_replica_loop_makes_one_call_per_run():
    from vae_training_amd.trainer import ReplicaLoop
    e = _StubEngine()
    ms = [_model(e, seed=s, lr=lr) for s, lr in ((69, 1e-3), (24, 2e-3), (48, 3e-3))]
    lp = ReplicaLoop(ms, loss_capacity=8)
    assert lp.R == 3 and lp.params.shape == (3, 4) and lp.grads.shape == (3, 8) and lp.rings.shape == (3, 8)
    # GraphLoop's seed, model by model; every model's own learning rate and dataset matrix
    assert lp.seeds.tolist() == [s ^ 2 ^ 4 for s in (69, 24, 48)]
    assert lp.lrs.tolist() == pytest.approx([1e-3, 2e-3, 3e-3]) and lp.a_stride == 3 and lp.A[:, 0].tolist() == [69.0, 24.0, 48.0]
    lp.run(5); lp.run(0); lp.run(3)
    lp.check()
    assert e.calls == [("train_loop_gen_replicas", 5, 3), ("train_loop_gen_replicas", 3, 3)]
    for m in ms:
        # the host mirror, the device counter and the parameters all came back to the model's own tensors
        assert m.optimizer.state.step == 8 and int(m.optimizer.state.step_dev) == 8 and m.model.flat.tolist() == [2.0] * 4
    assert "3 replicas" in lp.describe() and lp.describe().startswith("resident linear kernel")
    assert lp.losses(1).numel() == 8 and lp.view(2).losses().numel() == 8
    # without loss_capacity the rings hold every step of the schedule
    assert ReplicaLoop(ms).rings.shape == (3, 16)


def test_replica_loop_refusals():
    from vae_training_amd.trainer import ReplicaLoop
    e = _StubEngine()
    with pytest.raises(RuntimeError, match="shape"):                    # another parameter count
        ReplicaLoop([_model(e), _model(e, P=5)])
    with pytest.raises(RuntimeError, match="shape"):                    # another batch size
        ReplicaLoop([_model(e), _model(e, B=50)])
    with pytest.raises(RuntimeError, match="shape"):                    # another dataset kind
        ReplicaLoop([_model(e), _model(e, kind=0)])
    with pytest.raises(RuntimeError, match="shape"):                    # another data dimension
        ReplicaLoop([_model(e), _model(_StubEngine(D=9))])
    with pytest.raises(RuntimeError, match="vaek_train_loop_gen does not cover"):
        ReplicaLoop([_model(_StubEngine(resident=False))])
    with pytest.raises(RuntimeError, match="world"):
        ReplicaLoop([_model(_StubEngine(world=2))])
    with pytest.raises(RuntimeError, match="1025 models"):
        ReplicaLoop([_model(e) for _ in range(1025)], loss_capacity=1)
    with pytest.raises(RuntimeError):
        ReplicaLoop([])
    assert e.calls == []


def test_run_py_parses_the_sweep_flag():
    from vae_training_amd.run import parse_arguments
    base = ["sig", "--dataset", "sigmoid"]
    assert parse_arguments(base).sweep_dataset_seeds is None              # opt-in: without the flag nothing changes
    assert parse_arguments(base + ["--sweep_dataset_seeds", "69,24,48"]).sweep_dataset_seeds == [69, 24, 48]
    assert parse_arguments(base + ["--sweep_dataset_seeds", "7"]).sweep_dataset_seeds == [7]
    for bad in ("", "1,x"):
        with pytest.raises(SystemExit):
            parse_arguments(base + ["--sweep_dataset_seeds", bad])
