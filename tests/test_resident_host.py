"""Host side of vaek_train_loop_gen, no GPU: the C ABI surface of the two entry points, and which loop trainer.GraphLoop picks."""
import os
import types

import pytest
import torch

from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface_of_the_resident_loop():
    """include/vaek.h <-> the ctypes table <-> libvaek.so for the new symbols: declared, bound with as many arguments, exported;
    and the train-loop pair takes exactly the arguments of the train-steps pair it mirrors."""
    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    for name in ("vaek_supports_train_loop_gen", "vaek_train_loop_gen", "vaek_train_loop_steps_per_launch"):
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.load(), name), name
    assert _c_args(hdr, "vaek_train_loop_gen") == 19 and _c_args(hdr, "vaek_supports_train_loop_gen") == 3
    assert _lib.SIGNATURES["vaek_train_loop_gen"] == _lib.SIGNATURES["vaek_train_steps_gen"]
    assert _lib.SIGNATURES["vaek_supports_train_loop_gen"] == _lib.SIGNATURES["vaek_supports_train_steps_gen"]
    assert _lib.load().vaek_train_loop_steps_per_launch() == 1024


class _StubEngine:
    """What GraphLoop asks of an engine, on the CPU; records the library calls run() makes."""
    world, rank, D, L = 1, 0, 7, 6
    device = torch.device("cpu")
    train_loop_steps_per_launch = 1024

    def __init__(self, moments, resident):
        self._moments, self._resident, self.calls = moments, resident, []

    def supports_train_steps_gen(self, kind):
        return self._moments

    def supports_train_loop_gen(self, kind):
        return self._resident

    def set_loss_history(self, buf):
        pass

    def make_batch(self, *a, **kw):
        self.calls.append("make_batch")

    def train_steps_gen(self, *a, **kw):
        self.calls.append(("train_steps_gen", a[5]))

    def train_loop_gen(self, *a, **kw):
        self.calls.append(("train_loop_gen", a[5]))

    def train_step_gen(self, *a, **kw):
        self.calls.append("train_step_gen")


def _model(eng):
    z = torch.zeros(4)
    state = types.SimpleNamespace(step=0, grads=z, m=z, v=z, step_dev=torch.zeros(1, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=100, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (1, z, 3, 3, 3, 0.0), key=(1, 2))
    module = types.SimpleNamespace(engine=lambda B, gb: eng)
    return types.SimpleNamespace(dataset=ds, batch_size=100, optimizer=opt, key=(3, 4), model=types.SimpleNamespace(module=module, flat=z))


def test_graph_loop_takes_moments_first_resident_second_graph_last(monkeypatch):
    from vae_training_amd import trainer
    from vae_training_amd.trainer import GraphLoop
    # both available: the moments choice keeps priority, so every model that takes it today still does
    e = _StubEngine(True, True)
    lp = GraphLoop(_model(e), loss_capacity=8)
    assert lp.moments and not lp.resident and not lp.pipeline
    lp.run(7)
    assert e.calls == [("train_steps_gen", 7)] and "vaek_train_steps_gen" in lp.describe()
    with pytest.raises(RuntimeError):
        GraphLoop(_model(_StubEngine(True, True)), loss_capacity=8, resident=True)
    # ... and switching an available moments path off still means the per-sample hipGraph loop, unless the resident loop is asked for
    lp = GraphLoop(_model(_StubEngine(True, True)), loss_capacity=8, moments=False)
    assert not lp.moments and not lp.resident and lp.pipeline
    lp = GraphLoop(_model(_StubEngine(True, True)), loss_capacity=8, moments=False, resident=True)
    assert not lp.moments and lp.resident and not lp.pipeline
    # resident only: the default is the measurement's outcome; asked for, run(n) is ONE library call and check() polls nothing
    for default in (True, False):
        monkeypatch.setattr(trainer, "RESIDENT_DEFAULT", default)
        lp = GraphLoop(_model(_StubEngine(False, True)), loss_capacity=8)
        assert not lp.moments and lp.resident == default
    e = _StubEngine(False, True)
    m = _model(e)
    lp = GraphLoop(m, loss_capacity=8, resident=True)
    assert lp.resident and not lp.pipeline and not lp.bufs
    lp.run(5); lp.run(0); lp.run(3)
    lp.check()
    assert e.calls == [("train_loop_gen", 5), ("train_loop_gen", 3)] and m.optimizer.state.step == 8
    assert lp.describe() == "resident linear kernel, 1024 steps per launch"
    # switched off, or not supported: the hipGraph loop, which draws its first batch on construction
    e = _StubEngine(False, True)
    lp = GraphLoop(_model(e), loss_capacity=8, resident=False)
    assert not lp.resident and lp.pipeline and len(lp.bufs) == 2 and e.calls == ["make_batch"]
    e = _StubEngine(False, False)
    lp = GraphLoop(_model(e), loss_capacity=8)
    assert not lp.moments and not lp.resident and lp.pipeline and lp.describe().startswith("hipGraph of ")
    with pytest.raises(RuntimeError):
        GraphLoop(_model(_StubEngine(False, False)), loss_capacity=8, resident=True)
    with pytest.raises(RuntimeError):
        GraphLoop(_model(_StubEngine(False, False)), loss_capacity=8, moments=True)
