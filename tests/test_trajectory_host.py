"""Host side of the resident loop's trajectory ring, no GPU: the C ABI surface of the three new symbols, the slot rule, the loops on
stub engines (which library call run() makes, what trajectory() returns, what is refused), VAEModel's correlation ratio against a
float64 NumPy restatement of the reference's formula, and run.py's --trajectory_every flag."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.abi_util import _c_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vaek_trajectory_record_len", "vaek_train_loop_gen_traj", "vaek_train_loop_gen_replicas_traj")


def test_abi_surface_of_the_trajectory_ring():
    """include/vaek.h <-> the ctypes table <-> libvaek.so: declared, bound with as many arguments, exported; each traced entry takes
    its untraced twin's arguments plus one; vaek_trajectory is struct_size-guarded and its ctypes mirror has the header's fields in
    the header's order; a NULL context is refused before anything is touched, and traj == NULL is the plain call."""
    import ctypes as C

    from vae_training_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vaek.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert _c_args(hdr, name) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    for name in ("vaek_train_loop_gen", "vaek_train_loop_gen_replicas"):
        assert _c_args(hdr, name + "_traj") == _c_args(hdr, name) + 1 == 20
        assert _lib.SIGNATURES[name + "_traj"][1][:-1] == _lib.SIGNATURES[name][1]
        assert _lib.SIGNATURES[name + "_traj"][1][-1] is C.POINTER(_lib.VaekTrajectory)
    body = re.search(r"typedef struct vaek_trajectory \{(.*?)\} vaek_trajectory;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in _lib.VaekTrajectory._fields_] == ["struct_size", "every", "buf", "cap", "record_stride", "replica_stride"]
    assert C.sizeof(_lib.VaekTrajectory) == 40
    n = C.c_int64(7)
    assert lib.vaek_trajectory_record_len(None, C.byref(n)) == -1 and n.value == 7
    assert b"vaek_trajectory_record_len" in lib.vaek_last_error()
    tj = _lib.VaekTrajectory()
    tj.struct_size, tj.every, tj.cap, tj.record_stride = C.sizeof(_lib.VaekTrajectory), 1, 1, 1 << 20
    solo = (None, None, None, None, None, None, 1, None, 3, 3, 3, 0.0, 0, 0, 0, 1, 1e-3, None, None)
    reps = (None, None, None, None, None, None, None, 1, None, 3, 3, 3, 0.0, 0, 0, 1, 1e-3, None, None)
    assert lib.vaek_train_loop_gen_traj(*solo, C.byref(tj)) == -1 and b"vaek_train_loop_gen_traj" in lib.vaek_last_error()
    assert lib.vaek_train_loop_gen_replicas_traj(*reps, C.byref(tj)) == -1 and b"vaek_train_loop_gen_replicas_traj" in lib.vaek_last_error()
    # traj == NULL: the untraced entry answers, in its own name
    assert lib.vaek_train_loop_gen_traj(*solo, None) == -1 and lib.vaek_last_error().startswith(b"vaek_train_loop_gen:")
    assert lib.vaek_train_loop_gen_replicas_traj(*reps, None) == -1 and lib.vaek_last_error().startswith(b"vaek_train_loop_gen_replicas:")


def test_slot_rule():
    """Step t (1-based) with t % every == 0 -> slot (t / every - 1) % cap: the cases of tests/test_gpu_trajectory.py."""
    from vae_training_amd._lib import trajectory_slot as slot
    assert [slot(t, 1, 6) for t in range(0, 8)] == [None, 0, 1, 2, 3, 4, 5, 0]
    assert {t: slot(t, 3, 8) for t in range(1, 11) if slot(t, 3, 8) is not None} == {3: 0, 6: 1, 9: 2}          # n = 10 from step 0
    assert {t: slot(t, 3, 8) for t in range(8, 17) if slot(t, 3, 8) is not None} == {9: 2, 12: 3, 15: 4}        # resumed at 7, n = 9
    assert [slot(t, 2, 2) for t in (2, 4, 6, 8, 10)] == [0, 1, 0, 1, 0]                                         # cap 2, five records
    assert slot(1024, 512, 4) == 1 and slot(512, 512, 4) == 0 and slot(1025, 1025, 1) == 0 and slot(1024, 1025, 1) is None
    assert slot(0, 1, 4) is None and slot(-3, 3, 4) is None


def test_trajectory_view_reads_the_ring_in_step_order():
    """_trajectory_view on a host ring whose slot s holds the step that the slot rule puts there: the last `cap` records, oldest
    first, split at P and 2 P + 4 (a record stride above the length is skipped)."""
    from vae_training_amd._lib import trajectory_slot as slot
    from vae_training_amd.trainer import _trajectory_view
    P = 3

    def ring(cap, every, first, last, stride=2 * P + 4 + 2):
        r = torch.full((cap, stride), -1.0)
        for t in range(first + 1, last + 1):
            s = slot(t, every, cap)
            if s is not None:
                r[s, :P] = float(t)
                r[s, P:2 * P + 4] = float(-t)
        return r

    steps, th, g = _trajectory_view(ring(8, 3, 0, 10), 3, 0, 10, P)
    assert steps.tolist() == [3, 6, 9] and th.shape == (3, P) and g.shape == (3, P + 4)
    assert th[:, 0].tolist() == [3.0, 6.0, 9.0] and g[:, -1].tolist() == [-3.0, -6.0, -9.0]
    steps, th, g = _trajectory_view(ring(8, 3, 7, 16), 3, 7, 16, P)
    assert steps.tolist() == [9, 12, 15] and th[:, 0].tolist() == [9.0, 12.0, 15.0]
    steps, th, g = _trajectory_view(ring(2, 2, 0, 10), 2, 0, 10, P)                  # wrapped: the last two survive
    assert steps.tolist() == [8, 10] and th[:, 0].tolist() == [8.0, 10.0] and g[:, 0].tolist() == [-8.0, -10.0]
    steps, th, g = _trajectory_view(ring(4, 5, 0, 4), 5, 0, 4, P)                    # nothing recorded yet
    assert steps.numel() == 0 and th.shape == (0, P) and g.shape == (0, P + 4)


class _StubEngine:
    """What GraphLoop and ReplicaLoop ask of an engine, on the CPU; records the library calls run() makes."""
    world, rank = 1, 0
    device = torch.device("cpu")
    train_loop_steps_per_launch = 1024
    train_loop_max_replicas = 1024
    step_path = "linear"

    def __init__(self, moments=False, resident=True, P=4, D=7, L=6, world=1):
        self._moments, self._resident, self.P, self.D, self.L, self.world, self.calls = moments, resident, P, D, L, world, []

    @property
    def trajectory_record_len(self):
        return 2 * self.P + 4

    def supports_train_steps_gen(self, kind):
        return self._moments

    def supports_train_loop_gen(self, kind):
        return self._resident

    def supports_train_step_replicas(self):
        return False

    def set_loss_history(self, buf):
        pass

    def make_batch(self, *a, **kw):
        self.calls.append("make_batch")

    def train_loop_replicas_workspace(self, n):
        return 0

    def _record(self, t, ring, every):
        from vae_training_amd._lib import trajectory_slot
        s = trajectory_slot(t, every, ring.shape[0])
        if s is not None:
            ring[s, :self.P] = float(t - 1)              # "the state after t - 1 steps"
            ring[s, self.P:] = float(t)

    def train_loop_gen(self, params, grads, m, v, step_dev, n_steps, *a, trajectory=None, **kw):
        self.calls.append(("train_loop_gen", n_steps, None if trajectory is None else trajectory["every"]))
        for t in range(int(step_dev) + 1, int(step_dev) + n_steps + 1):
            if trajectory is not None:
                self._record(t, trajectory["buf"], trajectory["every"])
        step_dev += n_steps

    def train_loop_gen_replicas(self, params, grads, m, v, step_dev, n_steps, *a, trajectory=None, **kw):
        self.calls.append(("train_loop_gen_replicas", n_steps, None if trajectory is None else trajectory["every"]))
        for r in range(params.shape[0]):
            for t in range(int(step_dev[r]) + 1, int(step_dev[r]) + n_steps + 1):
                if trajectory is not None:
                    self._record(t, trajectory["buf"][r], trajectory["every"])
        step_dev += n_steps


def _model(eng, seed=1, num_batches=20, step=0, kind=1, B=100, dd=3):
    P = eng.P
    state = types.SimpleNamespace(step=step, grads=torch.zeros(P + 4), m=torch.zeros(P), v=torch.zeros(P),
                                  step_dev=torch.full((1,), step, dtype=torch.int32))
    opt = types.SimpleNamespace(global_batch=B, exchange=None, state=state, optimizer_def=types.SimpleNamespace(learning_rate=1e-3))
    ds = types.SimpleNamespace(device_spec=lambda: (kind, torch.full((3,), float(seed)), dd, 3, 3, 0.0), key=(seed, 2))
    module = types.SimpleNamespace(engine=lambda B_, gb: eng)
    return types.SimpleNamespace(dataset=ds, batch_size=B, optimizer=opt, key=(3, 4), num_batches=num_batches,
                                 model=types.SimpleNamespace(module=module, flat=torch.zeros(P)))


def test_graph_loop_owns_a_ring_and_stays_one_call_per_run():
    from vae_training_amd.trainer import GraphLoop
    e = _StubEngine()
    m = _model(e, num_batches=20)
    lp = GraphLoop(m, loss_capacity=8, resident=True, trajectory_every=4)
    assert lp.resident and lp.records_trajectory and lp.traj_ring.shape == (5, 12)          # ceil(20 / 4) records of 2 P + 4 floats
    assert lp.describe().startswith("resident linear kernel, 1024 steps per launch") and "every 4 steps" in lp.describe()
    lp.run(5); lp.run(0); lp.run(6)
    assert e.calls == [("train_loop_gen", 5, 4), ("train_loop_gen", 6, 4)] and m.optimizer.state.step == 11
    steps, th, g = lp.trajectory()
    assert steps.tolist() == [4, 8] and th.shape == (2, 4) and g.shape == (2, 8)
    assert th[:, 0].tolist() == [3.0, 7.0] and g[:, 0].tolist() == [4.0, 8.0]
    # a loop attached to a model that resumes at step 7: only this loop's steps count, in the slots the global step names
    e = _StubEngine()
    m = _model(e, num_batches=9, step=7)
    lp = GraphLoop(m, loss_capacity=8, resident=True, trajectory_every=3, trajectory_capacity=8)
    lp.run(9)
    assert lp.trajectory()[0].tolist() == [9, 12, 15] and lp.traj_ring[2:5, 0].tolist() == [8.0, 11.0, 14.0]
    # ceil, and a capacity the caller chooses; without the argument nothing is allocated and run() passes no trajectory
    assert GraphLoop(_model(_StubEngine(), num_batches=21), resident=True, loss_capacity=8, trajectory_every=4).traj_ring.shape[0] == 6
    assert GraphLoop(_model(_StubEngine()), resident=True, loss_capacity=8, trajectory_every=4, trajectory_capacity=2).traj_ring.shape[0] == 2
    e = _StubEngine()
    lp = GraphLoop(_model(e), loss_capacity=8, resident=True)
    lp.run(3)
    assert lp.traj_ring is None and not lp.records_trajectory and e.calls == [("train_loop_gen", 3, None)]
    assert lp.describe() == "resident linear kernel, 1024 steps per launch"
    with pytest.raises(RuntimeError, match="GraphLoop"):
        lp.trajectory()


def test_graph_loop_refusals_name_the_loop():
    from vae_training_amd.trainer import GraphLoop
    with pytest.raises(RuntimeError, match=r"GraphLoop\(resident=True\)"):          # a model the resident loop does not cover
        GraphLoop(_model(_StubEngine(resident=False)), loss_capacity=8, resident=True, trajectory_every=4)
    with pytest.raises(RuntimeError, match=r"GraphLoop\(trajectory_every=4\).*does not cover"):
        GraphLoop(_model(_StubEngine(resident=False)), loss_capacity=8, trajectory_every=4)
    with pytest.raises(RuntimeError, match=r"GraphLoop\(trajectory_every=4\).*resident=True"):      # covered, but not asked for
        GraphLoop(_model(_StubEngine()), loss_capacity=8, resident=False, trajectory_every=4)
    with pytest.raises(RuntimeError, match=r"GraphLoop\(trajectory_every=4\).*moments"):
        GraphLoop(_model(_StubEngine(moments=True)), loss_capacity=8, trajectory_every=4)
    with pytest.raises(RuntimeError, match=r"trajectory_every=0"):
        GraphLoop(_model(_StubEngine()), loss_capacity=8, resident=True, trajectory_every=0)
    with pytest.raises(RuntimeError, match="trajectory_capacity"):
        GraphLoop(_model(_StubEngine(), num_batches=0), loss_capacity=8, resident=True, trajectory_every=4)


def test_replica_loop_owns_a_ring_per_model():
    from vae_training_amd.trainer import ReplicaLoop
    e = _StubEngine()
    ms = [_model(e, seed=s, num_batches=nb) for s, nb in ((69, 20), (24, 22), (48, 20))]
    lp = ReplicaLoop(ms, trajectory_every=4)
    assert lp.traj_ring.shape == (3, 6, 12)                     # ceil(22 / 4): the longest schedule among the models
    lp.run(5); lp.run(7)
    assert e.calls == [("train_loop_gen_replicas", 5, 4), ("train_loop_gen_replicas", 7, 4)]
    for r in range(3):
        steps, th, g = lp.trajectory(r)
        assert steps.tolist() == [4, 8, 12] and th.shape == (3, 4) and g.shape == (3, 8) and g[:, 3].tolist() == [4.0, 8.0, 12.0]
        assert lp.view(r).records_trajectory and lp.view(r).trajectory()[0].tolist() == [4, 8, 12]
    assert "every 4 steps" in lp.describe() and "3 replicas" in lp.describe()
    plain = ReplicaLoop([_model(_StubEngine())])
    assert plain.traj_ring is None and not plain.view(0).records_trajectory
    with pytest.raises(RuntimeError, match="ReplicaLoop"):
        plain.trajectory(0)
    with pytest.raises(RuntimeError, match="ReplicaLoop: vaek_train_loop_gen does not cover"):
        ReplicaLoop([_model(_StubEngine(resident=False))], trajectory_every=4)
    with pytest.raises(RuntimeError, match=r"ReplicaLoop\(trajectory_every=-1\)"):
        ReplicaLoop([_model(_StubEngine())], trajectory_every=-1)


def _ratio_numpy(leaves, theta, g, star):
    """vae.py:143-179 restated leaf by leaf in float64 with plain loops of NumPy dot products (another summation order than the
    code under test, which runs one einsum per leaf over all records)."""
    inner, sq = 0.0, 0.0
    for name in ("Decoder/FC0/bias", "Decoder/FC0/kernel", "Encoder/FC0/bias", "Encoder/FC0/kernel", "epsilon", "epsilon_p"):
        if name not in leaves:
            assert name == "epsilon"
            continue
        off, shape = leaves[name]
        n = int(np.prod(shape))
        disp = star[off:off + n] - theta[off:off + n]
        sign = 1.0 if name == "epsilon" else -1.0
        inner += sign * float(np.dot(g[off:off + n][::-1], disp[::-1]))
        sq += float(np.linalg.norm(disp)) ** 2
    return inner / sq


@pytest.mark.parametrize("sig,tdv", [(True, True), (True, False), (False, True), (False, False)])
def test_correlation_ratios_against_a_float64_restatement(sig, tdv):
    """Random leaves, with and without a SigDecoder (never part of the ratio) and an `epsilon` leaf (left out without -tdv); both
    sides float64, differing in summation order only: relative 1e-12."""
    from vae_training_amd import layout
    from vae_training_amd.vae import correlation_ratios
    leaves, P = layout.leaves(7, 6, (), (), sig, tdv)
    rng = np.random.default_rng(3)
    n = 5
    theta = rng.standard_normal((n, P)).astype(np.float32)
    g = rng.standard_normal((n, P + 4)).astype(np.float32)
    star = rng.standard_normal(P).astype(np.float32)
    got = correlation_ratios(torch.from_numpy(theta), torch.from_numpy(g), torch.from_numpy(star), leaves)
    assert got.dtype == np.float64 and got.shape == (n,)
    want = np.array([_ratio_numpy(leaves, theta[i].astype(np.float64), g[i].astype(np.float64), star.astype(np.float64)) for i in range(n)])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    # the sign of the epsilon term is the reference's: flipping that gradient moves the ratio by twice the term
    if tdv:
        off = leaves["epsilon"][0]
        g2 = g.copy(); g2[:, off] = -g2[:, off]
        got2 = correlation_ratios(theta, g2, star, leaves)
        d = star.astype(np.float64)[off] - theta.astype(np.float64)[:, off]
        sq = np.array([_ratio_numpy(leaves, theta[i].astype(np.float64), np.zeros(P + 4), star.astype(np.float64)) for i in range(n)])
        assert np.all(sq == 0.0)
        norm2 = (got - got2) / (2.0 * g[:, off].astype(np.float64) * d)            # = 1 / squared norm, positive: the term enters with +
        assert np.all(norm2 > 0)
    # SigDecoder leaves do not enter: changing them changes nothing
    if sig:
        o, sh = leaves["SigDecoder/FC0/kernel"]
        th2 = theta.copy(); th2[:, o:o + int(np.prod(sh))] += 1.0
        assert np.array_equal(correlation_ratios(th2, g, star, leaves), got)
    with pytest.raises(KeyError, match="epsilon_p"):             # any other leaf missing is an error, not a shorter sum
        correlation_ratios(theta, g, star, {k: v for k, v in leaves.items() if k != "epsilon_p"})


def test_run_py_parses_the_trajectory_flag():
    from vae_training_amd.run import parse_arguments
    base = ["sig", "--dataset", "sigmoid"]
    assert parse_arguments(base).trajectory_every is None                 # opt-in: without the flag nothing changes
    assert parse_arguments(base + ["--trajectory_every", "5"]).trajectory_every == 5
    a = parse_arguments(base + ["--trajectory_every", "1", "--sweep_dataset_seeds", "69,24"])
    assert a.trajectory_every == 1 and a.sweep_dataset_seeds == [69, 24]
    for bad in ("0", "-2", "x", "1.5"):
        with pytest.raises(SystemExit):
            parse_arguments(base + ["--trajectory_every", bad])


def test_run_py_refuses_models_the_resident_loop_does_not_cover():
    """check_trajectory_model / sweep_loop on stub engines: refused before any library call, the message names the flag."""
    from vae_training_amd.run import check_trajectory_model, sweep_loop
    from vae_training_amd.trainer import ReplicaLoop
    for eng, kw in ((_StubEngine(resident=False), {}), (_StubEngine(world=2), {}), (_StubEngine(), dict(dd=17))):
        with pytest.raises(RuntimeError, match="--trajectory_every"):
            check_trajectory_model(_model(eng, **kw))
        with pytest.raises(RuntimeError, match="--trajectory_every"):
            sweep_loop([_model(eng, **kw)], trajectory_every=5)
        assert eng.calls == []
    e = _StubEngine()
    check_trajectory_model(_model(e))
    lp = sweep_loop([_model(e, seed=69), _model(e, seed=24)], trajectory_every=5)
    assert isinstance(lp, ReplicaLoop) and lp.traj_ring.shape == (2, 4, 12) and e.calls == []
    assert sweep_loop([_model(e, seed=69)]).traj_ring is None             # without the flag: today's loop


def test_write_trajectory_and_the_final_save(tmp_path):
    """run.py's write_trajectory on a stub loop: trajectory.npz holds steps, params, grads and the leaf table; and VAEModel's
    model_save_data(final=True) turns a recording loop's pairs into one Correlation Ratio per record (no GPU: the method is
    called on a bare object)."""
    from vae_training_amd import layout
    from vae_training_amd.run import write_trajectory
    from vae_training_amd.vae import VAEModel, correlation_ratios
    leaves, P = layout.leaves(3, 2, (), (), True, True)
    rng = np.random.default_rng(0)
    th, g = torch.from_numpy(rng.standard_normal((4, P)).astype(np.float32)), torch.from_numpy(rng.standard_normal((4, P + 4)).astype(np.float32))
    loop = types.SimpleNamespace(records_trajectory=True, trajectory=lambda: (torch.tensor([5, 10, 15, 20]), th, g), losses=lambda: torch.zeros(20))
    flat = torch.from_numpy(rng.standard_normal(P).astype(np.float32))
    m = types.SimpleNamespace(dirname=str(tmp_path), model=types.SimpleNamespace(flat=flat, module=types.SimpleNamespace(leaves=leaves)))
    write_trajectory(m, loop)
    z = np.load(os.path.join(str(tmp_path), "trajectory.npz"))               # no pickled objects in it
    assert z["steps"].tolist() == [5, 10, 15, 20] and z["params"].shape == (4, P) and z["grads"].shape == (4, P + 4)
    assert z["leaf_names"].tolist() == list(leaves) and z["leaf_offsets"].tolist() == [off for off, _ in leaves.values()]
    assert z["leaf_shapes"].tolist()[:2] == [[3, 2], [1, 2]] and int(np.prod(z["leaf_shapes"], axis=1).sum()) == P
    vm = VAEModel.__new__(VAEModel)
    vm.model, vm._graph_loop = m.model, loop
    vm.vae_losses, vm.var_dec, vm.var_enc, vm.correlation_ratios = [], [], [], []
    data = vm.model_save_data(final=True)
    assert np.array_equal(data["Correlation Ratio"], correlation_ratios(th, g, flat, leaves)) and np.isfinite(data["Correlation Ratio"]).all()
    assert "Correlation Ratio" not in vm.model_save_data(final=False)
    vm._graph_loop = types.SimpleNamespace(losses=lambda: torch.zeros(3))      # a loop that records nothing: empty, as today
    vm.correlation_ratios = []
    assert vm.model_save_data(final=True)["Correlation Ratio"] == []
