"""-m gpu: the trajectory ring of the resident loop -- vaek_train_loop_gen_traj, vaek_train_loop_gen_replicas_traj
(csrc/linear_resident.hip) -- and its callers: trainer.GraphLoop / ReplicaLoop with trajectory_every=K and `run.py --trajectory_every`.

The defining property is BITWISE, from the same start state and arguments:
  (a) the traced call leaves in params, m, v, grads, step_dev and the loss ring exactly what the untraced entry leaves;
  (b) for every recorded step t, record[0:P] equals the params an untraced call ending after t - 1 steps leaves and record[P:2P+4]
      the grads an untraced call ending after t steps leaves;
  (c) replica r's ring equals the ring of vaek_train_loop_gen_traj run alone on replica r's slices.
Every comparison is torch.equal.  The untraced references of a case (the state after k steps, for the k the tests ask for) are
computed once and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
SENT = -12345.0
NAMES = ("params", "grads", "m", "v", "step", "ring")
SOLO_LABEL, REPLICA_LABEL = "linear_resident_traj", "linear_resident_replicas_traj"


class _Case:
    """One engine and R models of its shape with random starts (randn * 0.3, as tests/test_gpu_resident.py), distinct seeds (one
    above 2^63), learning rates and dataset matrices; `warm` = {replica: step} resumes those replicas with a non-zero Adam counter
    and non-zero moments.  A state is [params [R, P], grads [R, P + 4], m, v, step [R], loss ring [R, 16]]."""

    def __init__(self, sig, kind, D, L, dd, pad, B, R=1, var=0.0, warm=None, tag=5, row0=1000):
        from vae_training_amd.engine import Engine
        self.eng = e = Engine(B, D, L, (), (), -3.0 if sig else -1.0, True, sig)
        assert e.supports_train_loop_gen(kind)
        self.kind, self.dd, self.did, self.pad, self.var, self.R, self.tag, self.row0 = kind, dd, dd, pad, var, R, tag, row0
        self.P, self.GL, self.len = e.P, e.grad_len, e.trajectory_record_len
        assert self.len == 2 * e.P + 4 == e.P + e.grad_len
        g = torch.Generator().manual_seed(11)
        alen = {0: dd * dd, 1: dd, 2: 0}[kind]
        self.A = torch.randn(R, alen, generator=g).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.seeds = [77 + 1000003 * r for r in range(R)]
        if R > 1:
            self.seeds[1] = 2 ** 63 + 5
        self.lrs = [LR * (1.0 + 0.5 * r) for r in range(R)]
        self.seeds_t, self.lrs_t = _i64(self.seeds), torch.tensor(self.lrs, dtype=torch.float32, device="cuda")
        self.p0 = (torch.randn(R, e.P, generator=g) * 0.3).cuda()
        self.m0, self.v0 = torch.zeros(R, e.P, device="cuda"), torch.zeros(R, e.P, device="cuda")
        self.step0 = torch.zeros(R, dtype=torch.int32, device="cuda")
        for r, step in (warm or {}).items():
            gw = torch.Generator().manual_seed(5 + r)
            self.m0[r] = (torch.randn(e.P, generator=gw) * 0.01).cuda()
            self.v0[r] = (torch.rand(e.P, generator=gw) * 1e-4).cuda()
            self.step0[r] = step
        nb = e.train_loop_replicas_workspace(R)
        self.ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
        self._refs = {}

    def state(self):
        return [self.p0.clone(), torch.zeros(self.R, self.GL, device="cuda"), self.m0.clone(), self.v0.clone(), self.step0.clone(),
                torch.zeros(self.R, 16, device="cuda")]

    def ring(self, cap, stride=None, R=None):
        """A sentinel-filled trajectory buffer: [cap, stride] or [R, cap, stride]."""
        shape = (cap, self.len if stride is None else stride)
        return torch.full(shape if R is None else (R,) + shape, SENT, dtype=torch.float32, device="cuda")

    def rows(self, st, r):
        return [st[0][r], st[1][r], st[2][r], st[3][r], st[4][r:r + 1], st[5][r]]

    def solo(self, st, r, n, traj=None):
        """vaek_train_loop_gen (traj: vaek_train_loop_gen_traj) in place on replica r's rows of `st`, its loss ring through
        vaek_set_loss_history."""
        b = self.rows(st, r)
        self.eng.set_loss_history(b[5])
        self.eng.train_loop_gen(*b[:5], n, self.lrs[r], self.kind, None if self.A is None else self.A[r], self.dd, self.did, self.pad,
                                self.var, self.seeds[r], tag=self.tag, row0=self.row0, trajectory=traj)
        torch.cuda.synchronize()
        self.eng.set_loss_history(None)

    def replicas(self, st, n, traj=None, **kw):
        a = dict(lrs=self.lrs_t, a_stride=self.a_stride, loss_hist=st[5], workspace=self.ws, tag=self.tag, row0=self.row0, trajectory=traj)
        a.update(kw)
        self.eng.train_loop_gen_replicas(*st[:5], n, 0.0, self.kind, self.A, self.dd, self.did, self.pad, self.var, self.seeds_t, **a)

    def ref(self, r, k):
        """Replica r's six buffers after k UNTRACED steps from the start state (k = 0: the start itself); computed once."""
        if (r, k) not in self._refs:
            st = self.state()
            if k:
                self.solo(st, r, k)
            self._refs[r, k] = [t.clone() for t in self.rows(st, r)]
        return self._refs[r, k]

    def check_record(self, rec, r, t):
        """Property (b) for one record of replica r and Adam step t (counted from the replica's start counter t0: the record is
        that of the (t - t0)-th step of a call from the start state)."""
        k = t - int(self.step0[r])
        theta, grads = self.ref(r, k - 1)[0], self.ref(r, k)[1]
        ok_p, ok_g = torch.equal(rec[:self.P], theta), torch.equal(rec[self.P:self.len], grads)
        print(f"  replica {r} step {t}: params {'equal' if ok_p else 'DIFFER'}, grads {'equal' if ok_g else 'DIFFER'}")
        assert ok_p and ok_g, (r, t)
        assert float(rec[2 * self.P + 3]) == 0.0 and bool(torch.isfinite(rec[:self.len]).all())


def _differing(a, b):
    return [what for x, y, what in zip(a, b, NAMES) if not torch.equal(x, y)]


SIG5 = dict(sig=True, kind=1, D=7, L=6, dd=3, pad=3, B=5)          # the first line of sigmoid_vae_padding_expts.sh, at batch 5


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "sig5":                  # two decoders, D = 7, L = 6: P + 4 = 157 < 256, one register slice per thread
        return _Case(**SIG5)
    if name == "sig5_resumed":
        return _Case(**SIG5, warm={0: 7})
    if name == "one28":                 # one decoder, D = 28, L = 24, batch 37: P + 4 = 1425, several slices per thread
        return _Case(False, 0, 28, 24, 8, 20, 37, var=0.25)
    if name == "sig5_r3":
        return _Case(**SIG5, R=3, warm={2: 7})
    if name == "staged_r3":             # two decoders, D = 28, L = 24, batch 37: the EXACT variant with the batch staged in memory
        return _Case(True, 1, 28, 24, 7, 20, 37, R=3, warm={1: 3})
    raise KeyError(name)


@pytest.mark.parametrize("name", ["sig5", "one28"])
def test_every_step_is_recorded(name):
    """every = 1, n = 6: record t against untraced calls of t - 1 and t steps (b), the final state against an untraced call (a)."""
    c = _case(name)
    assert (c.P + 4 < 256) == (name == "sig5")
    st, ring = c.state(), c.ring(6)
    c.solo(st, 0, 6, traj=(ring, 1))
    assert not _differing(c.rows(st, 0), c.ref(0, 6)), _differing(c.rows(st, 0), c.ref(0, 6))
    for t in range(1, 7):
        c.check_record(ring[t - 1], 0, t)
    assert not torch.equal(ring[0], ring[5])          # the model did move


def test_sparse_records_and_resume():
    """every = 3: n = 10 from step 0 records steps 3, 6, 9 in slots 0, 1, 2; resumed at step_dev = 7 with n = 9 it records steps 9, 12,
    15 in slots 2, 3, 4.  Every other slot keeps its sentinel."""
    c = _case("sig5")
    st, ring = c.state(), c.ring(8)
    c.solo(st, 0, 10, traj=(ring, 3))
    assert not _differing(c.rows(st, 0), c.ref(0, 10))
    for slot, t in ((0, 3), (1, 6), (2, 9)):
        c.check_record(ring[slot], 0, t)
    assert bool((ring[3:] == SENT).all())
    c = _case("sig5_resumed")
    st, ring = c.state(), c.ring(8)
    c.solo(st, 0, 9, traj=(ring, 3))
    assert int(st[4][0]) == 16 and not _differing(c.rows(st, 0), c.ref(0, 9))
    for slot, t in ((2, 9), (3, 12), (4, 15)):
        c.check_record(ring[slot], 0, t)
    assert bool((ring[:2] == SENT).all()) and bool((ring[5:] == SENT).all())


def test_ring_wrap_keeps_the_last_records():
    """cap = 2, every = 2, n = 10: five records; step 10's is in slot (5 - 1) % 2 = 0, step 8's in slot 1."""
    c = _case("sig5")
    st, ring = c.state(), c.ring(2)
    c.solo(st, 0, 10, traj=(ring, 2))
    assert not _differing(c.rows(st, 0), c.ref(0, 10))
    c.check_record(ring[0], 0, 10)
    c.check_record(ring[1], 0, 8)


def test_padding_and_unhit_slots_keep_their_sentinel():
    """record_stride = len + 5 (solo and replicas) and replica_stride = cap * record_stride + 7: the floats between two records and
    between two rings, and slot 2 (cap = 3, every = 2, n = 4 hits slots 0 and 1), keep the sentinel."""
    c = _case("sig5_r3")
    rs, cap = c.len + 5, 3
    st, ring = c.state(), c.ring(cap, rs)
    c.solo(st, 0, 4, traj=dict(buf=ring, every=2))
    c.check_record(ring[0], 0, 2)
    c.check_record(ring[1], 0, 4)
    assert bool((ring[:2, c.len:] == SENT).all()) and bool((ring[2] == SENT).all())
    stride = cap * rs + 7
    flat = torch.full((c.R * stride,), SENT, dtype=torch.float32, device="cuda")
    st = c.state()
    c.replicas(st, 4, traj=dict(buf=flat, every=2, cap=cap, record_stride=rs, replica_stride=stride))
    torch.cuda.synchronize()
    per = flat.view(c.R, stride)
    assert bool((per[:, cap * rs:] == SENT).all()), "floats between two rings were written"
    rings = per[:, :cap * rs].reshape(c.R, cap, rs)
    assert bool((rings[:, :2, c.len:] == SENT).all()), "floats between two records were written"
    for r in range(c.R):
        t0 = int(c.step0[r])                       # replica 2 resumes at 7: its calls' steps are 8 .. 11, recorded 8 and 10 in slots 3 % 3, 4 % 3
        hit = {(t // 2 - 1) % cap: t for t in range(t0 + 1, t0 + 5) if t % 2 == 0}
        for slot in range(cap):
            if slot in hit:
                c.check_record(rings[r, slot], r, hit[slot])
            else:
                assert bool((rings[r, slot] == SENT).all()), (r, slot)


def test_records_across_the_launch_boundary():
    """n = 1027 at batch 5 is two launches (1024 + 3).  every = 512: step 1024 is the first launch's last step; every = 1025: the only
    record falls in the second launch.  Two profile records under the traced label."""
    c = _case("sig5")
    assert c.eng.train_loop_steps_per_launch == 1024
    st, ring = c.state(), c.ring(2)
    c.solo(st, 0, 1, traj=(c.ring(1), 1))          # warm-up outside the profile (lazy kernel attributes)
    st = c.state()
    c.eng.profile_begin(64)
    c.solo(st, 0, 1027, traj=(ring, 512))
    rep = c.eng.profile_report()
    assert set(rep) == {SOLO_LABEL} and rep[SOLO_LABEL]["count"] == 2, rep
    assert not _differing(c.rows(st, 0), c.ref(0, 1027)), _differing(c.rows(st, 0), c.ref(0, 1027))
    c.check_record(ring[0], 0, 512)
    c.check_record(ring[1], 0, 1024)
    st, ring = c.state(), c.ring(1)
    c.solo(st, 0, 1027, traj=(ring, 1025))
    assert not _differing(c.rows(st, 0), c.ref(0, 1027))
    c.check_record(ring[0], 0, 1025)


@pytest.mark.parametrize("name,n", [("sig5_r3", 9), ("staged_r3", 4)])
def test_replica_rings_equal_solo_rings(name, n):
    """R = 3 with distinct seeds, learning rates, dataset matrices and starts (one replica resumed), every = 2: (c) replica r's ring
    and state equal those of the solo traced entry on its slices; (a) the state equals the untraced replica entry's.  `staged_r3`
    is the two-decoder D = 28, L = 24 variant whose batch image lives in the workspace, one region per replica."""
    c = _case(name)
    assert (c.eng.train_loop_replicas_workspace(1) > 0) == (name == "staged_r3")
    cap = 4
    st, rings = c.state(), c.ring(cap, R=c.R)
    c.eng.profile_begin(16)
    c.replicas(st, n, traj=(rings, 2))
    rep = c.eng.profile_report()
    assert set(rep) == {REPLICA_LABEL} and rep[REPLICA_LABEL]["count"] == 1, rep
    plain = c.state()
    c.replicas(plain, n)
    torch.cuda.synchronize()
    assert not _differing(st, plain), _differing(st, plain)                                        # (a)
    for r in range(c.R):
        alone, ring = c.state(), c.ring(cap)
        c.solo(alone, r, n, traj=(ring, 2))
        assert torch.equal(rings[r], ring), r                                                       # (c)
        assert not _differing(c.rows(st, r), c.rows(alone, r)), (r, _differing(c.rows(st, r), c.rows(alone, r)))
        t0 = int(c.step0[r])
        for t in [t for t in range(t0 + 1, t0 + n + 1) if t % 2 == 0][-cap:]:
            c.check_record(ring[(t // 2 - 1) % cap], r, t)                                          # (b), through the solo refs
    assert not torch.equal(rings[0], rings[1])          # another seed, another start: another trajectory


def test_traced_call_is_capturable():
    """A 4-step traced call with every = 2 captured on a side stream; two replays from a fresh state against 8 eager steps: the
    records of steps 2, 4, 6, 8 (the slot comes from the device-resident counter) and the final state are equal."""
    c = _case("sig5")
    b, ring_b = c.state(), c.ring(4)
    c.solo(b, 0, 8, traj=(ring_b, 2))               # eager (also the warm-up: lazy kernel attributes)
    a, ring_a = c.state(), c.ring(4)
    rows = c.rows(a, 0)
    c.eng.set_loss_history(rows[5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.eng.train_loop_gen(*rows[:5], 4, c.lrs[0], c.kind, c.A[0], c.dd, c.did, c.pad, c.var, c.seeds[0], tag=c.tag, row0=c.row0,
                                 trajectory=(ring_a, 2))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(a[4][0]) == 0 and bool((ring_a == SENT).all())          # capture does not execute
    g.replay(); g.replay()
    torch.cuda.synchronize()
    c.eng.set_loss_history(None)
    assert torch.equal(ring_a, ring_b) and not _differing(a, b), _differing(a, b)
    for slot, t in enumerate((2, 4, 6, 8)):
        c.check_record(ring_a[slot], 0, t)


def test_arguments():
    """Every refusal of include/vaek.h returns VAEK_ERR_INVALID with a message and leaves every buffer, the trajectory ring
    included, untouched; n_steps = 0 returns OK and touches nothing; traj = NULL is the untraced entry."""
    import ctypes as C

    from vae_training_amd import _lib
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c = _case("sig5_r3")
    e = c.eng

    def refused(why, replicas, traj, eng=None, **kw):
        st = c.state()
        ring = traj.get("buf")
        before, ring_before = [t.clone() for t in st], None if ring is None else ring.clone()
        with pytest.raises(VaekError) as ei:
            if replicas:
                (eng or e).train_loop_gen_replicas(*st[:5], 2, 0.0, kw.pop("kind", c.kind), c.A, c.dd, c.did, c.pad, c.var, c.seeds_t,
                                                   lrs=c.lrs_t, a_stride=c.a_stride, loss_hist=st[5], workspace=c.ws, trajectory=traj, **kw)
            else:
                b = c.rows(st, 0)
                (eng or e).train_loop_gen(*b[:5], 2, LR, kw.pop("kind", c.kind), c.A[0], c.dd, c.did, c.pad, c.var, c.seeds[0], trajectory=traj, **kw)
        assert ei.value.code == -1, (why, ei.value)                      # VAEK_ERR_INVALID
        assert len(str(ei.value)) > len("libvaek error -1: "), why
        torch.cuda.synchronize()
        assert not _differing(st, before), why
        assert ring is None or torch.equal(ring, ring_before), why

    for replicas in (False, True):
        ring = c.ring(4, R=c.R) if replicas else c.ring(4)
        ok = dict(buf=ring, every=2)
        refused("every = 0", replicas, dict(ok, every=0))
        refused("every = -1", replicas, dict(ok, every=-1))
        refused("cap = 0", replicas, dict(ok, cap=0))
        refused("cap = -2", replicas, dict(ok, cap=-2))
        refused("NULL buf", replicas, dict(buf=None, every=2, cap=4, record_stride=c.len, replica_stride=4 * c.len))
        refused("record_stride < len", replicas, dict(ok, record_stride=c.len - 1))
        refused("struct_size", replicas, dict(ok, struct_size=12))
        # everything the untraced entry refuses
        refused("kind 3", replicas, ok, kind=3)
        for why, eng in [("B = 257", Engine(257, 7, 6, (), (), -3.0, True, True)), ("one hidden layer", Engine(5, 7, 6, (64,), (64,), -3.0, True, True)),
                         ("force_generic", Engine(5, 7, 6, (), (), -3.0, True, True, force_generic=True))]:
            assert not eng.supports_train_loop_gen(1), why
            refused(why, replicas, ok, eng=eng)
    ring = c.ring(4, R=c.R)
    refused("replica_stride < cap * record_stride", True, dict(buf=ring, every=2, replica_stride=4 * c.len - 1))
    refused("no replicas", True, dict(buf=ring, every=2), n=0)
    refused("state_stride < P", True, dict(buf=ring, every=2), state_stride=c.P - 1)
    # the solo entry ignores replica_stride
    st, ring = c.state(), c.ring(4)
    c.solo(st, 0, 2, traj=dict(buf=ring, every=2, replica_stride=0))
    c.check_record(ring[0], 0, 2)
    # n_steps = 0: OK, nothing changes
    for replicas in (False, True):
        st = c.state()
        ring = c.ring(4, R=c.R) if replicas else c.ring(4)
        before = [t.clone() for t in st]
        if replicas:
            c.replicas(st, 0, traj=(ring, 1))
        else:
            c.solo(st, 0, 0, traj=(ring, 1))
        torch.cuda.synchronize()
        assert not _differing(st, before) and bool((ring == SENT).all())
    # traj = NULL through the traced symbols: the untraced entries
    ptr = lambda t: C.c_void_p(t.data_ptr())
    st = c.state()
    b = c.rows(st, 0)
    e.set_loss_history(b[5])
    rc = e.lib.vaek_train_loop_gen_traj(e.h, *[ptr(t) for t in b[:5]], c.kind, ptr(c.A[0]), c.dd, c.did, c.pad, c.var, c.row0, c.seeds[0], c.tag, 4,
                                        c.lrs[0], ptr(e.workspace), None, None)
    torch.cuda.synchronize()
    e.set_loss_history(None)
    assert rc == 0 and not _differing(b, c.ref(0, 4)), _differing(b, c.ref(0, 4))
    st, plain = c.state(), c.state()
    rep = _lib.VaekReplicas()
    rep.struct_size, rep.n, rep.state_stride, rep.grads_stride = C.sizeof(_lib.VaekReplicas), c.R, c.P, c.GL
    rep.seeds, rep.lrs, rep.a_stride, rep.loss_hist, rep.loss_hist_cap = c.seeds_t.data_ptr(), c.lrs_t.data_ptr(), c.a_stride, st[5].data_ptr(), 16
    rc = e.lib.vaek_train_loop_gen_replicas_traj(e.h, *[ptr(t) for t in st[:5]], C.byref(rep), c.kind, ptr(c.A), c.dd, c.did, c.pad, c.var, c.row0,
                                                 c.tag, 4, 0.0, None, None, None)
    c.replicas(plain, 4)
    torch.cuda.synchronize()
    assert rc == 0 and not _differing(st, plain), _differing(st, plain)


def _sigmoid_model(tmp_path, name, seed, lr=LR, num_batches=12):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([name, "--dataset", "sigmoid", "--padding_dim", "3", "-dd", "3"])
    ds = get_dataset("sigmoid", seed, 3, 100, args)
    d = tmp_path / name
    d.mkdir()
    return VAEModel(dirname=str(d), num_batches=num_batches, num_epochs=1, batch_size=100, learning_rate=lr, layer_sizes="",
                    encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=6, tunable_decoder_var=True, dataset_name="sigmoid", fast_loop=True)


def test_graph_loop_trajectory_equals_a_hand_cut_loop(tmp_path):
    """GraphLoop(resident=True, trajectory_every=4) run 12 steps in two calls against a twin cut by hand at steps 3, 4, 7, 8, 11, 12:
    the record of step t holds the twin's parameters after t - 1 steps and its grads after t; the final states are equal."""
    from vae_training_amd.trainer import GraphLoop
    a, b = _sigmoid_model(tmp_path, "a", 69), _sigmoid_model(tmp_path, "b", 69)
    lp = GraphLoop(a, resident=True, loss_capacity=12, trajectory_every=4)
    assert lp.traj_ring.shape == (3, lp.eng.trajectory_record_len) and "every 4 steps" in lp.describe()
    lp.run(5); lp.run(7)
    steps, th, g = lp.trajectory()
    assert steps.tolist() == [4, 8, 12] and th.shape == (3, a.model.flat.numel()) and g.shape == (3, a.model.flat.numel() + 4)
    cut = GraphLoop(b, resident=True, loss_capacity=12)
    for i in range(3):
        cut.run(3)
        torch.cuda.synchronize()
        assert torch.equal(th[i], b.model.flat.cpu()), i
        cut.run(1)
        torch.cuda.synchronize()
        assert torch.equal(g[i], b.optimizer.state.grads.cpu()), i
    sa, sb = a.optimizer.state, b.optimizer.state
    got, want = [a.model.flat, sa.grads, sa.m, sa.v, sa.step_dev, lp.losses()], [b.model.flat, sb.grads, sb.m, sb.v, sb.step_dev, cut.losses()]
    assert not _differing(got, want), _differing(got, want)
    ratios = a.compute_correlation_ratios(th, g)
    assert ratios.shape == (3,) and np.isfinite(ratios).all()


def test_replica_loop_trajectories_equal_three_solo_loops(tmp_path):
    """ReplicaLoop(trajectory_every=4) over three sigmoid models against three twins each in its own
    GraphLoop(resident=True, trajectory_every=4): steps, params and grads bitwise per model."""
    from vae_training_amd.trainer import GraphLoop, ReplicaLoop
    spec = [(69, 1e-3), (24, 2e-3), (48, 5e-4)]
    swept = [_sigmoid_model(tmp_path, f"s{s}", s, lr) for s, lr in spec]
    twins = [_sigmoid_model(tmp_path, f"t{s}", s, lr) for s, lr in spec]
    lp = ReplicaLoop(swept, trajectory_every=4)
    assert lp.traj_ring.shape == (3, 3, lp.eng.trajectory_record_len)
    lp.run(5); lp.run(7)
    for r, tw in enumerate(twins):
        gl = GraphLoop(tw, resident=True, loss_capacity=12, trajectory_every=4)
        gl.run(12)
        got, want = lp.trajectory(r), gl.trajectory()
        assert got[0].tolist() == want[0].tolist() == [4, 8, 12]
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), r
        assert torch.equal(swept[r].model.flat, tw.model.flat)
    assert not torch.equal(lp.trajectory(0)[1], lp.trajectory(1)[1])


RUN_LINE = ["--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "", "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3",
            "--epsilon", "-3", "-tdv", "--num_batches", "20", "--trajectory_every", "5"]
P_SIG = 7 * 6 + 6 + 2 * (6 * 7 + 7) + 6 + 1


def _check_outputs(d):
    z = np.load(os.path.join(d, "trajectory.npz"))
    assert z["steps"].tolist() == [5, 10, 15, 20]
    assert z["params"].shape == (4, P_SIG) and z["grads"].shape == (4, P_SIG + 4)
    assert np.isfinite(z["params"]).all() and np.isfinite(z["grads"]).all()
    assert "epsilon" in z["leaf_names"].tolist() and z["leaf_offsets"].shape == z["leaf_names"].shape and z["leaf_shapes"].shape == (len(z["leaf_names"]), 2)
    assert int(np.prod(z["leaf_shapes"], axis=1).sum()) == P_SIG
    losses = np.load(os.path.join(d, "losses.npz"), allow_pickle=True)
    ratio = np.asarray(losses["Correlation Ratio"], dtype=np.float64)
    assert ratio.shape == (4,) and np.isfinite(ratio).all(), ratio
    assert np.asarray(losses["VAE Loss"], dtype=np.float64).size == 21          # one evaluation loss, then the 20 train losses
    return z


def test_run_py_trajectory_in_a_fresh_process(tmp_path):
    """The first line of sigmoid_vae_padding_expts.sh, 20 batches, --trajectory_every 5, in a fresh process."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "sig"] + RUN_LINE
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train loop:")]
    assert len(lines) == 1 and lines[0].startswith("Train loop: resident linear kernel") and "every 5 steps" in lines[0], r.stdout[-1500:]
    _check_outputs(os.path.join(str(tmp_path), "data", "sig"))


def test_run_py_trajectory_sweep_in_a_fresh_process(tmp_path):
    """The same with --sweep_dataset_seeds 69,24: one trajectory.npz and one Correlation Ratio per output directory."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "sig"] + RUN_LINE + ["--sweep_dataset_seeds", "69,24"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train loop:")]
    assert len(lines) == 1 and "2 replicas" in lines[0] and "every 5 steps" in lines[0], r.stdout[-1500:]
    z = [_check_outputs(os.path.join(str(tmp_path), "data", f"sig_ds{seed}")) for seed in (69, 24)]
    assert not np.array_equal(z[0]["params"], z[1]["params"])          # two datasets, two runs
