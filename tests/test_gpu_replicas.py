"""-m gpu: vaek_train_loop_gen_replicas -- N independent small-batch linear VAEs of one shape trained by ONE launch of the resident
loop (csrc/linear_resident.hip), workgroup r training replica r -- and its callers, trainer.ReplicaLoop and
`run.py --sweep_dataset_seeds`.

The defining property is BITWISE: what the call leaves in replica r's params, m, v, grads, step_dev[r] and loss ring is what
vaek_train_loop_gen leaves when called alone on those buffers with seeds[r], lrs[r] and replica r's dataset matrix -- the same code
on the same inputs.  Every comparison below is torch.equal; the floats that lie between two replicas where a stride exceeds the
length hold a sentinel that must survive."""
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
SIG_ROW = dict(sig=True, kind=1, D=7, L=6, dd=3, pad=3, B=100)      # the first line of sigmoid_vae_padding_expts.sh
LABEL = "linear_resident_replicas"


def _engine(sig, D, L, B, **kw):
    from vae_training_amd.engine import Engine
    return Engine(B, D, L, (), (), -3.0 if sig else -1.0, True, sig, **kw)


class _Sweep:
    """One engine, R replicas with random starts (randn * 0.3, as tests/test_gpu_resident.py), distinct seeds (one of them above
    2^63), learning rates and dataset matrices, in stacks whose strides exceed the lengths by `extra` floats of sentinel."""

    def __init__(self, sig, kind, D, L, dd, pad, B, R, var=0.0, extra=(5, 3), tag=5, row0=1000):
        self.eng = e = _engine(sig, D, L, B)
        assert e.supports_train_loop_gen(kind)
        self.kind, self.dd, self.did, self.pad, self.var, self.R, self.tag, self.row0 = kind, dd, dd, pad, var, R, tag, row0
        self.P, self.GL = e.P, e.grad_len
        self.ss, self.gs = e.P + extra[0], e.grad_len + extra[1]
        g = torch.Generator().manual_seed(11)
        alen = {0: dd * dd, 1: dd, 2: 0}[kind]
        self.A = torch.randn(R, alen, generator=g).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.seeds = [77 + 1000003 * r for r in range(R)]
        if R > 1:
            self.seeds[1] = 2 ** 63 + 5
        self.lrs = [LR * (1.0 + 0.5 * (r % 7)) for r in range(R)]
        self.p0 = (torch.randn(R, e.P, generator=g) * 0.3).cuda()
        self.m0 = torch.zeros(R, e.P, device="cuda")
        self.v0 = torch.zeros(R, e.P, device="cuda")
        self.step0 = torch.zeros(R, dtype=torch.int32, device="cuda")
        nb = e.train_loop_replicas_workspace(R)
        self.ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
        self._tables = {}

    def warm(self, r, m_scale=0.01, v_scale=1e-4, step=7):
        """Replica r resumes a run: a non-zero Adam counter and non-zero moments."""
        g = torch.Generator().manual_seed(5 + r)
        self.m0[r] = (torch.randn(self.P, generator=g) * m_scale).cuda()
        self.v0[r] = (torch.rand(self.P, generator=g) * v_scale).cuda()
        self.step0[r] = step

    def state(self, cap):
        def stack(init, width, stride):
            t = torch.full((self.R, stride), SENT, dtype=torch.float32, device="cuda")
            t[:, :width] = init
            return t
        return [stack(self.p0, self.P, self.ss), stack(0.0, self.GL, self.gs), stack(self.m0, self.P, self.ss), stack(self.v0, self.P, self.ss),
                self.step0.clone(), torch.zeros(self.R, cap, dtype=torch.float32, device="cuda")]

    def tables(self, seeds=None):
        """The device tables of seeds and learning rates, built once per content: a call under stream capture must find them
        made (a host-to-device copy is not capturable)."""
        key = tuple(self.seeds if seeds is None else seeds), tuple(self.lrs)
        if key not in self._tables:
            self._tables[key] = (_i64(key[0]), torch.tensor(self.lrs, dtype=torch.float32, device="cuda"))
        return self._tables[key]

    def replicas(self, st, n, lrs="own", a_stride=None, seeds=None, lr=0.0, A="own"):
        seeds_t, lrs_t = self.tables(seeds)
        self.eng.train_loop_gen_replicas(*st[:5], n, lr, self.kind, self.A if isinstance(A, str) else A, self.dd, self.did, self.pad, self.var,
                                         seeds_t, lrs=lrs_t if isinstance(lrs, str) else lrs,
                                         a_stride=self.a_stride if a_stride is None else a_stride, loss_hist=st[5], workspace=self.ws,
                                         tag=self.tag, row0=self.row0)

    def single(self, st0, r, n, seed=None, lr=None, A="own"):
        """vaek_train_loop_gen alone on copies of replica r's slices of the START state st0 (its ring through
        vaek_set_loss_history); returns the six buffers it leaves."""
        P, GL = self.P, self.GL
        b = [st0[0][r, :P].clone(), st0[1][r, :GL].clone(), st0[2][r, :P].clone(), st0[3][r, :P].clone(), st0[4][r:r + 1].clone(), st0[5][r].clone()]
        Ar = (None if self.A is None else self.A[r].clone()) if isinstance(A, str) else A
        self.eng.set_loss_history(b[5])
        self.eng.train_loop_gen(*b[:5], n, self.lrs[r] if lr is None else lr, self.kind, Ar, self.dd, self.did, self.pad, self.var,
                                self.seeds[r] if seed is None else seed, tag=self.tag, row0=self.row0)
        torch.cuda.synchronize()
        self.eng.set_loss_history(None)
        return b

    def rows(self, st, r):
        return [st[0][r, :self.P], st[1][r, :self.GL], st[2][r, :self.P], st[3][r, :self.P], st[4][r:r + 1], st[5][r]]

    def sentinels_intact(self, st):
        return all(bool((t[:, w:] == SENT).all()) for t, w in ((st[0], self.P), (st[1], self.GL), (st[2], self.P), (st[3], self.P)))


def _differing(a, b):
    return [what for x, y, what in zip(a, b, NAMES) if not torch.equal(x, y)]


def _assert_replicas_equal_singles(sw, start, done, n, which=None):
    bad = {}
    for r in (range(sw.R) if which is None else which):
        d = _differing(sw.rows(done, r), sw.single(start, r, n))
        if d:
            bad[r] = d
    print(f"replicas against single calls, n = {n}: " + (f"buffers that differ, by replica: {bad}" if bad else "all bitwise equal"))
    assert not bad, bad


def _equal_singles_with_guards(sw, n, cap):
    """The replica call on a fresh state against single calls, with the sentinels between replicas and a sentinel-filled ring of
    vaek_set_loss_history (the ctx-level ring, which the replica call must not write) checked after it."""
    start, st = sw.state(cap), sw.state(cap)
    ctx_ring = torch.full((cap,), SENT, dtype=torch.float32, device="cuda")
    sw.eng.set_loss_history(ctx_ring)
    sw.replicas(st, n)
    torch.cuda.synchronize()
    sw.eng.set_loss_history(None)
    assert bool((ctx_ring == SENT).all()), "the replica call wrote the ring of vaek_set_loss_history"
    assert sw.sentinels_intact(st), "floats between two replicas were written"
    _assert_replicas_equal_singles(sw, start, st, n)
    for r in range(sw.R):
        t0 = int(start[4][r])
        assert int(st[4][r]) == t0 + n
        ring = st[5][r]
        idx = [(t0 + k) % cap for k in range(n)]
        assert bool(torch.isfinite(ring).all()) and bool((ring[idx] != 0).all())
    return st


def test_replicas_equal_single_calls():
    """R = 5 on the first sigmoid row, n = 9: distinct seeds, learning rates, dataset matrices and starts; replica 2 resumes at
    step 7 with non-zero m and v; state_stride = P + 5 and grads_stride = grad_len + 3 (the kernel needs no alignment of either)."""
    sw = _Sweep(**SIG_ROW, R=5)
    sw.warm(2)
    assert sw.ws is None and sw.eng.train_loop_replicas_workspace(5) == 0      # this variant's batch image fits LDS
    st = _equal_singles_with_guards(sw, 9, 16)
    assert st[4].tolist() == [9, 9, 16, 9, 9]
    # the replicas did train differently from each other
    assert len({float(st[5][r][(int(st[4][r]) - 1) % 16]) for r in range(5)}) == 5


def test_replicas_of_the_staged_variant_have_their_own_stage():
    """D = 28, L = 24, two decoders: the EXACT variant, whose batch image lives in the workspace -- replicas sharing one region
    would train on each other's batches."""
    import ctypes as C
    sw = _Sweep(True, 1, 28, 24, 7, 20, 100, R=3)
    e = sw.eng
    one = e.train_loop_replicas_workspace(1)
    assert one > 0 and one % 16 == 0 and [e.train_loop_replicas_workspace(n) for n in (2, 3, 1024)] == [2 * one, 3 * one, 1024 * one]
    assert one == 4 * (2 * 2800 + 2400)
    ws = C.c_size_t()
    assert e.lib.vaek_workspace_bytes(e.h, C.byref(ws)) == 0 and e.workspace.numel() == max(ws.value, 256)
    sw.warm(1, step=3)
    _equal_singles_with_guards(sw, 3, 8)
    ws2 = C.c_size_t()
    assert e.lib.vaek_workspace_bytes(e.h, C.byref(ws2)) == 0 and ws2.value == ws.value      # the context's workspace is what it was


def test_more_workgroups_than_cus():
    """R = 300 > 256 CUs, B = 5 (less than one 16-sample sub-tile), n = 2: the extra workgroups queue."""
    sw = _Sweep(**dict(SIG_ROW, B=5), R=300)
    start, st = sw.state(4), sw.state(4)
    sw.replicas(st, 2)
    torch.cuda.synchronize()
    assert sw.sentinels_intact(st)
    _assert_replicas_equal_singles(sw, start, st, 2, which=(0, 255, 256, 299))
    for r in range(300):
        assert all(bool(torch.isfinite(t).all()) for t in sw.rows(st, r)[:4]), r
    assert bool((st[4] == 2).all()) and bool((st[5][:, :2] != 0).all())


@pytest.mark.parametrize("sig,kind,D,L,dd,pad,B,var", [
    (False, 0, 12, 20, 3, 9, 37, 0.25),        # one decoder, dataset noise
    (False, 2, 6, 6, 3, 3, 130, 0.0),          # sphere: no dataset matrix at all
])
def test_one_decoder_and_shared_arguments(sig, kind, D, L, dd, pad, B, var):
    """R = 4 with lrs = NULL (the scalar lr for all) and a_stride = 0 (one shared matrix): equals the same call with explicit
    equal tables and equals single calls; replicas 0 and 2, given the same seed, start and lr, end bitwise equal."""
    sw = _Sweep(sig, kind, D, L, dd, pad, B, R=4, var=var)
    sw.seeds = [5, 9, 5, 11]
    sw.p0[2] = sw.p0[0]
    n, lr = 4, 2.5e-3
    A0 = None if sw.A is None else sw.A[0].clone()
    start, a, b = sw.state(8), sw.state(8), sw.state(8)
    sw.replicas(a, n, lrs=None, a_stride=0, lr=lr, A=A0)
    A_rep = None if A0 is None else A0.repeat(4, 1).contiguous()
    sw.replicas(b, n, lrs=torch.full((4,), lr, dtype=torch.float32, device="cuda"), lr=123.0, A=A_rep)
    torch.cuda.synchronize()
    assert not _differing(a, b), _differing(a, b)
    assert sw.sentinels_intact(a)
    bad = {r: _differing(sw.rows(a, r), sw.single(start, r, n, lr=lr, A=A0)) for r in range(4)}
    assert not any(bad.values()), bad
    assert not _differing(sw.rows(a, 0), sw.rows(a, 2))
    assert _differing(sw.rows(a, 0), sw.rows(a, 1))                # another seed, another start: another model
    assert a[4].tolist() == [n] * 4


def test_a_long_call_is_split_into_launches():
    """R = 2, 1027 steps in one call (two launches) = 1024 + 3 in two calls; exactly two profile records under the replica label."""
    sw = _Sweep(**SIG_ROW, R=2)
    cap = sw.eng.train_loop_steps_per_launch
    assert cap == 1024
    a, b = sw.state(cap + 8), sw.state(cap + 8)
    sw.replicas(b, cap); sw.replicas(b, 3)
    torch.cuda.synchronize()
    sw.eng.profile_begin(64)
    sw.replicas(a, cap + 3)
    rep = sw.eng.profile_report()
    assert set(rep) == {LABEL} and rep[LABEL]["count"] == 2, rep
    assert not _differing(a, b), _differing(a, b)
    assert a[4].tolist() == [cap + 3] * 2 and bool(torch.isfinite(a[5]).all()) and bool(torch.isfinite(a[0][:, :sw.P]).all())


def test_replica_call_is_capturable():
    """A 4-step call of R = 3 captured on a side stream; two replays from a fresh state = 8 eager steps."""
    sw = _Sweep(**SIG_ROW, R=3)
    a, b = sw.state(16), sw.state(16)
    sw.replicas(b, 8)                                # eager (also the warm-up: lazy kernel attributes)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sw.replicas(a, 4)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert a[4].tolist() == [0, 0, 0]                # capture does not execute
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert not _differing(a, b), _differing(a, b)


def test_arguments():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message and leaves the buffers untouched; n_steps = 0
    returns OK and changes nothing."""
    import ctypes as C

    from vae_training_amd import _lib
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    sw = _Sweep(**SIG_ROW, R=3)
    staged = _Sweep(True, 1, 28, 24, 7, 20, 100, R=2)
    wide = _Sweep(True, 1, 21, 6, 3, 17, 100, R=2)
    e = sw.eng
    seeds = _i64(sw.seeds)

    def call(s, st, eng=None, n_steps=2, kind=None, dd=None, did=None, pad=None, A=None, **kw):
        eng = s.eng if eng is None else eng
        a = dict(seeds=_i64(s.seeds), lrs=None, a_stride=s.a_stride, loss_hist=st[5], workspace=s.ws)
        a.update(kw)
        eng.train_loop_gen_replicas(*st[:5], n_steps, LR, s.kind if kind is None else kind, s.A if A is None else A, s.dd if dd is None else dd,
                                    s.did if did is None else did, s.pad if pad is None else pad, s.var, a.pop("seeds"), **a)

    def refused(why, s, **kw):
        st = s.state(4)
        before = [t.clone() for t in st]
        with pytest.raises(VaekError) as ei:
            call(s, st, **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert len(str(ei.value)) > len("libvaek error -1: "), why
        torch.cuda.synchronize()
        assert not _differing(st, before), why

    refused("n = 0", sw, n=0)
    refused("n over the cap", sw, n=1025)
    refused("state_stride < P", sw, state_stride=sw.P - 1)
    refused("grads_stride < grad_len", sw, grads_stride=sw.GL - 1)
    refused("seeds NULL", sw, seeds=None)
    refused("ring with cap 0", sw, loss_hist_cap=0)
    refused("ring with cap -3", sw, loss_hist_cap=-3)
    refused("a_stride < 0", sw, a_stride=-1)
    refused("workspace missing where the batch is staged", staged, workspace=None)
    refused("dd = 17", wide, dd=17, pad=3, A=torch.zeros(2, 17, device="cuda"))
    refused("did = 17", sw, did=17)
    refused("kind 3", sw, kind=3)
    for why, eng in [("B = 257", _engine(True, 7, 6, 257)), ("one hidden layer", Engine(100, 7, 6, (64,), (64,), -3.0, True, True)),
                     ("force_generic", _engine(True, 7, 6, 100, force_generic=True))]:
        assert not eng.supports_train_loop_gen(1), why
        refused(why, sw, eng=eng)
    # a wrong struct_size
    st = sw.state(4)
    rep = _lib.VaekReplicas()
    rep.struct_size, rep.n, rep.state_stride, rep.grads_stride, rep.seeds = 12, 3, sw.ss, sw.gs, seeds.data_ptr()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = e.lib.vaek_train_loop_gen_replicas(e.h, ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), ptr(st[4]), C.byref(rep), 1, ptr(sw.A), 3, 3, 3,
                                            0.0, 0, 0, 2, LR, None, None)
    assert rc == -1 and b"struct_size" in e.lib.vaek_last_error()
    # n_steps = 0: OK, nothing changes; and the very same arguments with n_steps = 2 do run
    st = sw.state(4)
    before = [t.clone() for t in st]
    call(sw, st, n_steps=0)
    torch.cuda.synchronize()
    assert not _differing(st, before)
    call(sw, st, n_steps=2)
    torch.cuda.synchronize()
    assert st[4].tolist() == [2, 2, 2] and _differing(st, before) == list(NAMES)
    # no ring: legal
    call(sw, st, n_steps=1, loss_hist=None)
    torch.cuda.synchronize()
    assert st[4].tolist() == [3, 3, 3] and bool((st[5][:, 2:] == 0).all())


def _sigmoid_model(tmp_path, name, seed, lr=LR):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([name, "--dataset", "sigmoid", "--padding_dim", "3", "-dd", "3"])
    ds = get_dataset("sigmoid", seed, 3, 100, args)
    d = tmp_path / name
    d.mkdir()
    return VAEModel(dirname=str(d), num_batches=12, num_epochs=1, batch_size=100, learning_rate=lr, layer_sizes="",
                    encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=6, tunable_decoder_var=True, dataset_name="sigmoid", fast_loop=True)


def test_replica_loop_equals_three_graph_loops(tmp_path):
    """Three sigmoid models (dataset seeds 69, 24, 48, three learning rates) trained 12 steps by ReplicaLoop against three fresh
    identical models each trained 12 steps by GraphLoop(resident=True): flat, m, v, step and the 12 losses bitwise per model, and
    compute_stats() on a swept model returns its twin's numbers."""
    from vae_training_amd.trainer import GraphLoop, ReplicaLoop
    spec = [(69, 1e-3), (24, 2e-3), (48, 5e-4)]
    swept = [_sigmoid_model(tmp_path, f"s{s}", s, lr) for s, lr in spec]
    twins = [_sigmoid_model(tmp_path, f"t{s}", s, lr) for s, lr in spec]
    lp = ReplicaLoop(swept)
    assert lp.R == 3 and lp.rings.shape == (3, 12) and "3 replicas" in lp.describe()
    lp.run(5); lp.run(0); lp.run(7)
    lp.check()
    for r, (a, b) in enumerate(zip(swept, twins)):
        gl = GraphLoop(b, resident=True, loss_capacity=12)
        assert gl.resident and gl.seed == int(lp.seeds[r]) % 2 ** 64
        gl.run(12)
        torch.cuda.synchronize()
        sa, sb = a.optimizer.state, b.optimizer.state
        got = [a.model.flat, sa.grads, sa.m, sa.v, sa.step_dev, lp.losses(r)]
        want = [b.model.flat, sb.grads, sb.m, sb.v, sb.step_dev, gl.losses()]
        assert not _differing(got, want), (r, _differing(got, want))
        assert sa.step == 12 == sb.step and got[5].numel() == 12 and bool(torch.isfinite(got[5]).all())
    xa, xb = swept[1].compute_stats(), twins[1].compute_stats()
    assert set(xa) == set(xb) and all(float(xa[k]) == float(xb[k]) for k in xa), (xa, xb)
    assert len({float(lp.losses(r)[-1]) for r in range(3)}) == 3


def test_run_py_sweep_in_a_fresh_process(tmp_path):
    """The first line of sigmoid_vae_padding_expts.sh, 30 batches, --sweep_dataset_seeds 69,24, in a fresh process."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "sig", "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30",
           "--sweep_dataset_seeds", "69,24"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train loop:")]
    assert len(lines) == 1 and lines[0].startswith("Train loop: resident linear kernel, 2 replicas"), r.stdout[-1500:]
    last = []
    for seed in (69, 24):
        d = os.path.join(str(tmp_path), "data", f"sig_ds{seed}")
        assert os.path.getsize(os.path.join(d, "model.pkl")) > 0
        z = np.load(os.path.join(d, "losses.npz"), allow_pickle=True)
        losses = np.asarray(z["VAE Loss"], dtype=np.float64)
        # one evaluation loss (the stats event at step 0), then the 30 train losses from replica r's ring
        assert losses.size == 31 and np.isfinite(losses).all(), (seed, losses)
        last.append(losses[-30:])
    assert not np.array_equal(last[0], last[1])          # two datasets, two runs
