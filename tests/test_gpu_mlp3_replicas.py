"""-m gpu: vaek_train_step_gen_replicas -- ONE train step of N independent three-hidden-layer MLP VAEs of one shape in the two
launches of csrc/fused_mlp3.hip, blockIdx.y = replica -- and its callers, trainer.ReplicaGraphLoop and
`run.py --sweep_dataset_seeds` on a sphere script line.

The defining property is BITWISE: what the call leaves in replica r's params, m, v, grads, step_dev[r], loss ring, next batch and
counter pair is what vaek_train_step_gen (no-draw form: vaek_train_step) leaves when called alone on those slices with seeds[r],
lrs[r], replica r's dataset matrix and counter + 2 r -- the same code on the same inputs.  Every comparison with the solo path
below is torch.equal, so no tolerance is introduced: accuracy against the float64 oracle is tests/test_gpu_mlp3.py's, inherited.
The floats between two replicas where a stride exceeds the length hold a sentinel that must survive."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import _i64
from tests.mlp3_cases import H3, MAX_BATCH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
SENT = -12345.0
NAMES = ("params", "grads", "m", "v", "step", "ring", "x0", "z1_0", "z2_0", "x1", "z1_1", "z2_1", "counter")
CHAIN, GRADS = "fused_mlp3_chain_replicas", "fused_mlp3_grads_adam_gen_replicas"


def _up4(n):
    return (n + 3) // 4 * 4


def _engine(D, L, hidden=H3, B=37, **kw):
    from vae_training_amd.engine import Engine
    return Engine(B, D, L, tuple(hidden), tuple(hidden), -3.0, True, False, **kw)


class _State:
    """The buffers of one replica call: sentinel-padded stacks, the rings, two stacked batch buffers (bufs[par] holds every
    replica's next batch), the [R, 2] generator counters."""

    def tensors(self):
        return [self.params, self.grads, self.m, self.v, self.step, self.rings, *self.bufs[0], *self.bufs[1], self.counter]


class _Sweep:
    """One engine and R replicas with random starts (randn * 0.1, as tests/test_gpu_mlp3.py), distinct seeds (one of them above
    2^63), learning rates and -- kind 0 -- dataset matrices, in stacks of stride roundup4(P) + 8 / grad_len + 5 whose padding holds
    a sentinel.  offset = 1: the params stack starts one float past a 16-byte boundary."""

    def __init__(self, dd=3, pad=3, L=6, hidden=H3, B=37, R=3, kind=2, var=0.0, offset=0, tag=5, row0=1000):
        self.eng = e = _engine(dd + pad, L, hidden, B)
        assert e.step_path == "mlp3" and e.supports_train_step_replicas()
        self.kind, self.dd, self.did, self.pad, self.var, self.R, self.B, self.tag, self.row0 = kind, dd, dd, pad, var, R, B, tag, row0
        self.D, self.L, self.P, self.GL, self.offset = dd + pad, L, e.P, e.grad_len, offset
        self.ss, self.gs = _up4(e.P) + 8, e.grad_len + 5
        g = torch.Generator().manual_seed(11)
        alen = {0: dd * dd, 2: 0}[kind]
        self.A = torch.randn(R, alen, generator=g).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.seeds = [77 + 1000003 * r for r in range(R)]
        if R > 1:
            self.seeds[1] = 2 ** 63 + 5
        self.lrs = [LR * (1.0 + 0.5 * (r % 7)) for r in range(R)]
        self.p0 = (torch.randn(R, e.P, generator=g) * 0.1).cuda()
        self.m0 = torch.zeros(R, e.P, device="cuda")
        self.v0 = torch.zeros(R, e.P, device="cuda")
        self.step0 = torch.zeros(R, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(e.train_step_replicas_workspace(R), dtype=torch.uint8, device="cuda")
        self._tables = None

    def warm(self, r, step=7):
        """Replica r resumes a run: a non-zero Adam counter (and generator counter) and non-zero moments."""
        g = torch.Generator().manual_seed(5 + r)
        self.m0[r] = (torch.randn(self.P, generator=g) * 0.01).cuda()
        self.v0[r] = (torch.rand(self.P, generator=g) * 1e-4).cuda()
        self.step0[r] = step

    def tables(self):
        """Device tables of seeds and learning rates, built once: a call under stream capture must find them made."""
        if self._tables is None:
            self._tables = (_i64(self.seeds), torch.tensor(self.lrs, dtype=torch.float32, device="cuda"))
        return self._tables

    def A_of(self, r):
        return None if self.A is None else self.A[r]

    def state(self, cap=8):
        R = self.R

        def stack(init, width, stride, off=0):
            flat = torch.full((R * stride + off,), SENT, dtype=torch.float32, device="cuda")
            t = flat[off:].view(R, stride)
            t[:, :width] = init
            return t
        st = _State()
        st.params = stack(self.p0, self.P, self.ss, self.offset)
        assert st.params.data_ptr() % 16 == 4 * self.offset
        st.grads, st.m, st.v = stack(0.0, self.GL, self.gs), stack(self.m0, self.P, self.ss), stack(self.v0, self.P, self.ss)
        st.step = self.step0.clone()
        st.rings = torch.zeros(R, cap, dtype=torch.float32, device="cuda")
        z = lambda w: torch.zeros(R, self.B, w, dtype=torch.float32, device="cuda")
        st.bufs = [(z(self.D), z(self.L), z(self.D)) for _ in range(2)]
        st.counter = torch.stack([self.step0, self.step0], dim=1).contiguous()
        st.par = 0
        for r in range(R):               # replica r's first batch: the solo generator on its slices (step = its counter)
            self.eng.make_batch(self.kind, self.A_of(r), self.dd, self.did, self.pad, self.var, self.B, self.seeds[r], tag=self.tag,
                                row0=self.row0, out=tuple(t[r] for t in st.bufs[0]), counter=st.counter[r], which=0)
        torch.cuda.synchronize()
        return st

    def steps(self, st, n, **kw):
        """n pipelined steps: ONE replica call each."""
        seeds_t, lrs_t = self.tables()
        a = dict(lrs=lrs_t, a_stride=self.a_stride, loss_hist=st.rings, workspace=self.ws, tag=self.tag, row0=self.row0)
        a.update(kw)
        for _ in range(n):
            p = st.par
            self.eng.train_step_gen_replicas(st.params, st.grads, st.m, st.v, st.step, st.bufs[p], 0.0, self.kind, self.A, self.dd, self.did,
                                             self.pad, self.var, st.bufs[p ^ 1], seeds_t, st.counter, p ^ 1, **a)
            st.par = p ^ 1

    def rows(self, st, r):
        return [st.params[r, :self.P], st.grads[r, :self.GL], st.m[r, :self.P], st.v[r, :self.P], st.step[r:r + 1], st.rings[r],
                *[t[r] for t in st.bufs[0]], *[t[r] for t in st.bufs[1]], st.counter[r]]

    def solo(self, st0, r, n):
        """n pipelined vaek_train_step_gen steps alone on copies of replica r's slices of the START state st0 (params at the
        replica slice's alignment, the ring through vaek_set_loss_history); returns the thirteen buffers it leaves."""
        P, GL = self.P, self.GL
        flat = torch.empty(P + 4, dtype=torch.float32, device="cuda")
        params = flat[self.offset:self.offset + P]
        params.copy_(st0.params[r, :P])
        assert params.data_ptr() % 16 == st0.params[r].data_ptr() % 16
        grads, m, v = st0.grads[r, :GL].clone(), st0.m[r, :P].clone(), st0.v[r, :P].clone()
        step, ring, counter = st0.step[r:r + 1].clone(), st0.rings[r].clone(), st0.counter[r].clone()
        bufs = [tuple(t[r].clone() for t in st0.bufs[0]), tuple(t[r].clone() for t in st0.bufs[1])]
        self.eng.set_loss_history(ring)
        par = st0.par
        for _ in range(n):
            self.eng.train_step_gen(params, grads, m, v, step, bufs[par], self.lrs[r], self.kind, self.A_of(r), self.dd, self.did, self.pad,
                                    self.var, bufs[par ^ 1], self.seeds[r], counter, par ^ 1, tag=self.tag, row0=self.row0)
            par ^= 1
        torch.cuda.synchronize()
        self.eng.set_loss_history(None)
        return [params, grads, m, v, step, ring, *bufs[0], *bufs[1], counter]

    def sentinels_intact(self, st):
        return all(bool((t[:, w:] == SENT).all()) for t, w in ((st.params, self.P), (st.grads, self.GL), (st.m, self.P), (st.v, self.P)))


def _differing(a, b, names=NAMES):
    return [what for x, y, what in zip(a, b, names) if not torch.equal(x, y)]


def _assert_replicas_equal_solo(sw, start, done, n, which=None):
    bad = {}
    for r in (range(sw.R) if which is None else which):
        d = _differing(sw.rows(done, r), sw.solo(start, r, n))
        if d:
            bad[r] = d
    print(f"replicas against solo calls, n = {n}: " + (f"buffers that differ, by replica: {bad}" if bad else "all bitwise equal"))
    assert not bad, bad


def _run_and_compare(sw, n, cap=8, which=None):
    """n pipelined replica steps from a fresh state against solo runs, with the sentinels between replicas and a sentinel-filled
    ring of vaek_set_loss_history (which the replica call must not write) checked after them."""
    start, st = sw.state(cap), sw.state(cap)
    assert not _differing(start.tensors(), st.tensors())
    ctx_ring = torch.full((cap,), SENT, dtype=torch.float32, device="cuda")
    sw.eng.set_loss_history(ctx_ring)
    sw.steps(st, n)
    torch.cuda.synchronize()
    sw.eng.set_loss_history(None)
    assert bool((ctx_ring == SENT).all()), "the replica call wrote the ring of vaek_set_loss_history"
    assert sw.sentinels_intact(st), "floats between two replicas were written"
    _assert_replicas_equal_solo(sw, start, st, n, which)
    for r in range(sw.R):
        t0 = int(start.step[r])
        assert int(st.step[r]) == t0 + n and sorted(st.counter[r].tolist()) == [t0 + n, t0 + n + 1]
        ring = st.rings[r]
        assert bool(torch.isfinite(ring).all()) and bool((ring[[(t0 + k) % cap for k in range(n)]] != 0).all())
    return start, st


@pytest.mark.parametrize("kind,var", [(2, 0.0), (0, 0.25)], ids=["sphere", "linear_gaussian-noise"])
def test_defining_property_with_everything_distinct(kind, var):
    """sphere(3, 3, 6), 200|200|200, B = 37 (three groups, the last with 5 valid rows), R = 3, five pipelined steps: distinct
    starts, seeds, learning rates (and, kind 0, dataset matrices with a_stride = 9 and dataset noise); replica 1 resumes at step 7
    with non-zero m and v and a matching counter; strides roundup4(P) + 8 and grad_len + 5 with sentinel padding."""
    sw = _Sweep(kind=kind, var=var)
    sw.warm(1)
    assert (sw.A is None) == (kind == 2) and sw.ss % 4 == 0 and sw.ss - sw.P >= 8
    start, st = _run_and_compare(sw, 5, cap=16)
    assert st.step.tolist() == [5, 12, 5]
    assert len({float(st.rings[r][(int(st.step[r]) - 1) % 16]) for r in range(3)}) == 3          # the replicas trained differently
    assert not torch.equal(st.bufs[0][0][0], st.bufs[0][0][2])                                     # ... on different batches


@pytest.mark.parametrize("kw", [
    dict(hidden=(66, 201, 130), B=100),          # no layer takes the 16-byte dX loads
    dict(pad=18, hidden=(64, 200, 96), B=100),   # D = 21: no float4 batch stores
    dict(B=5),                                   # one group
    dict(B=MAX_BATCH),                           # the cap
    dict(B=100, offset=1),                       # params base one float past a 16-byte boundary: every replica on dword loads, as solo
], ids=["no-vec-widths", "D21", "B5", "B128", "misaligned-base"])
def test_shapes_where_slicing_can_go_wrong(kw):
    _run_and_compare(_Sweep(R=2, **kw), 3)


def test_more_workgroups_than_cus():
    """R = 40 at B = 100: 280 chain workgroups on 256 CUs, three steps; replicas 0, 17 and 39 against solo; replicas 5 and 23, given
    equal tables and states, end equal."""
    sw = _Sweep(B=100, R=40)
    sw.seeds[23], sw.lrs[23] = sw.seeds[5], sw.lrs[5]
    sw.p0[23] = sw.p0[5]
    start, st = _run_and_compare(sw, 3, which=(0, 17, 39))
    assert not _differing(sw.rows(st, 5), sw.rows(st, 23))
    assert _differing(sw.rows(st, 5), sw.rows(st, 6))
    for r in range(40):
        assert all(bool(torch.isfinite(t).all()) for t in sw.rows(st, r)[:4]), r


def test_no_draw_form_is_train_step_per_replica():
    """x_next = z1_next = z2_next = NULL, seeds = A = counter = NULL: R = 3 x vaek_train_step on each slice, two steps on two
    given batches."""
    sw = _Sweep()
    sw.warm(2, step=3)
    st = sw.state()
    g = torch.Generator().manual_seed(3)
    batches = [tuple(torch.randn(3, sw.B, w, generator=g).cuda() for w in (sw.D, sw.L, sw.D)) for _ in range(2)]
    keep = [t.clone() for t in (st.params, st.grads, st.m, st.v, st.step, st.rings)]
    _, lrs_t = sw.tables()
    for cur in batches:
        sw.eng.train_step_gen_replicas(st.params, st.grads, st.m, st.v, st.step, cur, 0.0, 0, None, 0, 0, 0, 0.0, None, None, None, 0,
                                       lrs=lrs_t, loss_hist=st.rings, workspace=sw.ws)
    torch.cuda.synchronize()
    assert sw.sentinels_intact(st) and st.step.tolist() == [2, 2, 5]
    for r in range(3):
        b = [keep[0][r, :sw.P].clone(), keep[1][r, :sw.GL].clone(), keep[2][r, :sw.P].clone(), keep[3][r, :sw.P].clone(),
             keep[4][r:r + 1].clone(), keep[5][r].clone()]
        sw.eng.set_loss_history(b[5])
        for cur in batches:
            sw.eng.train_step(*b[:5], *[t[r].clone() for t in cur], sw.lrs[r])
        torch.cuda.synchronize()
        sw.eng.set_loss_history(None)
        d = _differing(sw.rows(st, r)[:6], b)
        assert not d, (r, d)


def test_replica_step_is_capturable():
    """Four pipelined steps of R = 3 captured on a side stream; two replays from a fresh state = 8 eager steps, bitwise."""
    sw = _Sweep()
    a, b = sw.state(16), sw.state(16)
    sw.steps(b, 8)                                   # eager (also the warm-up: lazy kernel attributes)
    torch.cuda.synchronize()
    keep = [t.clone() for t in a.tensors()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sw.steps(a, 4)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert a.par == 0 and not _differing(a.tensors(), keep)          # capture does not execute; an even count keeps the parity
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert a.step.tolist() == [8, 8, 8]
    assert not _differing(a.tensors(), b.tensors()), _differing(a.tensors(), b.tensors())


def test_two_launches_per_step_whatever_n_is():
    sw = _Sweep()
    st = sw.state()
    sw.steps(st, 1)
    torch.cuda.synchronize()
    sw.eng.profile_begin(64)
    sw.steps(st, 5)
    torch.cuda.synchronize()
    rep = sw.eng.profile_report()
    assert set(rep) == {CHAIN, GRADS} and rep[CHAIN]["count"] == 5 and rep[GRADS]["count"] == 5, rep
    print({k: round(1e3 * v["total_ms"] / v["count"], 2) for k, v in rep.items()}, "us per launch, R = 3, B = 37")


def _region_floats(D, L, hidden, B):
    """floats of the solo step's workspace region (csrc/fused_mlp3.hip: mlp3_layout + the partial rows), rounded up to 4"""
    G = (B + 15) // 16
    widths = [D, *hidden, L, *hidden, D]
    layers = list(zip(widths[:4], widths[1:5])) + list(zip(widths[4:8], widths[5:9]))
    assert len(layers) == 8
    return _up4(sum((i + o) * 16 * G for i, o in layers) + 40 * G)


def test_refusals_and_the_workspace_size():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message and leaves the buffers untouched; contexts off
    the mlp3 path are refused by vaek_supports_train_step_replicas and by the call; the workspace is n regions."""
    import ctypes as C

    from vae_training_amd import _lib
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    sw = _Sweep(kind=0, var=0.25)
    e = sw.eng
    seeds_t, lrs_t = sw.tables()
    one = 4 * _region_floats(6, 6, H3, 37)
    assert [e.train_step_replicas_workspace(n) for n in (1, 2, 3, 256)] == [one, 2 * one, 3 * one, 256 * one]
    assert 4 * _region_floats(21, 6, (64, 200, 96), 100) == _engine(21, 6, (64, 200, 96), 100).train_step_replicas_workspace(1)
    assert e.train_step_max_replicas == 256
    for n in (0, 257):
        with pytest.raises(VaekError):
            e.train_step_replicas_workspace(n)
    ws_ctx = C.c_size_t()
    assert e.lib.vaek_workspace_bytes(e.h, C.byref(ws_ctx)) == 0 and e.workspace.numel() == max(ws_ctx.value, 256)

    def call(st, eng=None, kind=None, dd=None, did=None, nxt="own", seeds="own", counter="own", workspace="own", **kw):
        a = dict(lrs=lrs_t, a_stride=sw.a_stride, loss_hist=st.rings, tag=sw.tag, row0=sw.row0)
        a.update(kw)
        (eng or e).train_step_gen_replicas(st.params, st.grads, st.m, st.v, st.step, st.bufs[0], 0.0, sw.kind if kind is None else kind, sw.A,
                                           sw.dd if dd is None else dd, sw.did if did is None else did, sw.pad, sw.var,
                                           st.bufs[1] if isinstance(nxt, str) else nxt, seeds_t if isinstance(seeds, str) else seeds,
                                           st.counter if isinstance(counter, str) else counter, 1,
                                           workspace=sw.ws if isinstance(workspace, str) else workspace, **a)

    st = sw.state(4)
    before = [t.clone() for t in st.tensors()]

    def refused(why, **kw):
        with pytest.raises(VaekError) as ei:
            call(st, **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert len(str(ei.value)) > len("libvaek error -1: "), why
        torch.cuda.synchronize()
        assert not _differing(st.tensors(), before), why

    refused("n = 0", n=0)
    refused("n over the cap", n=257)
    refused("state_stride < P", state_stride=_up4(sw.P) - 4)
    refused("state_stride no multiple of 4", state_stride=sw.ss + 1)
    refused("grads_stride < grad_len", grads_stride=sw.GL - 1)
    refused("ring with cap 0", loss_hist_cap=0)
    refused("a_stride < 0", a_stride=-1)
    refused("seeds NULL in the drawing form", seeds=None)
    refused("counter NULL in the drawing form", counter=None)
    refused("only x_next", nxt=(st.bufs[1][0], None, None))
    refused("z2_next missing", nxt=(st.bufs[1][0], st.bufs[1][1], None))
    refused("dd = 17", dd=17)
    refused("did = 17", did=17)
    refused("kind 3", kind=3)
    refused("workspace missing", workspace=None)
    refused("workspace misaligned", workspace=sw.ws[4:])
    for why, eng in [("linear", Engine(37, 6, 6)), ("one hidden layer", Engine(37, 6, 6, (64,), (64,), -3.0, True, False)),
                     ("B = 129", _engine(6, 6, B=MAX_BATCH + 1)), ("force_generic", _engine(6, 6, force_generic=True)),
                     ("world = 2", _engine(6, 6, world=2, rank=0, global_batch=74))]:
        assert not eng.supports_train_step_replicas(), why
        assert why == "world = 2" or eng.step_path != "mlp3", why
        refused(why, eng=eng)
    # a wrong struct_size
    rep = _lib.VaekReplicas()
    rep.struct_size, rep.n, rep.state_stride, rep.grads_stride, rep.seeds = 12, 3, sw.ss, sw.gs, seeds_t.data_ptr()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = e.lib.vaek_train_step_gen_replicas(e.h, ptr(st.params), ptr(st.grads), ptr(st.m), ptr(st.v), ptr(st.step), C.byref(rep),
                                            *[ptr(t) for t in st.bufs[0]], LR, ptr(sw.ws), 0, ptr(sw.A), 3, 3, 3, 0.25,
                                            *[ptr(t) for t in st.bufs[1]], 0, ptr(st.counter), 1, 0, None)
    assert rc == -1 and b"struct_size" in e.lib.vaek_last_error()
    torch.cuda.synchronize()
    assert not _differing(st.tensors(), before)
    # and the very same buffers with valid arguments do run
    call(st)
    torch.cuda.synchronize()
    assert st.step.tolist() == [1, 1, 1] and sw.sentinels_intact(st)


def _sphere_model(tmp_path, name, seed, lr):
    """line 1 of sphere_vae_padding_expts.sh as run.py builds it, with its dataset seed"""
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([name, "--dataset", "sphere", "--padding_dim", "3", "-dd", "3"])
    ds = get_dataset("sphere", seed, 3, 100, args)
    d = tmp_path / name
    d.mkdir()
    return VAEModel(dirname=str(d), num_batches=11, num_epochs=1, batch_size=100, learning_rate=lr, layer_sizes="200|200|200",
                    encoder_layer_sizes="200|200|200", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=6, tunable_decoder_var=True, dataset_name="sphere", fast_loop=True)


def test_replica_graph_loop_equals_three_graph_loops(tmp_path):
    """Three sphere models (dataset seeds 69, 24, 48, three learning rates), steps_per_graph = 4, 11 steps as run(6) + run(5):
    the warm-up step, capture, a replay and an eager tail step in the first run, the parity step and a replay in the second --
    against three fresh identical models each trained 11 steps by GraphLoop(pipeline=True, moments=False, resident=False,
    steps_per_graph=4): flat, grads, m, v, step and the 11 losses bitwise per model."""
    from vae_training_amd.trainer import GraphLoop, ReplicaGraphLoop
    spec = [(69, 1e-3), (24, 2e-3), (48, 5e-4)]
    swept = [_sphere_model(tmp_path, f"s{s}", s, lr) for s, lr in spec]
    twins = [_sphere_model(tmp_path, f"t{s}", s, lr) for s, lr in spec]
    lp = ReplicaGraphLoop(swept, steps_per_graph=4)
    assert lp.R == 3 and lp.G == 4 and lp.rings.shape == (3, 11) and lp.params.shape == (3, _up4(lp.P)) and "3 replicas" in lp.describe()
    lp.run(6)
    assert lp.graph is not None and lp.par != lp.graph_parity        # warm-up 1 + replay 4 + tail 1: off the graph's parity
    lp.run(0)
    lp.run(5)                                                           # the parity step, then a replay
    lp.check()
    torch.cuda.synchronize()
    for r, (a, b) in enumerate(zip(swept, twins)):
        gl = GraphLoop(b, pipeline=True, moments=False, resident=False, steps_per_graph=4, loss_capacity=16)
        assert gl.pipeline and gl.eng.step_path == "mlp3" and gl.seed % 2 ** 64 == int(lp.seeds[r]) % 2 ** 64
        gl.run(11)
        torch.cuda.synchronize()
        assert gl.graph is not None
        sa, sb = a.optimizer.state, b.optimizer.state
        got = [a.model.flat, sa.grads, sa.m, sa.v, sa.step_dev, lp.losses(r)]
        want = [b.model.flat, sb.grads, sb.m, sb.v, sb.step_dev, gl.losses()]
        d = _differing(got, want)
        assert not d, (r, d)
        assert sa.step == 11 == sb.step and got[5].numel() == 11 and bool(torch.isfinite(got[5]).all())
        assert torch.equal(lp.view(r).losses(), got[5])
    assert len({float(lp.losses(r)[-1]) for r in range(3)}) == 3


def test_run_py_sweep_on_the_sphere_line_in_a_fresh_process(tmp_path):
    """Line 1 of sphere_vae_padding_expts.sh, 12 batches, --sweep_dataset_seeds 69,24, in a fresh process: before the replica form
    of the mlp3 step existed this command was refused (the resident loop does not cover the model)."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "sph", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes",
           "200|200|200", "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "12",
           "--sweep_dataset_seeds", "69,24"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Train step: mlp3 kernels" in r.stdout, r.stdout[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train loop:")]
    assert len(lines) == 1 and lines[0].startswith("Train loop: hipGraph of 200 steps, 2 replicas per step (vaek_train_step_gen_replicas)"), r.stdout[-1500:]
    last = []
    for seed in (69, 24):
        d = os.path.join(str(tmp_path), "data", f"sph_ds{seed}")
        assert os.path.getsize(os.path.join(d, "model.pkl")) > 0
        z = np.load(os.path.join(d, "losses.npz"), allow_pickle=True)
        losses = np.asarray(z["VAE Loss"], dtype=np.float64)
        # one evaluation loss (the stats event at step 0), then the 12 train losses from replica r's ring
        assert losses.size == 13 and np.isfinite(losses).all(), (seed, losses)
        last.append(losses[-12:])
    assert not np.array_equal(last[0], last[1])          # two datasets, two runs
