"""-m gpu: vaek_train_loop_gen -- N train steps of a small-batch linear VAE (one or two decoders) as a loop inside ONE workgroup
(csrc/linear_resident.hip): parameters and Adam state on chip between steps, batches drawn in the kernel -- and its callers,
trainer.GraphLoop(resident=True) and `run.py --fast_loop` on a sigmoid line.  The checks are (i) against vaek_make_batch +
vaek_train_step on the SAME Philox streams, step by step, to the tolerances tests/test_gpu_steps.py uses between two GPU paths;
(ii) against the float64 oracle on batches copied back from the device generator; (iii) bitwise between different splits of the
same steps into calls and launches: the state a launch leaves is in HBM, whole."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests.gpu_util import dev, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
SIG_ROW = dict(sig=True, kind=1, D=7, L=6, dd=3, pad=3, B=100)      # the first line of sigmoid_vae_padding_expts.sh


def _spec(kind, dd, did):
    g = torch.Generator().manual_seed(11)
    if kind == 0:
        return torch.randn(dd, did, generator=g).cuda().contiguous()
    if kind == 1:
        return torch.randn(dd, generator=g).cuda().contiguous()
    return None


def _engine(sig, D, L, B, **kw):
    from vae_training_amd.engine import Engine
    return Engine(B, D, L, (), (), -3.0 if sig else -1.0, True, sig, **kw)


class _Run:
    """One engine, one dataset, one random start (randn * 0.3, as tests/test_gpu_loop.py): fresh states and the two ways to step."""

    def __init__(self, sig, kind, D, L, dd, pad, B, var=0.0, seed=77, tag=5, row0=1000):
        self.eng = _engine(sig, D, L, B)
        self.kind, self.dd, self.did, self.pad, self.B, self.var = kind, dd, dd, pad, B, var
        self.seed, self.tag, self.row0 = seed, tag, row0
        self.A = _spec(kind, dd, dd)
        assert self.eng.supports_train_loop_gen(kind)
        torch.manual_seed(0)
        self.p0 = (torch.randn(self.eng.P, device="cuda") * 0.3).contiguous()

    def state(self, ring_len):
        e = self.eng
        return [self.p0.clone(), e.new_flat(e.grad_len), e.new_flat(), e.new_flat(), torch.zeros(1, dtype=torch.int32, device="cuda"),
                torch.zeros(ring_len, dtype=torch.float32, device="cuda")]

    def loop(self, st, n):
        self.eng.set_loss_history(st[5])
        self.eng.train_loop_gen(*st[:5], n, LR, self.kind, self.A, self.dd, self.did, self.pad, self.var, self.seed, tag=self.tag,
                                row0=self.row0)

    def batch(self, t):
        return self.eng.make_batch(self.kind, self.A, self.dd, self.did, self.pad, self.var, self.B, self.seed, step=t, tag=self.tag,
                                   row0=self.row0)

    def stepwise(self, st, n, t0=0):
        self.eng.set_loss_history(st[5])
        for t in range(t0, t0 + n):
            self.eng.train_step(*st[:5], *self.batch(t), LR)


def _close(a, b, n):
    """The tolerances tests/test_gpu_steps.py uses between two GPU paths."""
    pa, ga, ma, va, sa, ra = a
    pb, gb, mb, vb, sb, rb = b
    P = pa.numel()
    assert int(sa.item()) == n == int(sb.item())
    la, lb = ra[:n].double(), rb[:n].double()
    assert bool(torch.isfinite(la).all())
    rel = float(((la - lb).abs() / lb.abs()).max())
    dp = float((pa - pb).abs().max())
    dm = float((ma - mb).abs().max()) / max(float(mb.abs().max()), 1e-30)
    dv = float((va - vb).abs().max()) / max(float(vb.abs().max()), 1e-30)
    dg = abs(float(ga[P]) - float(gb[P])) / abs(float(gb[P]))
    print(f"loss rel {rel:.3e}  params {dp:.3e} (bound {0.02 * LR:.1e})  m {dm:.3e}  v {dv:.3e}  last loss rel {dg:.3e}  "
          f"bitwise {all(torch.equal(x, y) for x, y in zip(a, b))}")
    assert rel <= 1e-5 and dp <= 0.02 * LR and dm <= 1e-5 and dv <= 1e-5 and dg <= 1e-5


@pytest.mark.parametrize("sig,kind,D,L,dd,pad,B,n,var", [
    (True, 1, 7, 6, 3, 3, 100, 5, 0.0),
    (True, 1, 28, 24, 7, 20, 100, 3, 0.0),      # the EXACT variant; its batch is staged in the workspace
    (True, 1, 9, 10, 5, 3, 256, 3, 0.0),        # the batch cap
    (True, 1, 7, 6, 3, 3, 5, 3, 0.0),           # less than one 16-sample sub-tile
    (True, 1, 11, 10, 5, 5, 37, 3, 0.0),        # ragged, odd D
    (False, 0, 12, 20, 3, 9, 100, 4, 0.25),     # one decoder, dataset noise
    (False, 2, 6, 6, 3, 3, 130, 4, 0.0),        # sphere
    (False, 0, 28, 24, 7, 21, 64, 3, 0.0),      # L + 2 D + 1 = 81: no moment form exists
])
def test_resident_loop_equals_the_step_by_step_path(sig, kind, D, L, dd, pad, B, n, var):
    """vaek_train_loop_gen(n) against vaek_make_batch(step = t) + vaek_train_step for t = 0 .. n-1 from the same start."""
    r = _Run(sig, kind, D, L, dd, pad, B, var)
    a, b = r.state(n + 4), r.state(n + 4)
    r.loop(a, n)
    r.stepwise(b, n)
    torch.cuda.synchronize()
    r.eng.set_loss_history(None)
    _close(a, b, n)
    assert float(a[1][r.eng.P + 3]) == 0.0 and bool(torch.isfinite(a[1]).all())


def test_resident_loop_follows_the_oracle_on_the_generated_batches():
    """Three steps of the first sigmoid row against three float64 oracle steps (networks.py:87-101) on the batches the device
    generator draws for those RNG steps (copied back): loss 1e-5 relative per step, parameters within 2 % of an Adam step per
    step.  (No relu in these models: no kinks to avoid.)"""
    cfg = O.Config(7, 6, (), (), -3.0, True, "sigmoid")
    B, n = 100, 3
    eng = _engine(True, 7, 6, B)
    A = _spec(1, 3, 3)
    r32 = lambda t: np.asarray(t, np.float32).astype(np.float64)
    p = {k: r32(v) for k, v in O.init_params(cfg, seed=3).items()}
    params = dev(O.flatten(cfg, p)); grads = eng.new_flat(eng.grad_len); m = eng.new_flat(); v = eng.new_flat()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    ring = torch.zeros(8, dtype=torch.float32, device="cuda")
    eng.set_loss_history(ring)
    eng.train_loop_gen(params, grads, m, v, step, n, LR, 1, A, 3, 3, 3, 0.0, 123)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    st = O.adam_init(p)
    for t in range(n):
        x, z1, z2 = (r32(host(a)) for a in eng.make_batch(1, A, 3, 3, 3, 0.0, B, 123, step=t))
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, LR)
        assert abs(float(ring[t]) - loss) <= 1e-5 * abs(loss), (t, float(ring[t]), loss)
    assert np.max(np.abs(host(params) - O.flatten(cfg, p))) <= 0.02 * LR * n


def _same(a, b):
    for x, y, what in zip(a, b, ("params", "grads", "m", "v", "step", "ring")):
        assert torch.equal(x, y), what


def test_state_lives_in_hbm_between_launches_and_calls():
    """Bitwise: 9 steps in one call = 5 + 4 in two; kResidentMaxSteps + 3 steps in one call (two launches) = the same split made by
    the caller; the same call twice from the same state gives the same bits."""
    r = _Run(**SIG_ROW)
    cap = r.eng.train_loop_steps_per_launch
    assert cap == 1024
    a, b, c = r.state(16), r.state(16), r.state(16)
    r.loop(a, 9)
    r.loop(b, 5); r.loop(b, 4)
    r.loop(c, 9)
    torch.cuda.synchronize()
    _same(a, b)
    _same(a, c)
    assert int(a[4].item()) == 9 and bool((a[5][:9] != 0).all()) and bool((a[5][9:] == 0).all())
    a, b = r.state(cap + 8), r.state(cap + 8)
    r.loop(a, cap + 3)
    r.loop(b, cap); r.loop(b, 3)
    torch.cuda.synchronize()
    r.eng.set_loss_history(None)
    _same(a, b)
    assert int(a[4].item()) == cap + 3 and bool(torch.isfinite(a[5]).all()) and bool(torch.isfinite(a[0]).all())


def test_resident_loop_is_capturable():
    """One call of n = 4 captured on a side stream, as GraphLoop._capture does; two replays from a fresh state = 8 eager steps."""
    r = _Run(**SIG_ROW)
    a, b = r.state(16), r.state(16)
    r.loop(b, 8)                                  # eager (also the warm-up: lazy kernel attributes)
    torch.cuda.synchronize()
    r.eng.set_loss_history(a[5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            r.loop(a, 4)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert int(a[4].item()) == 0                  # capture does not execute
    g.replay(); g.replay()
    torch.cuda.synchronize()
    r.eng.set_loss_history(None)
    _same(a, b)


def test_twenty_steps_are_one_launch():
    r = _Run(**SIG_ROW)
    a = r.state(32)
    r.loop(a, 2)
    torch.cuda.synchronize()
    r.eng.profile_begin(64)
    r.loop(a, 20)
    rep = r.eng.profile_report()
    r.eng.set_loss_history(None)
    assert set(rep) == {"linear_resident"} and rep["linear_resident"]["count"] == 1, rep
    assert int(a[4].item()) == 22


def test_the_fence():
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    A = _spec(1, 3, 3)

    def refuses(eng, kind=1, dd=3, pad=None, A_=A):
        st = [eng.new_flat(), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(), torch.zeros(1, dtype=torch.int32, device="cuda")]
        pad = eng.D - dd - (1 if kind == 1 else 0) if pad is None else pad
        with pytest.raises(VaekError):
            eng.train_loop_gen(*st, 2, LR, kind, A_, dd, dd, pad, 0.0, 1)
        torch.cuda.synchronize()
        assert int(st[4].item()) == 0

    for why, eng, kind in [
        ("B = 257", Engine(257, 7, 6, (), (), -3.0, True, True), 1),
        ("world = 2", Engine(100, 7, 6, (), (), -3.0, True, True, world=2, rank=0), 1),
        ("bf16", Engine(100, 7, 6, (), (), -3.0, True, True, dtype="bf16"), 1),
        ("one hidden layer", Engine(100, 7, 6, (64,), (64,), -3.0, True, True), 1),
        ("D = 33", Engine(100, 33, 6, (), (), -1.0, True, False), 0),
        ("force_generic", Engine(100, 7, 6, (), (), -3.0, True, True, force_generic=True), 1),
    ]:
        assert not eng.supports_train_loop_gen(kind), why
        refuses(eng, kind=kind, A_=A if kind == 1 else _spec(0, 3, 3))
    ok = _engine(True, 7, 6, 100)
    assert ok.supports_train_loop_gen(1) and ok.supports_train_loop_gen(0) and ok.supports_train_loop_gen(2)
    assert not ok.supports_train_loop_gen(3) and not ok.supports_train_loop_gen(-1)
    refuses(ok, kind=3)
    wide = _engine(True, 21, 6, 100)
    assert wide.supports_train_loop_gen(1)
    refuses(wide, kind=1, dd=17, pad=3, A_=torch.zeros(17, device="cuda"))
    # what the older entry points say about a sigmoid context is unchanged
    assert not ok.supports_train_steps() and not ok.supports_train_steps_gen(0)


def _sigmoid_model(tmp_path, name):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([name, "--dataset", "sigmoid", "--padding_dim", "3", "-dd", "3"])
    ds = get_dataset("sigmoid", args.dataset_seed, 3, 100, args)
    return VAEModel(dirname=str(tmp_path), num_batches=10, num_epochs=1, batch_size=100, learning_rate=LR, layer_sizes="",
                    encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-3.0, tqdm=False, dataset=ds,
                    latent_dimension=6, tunable_decoder_var=True, dataset_name="sigmoid", fast_loop=True)


def test_graph_loop_takes_the_resident_kernel(tmp_path):
    """GraphLoop(model) on a sigmoid model resolves `resident` as the measurement left it (trainer.RESIDENT_DEFAULT);
    resident=True against resident=False (the hipGraph loop of vaek_train_step_gen) for 12 steps, same Philox batches."""
    from vae_training_amd import trainer
    from vae_training_amd.trainer import GraphLoop
    n = 12
    a, b, c = (_sigmoid_model(tmp_path, k) for k in "abc")
    lc = GraphLoop(c, seed=9)
    assert not lc.moments and lc.resident == trainer.RESIDENT_DEFAULT
    la, lb = GraphLoop(a, seed=9, resident=True), GraphLoop(b, seed=9, resident=False, steps_per_graph=4)
    assert la.resident and not la.bufs and not la.pipeline and not lb.resident and lb.bufs
    la.run(n // 2); la.run(n - n // 2)
    lb.run(n)
    la.check()
    sa, sb = a.optimizer.state, b.optimizer.state
    assert sa.step == n == sb.step
    xa, xb = la.losses(), lb.losses()
    assert xa.numel() == n
    _close([a.model.flat, sa.grads, sa.m, sa.v, sa.step_dev, xa.cuda()], [b.model.flat, sb.grads, sb.m, sb.v, sb.step_dev, xb.cuda()], n)


def test_run_py_fast_loop_on_a_sigmoid_line(tmp_path):
    """The first line of sigmoid_vae_padding_expts.sh, 12 batches, --fast_loop, in a fresh process."""
    from vae_training_amd import trainer
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "sig", "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "12", "--fast_loop"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Train step: linear kernels" in r.stdout, r.stdout[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train loop:")]
    assert len(lines) == 1, r.stdout[-1500:]
    if trainer.RESIDENT_DEFAULT:
        assert lines[0] == "Train loop: resident linear kernel, 1024 steps per launch", lines[0]
    z = np.load(os.path.join(str(tmp_path), "data", "sig", "losses.npz"), allow_pickle=True)
    losses = np.asarray(z["VAE Loss"], dtype=np.float64)
    assert losses.size >= 12 and np.isfinite(losses).all()
