"""-m gpu: vaek_stats_event_replicas -- the stats event of N small linear VAEs of one shape in ONE launch (csrc/linear_stats.hip),
workgroup r evaluating model r -- and its callers, trainer.ReplicaStats and `run.py --sweep_dataset_seeds --fused_stats`.

A record is [loss, mean Dkl, mean mse, eps, score, score, 0, 0, epsilon_p].  Three references:
  - the float64 oracle on the very draws vaek_make_batch writes for the same (seed, step, tag): loss slots within LOSS_RTOL = 1e-5 of
    |loss| (the bound of tests/test_gpu_parity.py), eps within 1e-6, each score within 1e-5 of its own value, epsilon_p bitwise.  A
    wrong counter in the in-kernel draw is an O(1) error here; a wrong sample_eps shows in the score slots alone;
  - the host path the event replaces (vaek_loss_eval + vaek_forward(sampling) + score_batch on those draws), same bounds;
  - itself, BITWISE: replica r of an n = 3 call against an n = 1 call on its slices, two runs, a captured call replayed twice.
The shapes are the smallest that reach every branch: every dataset kind, one and two decoders, with and without -tdv, L below / equal
to / not a multiple of 4 away from D, dataset noise, a padded variant larger than the shape and the 28 x 24 one; rows 37 (one
partial tile), 256, 257 (a second tile of one row) and 1000 (the reference's print batch)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL = 1e-5
SCORE_RTOL = 1e-5
SENT = -12345.0
LABEL = "linear_stats_replicas"
R = 3
SAMPLE_EPS = (-3.0, 0.5, -1.0)
X_TAG, Z_TAG = 1, 2
SHAPES = {
    "sigmoid": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=7, L=6, dd=3, did=1, pad=3, var=0.0),
    "linear_gaussian": dict(sig=False, tdv=False, eps=-1.0, kind=0, D=5, L=5, dd=3, did=2, pad=2, var=0.01),
    "sphere": dict(sig=False, tdv=True, eps=-1.0, kind=2, D=7, L=4, dd=3, did=3, pad=4, var=0.0),
    "sigmoid28x24": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=28, L=24, dd=7, did=1, pad=20, var=0.0),
}
ROWS = (37, 256, 257, 1000)


class _Event:
    """One engine and R replicas with distinct parameters (randn * 0.3), seeds (one above 2^63), steps (one above 2^31), dataset
    matrices and sample_eps, in a parameter stack whose stride exceeds P by 5 sentinel floats; records go to a sentinel-filled
    [R, record length + 3] buffer."""

    def __init__(self, name):
        from vae_training_amd.engine import Engine
        s = self.s = SHAPES[name]
        self.eng = e = Engine(100, s["D"], s["L"], (), (), s["eps"], s["tdv"], s["sig"])
        assert e.supports_stats_event(s["kind"]) and e.supports_train_loop_gen(s["kind"])
        self.len = e.stats_record_len
        assert self.len == 8 + s["L"]
        g = torch.Generator().manual_seed(23)
        alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
        self.A = torch.randn(R, alen, generator=g).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.P, self.ss, self.os = e.P, e.P + 5, self.len + 3
        self.params = torch.full((R, self.ss), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :e.P] = (torch.randn(R, e.P, generator=g) * 0.3).cuda()
        self.x_seeds, self.z_seeds = [77, 2 ** 63 + 5, 1000003], [2 ** 64 - 3, 991, 31337]
        self.x_steps, self.z_steps = [1, 4, 2 ** 31 + 7], [3, 2 ** 32 - 1, 2]
        self.tabs = (_i64(self.x_seeds), _i32(self.x_steps), _i64(self.z_seeds), _i32(self.z_steps),
                     torch.tensor(SAMPLE_EPS, dtype=torch.float32, device="cuda"))

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float32, device="cuda")

    def call(self, out, rows, rs=None, **kw):
        """The event of replicas `rs` (default: all R) into `out`; kw overrides any argument."""
        s = self.s
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, kind=s["kind"], A=None if self.A is None else self.A[sl], dd=s["dd"], did=s["did"], pad=s["pad"],
                 var_added=s["var"], x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl], z_steps=self.tabs[3][sl],
                 sample_eps=self.tabs[4][sl], out=out, a_stride=self.a_stride, x_tag=X_TAG, z_tag=Z_TAG)
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.stats_event_replicas(**a)

    def records(self, rows):
        out = self.out()
        self.call(out, rows)
        torch.cuda.synchronize()
        return out

    def draws(self, r, rows):
        """x, z1, z2 of replica r as vaek_make_batch writes them on the same (seed, step, tag)."""
        s, e = self.s, self.eng
        Ar = None if self.A is None else self.A[r].clone()
        x, _, _ = e.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG, want_z=False)
        _, z1, z2 = e.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, self.z_seeds[r], step=self.z_steps[r], tag=Z_TAG,
                                 want_x=False)
        return x, z1, z2


@functools.lru_cache(maxsize=None)
def _event(name):
    return _Event(name)


def _score64(s, A, fake):
    """datasets.py score_batch in float64, the sigmoid dataset's (B,) against (B, 1) broadcast as a true B x B array."""
    dd = s["dd"]
    if s["kind"] == 0:
        return [np.square(fake[:, dd:]).sum(axis=1).mean()]
    if s["kind"] == 1:
        cod = fake[:, :dd] @ A.reshape(dd, 1)                                # (B, 1)
        return [np.square(fake[:, dd + 1:]).sum(axis=1).mean(), np.square(fake[:, dd] - cod).mean()]
    return [np.square(np.linalg.norm(fake[:, :dd], axis=1) - 1.0).mean(), np.square(fake[:, dd:]).sum(axis=1).mean()]


def _host_score(s, A, fake):
    """The dataset class's own score_batch (torch, float32) on the fake batch."""
    from vae_training_amd.datasets import LinearGaussianDataset, SigmoidDataset, SphereDataset
    if s["kind"] == 0:
        ds = LinearGaussianDataset(1, dimension=s["dd"], intrinsic_dimension=s["did"], padding_dimension=s["pad"], var_added=s["var"], device="cuda")
    elif s["kind"] == 1:
        ds = SigmoidDataset(1, dimension=s["dd"], padding_dimension=s["pad"], device="cuda")
        ds.A = A.reshape(s["dd"], 1)
    else:
        ds = SphereDataset(1, dimension=s["dd"], padding_dimension=s["pad"], device="cuda")
    return [float(v) for v in ds.score_batch(fake).values()]


@functools.lru_cache(maxsize=None)
def _case(name, rows):
    """Computed once per (shape, rows) and shared by the parity tests: the fused records, and per replica the oracle's and the host
    path's numbers on the draws vaek_make_batch writes."""
    from vae_training_amd.engine import Engine
    ev = _event(name)
    s = ev.s
    rec = ev.records(rows).cpu().numpy().astype(np.float64)
    cfg = O.Config(s["D"], s["L"], (), (), s["eps"], s["tdv"], "sigmoid" if s["sig"] else None)
    host_eng = Engine(rows, s["D"], s["L"], (), (), s["eps"], s["tdv"], s["sig"])
    oracle, host = [], []
    for r in range(R):
        x, z1, z2 = ev.draws(r, rows)
        flat = ev.params[r, :ev.P].contiguous()
        p = O.unflatten(cfg, flat.cpu().numpy().astype(np.float64))
        x64, z164, z264 = (t.cpu().numpy().astype(np.float64) for t in (x, z1, z2))
        loss, dkl, mse, _, eps = O.loss_eval(cfg, p, x64, z164, z264)
        (fake, _, _, _), _ = O.vae_forward(cfg, p, None, z164, z264, sampling=True, epsilon=SAMPLE_EPS[r])
        A64 = None if ev.A is None else ev.A[r].cpu().numpy().astype(np.float64)
        oracle.append([loss, dkl, mse, float(np.asarray(eps).reshape(-1)[0])] + _score64(s, A64, fake))
        out4 = host_eng.loss_eval(flat, x, z1, z2).cpu().numpy().astype(np.float64)
        fake32, _ = host_eng.forward(flat, None, z1, z2, sampling=True, eps=SAMPLE_EPS[r], want_mu=False)
        host.append(list(out4) + _host_score(s, None if ev.A is None else ev.A[r], fake32))
    return dict(rec=rec, oracle=oracle, host=host)


def _check_against(name, rows, which):
    ev, c = _event(name), _case(name, rows)
    bad = []
    for r in range(R):
        got, ref = c["rec"][r], c[which][r]
        nscore = len(ref) - 4
        tol = LOSS_RTOL * abs(ref[0])
        errs = [abs(got[k] - ref[k]) for k in range(3)]
        score_rel = [abs(got[4 + k] - ref[4 + k]) / abs(ref[4 + k]) for k in range(nscore)]
        print(f"{name} rows {rows} replica {r} against {which}: loss {ref[0]:.6f} |err| of loss/dkl/mse {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} "
              f"(bound {tol:.2e}), eps err {abs(got[3] - ref[3]):.2e}, scores {[f'{v:.4f}' for v in ref[4:]]} rel err {[f'{v:.2e}' for v in score_rel]}")
        assert all(v >= 0.05 for v in ref[4:]), ("a reference score near zero makes the relative bound meaningless", ref[4:])
        if max(errs) > tol or abs(got[3] - ref[3]) > 1e-6 or max(score_rel) > SCORE_RTOL:
            bad.append((r, errs, tol, score_rel))
        if nscore == 1:
            assert got[5] == 0.0
        assert got[6] == 0.0 and got[7] == 0.0
    assert not bad, bad
    # epsilon_p, copied: bitwise (float32 -> float64 is exact on both sides)
    off = ev.eng.leaves["epsilon_p"][0]
    assert np.array_equal(c["rec"][:, 8:ev.len], ev.params[:, off:off + ev.s["L"]].cpu().numpy().astype(np.float64))
    assert np.all(c["rec"][:, ev.len:] == SENT)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_against_the_oracle(name, rows):
    _check_against(name, rows, "oracle")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_against_the_host_path(name, rows):
    _check_against(name, rows, "host")


@pytest.mark.parametrize("name,rows", [("sigmoid", 1000), ("sigmoid", 257), ("linear_gaussian", 37), ("sphere", 256), ("sigmoid28x24", 1000)])
def test_records_are_bitwise_reproducible(name, rows):
    """Replica r of the n = 3 call = the n = 1 call on its slices; two runs equal; floats between records and params untouched."""
    ev = _event(name)
    before = ev.params.clone()
    a, b = ev.records(rows), ev.records(rows)
    assert torch.equal(a, b)
    assert bool((a[:, ev.len:] == SENT).all()), "floats between two records were written"
    assert bool((a[:, :ev.len] != SENT).all())
    assert torch.equal(ev.params, before), "params were written"
    for r in range(R):
        one = ev.out(1)
        ev.call(one, rows, rs=slice(r, r + 1))
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[r]), (r, one[0], a[r])


def test_stats_event_is_capturable():
    """A captured call replayed twice = the eager call."""
    ev = _event("sigmoid")
    eager = ev.records(1000)                             # eager (also the warm-up)
    out = ev.out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ev.call(out, 1000)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                     # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        out[:, :ev.len] = 0.0


def test_arguments_and_profile_label():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message and leaves the sentinel buffers unchanged; one
    profile record per call."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    ev, lin, sph = _event("sigmoid"), _event("linear_gaussian"), _event("sphere")

    def refused(why, e, **kw):
        out = e.out()
        before = e.params.clone()
        with pytest.raises(VaekError) as ei:
            e.call(out, kw.pop("rows", 37), **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert "vaek_stats_event_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(e.params, before), why

    for why, eng in [("B = 257", Engine(257, 7, 6, (), (), -3.0, True, True)), ("one hidden layer", Engine(100, 7, 6, (64,), (64,), -3.0, True, True)),
                     ("force_generic", Engine(100, 7, 6, (), (), -3.0, True, True, force_generic=True))]:
        assert not eng.supports_stats_event(1) and not eng.supports_train_loop_gen(1), why
        refused(why, ev, eng=eng)
    refused("struct_size", ev, struct_size=12)
    refused("n = 0", ev, n=0)
    refused("n over the cap", ev, n=1025)
    refused("rows = 0", ev, rows=0)
    refused("rows over the cap", ev, rows=4097)
    for name in ("x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps"):
        refused(name + " NULL", ev, **{name: None})
    with pytest.raises(VaekError) as ei:
        ev.call(None, 37, out_stride=ev.os)
    assert ei.value.code == -1 and "out" in str(ei.value)
    refused("state_stride < P", ev, state_stride=ev.P - 1)
    refused("out_stride < record length", ev, out_stride=ev.len - 1)
    refused("a_stride < 0", ev, a_stride=-1)
    refused("A NULL, kind 1", ev, A=None)
    refused("A NULL, kind 0", lin, A=None)
    refused("dd = 17", ev, dd=17)
    refused("did = 17", lin, did=17)
    refused("kind 3", ev, kind=3)
    refused("kind -1", ev, kind=-1)
    refused("x_tag = 2^30", ev, x_tag=2 ** 30)
    refused("z_tag = 2^30", ev, z_tag=2 ** 30)
    refused("dataset dimension != data_dim", ev, pad=4)
    # kind 2 needs no A; a shared A (a_stride 0) is legal; exactly one profile record per call
    sph.call(sph.out(), 37, A=None)
    ev.eng.profile_begin(16)
    out = ev.out()
    ev.call(out, 37, a_stride=0, A=ev.A[0].clone())
    ev.call(out, 1000)
    torch.cuda.synchronize()
    rep = ev.eng.profile_report()
    assert list(rep) == [LABEL] and rep[LABEL]["count"] == 2, rep
    assert ev.eng.stats_event_max_rows == 4096


def _run_py(tmp_path, name, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def test_run_py_fused_stats_in_a_fresh_process(tmp_path):
    """The first line of sigmoid_vae_padding_expts.sh, 30 batches, --sweep_dataset_seeds 69,24, with and without --fused_stats: the
    same keys in losses.npz, the 30 train losses per seed BITWISE equal (the host RNG bookkeeping of the fused event did not shift
    anything), the step-0 evaluation stats equal to 1e-5 relative."""
    runs = {}
    for name, extra in (("host", ()), ("fused", ("--fused_stats",))):
        r = _run_py(tmp_path, name, "--sweep_dataset_seeds", "69,24", *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("Stats events: one launch for 2 models" in r.stdout) == (name == "fused"), r.stdout[-1500:]
        runs[name] = {seed: dict(np.load(os.path.join(str(tmp_path), "data", f"{name}_ds{seed}", "losses.npz"), allow_pickle=True))
                      for seed in (69, 24)}
    for seed in (69, 24):
        h, f = runs["host"][seed], runs["fused"][seed]
        assert list(h) == list(f), (list(h), list(f))
        lh, lf = np.asarray(h["VAE Loss"], dtype=np.float32), np.asarray(f["VAE Loss"], dtype=np.float32)
        assert lh.size == 31 == lf.size and np.array_equal(lh[-30:], lf[-30:]), (seed, lh, lf)
        for key in ("VAE Loss", "KL divergence", "mse", "Squared Norm of Padding Dimensions", "Squared Norm of Manifold Dimension"):
            a, b = float(np.asarray(h[key], dtype=np.float64).reshape(-1)[0]), float(np.asarray(f[key], dtype=np.float64).reshape(-1)[0])
            print(f"seed {seed} step-0 {key}: host {a:.7f} fused {b:.7f}")
            assert abs(a - b) <= 1e-5 * abs(a), (seed, key, a, b)
        assert np.array_equal(np.asarray(h["Encoder Variance"], dtype=np.float32), np.asarray(f["Encoder Variance"], dtype=np.float32))
        np.testing.assert_allclose(np.asarray(f["Decoder Variance"], dtype=np.float64), np.asarray(h["Decoder Variance"], dtype=np.float64), atol=1e-6)
    assert not np.array_equal(runs["fused"][69]["VAE Loss"], runs["fused"][24]["VAE Loss"])


def test_run_py_refuses_fused_stats_on_an_mlp3_sweep(tmp_path):
    """Line 1 of sphere_vae_padding_expts.sh (step path "mlp3": one decoder, three hidden layers both ways) as a sweep: its events stay
    per model, so --fused_stats is refused before any step, with a message that says why."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "m3", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes",
           "200|200|200", "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30",
           "--sweep_dataset_seeds", "69,24", "--fused_stats"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--fused_stats needs" in r.stderr and "mlp3" in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
    assert "Batch |" not in r.stdout
