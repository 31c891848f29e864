"""-m gpu: vaek_mlp3_stats_event_replicas -- the stats event of N three-hidden-layer MLP VAEs of one shape in one call, two launches
(csrc/mlp3_stats.hip) -- and its callers, trainer.ReplicaStatsMlp3 and `run.py --sweep_dataset_seeds --mlp_fused_stats`.

A record is [loss, mean Dkl, mean mse, eps, score, score, 0, 0, epsilon_p ...] (vaek_stats_record_len = 8 + L).  References:
  - a float64 NumPy evaluation through oracle.fcn_forward (record64 below) on the x, z1, z2 vaek_make_batch writes for the same (seed,
    step, tag): the inputs are the device's own bits, so the reference is exact on them;
  - the host path the event replaces, which shares no kernel with it: vaek_loss_eval + vaek_forward(sampling) + the dataset class's
    score_batch on those draws;
  - itself, BITWISE: replica r of n = 3 against n = 1 on its slices, two runs, a captured call, engines of other batch sizes and
    force_generic, two parameter strides (one a multiple of 4, one not).
BOUNDS, the project's contract: slots 0 .. 2 within 1e-5 of |loss|, eps within 1e-6, each score within 1e-5 of its own value,
epsilon_p bitwise.  SHAPES, PARAMETERS, seeds and steps are those of tests/test_gpu_mlp3_log_likelihood.py (its docstring); sample_eps
= (-3, 0.5, -1); rows 1 (a tile of one live row), 31, 32, 33 (a second tile of one row), 130, 1000 (the print batch, last tile 8 rows).
HOW WELL FLOAT32 CAN MEET THEM, from the CPU alone (tools/mlp3_stats_event_reference.py, run before any run of the kernel; rows from
the oracle's own datasets, latents from oracle/philox.py): for every (shape, rows) the record in float64 and as a float32 NumPy
restatement (record32 below), the distance per slot.  A (case, slot) whose restatement is further than a fifth of its bound from
float64 is held to the larger of the bound and five times that distance: LOOSE below, written by the tool and fixed before the
kernel ran.  No case is left out.
The tool found NO (case, slot) further than a fifth of its bound (largest distances over all 42 cases: 1.3e-7 on the loss slots,
1.9e-6 on a score -- the sphere error of a single row), so LOOSE is empty and every case is held to the contract.
OBSERVED on one MI355X, the largest error over all 42 cases x 3 replicas against the float64 evaluation, in the unit of
each slot's bound: loss 1.6e-7 (256|256|256, rows 1), Dkl 1.8e-8 (66|201|130, rows 1), mse 1.2e-7 (256|256|256, rows 1), first score
5.9e-6 (sphere6, rows 1: one row's (|fake| - 1)^2; with >= 31 rows below 4e-7), second score 2.3e-7 (mixed, rows 1), eps 0; against
the host path (rows 37 and 1000) 1.3e-7, 4.9e-8, 8.3e-8, 1.5e-7, 2.2e-7, eps 0.  OBSERVED below has the same figures.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import test_gpu_mlp3_log_likelihood as LL
from tests import test_gpu_stats_event as SE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_RTOL, SCORE_RTOL, EPS_ATOL = 1e-5, 1e-5, 1e-6
SENT = -12345.0
LABELS = ["mlp3_stats_tile", "mlp3_stats_finalize"]
R = 3
SAMPLE_EPS = (-3.0, 0.5, -1.0)
X_TAG, Z_TAG = 1, 2
SHAPES = LL.SHAPES
ROWS = (1, 31, 32, 33, 130, 1000)
HOST_ROWS = (37, 1000)
X_SEEDS, Z_SEEDS = [77, 2 ** 63 + 5, 1000003], [2 ** 64 - 3, 991, 31337]
X_STEPS, Z_STEPS = [1, 4, 2 ** 31 + 7], [3, 2 ** 32 - 1, 2]
SLOTS = ("loss", "dkl", "mse", "score0", "score1")
# LOOSE_BEGIN (written by tools/mlp3_stats_event_reference.py: (shape, rows) -> {slot: distance of the float32 restatement from float64,
# in the unit of the slot's bound} for the slots further than a fifth of the bound)
LOOSE = {
}
# LOOSE_END
# OBSERVED on one MI355X, largest over the 42 cases x 3 replicas, in the unit of each slot's bound (|err| / |loss| for slots 0 .. 2,
# |err| / |score| for the scores), from one run of test_records_against_the_float64_oracle; eps: 0
OBSERVED = {"loss": 1.62e-07, "dkl": 1.82e-08, "mse": 1.19e-07, "score0": 5.91e-06, "score1": 2.32e-07}


def nscores(s):
    return 1 if s["kind"] == 0 else 2


def record_from(s, A, eps, sample_eps, lv, mu, y, yf, x, z2, f):
    """The record's first 4 + nscores values from the networks' outputs, every per-element operation in dtype `f` (np.float64: the
    reference; np.float32: the restatement, whose per-row values then go to float64 as the kernel's do).  mu = Encoder(x), y =
    Decoder(samples), yf = Decoder(z1), all [rows, .] arrays of dtype f."""
    D, dd, kind = s["D"], s["dd"], s["kind"]
    eps, sample_eps = f(eps), f(sample_eps)
    x_hat = y + z2 * np.exp(eps / f(2))
    rsq = np.square(x_hat - x).sum(axis=1, dtype=f)
    musq = np.square(mu).sum(axis=1, dtype=f)
    n = float(x.shape[0])
    klc = np.sum((f(1) + lv - np.exp(lv)).astype(np.float64))
    dkl = 0.5 * np.sum(musq.astype(np.float64)) / n - 0.5 * klc
    mse = np.sum((f(0.5) * rsq * np.exp(-eps)).astype(np.float64)) / n + 0.5 * D * (np.log(2 * np.pi) + float(eps))
    fake = (yf + z2 * np.exp(sample_eps / f(2))).astype(f)
    if f is np.float64:
        scores = SE._score64(s, A, fake)
    else:
        sq = np.square(fake)
        if kind == 0:
            scores = [sq[:, dd:].sum(axis=1, dtype=f).astype(np.float64).mean()]
        elif kind == 1:
            yv = fake[:, dd].astype(np.float64)
            cv = (fake[:, :dd] * A.astype(f)).sum(axis=1, dtype=f).astype(np.float64)
            scores = [sq[:, dd + 1:].sum(axis=1, dtype=f).astype(np.float64).mean(),
                      np.square(yv).mean() - 2.0 * yv.mean() * cv.mean() + np.square(cv).mean()]
        else:
            e = np.sqrt(sq[:, :dd].sum(axis=1, dtype=f)) - f(1)
            scores = [np.square(e).astype(np.float64).mean(), sq[:, dd:].sum(axis=1, dtype=f).astype(np.float64).mean()]
    return [dkl + mse, dkl, mse, float(eps)] + [float(v) for v in scores]


def _record(s, p, A, x, z1, z2, sample_eps, f):
    cfg = LL._cfg(s)
    p = {k: np.asarray(v, f) for k, v in p.items()}
    x, z1, z2 = (np.asarray(t, f) for t in (x, z1, z2))
    eps = (p["epsilon"][0] * f(s["eps"])) if s["tdv"] else f(s["eps"])
    lv = p["epsilon_p"]
    mu = O.fcn_forward(p, "Encoder", x, cfg.enc_sizes)[0]
    samples = mu + np.exp(lv / f(2)) * z1
    y = O.fcn_forward(p, "Decoder", samples, cfg.dec_sizes)[0]
    yf = O.fcn_forward(p, "Decoder", z1, cfg.dec_sizes)[0]
    assert mu.dtype == f and y.dtype == f and yf.dtype == f
    return record_from(s, A, eps, sample_eps, lv, mu, y, yf, x, z2, f)


def record64(s, p, A, x, z1, z2, sample_eps):
    """[loss, mean Dkl, mean mse, eps, scores ...] in float64 on the given draws (p: the float64 tree of float32 parameters)."""
    return _record(s, p, A, x, z1, z2, sample_eps, np.float64)


def record32(s, p, A, x, z1, z2, sample_eps):
    """The same in float32 NumPy, every sum over rows in float64 as the kernel takes it."""
    return _record(s, p, A, x, z1, z2, sample_eps, np.float32)


def distances(s, got, ref):
    """Per SLOTS entry |got - ref| in the unit of the slot's bound, and the eps error."""
    d = [abs(got[k] - ref[k]) / abs(ref[0]) for k in range(3)]
    d += [abs(got[4 + k] - ref[4 + k]) / abs(ref[4 + k]) for k in range(nscores(s))]
    return d, abs(got[3] - ref[3])


def bounds(name, rows):
    loose = LOOSE.get((name, rows), {})
    base = dict(loss=LOSS_RTOL, dkl=LOSS_RTOL, mse=LOSS_RTOL, score0=SCORE_RTOL, score1=SCORE_RTOL)
    return [max(base[k], 5.0 * loose.get(k, 0.0)) for k in SLOTS]


class _Event:
    """One engine and R replicas with distinct parameters, seeds (one above 2^63), steps (one above 2^31), dataset matrices and
    sample_eps, in a sentinel-padded parameter stack whose stride is NOT a multiple of 4; records go to a sentinel-filled [R, record
    length + 3] buffer, the tile partials to a workspace filled with a byte pattern."""

    def __init__(self, name, batch=100, **ekw):
        s = self.s = SHAPES[name]
        self.name = name
        self.eng = e = LL._engine(s, batch, **ekw)
        assert e.supports_mlp3_stats_event(s["kind"]) and not e.supports_stats_event(s["kind"])
        self.len = e.stats_record_len
        assert self.len == 8 + s["L"]
        rng = np.random.default_rng(29)
        alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
        self.A = torch.as_tensor(rng.standard_normal((R, alen)), dtype=torch.float32).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.P, self.os = e.P, self.len + 3
        self.ss = e.P + 5 if (e.P + 5) % 4 else e.P + 6
        cfg = LL._cfg(s)
        flats = LL.make_flats_cached(name)
        assert flats[0].size == e.P
        self.params = self.stack(self.ss)
        self.trees = [O.unflatten(cfg, f.astype(np.float64)) for f in flats]
        self.tabs = (LL._i64(X_SEEDS), LL._i32(X_STEPS), LL._i64(Z_SEEDS), LL._i32(Z_STEPS),
                     torch.tensor(SAMPLE_EPS, dtype=torch.float32, device="cuda"))
        self.ws = torch.full((e.mlp3_stats_event_workspace(R, 4096),), 0xA5, dtype=torch.uint8, device="cuda")

    def stack(self, stride):
        st = torch.full((R, stride), SENT, dtype=torch.float32, device="cuda")
        st[:, :self.P] = torch.as_tensor(np.stack(LL.make_flats_cached(self.name))).cuda()
        return st

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float32, device="cuda")

    def call(self, out, rows, rs=None, **kw):
        """The event of replicas `rs` (default: all R) into `out`; kw overrides any argument."""
        s = self.s
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, kind=s["kind"], A=None if self.A is None else self.A[sl], dd=s["dd"], did=s["did"], pad=s["pad"],
                 var_added=s["var"], x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl], z_steps=self.tabs[3][sl],
                 sample_eps=self.tabs[4][sl], out=out, workspace=self.ws, a_stride=self.a_stride, x_tag=X_TAG, z_tag=Z_TAG)
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.mlp3_stats_event_replicas(**a)

    def records(self, rows, **kw):
        out = self.out()
        self.call(out, rows, **kw)
        torch.cuda.synchronize()
        return out

    def draws(self, r, rows):
        """x, z1, z2 of replica r as vaek_make_batch writes them on the same (seed, step, tag)."""
        s, e = self.s, self.eng
        Ar = None if self.A is None else self.A[r].clone()
        x, _, _ = e.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, X_SEEDS[r], step=X_STEPS[r], tag=X_TAG, want_z=False)
        _, z1, z2 = e.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, Z_SEEDS[r], step=Z_STEPS[r], tag=Z_TAG, want_x=False)
        return x, z1, z2


@functools.lru_cache(maxsize=None)
def _event(name):
    return _Event(name)


@functools.lru_cache(maxsize=None)
def _draws(name, r, rows):
    return _event(name).draws(r, rows)


@functools.lru_cache(maxsize=None)
def _records(name, rows):
    return _event(name).records(rows).cpu().numpy().astype(np.float64)


def _check(what, s, got, ref, tols):
    """Prints every figure before the caller asserts; True where every slot is inside its bound."""
    d, eps_err = distances(s, got, ref)
    print(f"{what}: loss {ref[0]:.6f} scores {[f'{v:.5f}' for v in ref[4:]]}; " + " ".join(f"{k} {v:.2e}/{t:.1e}" for k, v, t in zip(SLOTS, d, tols)) +
          f" eps err {eps_err:.2e}")
    return all(v <= t for v, t in zip(d, tols)) and eps_err <= EPS_ATOL, d


def _check_layout(ev, rec):
    s = ev.s
    if nscores(s) == 1:
        assert np.all(rec[:, 5] == 0.0)
    assert np.all(rec[:, 6:8] == 0.0)
    off = ev.eng.leaves["epsilon_p"][0]
    assert np.array_equal(rec[:, 8:ev.len], ev.params[:, off:off + s["L"]].cpu().numpy().astype(np.float64))      # epsilon_p, copied: bitwise
    assert np.all(rec[:, ev.len:] == SENT), "floats between two records were written"
    assert bool((ev.params[:, ev.P:] == SENT).all()), "floats behind a replica's parameters were written"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_against_the_float64_oracle(name, rows):
    ev, rec = _event(name), _records(name, rows)
    s, tols, bad = ev.s, bounds(name, rows), []
    for r in range(R):
        x, z1, z2 = (t.cpu().numpy().astype(np.float64) for t in _draws(name, r, rows))
        A64 = None if ev.A is None else ev.A[r].cpu().numpy().astype(np.float64)
        ref = record64(s, ev.trees[r], A64, x, z1, z2, SAMPLE_EPS[r])
        ok, d = _check(f"{name} rows {rows} replica {r}", s, rec[r], ref, tols)
        if not ok:
            bad.append((r, d))
    _check_layout(ev, rec)
    assert not bad, (bad, tols)


@pytest.mark.parametrize("rows", HOST_ROWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_records_against_the_host_path(name, rows):
    """vaek_loss_eval + vaek_forward(sampling) + score_batch on vaek_make_batch's draws: the layer-by-layer kernels of an engine whose
    batch is `rows`."""
    ev, rec = _event(name), _records(name, rows)
    s, bad = ev.s, []
    host_eng = LL._engine(s, rows)
    for r in range(R):
        x, z1, z2 = _draws(name, r, rows)
        flat = ev.params[r, :ev.P].contiguous()
        out4 = host_eng.loss_eval(flat, x, z1, z2).cpu().numpy().astype(np.float64)
        fake32, _ = host_eng.forward(flat, None, z1, z2, sampling=True, eps=SAMPLE_EPS[r], want_mu=False)
        ref = list(out4) + SE._host_score(s, None if ev.A is None else ev.A[r], fake32)
        ok, d = _check(f"{name} rows {rows} replica {r} (host path)", s, rec[r], ref, bounds(name, rows))
        if not ok:
            bad.append((r, d))
    _check_layout(ev, rec)
    assert not bad, bad


@pytest.mark.parametrize("name,rows", [("sphere6", 1000), ("odd", 33), ("wide", 130), ("narrow", 1), ("mixed", 31), ("notdv", 32), ("sphere21", 130)])
def test_records_are_bitwise_reproducible(name, rows):
    """Two runs equal; replica r of the n = 3 call = the n = 1 call on its slices; a parameter stride that is a multiple of 4 leaves
    the bits of one that is not; floats between records, behind each replica's parameters and A untouched."""
    ev = _event(name)
    before, a_before = ev.params.clone(), None if ev.A is None else ev.A.clone()
    a, b = ev.records(rows), ev.records(rows)
    assert torch.equal(a, b)
    assert bool((a[:, ev.len:] == SENT).all()), "floats between two records were written"
    assert bool((a[:, :ev.len] != SENT).all())
    for r in range(R):
        one = ev.out(1)
        ev.call(one, rows, rs=slice(r, r + 1))
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[r]), (r, one[0], a[r])
    assert ev.ss % 4 != 0
    s4 = (ev.P + 8) & ~3
    p4 = ev.stack(s4)
    assert torch.equal(ev.records(rows, params=p4), a)
    assert bool((p4[:, ev.P:] == SENT).all())
    assert torch.equal(ev.params, before), "params, or the floats between two replicas' parameters, were written"
    assert ev.A is None or torch.equal(ev.A, a_before), "A was written"


def test_mlp3_stats_event_is_capturable():
    """A captured call replayed twice = the eager call."""
    ev = _event("sphere6")
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


@pytest.mark.parametrize("name", ["sphere6", "odd"])
def test_the_batch_size_of_the_engine_does_not_matter(name):
    """Engines of batch 5, 100, 257 and one with force_generic leave bitwise the same records."""
    ev = _event(name)
    s = ev.s
    want = {rows: ev.records(rows) for rows in (33, 1000)}
    for batch, kw in ((5, {}), (100, {}), (257, {}), (100, dict(force_generic=True))):
        eng = LL._engine(s, batch, **kw)
        assert eng.supports_mlp3_stats_event(s["kind"]) and not eng.supports_stats_event(s["kind"]), (batch, kw)
        for rows, rec in want.items():
            assert torch.equal(ev.records(rows, eng=eng), rec), (batch, kw, rows)


@pytest.mark.parametrize("name", ["narrow", "sphere21", "odd"])
def test_sample_eps_moves_the_scores_only(name):
    """Changing sample_eps alone changes slots 4 and 5 (5 stays 0 for a kind with one score) and leaves every other float bitwise."""
    ev = _event(name)
    a = ev.records(130)
    b = ev.records(130, sample_eps=torch.tensor([0.25, -2.0, 1.5], dtype=torch.float32, device="cuda"))
    keep = [k for k in range(ev.os) if k not in (4, 5)]
    assert torch.equal(a[:, keep], b[:, keep])
    assert bool((a[:, 4] != b[:, 4]).all())
    if nscores(ev.s) == 2:
        assert bool((a[:, 5] != b[:, 5]).all())
    else:
        assert bool((b[:, 5] == 0.0).all())


def test_arguments_predicate_and_profile_labels():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message that names the entry and leaves `out`, the
    parameters and the workspace unchanged; the predicate (false for the shapes vaek_supports_mlp3_log_likelihood rejects, true for a
    batch-257 context); vaek_stats_event_replicas still refuses an mlp3 context; the workspace query; one profile record per launch."""
    from vae_training_amd import _lib
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c, lin, sph = _event("narrow"), _event("odd"), _event("sphere6")

    def refused(why, e, **kw):
        out = e.out()
        before, ws_before = e.params.clone(), e.ws.clone()
        with pytest.raises(VaekError) as ei:
            e.call(out, kw.pop("rows", 37), **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert "vaek_mlp3_stats_event_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(e.params, before) and torch.equal(e.ws, ws_before), why

    H = (200, 200, 200)
    assert Engine(257, 6, 6, H, H, -1.0, True, False).supports_mlp3_stats_event(2)                           # batch 257: trains layer by layer
    assert Engine(257, 6, 6, H, H, -1.0, True, False).step_path != "mlp3"
    assert Engine(100, 6, 6, H, H, -1.0, True, False, force_generic=True).supports_mlp3_stats_event(2)
    assert Engine(100, 32, 32, (64, 256, 64), (256, 64, 256), -1.0, False, False).supports_mlp3_stats_event(0)
    no = [("two hidden layers", Engine(100, 6, 6, (200, 200), (200, 200), -1.0, True, False), 2),
          ("four hidden layers", Engine(100, 6, 6, H + (200,), H + (200,), -1.0, True, False), 2),
          ("two encoder layers only", Engine(100, 6, 6, (200, 200), H, -1.0, True, False), 2),
          ("width 63", Engine(100, 6, 6, (200, 63, 200), H, -1.0, True, False), 2),
          ("width 257", Engine(100, 6, 6, H, (200, 200, 257), -1.0, True, False), 2),
          ("D = 33", Engine(100, 33, 6, H, H, -1.0, True, False), 0),
          ("L = 33", Engine(100, 6, 33, H, H, -1.0, True, False), 2),
          ("two decoders", Engine(100, 7, 6, H, H, -1.0, True, True), 1),
          ("bf16", Engine(100, 6, 6, (192, 192, 192), (192, 192, 192), -1.0, True, False, dtype="bf16"), 2),
          ("a linear model", Engine(100, 6, 6, (), (), -1.0, True, False), 2)]
    for why, eng, kind in no:
        assert not eng.supports_mlp3_stats_event(kind) and not eng.supports_mlp3_log_likelihood(kind), why
        refused(why, sph, eng=eng)
    assert not c.eng.supports_mlp3_stats_event(3) and not c.eng.supports_mlp3_stats_event(-1)
    # the linear entry keeps refusing an mlp3 context
    out = sph.out()
    with pytest.raises(VaekError) as ei:
        sph.eng.stats_event_replicas(sph.params, 37, 2, None, 3, 3, 3, 0.0, *sph.tabs, out, x_tag=X_TAG, z_tag=Z_TAG)
    assert ei.value.code == -1 and "vaek_stats_event_replicas" in str(ei.value) and bool((out == SENT).all())
    refused("struct_size", c, struct_size=12)
    refused("n = 0", c, n=0)
    refused("n over the cap", c, n=c.eng.train_loop_max_replicas + 1)
    refused("rows = 0", c, rows=0)
    refused("rows over the cap", c, rows=4097)
    for name in ("x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps"):
        refused(name + " NULL", c, **{name: None})
    with pytest.raises(VaekError) as ei:
        c.call(None, 37, out_stride=c.os)
    assert ei.value.code == -1 and "out" in str(ei.value) and "vaek_mlp3_stats_event_replicas" in str(ei.value)
    with pytest.raises(VaekError) as ei:
        c.call(c.out(), 37, params=None, n=R, state_stride=c.ss)
    assert ei.value.code == -1 and "vaek_mlp3_stats_event_replicas" in str(ei.value)
    refused("state_stride < P", c, state_stride=c.P - 1)
    refused("out_stride < record length", c, out_stride=c.len - 1)
    refused("workspace NULL", c, workspace=None)
    refused("workspace misaligned", c, workspace=c.ws.data_ptr() + 8)
    refused("a_stride < 0", c, a_stride=-1)
    refused("A NULL, kind 1", c, A=None)
    refused("A NULL, kind 0", lin, A=None)
    refused("dd = 17", c, dd=17)
    refused("did = 17", lin, did=17)
    refused("kind 3", c, kind=3)
    refused("kind -1", c, kind=-1)
    refused("x_tag = 2^30", c, x_tag=2 ** 30)
    refused("z_tag = 2^30", c, z_tag=2 ** 30)
    refused("dataset dimension != data_dim", c, pad=4)
    b = _lib.C.c_size_t(7)
    for n, rows in ((0, 37), (c.eng.train_loop_max_replicas + 1, 37), (1, 0), (1, 4097)):
        assert c.eng.lib.vaek_mlp3_stats_event_workspace_bytes(c.eng.h, n, rows, _lib.C.byref(b)) == -1 and b.value == 7, (n, rows)
    assert c.eng.mlp3_stats_event_workspace(1, 1) == 64 and c.eng.mlp3_stats_event_workspace(3, 1000) == 3 * 32 * 64
    assert c.eng.mlp3_stats_event_workspace(1, 33) == 128 and c.eng.stats_event_max_rows == 4096
    # kind 2 needs no A; a shared A (a_stride 0) is legal; the row cap itself is legal; exactly one profile record per launch
    sph.call(sph.out(), 37, A=None)
    c.call(c.out(), 4096)
    c.eng.profile_begin(16)
    out = c.out()
    c.call(out, 37, a_stride=0, A=c.A[0].clone())
    c.call(out, 1000)
    torch.cuda.synchronize()
    rep = c.eng.profile_report()
    assert sorted(rep) == sorted(LABELS) and all(rep[k]["count"] == 2 for k in LABELS), rep


def _host_state(m):
    return (m.key, m.dataset._draws, m._latent_draws, np.asarray(torch.as_tensor(m.current_epsilon).cpu()).tolist(), len(m.vae_losses),
            len(m.var_enc), len(m.var_dec))


def test_replica_stats_mlp3_against_compute_stats(tmp_path):
    """ReplicaStatsMlp3.event() on three sphere models (dataset seeds 69, 24, 48) against compute_stats() on their copies -- twins
    built from the same arguments, bitwise the same parameters and keys (asserted): a model holds a library handle, which
    copy.deepcopy cannot take --: the stats within the bounds, the host state identical afterwards; then a host event on the swept
    models and a fused one on the twins (mixed), and both again."""
    from tests.test_gpu_mlp3_replicas import _sphere_model
    from vae_training_amd.trainer import ReplicaStatsMlp3
    ms = [_sphere_model(tmp_path, f"s{seed}", seed, 1e-3) for seed in (69, 24, 48)]
    twins = [_sphere_model(tmp_path, f"t{seed}", seed, 1e-3) for seed in (69, 24, 48)]
    for m, t in zip(ms, twins):
        assert torch.equal(m.model.flat, t.model.flat) and m.key == t.key and m.dataset.key == t.dataset.key
    rs, rt = ReplicaStatsMlp3(ms), ReplicaStatsMlp3(twins)
    assert rs.rows == 1000 and rs.eng.step_path == "mlp3"

    def compare(fused, host, who):
        for r, (f, h) in enumerate(zip(fused, host)):
            assert list(f) == list(h), (list(f), list(h))
            loss = abs(float(h["VAE Loss"]))
            for k in f:
                a, b = float(h[k]), float(f[k])
                tol = LOSS_RTOL * loss if k in ("VAE Loss", "KL divergence", "mse") else SCORE_RTOL * abs(a)
                print(f"{who} model {r} {k}: host {a:.7f} fused {b:.7f} |diff| {abs(a - b):.2e} (bound {tol:.2e})")
                assert abs(a - b) <= tol, (who, r, k, a, b)

    fused = rs.event()
    host = [t.compute_stats() for t in twins]
    compare(fused, host, "event 1")
    assert [_host_state(m) for m in ms] == [_host_state(t) for t in twins]
    host = [m.compute_stats() for m in ms]                               # mixed: the roles swapped
    fused = rt.event()
    compare(fused, host, "event 2 (swapped)")
    assert [_host_state(m) for m in ms] == [_host_state(t) for t in twins]
    compare(rs.event(), [t.compute_stats() for t in twins], "event 3")
    assert [_host_state(m) for m in ms] == [_host_state(t) for t in twins]
    for m, t in zip(ms, twins):
        assert torch.equal(m.var_enc[-1].cpu(), t.var_enc[-1].cpu()) and _host_state(m)[1] == 3


def _run_py(tmp_path, name, *extra, layers="200|200|200", dataset="sphere"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", dataset, "--encoder_layer_sizes", layers, "--layer_sizes", layers,
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


STATS_LINE = "Stats events: one call for 2 models (vaek_mlp3_stats_event_replicas)"


def test_run_py_mlp_fused_stats_in_a_fresh_process(tmp_path):
    """Line 1 of sphere_vae_padding_expts.sh, 30 batches, --sweep_dataset_seeds 69,24, with and without --mlp_fused_stats: the same
    keys in losses.npz, the 30 train losses per seed and model.pkl BITWISE equal (the host RNG bookkeeping of the fused event did not
    shift anything), the step-0 stats within the bounds; a linear sweep refuses the flag and names --fused_stats."""
    runs = {}
    for name, extra in (("host", ()), ("fused", ("--mlp_fused_stats",))):
        r = _run_py(tmp_path, name, "--sweep_dataset_seeds", "69,24", *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert (STATS_LINE in r.stdout) == (name == "fused"), r.stdout[-1500:]
        assert "Stats events: one launch" not in r.stdout
        runs[name] = {seed: LL._outputs(tmp_path, f"{name}_ds{seed}") for seed in (69, 24)}
    for seed in (69, 24):
        (h, ckpt_h), (f, ckpt_f) = runs["host"][seed], runs["fused"][seed]
        assert list(h) == list(f), (list(h), list(f))
        lh, lf = np.asarray(h["VAE Loss"], dtype=np.float32), np.asarray(f["VAE Loss"], dtype=np.float32)
        assert lh.size == 31 == lf.size and np.array_equal(lh[-30:], lf[-30:]), (seed, lh, lf)
        assert LL._same(ckpt_h, ckpt_f), seed
        loss = abs(float(np.asarray(h["VAE Loss"], dtype=np.float64).reshape(-1)[0]))
        for key in ("VAE Loss", "KL divergence", "mse", "Sphere Error", "Padding Error"):
            a, b = float(np.asarray(h[key], dtype=np.float64).reshape(-1)[0]), float(np.asarray(f[key], dtype=np.float64).reshape(-1)[0])
            tol = LOSS_RTOL * loss if key in ("VAE Loss", "KL divergence", "mse") else SCORE_RTOL * abs(a)
            print(f"seed {seed} step-0 {key}: host {a:.7f} fused {b:.7f} (bound {tol:.2e})")
            assert abs(a - b) <= tol, (seed, key, a, b)
        assert np.array_equal(np.asarray(h["Encoder Variance"], dtype=np.float32), np.asarray(f["Encoder Variance"], dtype=np.float32))
        np.testing.assert_allclose(np.asarray(f["Decoder Variance"], dtype=np.float64), np.asarray(h["Decoder Variance"], dtype=np.float64), atol=1e-6)
    assert not np.array_equal(runs["fused"][69][0]["VAE Loss"], runs["fused"][24][0]["VAE Loss"])
    r = _run_py(tmp_path, "lin", "--sweep_dataset_seeds", "69,24", "--mlp_fused_stats", layers="", dataset="sigmoid")
    assert r.returncode != 0 and "--mlp_fused_stats needs" in r.stderr and "use --fused_stats" in r.stderr and "'linear'" in r.stderr, r.stderr[-1500:]
    assert "Batch |" not in r.stdout
