"""-m gpu: vaek_log_likelihood_replicas -- the importance-weighted log-likelihood of N small linear VAEs of one shape in one call
(csrc/linear_loglik.hip) -- and its callers, trainer.ReplicaLogLik and `run.py --log_likelihood_samples`.

A record is [IWAE-K bound, K-sample ELBO estimate, normalised effective sample size, eps].  References:
  - a float64 NumPy evaluation written here, on the rows vaek_make_batch writes for the same (seed, step, tag) and on normals drawn
    with oracle/philox.py by the block rule of include/vaek.h (sample k of row i: blocks k ceil(L / 4) + j of the latent stream):
    slots 0 and 1 within RTOL = 1e-5 of |value| (the ELBO contract), slot 2 within 1e-5 relative, slot 3 within 1e-6;
  - the closed form: a one-decoder model whose decoder kernel has orthogonal rows and whose encoder is the exact posterior has
    every weight equal to p(x), so slots 0 and 1 are mean log N(x; b_d, W_d^T W_d + e^eps I) and slot 2 is 1, for any K;
  - itself, BITWISE: drawing mode against explicit rows, replica r of n = 3 against n = 1 on its slices, two runs, a captured call,
    engines of different batch sizes.
PARAMETERS of the oracle cases: lecun-normal kernels (oracle.init_params) perturbed by 0.05 N(0, 1), epsilon_p = -2 + 0.3 N(0, 1) (a
posterior narrower than the prior, as a trained encoder's is), epsilon = 1 + 0.05 N(0, 1) under -tdv, eps_cli = -1.  The scale was
chosen on the CPU from the float64 evaluation ALONE: perturbing every normal and every row by the device Box-Muller's documented
distance from float64 (5e-6, tests/test_rng.py) moves slots 0 and 1 by at most 5e-6 relative at every (shape, rows, K) below and
slot 2 by at most 2e-5 in the worst single-row case (rows = 1, K = 64: one row's weights, no averaging), typically 1e-6.  With
epsilon_p = 1 and eps_cli = -3 (an untrained model scored against a tight decoder) the same perturbation moves slot 2 by 1e-4: the
reference itself is then not defined to 1e-5, so those parameters would test the perturbation, not the kernel.
The shapes are the issue's: sigmoid D = 7, L = 6 (two decoders, neither side a multiple of 4), linear_gaussian D = 12, L = 20 (L > D,
-tdv, dataset noise), sphere D = 6, L = 6 without -tdv (no epsilon leaf), two decoders at D = 28, L = 24; rows 1, 37 (one partial
tile), 256, 257 (a second tile of one row), 1000; K 1, 2, 5, 64; n 1 and 3.  One more shape, two decoders at D = 28, L = 32, launches
the 32 x 32 two-decoder instantiation (256 VGPRs + 69 AGPRs, the one most at risk from register pressure).
READING A FAILURE of slot 2 at rows = 1, K = 64: that case is ONE row's weights, the largest error observed on an MI355X is 7.5e-6
of the 1e-5 bound, and the float64 reference itself moves by up to 2e-5 there under the Box-Muller distance.  If a new
compiler or math library pushes it over, compare the normals first (tests/test_rng.py) before blaming the kernel; the cases with 37
rows or more (all below 2e-6) are the ones that say whether the kernel is right."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from oracle import philox as PH
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
SENT = -12345.0
LABELS = ["linear_loglik_replicas", "linear_loglik_finalize"]
R = 3
X_TAG, Z_TAG = 3, 4
MAXR = 1000
SHAPES = {
    "sigmoid": dict(sig=True, tdv=True, eps=-1.0, kind=1, D=7, L=6, dd=3, did=1, pad=3, var=0.0),
    "linear_gaussian": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=12, L=20, dd=3, did=3, pad=9, var=0.01),
    "sphere": dict(sig=False, tdv=False, eps=-1.0, kind=2, D=6, L=6, dd=3, did=3, pad=3, var=0.0),
    "two_decoder": dict(sig=True, tdv=True, eps=-1.0, kind=1, D=28, L=24, dd=7, did=1, pad=20, var=0.0),
    # beyond the issue's four: the 32 x 32 two-decoder instantiation, the only one whose registers reach into the AGPRs
    "two_decoder_wide": dict(sig=True, tdv=True, eps=-1.0, kind=1, D=28, L=32, dd=7, did=1, pad=20, var=0.0),
}
# a mixing matrix that is not square (the A[d * did + k] stride), did > 4 with noise (the noise normals start at Philox block 3, not
# 1), latent streams with L % 4 = 1 and L % 4 = 3: only the drawn-against-supplied comparison runs on these
OFF_SQUARE = {
    "did9_L5": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=7, L=5, dd=5, did=9, pad=2, var=0.25),
    "did9_L7": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=7, L=7, dd=5, did=9, pad=2, var=0.25),
}
ROWS = (1, 37, 256, 257, 1000)
KS = (1, 2, 5, 64)


def _cfg(s):
    return O.Config(s["D"], s["L"], (), (), s["eps"], s["tdv"], "sigmoid" if s["sig"] else None)


def _xi64(seed, step, tag, rows, K, L):
    """[rows, K, L] float64 normals by the block rule: sample k of row i = blocks k * ceil(L / 4) + j, j < ceil(L / 4), of the latent
    stream (counter (row, block, step, tag + 2^30), key = the seed's two words), the first L of the sample's 4 ceil(L / 4) normals."""
    nlb = (L + 3) // 4
    ctr = np.zeros((rows, K * nlb, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(rows, dtype=np.uint32)[:, None]
    ctr[..., 1] = np.arange(K * nlb, dtype=np.uint32)[None, :]
    ctr[..., 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32(tag + 2 ** 30)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return PH.normals_from_bits(PH.philox4x32(ctr, key)).reshape(rows, K, nlb * 4)[:, :, :L]


def _rows64(s, p, x, xi):
    """Per row [IWAE-K bound, mean log w, normalised ESS] in float64: x [rows, D], xi [rows, K, L], p the parameter tree."""
    eps = float(p["epsilon"][0]) * s["eps"] if s["tdv"] else s["eps"]
    lv = p["epsilon_p"]
    mu = x @ p["Encoder/FC0/kernel"] + p["Encoder/FC0/bias"]
    z = mu[:, None, :] + np.exp(lv / 2) * xi
    y = z @ p["Decoder/FC0/kernel"] + p["Decoder/FC0/bias"]
    if s["sig"]:
        y = y + 1.0 / (1.0 + np.exp(-(z @ p["SigDecoder/FC0/kernel"] + p["SigDecoder/FC0/bias"])))
    rsq = np.square(y - x[:, None, :]).sum(-1)
    lw = -0.5 * (rsq * np.exp(-eps) + s["D"] * (eps + np.log(2 * np.pi))) + 0.5 * (np.square(xi) - np.square(z) + lv).sum(-1)
    m = lw.max(axis=1, keepdims=True)
    w = np.exp(lw - m)
    K = lw.shape[1]
    return np.stack([m[:, 0] + np.log(w.sum(1)) - np.log(K), lw.mean(1), np.square(w.sum(1)) / (K * np.square(w).sum(1))], axis=1), eps


class _Case:
    """One engine and R replicas with distinct parameters, seeds (one above 2^63), steps (one above 2^31) and dataset matrices, in a
    parameter stack whose stride exceeds P by 5 sentinel floats; records go to a sentinel-filled [R, 4 + 3] buffer."""

    def __init__(self, name, batch=100, **ekw):
        from vae_training_amd.engine import Engine
        s = self.s = SHAPES[name] if name in SHAPES else OFF_SQUARE[name]
        self.eng = e = Engine(batch, s["D"], s["L"], (), (), s["eps"], s["tdv"], s["sig"], **ekw)
        assert e.supports_log_likelihood(s["kind"])
        assert e.log_likelihood_record_len == 4
        cfg = _cfg(s)
        rng = np.random.default_rng(23)
        alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
        self.A = torch.as_tensor(rng.standard_normal((R, alen)), dtype=torch.float32).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.P, self.ss, self.os = e.P, e.P + 5, 4 + 3
        flats = []
        for r in range(R):
            p = {k: v + 0.05 * rng.standard_normal(v.shape) for k, v in O.init_params(cfg, seed=r).items()}
            p["epsilon_p"] = -2.0 + 0.3 * rng.standard_normal(s["L"])
            flats.append(O.flatten(cfg, p, np.float32))
        self.params = torch.full((R, self.ss), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :e.P] = torch.as_tensor(np.stack(flats)).cuda()
        self.trees = [O.unflatten(cfg, f.astype(np.float64)) for f in flats]
        self.x_seeds, self.z_seeds = [77, 2 ** 63 + 5, 1000003], [2 ** 64 - 3, 991, 31337]
        self.x_steps, self.z_steps = [1, 4, 2 ** 31 + 7], [3, 2 ** 32 - 1, 2]
        self.tabs = (_i64(self.x_seeds), _i32(self.x_steps), _i64(self.z_seeds), _i32(self.z_steps))
        self.ws = torch.empty(e.log_likelihood_workspace(R, 4096), dtype=torch.uint8, device="cuda")
        assert self.ws.numel() == 8 * 4 * R * 16 and e.log_likelihood_workspace(1, 257) == 64

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float32, device="cuda")

    def call(self, out, rows, K, rs=None, **kw):
        """The records of replicas `rs` (default: all R) into `out`, drawing mode; kw overrides any argument."""
        s = self.s
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, samples=K, z_seeds=self.tabs[2][sl], z_steps=self.tabs[3][sl], out=out, workspace=self.ws,
                 kind=s["kind"], A=None if self.A is None else self.A[sl], dd=s["dd"], did=s["did"], pad=s["pad"], var_added=s["var"],
                 x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], a_stride=self.a_stride, x_tag=X_TAG, z_tag=Z_TAG)
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.log_likelihood_replicas(**a)

    def records(self, rows, K, **kw):
        out = self.out()
        self.call(out, rows, K, **kw)
        torch.cuda.synchronize()
        return out

    def x_rows(self, r, rows):
        """Replica r's rows as vaek_make_batch writes them on the same (seed, step, tag)."""
        s = self.s
        Ar = None if self.A is None else self.A[r].clone()
        return self.eng.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG,
                                   want_z=False)[0]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, K):
    """Per replica the float64 per-row values of the first MAXR rows (row i and its samples do not depend on `rows`), and eps."""
    c = _case(name)
    s = c.s
    res = []
    for r in range(R):
        x = c.x_rows(r, MAXR).cpu().numpy().astype(np.float64)
        xi = _xi64(c.z_seeds[r], c.z_steps[r], Z_TAG, MAXR, K, s["L"])
        res.append(_rows64(s, c.trees[r], x, xi))
    return res


@functools.lru_cache(maxsize=None)
def _records(name, rows, K):
    return _case(name).records(rows, K).cpu().numpy().astype(np.float64)


def _check(what, got, ref, eps):
    errs = [abs(got[k] - ref[k]) for k in range(3)]
    print(f"{what}: IWAE {ref[0]:.6f} ELBO {ref[1]:.6f} ESS {ref[2]:.6f}; |err| / |value| {errs[0] / abs(ref[0]):.2e} {errs[1] / abs(ref[1]):.2e} "
          f"{errs[2] / abs(ref[2]):.2e} (bound {RTOL:.0e}), eps err {abs(got[3] - eps):.2e}")
    return all(errs[k] <= RTOL * abs(ref[k]) for k in range(3)) and abs(got[3] - eps) <= 1e-6


# the issue's four shapes at every (rows, K); the added shape where its float64 reference is defined to the bound: at L = 32 the
# Box-Muller distance alone moves the reference's slot 2 by up to 5e-5 on a single row and 1.4e-5 on 37 (measured on the CPU with the
# experiment of the module docstring, before any run of the kernel), against at most 2e-6 from 257 rows on
ORACLE_CASES = ([(name, rows, K) for name in list(SHAPES)[:4] for rows in ROWS for K in KS]
                + [("two_decoder_wide", rows, K) for rows in (257, 1000) for K in KS])


@pytest.mark.parametrize("name,rows,K", ORACLE_CASES)
def test_records_against_the_float64_oracle(name, rows, K):
    rec, ref = _records(name, rows, K), _oracle_rows(name, K)
    bad = []
    for r in range(R):
        per_row, eps = ref[r]
        if not _check(f"{name} rows {rows} K {K} replica {r}", rec[r], per_row[:rows].mean(axis=0), eps):
            bad.append(r)
        if K == 1:
            assert rec[r][0] == rec[r][1] or abs(rec[r][0] - rec[r][1]) <= 1e-6 * abs(rec[r][1])
            assert abs(rec[r][2] - 1.0) <= 1e-6
    assert not bad, bad
    assert np.all(rec[:, 4:] == SENT)


def _closed_form_model(D, L, rows, seed):
    """A one-decoder -tdv model (eps_cli = -1, epsilon = 0.8) whose decoder kernel [L, D] has orthogonal rows (min(L, D) scaled
    columns of an orthogonal matrix, zero rows behind them where L > D) and whose encoder is the exact posterior of that decoder;
    rows of data; the float64 mean log N(x; b_d, W_d^T W_d + e^eps I) on the float32-rounded decoder, eps and rows."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    Wd = np.zeros((L, D))
    k = min(L, D)
    Wd[:k] = (q[:, :k] * rng.uniform(0.5, 1.5, k)).T
    Wd = Wd.astype(np.float32).astype(np.float64)
    bd = (0.5 * rng.standard_normal(D)).astype(np.float32).astype(np.float64)
    epar = np.float32(0.8)
    eps = float(epar * np.float32(-1.0))
    lam = 1.0 + np.square(Wd).sum(1) * np.exp(-eps)
    We = Wd.T / lam * np.exp(-eps)                                         # [D, L]
    flat = np.concatenate([We.reshape(-1), -bd @ We, Wd.reshape(-1), bd, -np.log(lam), [epar]]).astype(np.float32)
    x = (bd + rng.standard_normal((rows, D))).astype(np.float32)
    C = Wd.T @ Wd + np.exp(eps) * np.eye(D)
    d = x.astype(np.float64) - bd
    logp = -0.5 * (np.einsum("id,id->i", d @ np.linalg.inv(C), d) + np.linalg.slogdet(C)[1] + D * np.log(2 * np.pi))
    return flat, x, float(logp.mean()), eps


@pytest.mark.parametrize("D,L", [(7, 6), (12, 20), (28, 24)])
def test_exact_posterior_gives_the_closed_form_log_likelihood(D, L):
    """Every weight equals p(x): slots 0 and 1 are the closed form and slot 2 is 1, for K = 1 and K = 64; slot 0 never exceeds it."""
    from vae_training_amd.engine import Engine
    rows = 257
    eng = Engine(100, D, L, (), (), -1.0, True, False)
    assert eng.supports_log_likelihood(0)
    flat, x, closed, eps = _closed_form_model(D, L, rows, seed=D * 100 + L)
    assert flat.size == eng.P
    params = torch.as_tensor(flat).cuda().reshape(1, -1)
    xs = torch.as_tensor(x).cuda().contiguous()
    ws = torch.empty(eng.log_likelihood_workspace(1, rows), dtype=torch.uint8, device="cuda")
    for K in (1, 64):
        out = torch.full((1, 4), SENT, dtype=torch.float32, device="cuda")
        eng.log_likelihood_replicas(params, rows, K, _i64([12345]), _i32([7]), out, ws, x=xs)
        torch.cuda.synchronize()
        got = out[0].cpu().numpy().astype(np.float64)
        print(f"D {D} L {L} K {K}: closed form {closed:.7f}, IWAE {got[0]:.7f} ELBO {got[1]:.7f} ESS {got[2]:.7f}; rel err "
              f"{abs(got[0] - closed) / abs(closed):.2e} {abs(got[1] - closed) / abs(closed):.2e}, |ESS - 1| {abs(got[2] - 1):.2e}")
        assert abs(got[0] - closed) <= RTOL * abs(closed) and abs(got[1] - closed) <= RTOL * abs(closed)
        assert abs(got[2] - 1.0) <= RTOL
        assert got[0] <= closed + RTOL * abs(closed)                       # Jensen: a lower bound on log p(x)
        assert abs(got[3] - eps) <= 1e-6


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_iwae_bound_is_not_below_the_elbo_estimate(name):
    """Jensen, per row and so for the means: logsumexp_k(lw) - log K >= mean_k lw."""
    for rows in (1, 257, 1000):
        for K in KS:
            rec = _records(name, rows, K)
            for r in range(R):
                assert rec[r][0] >= rec[r][1] - RTOL * abs(rec[r][1]), (rows, K, r, rec[r])
                assert 1.0 / K - 1e-6 <= rec[r][2] <= 1.0 + 1e-6, (rows, K, r, rec[r])


@pytest.mark.parametrize("name,rows,K", [("sigmoid", 1000, 64), ("linear_gaussian", 37, 5), ("sphere", 257, 2), ("two_decoder", 256, 1)])
def test_records_are_bitwise_reproducible(name, rows, K):
    """Two runs equal; drawing mode = explicit mode on vaek_make_batch's rows (where the dataset arguments are ignored); replica r of
    the n = 3 call = the n = 1 call on its slices, in both modes; shared rows (x_stride 0); floats between records, params and A
    untouched."""
    c = _case(name)
    before, a_before = c.params.clone(), None if c.A is None else c.A.clone()
    a, b = c.records(rows, K), c.records(rows, K)
    assert torch.equal(a, b)
    assert bool((a[:, 4:] == SENT).all()), "floats between two records were written"
    assert bool((a[:, :4] != SENT).all())
    xs = torch.stack([c.x_rows(r, rows) for r in range(R)]).contiguous()          # [R, rows, D]
    e = c.records(rows, K, x=xs, kind=9, A=None, dd=99, did=-4, pad=-1, x_seeds=None, x_steps=None, x_tag=2 ** 31, a_stride=-7)
    assert torch.equal(e, a), (e, a)
    for r in range(R):
        one = c.out(1)
        c.call(one, rows, K, rs=slice(r, r + 1))
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[r]), (r, one[0], a[r])
        one = c.out(1)
        c.call(one, rows, K, rs=slice(r, r + 1), x=xs[r].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[r]), (r, one[0], a[r])
    shared = c.records(rows, K, x=xs[0].contiguous())                            # [rows, D]: x_stride 0, every replica on replica 0's rows
    assert torch.equal(shared[0], a[0]) and not torch.equal(shared[1], a[1])
    assert torch.equal(c.params, before), "params were written"
    assert c.A is None or torch.equal(c.A, a_before), "A was written"


@pytest.mark.parametrize("name", list(OFF_SQUARE))
def test_drawn_rows_equal_make_batch_rows_off_the_square_matrix(name):
    """Drawing mode = explicit mode on vaek_make_batch's rows, bitwise as in test_records_are_bitwise_reproducible, where the in-launch
    draw leaves the line every other shape is on: dd = 5, did = 9, dataset noise, L % 4 = 1 and 3."""
    c = _case(name)
    rows, K = 257, 5
    a = c.records(rows, K)
    assert bool((a[:, :4] != SENT).all()) and bool(torch.isfinite(a[:, :4]).all())
    xs = torch.stack([c.x_rows(r, rows) for r in range(R)]).contiguous()
    assert not torch.equal(xs[0], xs[1]) and bool((xs[:, :, c.s["dd"]:] != 0).all())         # noise reaches the padding columns
    assert torch.equal(c.records(rows, K, x=xs), a)


def test_log_likelihood_is_capturable():
    """A captured call replayed twice = the eager call."""
    c = _case("sigmoid")
    eager = c.records(1000, 5)                           # eager (also the warm-up)
    out = c.out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.call(out, 1000, 5)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                     # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        out[:, :4] = 0.0


@pytest.mark.parametrize("name", ["sigmoid", "linear_gaussian"])
def test_sample_zero_is_make_batch_z1_and_the_batch_size_does_not_matter(name):
    """K = 1: the record equals the float64 evaluation on the z1 vaek_make_batch returns under the samples' (seed, step, tag); engines of
    batch 65 536 and of batch 5 (and one with force_generic) leave bitwise the record of the batch-100 engine."""
    from vae_training_amd.engine import Engine
    c = _case(name)
    s = c.s
    rows = 257
    rec = c.records(rows, 1)
    got = rec.cpu().numpy().astype(np.float64)
    for r in range(R):
        Ar = None if c.A is None else c.A[r].clone()
        _, z1, _ = c.eng.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, c.z_seeds[r], step=c.z_steps[r], tag=Z_TAG, want_x=False)
        x = c.x_rows(r, rows).cpu().numpy().astype(np.float64)
        per_row, eps = _rows64(s, c.trees[r], x, z1.cpu().numpy().astype(np.float64)[:, None, :])
        assert _check(f"{name} K 1 on make_batch's z1, replica {r}", got[r], per_row.mean(axis=0), eps)
    for batch, kw in ((65536, {}), (5, {}), (257, {}), (100, dict(force_generic=True))):
        eng = Engine(batch, s["D"], s["L"], (), (), s["eps"], s["tdv"], s["sig"], **kw)
        assert eng.supports_log_likelihood(s["kind"]), (batch, kw)
        assert torch.equal(c.records(rows, 1, eng=eng), rec), (batch, kw)
        assert torch.equal(c.records(rows, 64, eng=eng), c.records(rows, 64)), (batch, kw)


def test_arguments_predicate_and_profile_labels():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message and leaves the sentinel buffers unchanged; the
    predicate on engines the call does not cover; one profile record per launch."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c, lin, sph = _case("sigmoid"), _case("linear_gaussian"), _case("sphere")
    xs = torch.stack([c.x_rows(r, 37) for r in range(R)]).contiguous()

    def refused(why, e, **kw):
        out = e.out()
        before = e.params.clone()
        with pytest.raises(VaekError) as ei:
            e.call(out, kw.pop("rows", 37), kw.pop("K", 5), **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert "vaek_log_likelihood_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(e.params, before), why

    for why, eng, kind in [("mlp3", Engine(100, 6, 6, (200, 200, 200), (200, 200, 200), -1.0, False, False), 2),
                           ("one hidden layer", Engine(100, 7, 6, (64,), (64,), -1.0, True, True), 1),
                           ("bf16", Engine(100, 7, 6, (), (), -1.0, True, True, dtype="bf16"), 1)]:
        assert not eng.supports_log_likelihood(kind), why
        refused(why, sph if kind == 2 else c, eng=eng)
    assert Engine(100, 7, 6, (200, 200, 200), (200, 200, 200), -1.0, True, True).step_path != "linear"
    assert not Engine(100, 33, 6, (), (), -1.0, True, False).supports_log_likelihood(0)       # D > 32
    assert not Engine(100, 6, 33, (), (), -1.0, True, False).supports_log_likelihood(0)       # L > 32
    assert not Engine(100, 29, 6, (), (), -1.0, True, True).supports_log_likelihood(1)        # two decoders: D <= 28
    assert Engine(100, 32, 32, (), (), -1.0, True, False).supports_log_likelihood(0)
    assert Engine(100, 28, 32, (), (), -1.0, True, True).supports_log_likelihood(1)
    assert not c.eng.supports_log_likelihood(3) and not c.eng.supports_log_likelihood(-1)
    refused("struct_size", c, struct_size=12)
    refused("n = 0", c, n=0)
    refused("n over the cap", c, n=1025)
    refused("rows = 0", c, rows=0)
    refused("rows over the cap", c, rows=4097)
    refused("samples = 0", c, K=0)
    refused("samples over the cap", c, K=1025)
    for name in ("x_seeds", "x_steps", "z_seeds", "z_steps"):
        refused(name + " NULL", c, **{name: None})
    refused("z_seeds NULL, explicit rows", c, x=xs, z_seeds=None)
    with pytest.raises(VaekError) as ei:
        c.call(None, 37, 5, out_stride=c.os)
    assert ei.value.code == -1 and "out" in str(ei.value)
    refused("state_stride < P", c, state_stride=c.P - 1)
    refused("out_stride < record length", c, out_stride=3)
    refused("workspace NULL", c, workspace=None)
    refused("workspace misaligned", c, workspace=c.ws.data_ptr() + 4)
    refused("x_stride < 0", c, x=xs, x_stride=-1)
    refused("0 < x_stride < rows * D", c, x=xs, x_stride=37 * 7 - 1)
    refused("a_stride < 0", c, a_stride=-1)
    refused("A NULL, kind 1", c, A=None)
    refused("A NULL, kind 0", lin, A=None)
    refused("dd = 17", c, dd=17)
    refused("did = 17", lin, did=17)
    refused("kind 3", c, kind=3)
    refused("kind -1", c, kind=-1)
    refused("x_tag = 2^30", c, x_tag=2 ** 30)
    refused("z_tag = 2^30", c, z_tag=2 ** 30)
    refused("z_tag = 2^30, explicit rows", c, x=xs, z_tag=2 ** 30)
    refused("dataset dimension != data_dim", c, pad=4)
    from vae_training_amd import _lib
    b = _lib.C.c_size_t(7)
    for n, rows in ((0, 37), (1025, 37), (1, 0), (1, 4097)):
        assert c.eng.lib.vaek_log_likelihood_workspace_bytes(c.eng.h, n, rows, _lib.C.byref(b)) == -1 and b.value == 7
    # kind 2 needs no A; a shared A (a_stride 0) is legal; the caps themselves are legal; exactly one profile record per launch
    sph.call(sph.out(), 37, 5, A=None)
    c.call(c.out(), 4096, 1)
    c.call(c.out(), 1, 1024)
    c.eng.profile_begin(16)
    out = c.out()
    c.call(out, 37, 5, a_stride=0, A=c.A[0].clone())
    c.call(out, 1000, 2)
    torch.cuda.synchronize()
    rep = c.eng.profile_report()
    assert sorted(rep) == sorted(LABELS) and all(rep[k]["count"] == 2 for k in LABELS), rep
    assert c.eng.log_likelihood_max_rows == 4096 and c.eng.log_likelihood_max_samples == 1024


def _run_py(tmp_path, name, *extra, layers="", dataset="sigmoid"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", dataset, "--encoder_layer_sizes", layers, "--layer_sizes", layers,
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def _same(a, b):
    """Bitwise equality of two values as np.load / the checkpoint loader return them: arrays (object arrays element by element), dicts,
    lists, scalars."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == object:
        return all(_same(u, v) for u, v in zip(a.reshape(-1), b.reshape(-1)))
    return a.tobytes() == b.tobytes()


def _outputs(tmp_path, name):
    from vae_training_amd.model import load_checkpoint
    d = os.path.join(str(tmp_path), "data", name)
    return dict(np.load(os.path.join(d, "losses.npz"), allow_pickle=True)), load_checkpoint(os.path.join(d, "model.pkl"))


NEW_KEYS = ("Average Log Likelihood", "ELBO estimate", "Effective Sample Size")


def _check_pair(plain, flagged, ckpt_plain, ckpt_flagged, who):
    """The run with the flag against the run without: every stat of the plain run and the checkpoint bitwise equal; the three new
    entries, one per n_print event (30 batches: the event of step 0)."""
    assert sorted(k for k in flagged if k not in NEW_KEYS[1:]) == sorted(plain), (who, list(plain), list(flagged))
    for k in plain:
        if k != NEW_KEYS[0]:
            assert _same(plain[k], flagged[k]), (who, k, plain[k], flagged[k])
    assert np.asarray(plain["VAE Loss"]).size == 31
    assert _same(ckpt_plain, ckpt_flagged), who
    assert np.asarray(plain[NEW_KEYS[0]]).size == 0
    vals = [np.asarray(flagged[k], dtype=np.float64).reshape(-1) for k in NEW_KEYS]
    print(who, {k: v.tolist() for k, v in zip(NEW_KEYS, vals)})
    assert all(v.size == 1 and np.isfinite(v).all() for v in vals), (who, vals)
    assert vals[0][0] >= vals[1][0] - RTOL * abs(vals[1][0]) and 1.0 / 8 - 1e-6 <= vals[2][0] <= 1.0 + 1e-6, (who, vals)


@pytest.mark.parametrize("fused", [(), ("--fused_stats",)], ids=["compute_stats", "fused_stats"])
def test_run_py_sweep_with_and_without_the_flag(tmp_path, fused):
    """Line 1 of sigmoid_vae_padding_expts.sh, 30 batches, --sweep_dataset_seeds 69,24, with and without --log_likelihood_samples 8
    (the stats events through compute_stats() and through --fused_stats): the evaluation does not perturb the run."""
    runs = {}
    for name, extra in (("plain", ()), ("ll", ("--log_likelihood_samples", "8"))):
        r = _run_py(tmp_path, name, "--sweep_dataset_seeds", "69,24", *fused, *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("Log-likelihood events: 8 samples × 1000 rows (vaek_log_likelihood_replicas)" in r.stdout) == (name == "ll"), r.stdout[-1500:]
        runs[name] = {seed: _outputs(tmp_path, f"{name}_ds{seed}") for seed in (69, 24)}
    for seed in (69, 24):
        _check_pair(*runs["plain"][seed][:1], *runs["ll"][seed][:1], runs["plain"][seed][1], runs["ll"][seed][1], f"seed {seed}")
    assert not _same(runs["ll"][69][0][NEW_KEYS[0]], runs["ll"][24][0][NEW_KEYS[0]])


def test_run_py_single_model_and_the_refusal(tmp_path):
    """The single-model form (the helper of model.py), against the same run without the flag; and a 200|200|200 line (line 1 of
    sphere_vae_padding_expts.sh, step path "mlp3") is refused before any step, alone and as a sweep, with a message that names the
    step path."""
    outs = {}
    for name, extra in (("plain1", ()), ("ll1", ("--log_likelihood_samples", "8"))):
        r = _run_py(tmp_path, name, *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("Log-likelihood events: 8 samples × 1000 rows (vaek_log_likelihood_replicas)" in r.stdout) == (name == "ll1"), r.stdout[-1500:]
        assert ("Average Log Likelihood |" in r.stdout) == (name == "ll1")
        outs[name] = _outputs(tmp_path, name)
    _check_pair(outs["plain1"][0], outs["ll1"][0], outs["plain1"][1], outs["ll1"][1], "single model")
    for extra in ((), ("--sweep_dataset_seeds", "69,24")):
        r = _run_py(tmp_path, "m3", "--log_likelihood_samples", "8", *extra, layers="200|200|200", dataset="sphere")
        assert r.returncode != 0 and "--log_likelihood_samples needs" in r.stderr and "step path: mlp3" in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
        assert "Batch |" not in r.stdout
