"""-m gpu: vaek_exact_log_likelihood_replicas -- the exact log-likelihood, the exact ELBO and the posterior gap of N one-decoder linear
VAEs in one launch (csrc/cov_spectrum.hip) -- and its callers, trainer.ReplicaExactLogLik and `run.py --exact_log_likelihood`.

References (cases and bounds: tests/exact_loglik_cases.py):
  - the float64 restatement tools/exact_log_likelihood_reference.py on the identical rows and parameters (itself held to a 60-digit
    evaluation by tests/test_exact_log_likelihood_host.py): record slots 0 .. 2 and row_out within the bounds computed from the
    device's own off_F and |G|_F (slots 6, 7), the means within the mean of the per-row bounds, logdet within D * slot 8 + 64 D 2^-53
    |logdet|, the eigenvalues against LAPACK within off_F + 64 D 2^-53 |G|_F;
  - itself, BITWISE: replica r of n = 3 against n = 1, two runs, a captured replay, drawing mode against explicit rows, engines of
    other batch sizes, row_out = NULL;
  - vaek_log_likelihood_replicas at K = 1024 on the same rows: its ELBO estimate is the exact ELBO within the Monte-Carlo error, its
    IWAE bound does not exceed the exact log-likelihood."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import exact_loglik_cases as K
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
R = 3
X_TAG = 3
PAD_OUT, PAD_ROW = 3, 5                     # sentinel doubles behind a record and behind a row block
DRAW = {(12, 20): dict(kind=0, dd=3, did=3, pad=9, var=0.01), (7, 7): dict(kind=2, dd=4, did=4, pad=3, var=0.0),
        # a mixing matrix that is not square, did > 4 with noise (noise normals from Philox block 3), L % 4 = 1 and 3
        (8, 5): dict(kind=0, dd=5, did=9, pad=3, var=0.25), (8, 7): dict(kind=0, dd=5, did=9, pad=3, var=0.25)}


@functools.lru_cache(maxsize=None)
def _ref():
    spec = importlib.util.spec_from_file_location("exact_log_likelihood_reference", os.path.join(ROOT, "tools", "exact_log_likelihood_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _last(t):
    return t.shape[-1] if torch.is_tensor(t) else None


class _Case:
    """One engine and R replicas of one (D, L, eps_cli) with distinct parameters and rows, in a parameter stack whose stride exceeds P
    by 5 sentinel floats; records go to a sentinel-filled [R, 10 + D + PAD_OUT] buffer, rows to [R, 2 rows + PAD_ROW]."""

    def __init__(self, D, L, eps_cli, batch=100, **ekw):
        from vae_training_amd.engine import Engine
        self.D, self.L, self.eps_cli = D, L, eps_cli
        models = [K.make_model(D, L, eps_cli, seed=r) for r in range(R)]
        self.tdv = models[0][1]
        self.trees, self.eps = [m[0] for m in models], [m[3] for m in models]
        self.cfg = cfg = O.Config(D, L, (), (), eps_cli, self.tdv, None)
        self.eng = e = Engine(batch, D, L, (), (), eps_cli, self.tdv, False, **ekw)
        self.len = 10 + D
        assert e.exact_log_likelihood_record_len == self.len
        self.P, self.ss, self.os = e.P, e.P + 5, self.len + PAD_OUT
        self.params = torch.full((R, self.ss), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :e.P] = torch.as_tensor(np.stack([O.flatten(cfg, t, np.float32) for t in self.trees])).cuda()
        self.x64 = [K.make_rows(self.trees[r], self.eps[r], K.MAX_ROWS, seed=r) for r in range(R)]
        self.x = torch.as_tensor(np.stack(self.x64), dtype=torch.float32).cuda().contiguous()          # [R, MAX_ROWS, D]
        d = DRAW.get((D, L))
        self.draw = d
        if d is not None:
            assert e.supports_exact_log_likelihood(d["kind"])
            alen = {0: d["dd"] * d["did"], 2: 0}[d["kind"]]
            rng = np.random.default_rng(23)
            self.A = torch.as_tensor(rng.standard_normal((R, alen)), dtype=torch.float32).cuda().contiguous() if alen else None
            self.a_stride = alen
            self.x_seeds, self.x_steps = [77, 2 ** 63 + 5, 1000003], [1, 4, 2 ** 31 + 7]
            self.tabs = (_i64(self.x_seeds), _i32(self.x_steps))

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float64, device="cuda")

    def row_out(self, rows, n=R):
        return torch.full((n, 2 * rows + PAD_ROW), SENT, dtype=torch.float64, device="cuda")

    def call(self, out, rows, rs=None, row_out=None, **kw):
        """Explicit mode on the first `rows` rows of replicas `rs` (default: all R); kw overrides any argument."""
        sl = slice(None) if rs is None else rs
        x = self.x[sl, :rows].contiguous()
        a = dict(params=self.params[sl], rows=rows, out=out, x=x, row_out=row_out, row_stride=_last(row_out))
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.exact_log_likelihood_replicas(**a)

    def call_draw(self, out, rows, rs=None, row_out=None, **kw):
        d = self.draw
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, out=out, kind=d["kind"], A=None if self.A is None else self.A[sl], dd=d["dd"],
                 did=d["did"], pad=d["pad"], var_added=d["var"], x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl],
                 a_stride=self.a_stride, x_tag=X_TAG, row_out=row_out, row_stride=_last(row_out))
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.exact_log_likelihood_replicas(**a)

    def records(self, rows, **kw):
        out, ro = self.out(), self.row_out(rows)
        self.call(out, rows, row_out=ro, **kw)
        torch.cuda.synchronize()
        return out, ro

    def drawn_rows(self, r, rows):
        d = self.draw
        Ar = None if self.A is None else self.A[r].clone()
        return self.eng.make_batch(d["kind"], Ar, d["dd"], d["did"], d["pad"], d["var"], rows, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG,
                                   want_z=False)[0]


@functools.lru_cache(maxsize=None)
def _case(D, L, eps_cli):
    return _Case(D, L, eps_cli)


@functools.lru_cache(maxsize=None)
def _restated(D, L, eps_cli):
    """Per replica the restatement's evaluation of all MAX_ROWS rows (a row's values do not depend on the row count); computed once."""
    c = _case(D, L, eps_cli)
    return [_ref().evaluate(c.trees[r], c.eps[r], c.x64[r]) for r in range(R)]


CASES = [(name, D, L, e, rows) for (name, D, L, e) in K.all_cases() for rows in K.ROWS]


@pytest.mark.parametrize("name,D,L,eps_cli,rows", CASES, ids=[f"{c[0]}_rows{c[4]}" for c in CASES])
def test_records_and_rows_against_the_restatement(name, D, L, eps_cli, rows):
    c = _case(D, L, eps_cli)
    before = c.params.clone()
    out, ro = c.records(rows)
    rec, per = out.cpu().numpy(), ro.cpu().numpy()
    assert np.all(rec[:, c.len:] == SENT) and np.all(per[:, 2 * rows:] == SENT), "doubles between two records or row blocks were written"
    assert torch.equal(c.params, before)
    bad = []
    for r in range(R):
        ref, g = _restated(D, L, eps_cli)[r], rec[r]
        eps = c.eps[r]
        off, norm = g[6], g[7]
        assert g[3] == eps and g[9] == rows and 0 <= g[5] < 32 and g[5] == int(g[5]), g[:10]
        assert off <= 2.0 ** -43 * norm and np.isfinite(g).all()
        assert abs(norm - ref["norm"]) <= 64 * L * K.U * ref["norm"]             # the chains' order differs from NumPy's
        cond = K.conditioning(D, off, norm, eps)
        assert abs(g[8] - cond) <= 1e-12 * cond
        quad, M = ref["quad"][:rows], ref["M"][:rows]
        b1 = K.logp_bound(D, quad, ref["logdet"], off, norm, eps)
        b2 = K.elbo_bound(M)
        lp, el = per[r, 0:2 * rows:2], per[r, 1:2 * rows:2]
        e_lp, e_el = np.abs(lp - ref["logp"][:rows]), np.abs(el - ref["elbo"][:rows])
        m_err = [abs(g[0] - ref["logp"][:rows].mean()), abs(g[1] - ref["elbo"][:rows].mean()), abs(g[2] - ref["gap"][:rows].mean())]
        m_bnd = [b1.mean(), b2.mean(), (b1 + b2).mean()]
        e_ld, b_ld = abs(g[4] - ref["logdet"]), D * g[8] + 64.0 * D * K.U * abs(ref["logdet"])
        kd = c.trees[r][K.KD]
        e_eig, b_eig = np.max(np.abs(g[10:10 + D] - np.linalg.eigvalsh(kd.T @ kd))), K.eig_bound(D, off, norm)
        print(f"{name} rows {rows} replica {r}: sweeps {int(g[5])} conditioning {g[8]:.2e}; rows |d log p| {e_lp.max():.2e} = "
              f"{np.max(e_lp / b1):.4f}, |d ELBO| {e_el.max():.2e} = {np.max(e_el / b2):.4f}; means {m_err[0] / m_bnd[0]:.4f} {m_err[1] / m_bnd[1]:.4f} "
              f"{m_err[2] / m_bnd[2]:.4f}; logdet {e_ld / b_ld:.4f}; eigenvalues {e_eig / b_eig:.4f} (units of the bounds)")
        ok = (np.all(e_lp <= b1) and np.all(e_el <= b2) and all(e <= b for e, b in zip(m_err, m_bnd)) and e_ld <= b_ld and e_eig <= b_eig
              and np.all(np.diff(g[10:10 + D]) >= 0) and np.all(lp - el >= -(b1 + b2)) and g[1] <= g[0] + m_bnd[2])
        if not ok:
            bad.append(r)
    assert not bad, bad


def test_the_ill_conditioned_case_is_reported_not_hidden():
    """eps = -30: only that slot 8 says so and that the record is finite."""
    (name, D, L, e), = K.all_cases(ill=True)
    c = _case(D, L, e)
    out, ro = c.records(257)
    rec = out.cpu().numpy()
    print(name, "conditioning", rec[:, 8], "log p", rec[:, 0], "ELBO", rec[:, 1])
    assert np.all(rec[:, 8] > 1e-3)
    assert np.isfinite(rec[:, :c.len]).all() and np.isfinite(ro.cpu().numpy()[:, :2 * 257]).all()


@pytest.mark.parametrize("D,L,rows", [(12, 20, 257), (7, 7, 1000)], ids=["kind0_D12_L20", "kind2_D7_L7"])
def test_records_are_bitwise_reproducible(D, L, rows):
    """Two runs; replica r of n = 3 against n = 1 on its slices; drawing mode against explicit mode on vaek_make_batch's rows (where
    the dataset arguments are ignored); row_out = NULL; shared rows; engines of batch 5 and 65 536; params and A untouched."""
    from vae_training_amd.engine import Engine
    c = _case(D, L, -8.0)
    before, a_before = c.params.clone(), None if c.A is None else c.A.clone()
    (a, ra), (b, rb) = c.records(rows), c.records(rows)
    assert torch.equal(a, b) and torch.equal(ra, rb)
    none = c.out()
    c.call(none, rows)
    torch.cuda.synchronize()
    assert torch.equal(none, a), "row_out = NULL changed the record"
    for r in range(R):
        one, ro = c.out(1), c.row_out(rows, 1)
        c.call(one, rows, rs=slice(r, r + 1), row_out=ro)
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[r]) and torch.equal(ro[0], ra[r]), r
    shared = c.out()
    c.call(shared, rows, x=c.x[0, :rows].contiguous())                     # [rows, D]: x_stride 0, every replica on replica 0's rows
    torch.cuda.synchronize()
    assert torch.equal(shared[0], a[0]) and not torch.equal(shared[1], a[1])
    # drawing mode
    d, rd = c.out(), c.row_out(rows)
    c.call_draw(d, rows, row_out=rd)
    torch.cuda.synchronize()
    assert bool((d[:, c.len:] == SENT).all()) and bool((rd[:, 2 * rows:] == SENT).all()) and bool((d[:, :c.len] != SENT).all())
    xs = torch.stack([c.drawn_rows(r, rows) for r in range(R)]).contiguous()
    e, re_ = c.out(), c.row_out(rows)
    c.call(e, rows, x=xs, row_out=re_, kind=9, A=None, dd=99, did=-4, pad=-1, x_seeds=None, x_steps=None, x_tag=2 ** 31, a_stride=-7)
    torch.cuda.synchronize()
    assert torch.equal(e, d) and torch.equal(re_, rd)
    for r in range(R):
        one = c.out(1)
        c.call_draw(one, rows, rs=slice(r, r + 1))
        torch.cuda.synchronize()
        assert torch.equal(one[0], d[r]), r
    for batch in (5, 65536):
        eng = Engine(batch, D, L, (), (), c.eps_cli, c.tdv, False)
        assert eng.supports_exact_log_likelihood(c.draw["kind"])
        o2 = c.out()
        c.call_draw(o2, rows, eng=eng)
        o3 = c.out()
        c.call(o3, rows, eng=eng)
        torch.cuda.synchronize()
        assert torch.equal(o2, d) and torch.equal(o3, a), batch
    assert torch.equal(c.params, before), "params were written"
    assert c.A is None or torch.equal(c.A, a_before), "A was written"


@pytest.mark.parametrize("D,L", [(8, 5), (8, 7)], ids=["did9_L5", "did9_L7"])
def test_drawn_rows_equal_make_batch_rows_off_the_square_matrix(D, L):
    """Drawing mode = explicit mode on vaek_make_batch's rows, bitwise as in test_records_are_bitwise_reproducible, at dd = 5,
    did = 9 with dataset noise."""
    c = _case(D, L, -8.0)
    rows = 257
    d, rd = c.out(), c.row_out(rows)
    c.call_draw(d, rows, row_out=rd)
    torch.cuda.synchronize()
    assert bool((d[:, :c.len] != SENT).all()) and bool(torch.isfinite(d[:, :c.len]).all())
    xs = torch.stack([c.drawn_rows(r, rows) for r in range(R)]).contiguous()
    assert not torch.equal(xs[0], xs[1]) and bool((xs[:, :, c.draw["dd"]:] != 0).all())      # noise reaches the padding columns
    e, re_ = c.out(), c.row_out(rows)
    c.call(e, rows, x=xs, row_out=re_)
    torch.cuda.synchronize()
    assert torch.equal(e, d) and torch.equal(re_, rd)


def test_exact_log_likelihood_is_capturable():
    """A captured call replayed twice = the eager call."""
    c = _case(12, 20, -8.0)
    rows = 1000
    eager, eager_rows = c.out(), c.row_out(rows)
    c.call_draw(eager, rows, row_out=eager_rows)                          # eager (also the warm-up)
    torch.cuda.synchronize()
    out, ro = c.out(), c.row_out(rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.call_draw(out, rows, row_out=ro)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                      # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(ro, eager_rows)
        out[:, :c.len] = 0.0


def test_against_the_importance_weighted_estimator():
    """(12, 20), eps_cli = -0.8, 1000 explicit rows, vaek_log_likelihood_replicas at K = 1024 on the same rows: its ELBO estimate is the
    exact ELBO within 6 s / sqrt(rows K) + 1e-5 |value|, its IWAE bound is at most the exact log-likelihood plus that; s is the
    standard deviation of log w (the root of the mean over rows of its variance over the samples) from a float64 evaluation with
    NumPy draws, 1000 rows x 64 samples.  All seeds are fixed."""
    c = _case(12, 20, -0.8)
    rows, samples = 1000, 1024
    rec = c.records(rows)[0].cpu().numpy()
    ll = torch.zeros(R, 4, dtype=torch.float32, device="cuda")
    ws = torch.empty(c.eng.log_likelihood_workspace(R, rows), dtype=torch.uint8, device="cuda")
    c.eng.log_likelihood_replicas(c.params, rows, samples, _i64([11, 12, 13]), _i32([1, 2, 3]), ll, ws, x=c.x[:, :rows].contiguous())
    torch.cuda.synchronize()
    est = ll.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(5)
    for r in range(R):
        p, eps, x = c.trees[r], c.eps[r], c.x64[r][:rows]
        xi = rng.standard_normal((rows, 64, c.L))
        mu = x @ p[K.KE] + p[K.BE]
        z = mu[:, None, :] + np.exp(p[K.LV] / 2) * xi
        rsq = np.square(z @ p[K.KD] + p[K.BD] - x[:, None, :]).sum(-1)
        lw = -0.5 * (rsq * np.exp(-eps) + c.D * (eps + np.log(2 * np.pi))) + 0.5 * (np.square(xi) - np.square(z) + p[K.LV]).sum(-1)
        s = float(np.sqrt(np.mean(np.var(lw, axis=1, ddof=1))))
        tol = 6.0 * s / np.sqrt(rows * samples)
        print(f"replica {r}: exact log p {rec[r, 0]:.6f}, exact ELBO {rec[r, 1]:.6f}, gap {rec[r, 2]:.6f}; IWAE-1024 {est[r, 0]:.6f}, ELBO estimate "
              f"{est[r, 1]:.6f} (|d| {abs(est[r, 1] - rec[r, 1]):.2e}, Monte-Carlo tolerance {tol:.2e}, s {s:.3f}); float64 host mean log w {lw.mean():.6f}")
        assert abs(est[r, 1] - rec[r, 1]) <= tol + 1e-5 * abs(rec[r, 1])
        assert est[r, 0] <= rec[r, 0] + tol + 1e-5 * abs(rec[r, 0])
        assert rec[r, 1] <= rec[r, 0] and abs(est[r, 3] - rec[r, 3]) <= 1e-6


def test_arguments_predicate_and_profile_label():
    """Every invalid case of include/vaek.h returns VAEK_ERR_INVALID with a message that names the function and leaves `out` alone; the
    predicate on engines the call does not cover; one profile record per call."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c, sph = _case(12, 20, -8.0), _case(7, 7, -8.0)
    rows = 37

    def refused(why, e, draw=True, **kw):
        out = kw.pop("out", None)
        out = e.out() if out is None else out
        before = e.params.clone()
        with pytest.raises(VaekError) as ei:
            (e.call_draw if draw else e.call)(kw.pop("out_arg", out), kw.pop("rows", rows), **kw)
        assert ei.value.code == -1, (why, ei.value)                     # VAEK_ERR_INVALID
        assert "vaek_exact_log_likelihood_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(e.params, before), why

    two = Engine(100, 7, 6, (), (), -1.0, True, True)                      # a two-decoder (sigmoid) context
    assert two.supports_log_likelihood(1) and not two.supports_exact_log_likelihood(1)
    for why, eng in [("two decoders", two), ("mlp3", Engine(100, 7, 7, (200, 200, 200), (200, 200, 200), -1.0, False, False)),
                     ("one hidden layer", Engine(100, 7, 7, (64,), (64,), -1.0, False, False)),
                     ("bf16", Engine(100, 7, 7, (), (), -1.0, False, False, dtype="bf16"))]:
        assert not eng.supports_exact_log_likelihood(2), why
        refused(why, sph, eng=eng)
    assert not Engine(100, 33, 6, (), (), -1.0, True, False).supports_exact_log_likelihood(0)      # D > 32
    assert not Engine(100, 6, 33, (), (), -1.0, True, False).supports_exact_log_likelihood(0)      # L > 32
    assert Engine(100, 32, 32, (), (), -1.0, True, False).supports_exact_log_likelihood(0)
    assert not c.eng.supports_exact_log_likelihood(3) and not c.eng.supports_exact_log_likelihood(-1)
    refused("struct_size", c, struct_size=12)
    refused("n = 0", c, n=0)
    refused("n over the cap", c, n=1025)
    refused("rows = 0", c, rows=0)
    refused("rows over the cap", c, rows=4097)
    refused("x_seeds NULL", c, x_seeds=None)
    refused("x_steps NULL", c, x_steps=None)
    with pytest.raises(VaekError) as ei:
        c.call_draw(None, rows, out_stride=c.os)
    assert ei.value.code == -1 and "out" in str(ei.value)
    refused("state_stride < P", c, state_stride=c.P - 1)
    refused("out_stride < record length", c, out_stride=c.len - 1)
    o = c.out()
    refused("out misaligned", c, out=o, out_arg=o.data_ptr() + 4, out_stride=c.os)
    ro = c.row_out(rows)
    refused("row_out misaligned", c, row_out=ro.data_ptr() + 4, row_stride=2 * rows)
    refused("0 < row_stride < 2 rows", c, row_out=ro, row_stride=2 * rows - 1)
    refused("row_stride 0 with three replicas", c, row_out=ro, row_stride=0)
    refused("row_stride < 0", c, row_out=ro, row_stride=-1)
    assert bool((ro == SENT).all())
    refused("x_stride < 0", c, draw=False, x_stride=-1)
    refused("0 < x_stride < rows * D", c, draw=False, x_stride=rows * c.D - 1)
    refused("a_stride < 0", c, a_stride=-1)
    refused("A NULL, kind 0", c, A=None)
    refused("dd = 17", c, dd=17)
    refused("did = 17", c, did=17)
    refused("kind 3", c, kind=3)
    refused("kind -1", c, kind=-1)
    refused("x_tag = 2^30", c, x_tag=2 ** 30)
    refused("dataset dimension != data_dim", c, pad=4)
    # kind 2 needs no A; a shared A (a_stride 0) is legal; the caps are legal; row_stride 0 with one replica; one profile record per call
    sph.call_draw(sph.out(), rows, A=None)
    c.call_draw(c.out(), 4096)
    one = c.row_out(rows, 1)
    c.call_draw(c.out(1), rows, rs=slice(0, 1), row_out=one, row_stride=0)
    c.eng.profile_begin(16)
    out = c.out()
    c.call_draw(out, rows, a_stride=0, A=c.A[0].clone())
    c.call(out, 1000)
    torch.cuda.synchronize()
    rep = c.eng.profile_report()
    assert list(rep) == ["exact_loglik_replicas"] and rep["exact_loglik_replicas"]["count"] == 2, rep


def _cli_model(tmp_path, seed):
    from vae_training_amd.run import get_dataset, parse_arguments
    from vae_training_amd.vae import VAEModel
    args = parse_arguments([f"m{seed}", "--dataset", "linear_gaussian", "--padding_dim", "9", "-dd", "3", "-ds", str(seed)])
    ds = get_dataset("linear_gaussian", seed, 9, 100, args)
    d = tmp_path / f"m{seed}"
    d.mkdir()
    return VAEModel(dirname=str(d), num_batches=10, num_epochs=1, batch_size=100, learning_rate=1e-3, layer_sizes="",
                    encoder_layer_sizes="", state_dict=None, data_fn=None, epsilon=-1.0, tqdm=False, dataset=ds,
                    latent_dimension=20, tunable_decoder_var=True, dataset_name="linear_gaussian")


def test_replica_exact_loglik_on_three_models(tmp_path):
    """trainer.ReplicaExactLogLik on three linear_gaussian models (dataset seeds 69, 24, 48): its stats are the record slots of a direct
    call on vaek_make_batch's rows under (dataset.key[0] ^ dataset.key[1], the counter, tag 3), bitwise; the run's RNG state is left
    alone; with a ReplicaLogLik event before it both score the same rows and the gap to the IWAE bound is not negative."""
    from vae_training_amd.trainer import ReplicaExactLogLik, ReplicaLogLik
    ms = [_cli_model(tmp_path, s) for s in (69, 24, 48)]
    state = [(m.key, getattr(m.dataset, "_draws", 0), getattr(m, "_latent_draws", 0)) for m in ms]
    ex = ReplicaExactLogLik(ms, rows=257)
    for event in (1, 2):
        stats = ex.event()
        for r, m in enumerate(ms):
            kind, A, dd, did, pad, var = m.dataset.device_spec()
            seed = m.dataset.key[0] ^ m.dataset.key[1]
            x = ex.eng.make_batch(kind, A, dd, did, pad, var, 257, seed, step=event, tag=3, want_z=False)[0]
            out = torch.zeros(1, ex.record_len, dtype=torch.float64, device="cuda")
            ex.eng.exact_log_likelihood_replicas(m.model.flat.reshape(1, -1), 257, out, x=x.contiguous())
            rec = out.cpu().numpy()[0]
            assert [stats[r][k] for k in ex.KEYS] == [rec[0], rec[1], rec[2], rec[8]], (event, r)
            assert stats[r]["Posterior KL"] >= 0.0 and stats[r]["Exact ELBO"] <= stats[r]["Exact Log Likelihood"]
            assert m._exact_loglik_draws == event
    assert [(m.key, getattr(m.dataset, "_draws", 0), getattr(m, "_latent_draws", 0)) for m in ms] == state
    ll = ReplicaLogLik(ms, 64, rows=257)
    iw = ll.event()
    both = ex.event_after(iw)
    again = ex.event(step=[m._loglik_draws for m in ms])
    for r in range(3):
        assert {k: both[r][k] for k in ex.KEYS} == again[r]
        gap = both[r]["IWAE Gap"]
        print(f"model {r}: exact {both[r]['Exact Log Likelihood']:.6f}, IWAE-64 {float(iw[r]['Average Log Likelihood']):.6f}, gap {gap:.3e}, "
              f"posterior KL {both[r]['Posterior KL']:.6f}")
        assert gap == both[r]["Exact Log Likelihood"] - float(iw[r]["Average Log Likelihood"])
        assert -1e-5 * abs(both[r]["Exact Log Likelihood"]) <= gap <= both[r]["Posterior KL"] + 1e-5 * abs(both[r]["Exact ELBO"])
    assert all(m._exact_loglik_draws == 2 for m in ms)


def _run_py(tmp_path, name, *extra, dataset="linear_gaussian"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", dataset, "--encoder_layer_sizes", "", "--layer_sizes", "",
           "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def _same(a, b):
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


NEW_KEYS = ("Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning", "IWAE Gap")


def test_run_py_sweep_with_and_without_the_flag_and_the_refusal(tmp_path):
    """A linear_gaussian line, 30 batches, --log_likelihood_samples 64 --sweep_dataset_seeds 69,24, with and without
    --exact_log_likelihood: the new keys and IWAE Gap are in losses.npz, every other stat and model.pkl are bitwise the run without the
    flag.  A sigmoid (two-decoder) model is refused before any step, with the step path in the message."""
    runs = {}
    for name, extra in (("plain", ()), ("exact", ("--exact_log_likelihood",))):
        r = _run_py(tmp_path, name, "--sweep_dataset_seeds", "69,24", "--log_likelihood_samples", "64", *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("(vaek_exact_log_likelihood_replicas)" in r.stdout) == (name == "exact"), r.stdout[-1500:]
        assert ("Exact Log Likelihood |" in r.stdout) == (name == "exact")
        runs[name] = {seed: _outputs(tmp_path, f"{name}_ds{seed}") for seed in (69, 24)}
    for seed in (69, 24):
        (plain, ck_plain), (exact, ck_exact) = runs["plain"][seed], runs["exact"][seed]
        assert sorted(k for k in exact if k not in NEW_KEYS) == sorted(plain), (list(plain), list(exact))
        assert not any(k in plain for k in NEW_KEYS)
        for k in plain:
            assert _same(plain[k], exact[k]), (seed, k, plain[k], exact[k])
        assert np.asarray(plain["VAE Loss"]).size == 31 and _same(ck_plain, ck_exact), seed
        vals = {k: np.asarray(exact[k], dtype=np.float64).reshape(-1) for k in NEW_KEYS}
        print(seed, {k: v.tolist() for k, v in vals.items()})
        assert all(v.size == 1 and np.isfinite(v).all() for v in vals.values()), vals
        iwae = float(np.asarray(exact["Average Log Likelihood"], dtype=np.float64).reshape(-1)[0])
        assert vals["IWAE Gap"][0] == vals["Exact Log Likelihood"][0] - iwae
        assert vals["Posterior KL"][0] >= 0.0 and vals["Exact ELBO"][0] <= vals["Exact Log Likelihood"][0]
        assert vals["IWAE Gap"][0] >= -1e-5 * abs(vals["Exact Log Likelihood"][0])
    assert not _same(runs["exact"][69][0][NEW_KEYS[0]], runs["exact"][24][0][NEW_KEYS[0]])
    for extra in ((), ("--sweep_dataset_seeds", "69,24")):
        r = _run_py(tmp_path, "sig", "--exact_log_likelihood", *extra, dataset="sigmoid")
        assert r.returncode != 0 and "--exact_log_likelihood needs" in r.stderr and "step path: " in r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
        assert "Batch |" not in r.stdout
