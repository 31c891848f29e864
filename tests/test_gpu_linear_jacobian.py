"""-m gpu: vaek_linear_decoder_jacobian_replicas -- the spectra of the decoder Jacobian J(z) = K_d^T + diag(sigmoid'(z K_s + b_s)) K_s^T of N
linear VAEs of one shape, one or two decoders, in one call (csrc/linear_jacobian.hip) -- and its callers, trainer.ReplicaJacobianLinear and
`run.py --linear_decoder_jacobian`.

The records are those of vaek_mlp3_decoder_jacobian_replicas (tests/test_gpu_decoder_jacobian.py).  References:
  - the float64 NumPy reference of tests/linear_jacobian_cases.py on the cases' explicit latents, every row through row_out:
    |lambda_k - ref| and |diag G - ref| <= (2^-43 + GRAM_FACTOR x worst + 64 L 2^-53) |G_ref|_F, |G|_F within GRAM_FACTOR x worst
    relative, the rank exactly; the model record's means within the same bound with the mean |G_ref|_F, its counts exact;
  - a merged kernel: with one decoder the min(D, L) largest lambda of every row against the largest eigenvalues of K^T K in the
    record of vaek_exact_log_likelihood_replicas, within (2 x 2^-43 + 64 x 32 x 2^-53) |G|_F, all rows of a replica bitwise equal;
  - itself, BITWISE: a two-decoder context with K_s = 0, b_s = +800 or b_s = -800 against the one-decoder context with the same K_d;
    drawing mode against explicit mode on the z1 vaek_make_batch writes, replica r of n = 3 against n = 1 on its slices, two runs, a
    captured call, engines of two batch sizes, two parameter strides (one not a multiple of 4), a row of a 37-row call against the
    same latent in a 2-row call, row_out given or NULL, sentinels between the records;
  - planted rank (rows l >= k of K_d and K_s zero: rank k on every row, diag G[l >= k] exactly 0) and a dead decoder.
HOW WELL THE REFERENCE IS DEFINED (tools/linear_jacobian_reference.py, on the CPU, before any run of the kernel; TABLE below): per case
`worst`, the worst |G_64 - G_longdouble|_F / |G|_F over rows and replicas.  tests/test_linear_jacobian_inputs.py recomputes the table
without a GPU and checks every case's rank threshold.
OBSERVED on one MI355X: the comment below the table.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import linear_jacobian_cases as LC
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
LABELS = ["linear_jacobian_rows", "linear_jacobian_finalize"]
R = LC.R
# LINEAR_JACOBIAN_TABLE_BEGIN (written by tools/linear_jacobian_reference.py: per case the worst |G_64 - G_longdouble|_F / |G|_F)
TABLE = {
    ('sig_script1', 1): 1.191e-16,
    ('sig_script1', 2): 1.800e-16,
    ('sig_script1', 37): 2.962e-16,
    ('sig_script1', 257): 2.962e-16,
    ('sig_script6', 1): 2.586e-16,
    ('sig_script6', 2): 2.841e-16,
    ('sig_script6', 37): 3.309e-16,
    ('sig_null', 1): 3.396e-16,
    ('sig_null', 2): 3.674e-16,
    ('sig_null', 37): 7.044e-16,
    ('sig_one_latent', 1): 4.092e-17,
    ('sig_one_latent', 2): 1.312e-16,
    ('sig_one_latent', 37): 4.554e-16,
    ('sig_odd', 1): 1.951e-16,
    ('sig_odd', 2): 2.306e-16,
    ('sig_odd', 37): 3.434e-16,
    ('lin_odd', 1): 7.547e-17,
    ('lin_odd', 2): 7.547e-17,
    ('lin_odd', 37): 7.547e-17,
    ('lin_wide', 1): 1.343e-16,
    ('lin_wide', 2): 1.343e-16,
    ('lin_wide', 37): 1.343e-16,
    ('lin_narrow', 1): 2.832e-16,
    ('lin_narrow', 2): 2.832e-16,
    ('lin_narrow', 37): 2.832e-16,
}
GRAM_WORST = 7.044e-16
# LINEAR_JACOBIAN_TABLE_END
# OBSERVED on one MI355X, all 25 cases x 3 replicas, relative to |G_ref|_F: lambda 7.4e-15 at worst (sig_null, 37 rows, L = 32, 10 sweeps;
# 2.2e-15 at script line 1, 4.3e-15 at line 6) against bounds of 1.1e-13 and up; diag G 4.3e-16 and |G|_F 4.3e-16 at worst (sig_one_latent,
# 37 rows, where G is one number; bound 3.6e-15); with one decoder diag G is bitwise the reference's and |G|_F within 2.2e-16; at most
# 10 sweeps, 0 at L = 1.  The tightest case is ('sig_one_latent', 1): G is the single number sum_d J_d^2 = 3.2143... and the reference
# happens to sit 0.3 ulp (4.09e-17) from long double there, so 8 x worst = 3.27e-16 = 2.4 ulp; the kernel is 1 ulp (1.38e-16) away.
# THE FINDING this case made: with the slope taken as e / ((1 + e) (1 + e)) in plain float64 -- three roundings after exp -- the kernel
# was 3 ulp (4.14e-16) from the reference AND from long double on replica 1, outside the bound.  The kernel now rounds that quotient
# essentially once (csrc/linear_jacobian.hip); an exact-arithmetic replay of both forms on the CPU (tools/replay_linear_jacobian_slope.py)
# gives the same 4.14e-16 and 1.38e-16, the second unchanged when exp's result is moved by an ulp either way.
STOP = 2.0 ** -43


def _engine(s, batch=100, **ekw):
    from vae_training_amd.engine import Engine
    return Engine(batch, s["D"], s["L"], (), (), -1.0, True, s["sig"], **ekw)


class _Shape:
    """One engine of a shape and its R replicas' parameters in a stack whose stride exceeds P by sentinel floats and is NOT a multiple
    of 4; model records go to a sentinel-filled [n, 2 L + 8 + 3] buffer, row records to a sentinel-filled [n, rows, 2 L + 4] one."""

    def __init__(self, name, batch=100):
        s = self.s = LC.SHAPES[name]
        self.name, self.L, self.D, self.sig = name, s["L"], s["D"], s["sig"]
        self.eng = e = _engine(s, batch)
        assert e.supports_linear_decoder_jacobian()
        self.P = e.P
        self.ss = e.P + 5 if (e.P + 5) % 4 else e.P + 6
        self.flats = LC.make_flats(name)
        assert self.flats[0].size == e.P
        self.params = self.stack(self.ss)
        self.len, self.rlen = e.decoder_jacobian_record_len, e.decoder_jacobian_row_record_len
        assert (self.len, self.rlen) == (2 * self.L + 8, 2 * self.L + 4)
        self.os = self.len + 3
        nbytes = e.linear_decoder_jacobian_workspace(R, max(LC.ROWS[name]))
        assert nbytes == R * max(LC.ROWS[name]) * self.rlen * 8            # the row records only
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def stack(self, stride, flats=None):
        p = torch.full((R, stride), SENT, dtype=torch.float32, device="cuda")
        for r, f in enumerate(self.flats if flats is None else flats):
            p[r, :self.P] = torch.as_tensor(f)
        return p

    def edited(self, edit):
        """The R flats with edit(tree) applied to each (a dict of float64 leaves, edited in place)."""
        cfg = LC.cfg_of(self.s)
        out = []
        for f in self.flats:
            p = dict(O.unflatten(cfg, f.astype(np.float64)))
            edit(p)
            out.append(O.flatten(cfg, p, np.float32))
        return out

    def call(self, rows, z=None, seeds=None, steps=None, tol=LC.RANK_TOL, n=R, params=None, rows_out=True, eng=None, first=0, **kw):
        """(model records [n, 2 L + 8], row records [n, rows, 2 L + 4] or None), sentinels checked."""
        params = self.params if params is None else params
        out = torch.full((n, self.os), SENT, dtype=torch.float64, device="cuda")
        ro = torch.full((n, rows, self.rlen), SENT, dtype=torch.float64, device="cuda") if rows_out else None
        (eng or self.eng).linear_decoder_jacobian_replicas(
            params[first:first + n], rows, out, self.ws, z_seeds=None if seeds is None else _i64(seeds), z_steps=None if steps is None else _i32(steps),
            z=z, rank_tol=tol, row_out=ro, z_tag=LC.Z_TAG, n=n, state_stride=params.shape[1], **kw)
        torch.cuda.synchronize()
        assert bool((out[:, self.len:] == SENT).all()) and bool((params[:, self.P:] == SENT).all())
        return out[:, :self.len].cpu().numpy(), None if ro is None else ro.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _shape(name, batch=100):
    return _Shape(name, batch)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per replica (lambda, diag, rank, |G|_F) of the case in float64."""
    z = LC.case_latents(case)
    return [LC.row_records64(LC.jacobian64(p, z[r])[0], LC.case_tol(case))[:4] for r, p in enumerate(LC.trees_of(case[0]))]


def _zdev(z):
    return torch.as_tensor(np.ascontiguousarray(z), dtype=torch.float32).cuda().contiguous()


def _check_rows(L, rec, lam, dg, rank, ng, gram, who, worst):
    """Row records [rows, 2 L + 4] of one replica against its float64 reference and against themselves."""
    bound = (STOP + gram + 64 * L * 2.0 ** -53) * ng
    el = np.abs(rec[:, :L] - lam).max(1)
    ed = np.abs(rec[:, L:2 * L] - dg).max(1)
    en = np.abs(rec[:, 2 * L + 3] - ng)
    for key, e in (("lambda / |G|", el), ("diag / |G|", ed), ("|G| rel", en)):
        worst[key] = max(worst.get(key, 0.0), float((e[ng > 0] / ng[ng > 0]).max(initial=0.0)))
    print(who, "bound / |G|", STOP + gram + 64 * L * 2.0 ** -53, "middle term", gram, {k: f"{v:.2e}" for k, v in worst.items()})
    assert (el <= bound).all(), (who, "lambda", el.max(), bound.min())
    assert (ed <= bound).all(), (who, "diag", ed.max(), bound.min())
    assert (en <= gram * ng).all(), (who, "|G|_F", en.max(), (gram * ng).min())
    assert (rec[:, 2 * L] == rank).all(), (who, "rank", rec[:, 2 * L], rank)
    _check_self(L, rec, who)


def _check_self(L, rec, who):
    lam, dg = rec[:, :L], rec[:, L:2 * L]
    sweeps, off, ng = rec[:, 2 * L + 1], rec[:, 2 * L + 2], rec[:, 2 * L + 3]
    assert np.isfinite(rec).all(), who
    assert (np.abs(lam.sum(1) - dg.sum(1)) <= 1e-12 * np.abs(dg.sum(1))).all(), (who, "trace")
    assert (off <= STOP * ng).all() and (sweeps <= 32).all() and (sweeps == np.round(sweeps)).all(), (who, sweeps, off, ng)
    assert (np.diff(lam, axis=1) <= 0).all(), (who, "descending")


def _check_model(L, mrec, rrec, rows, tol, lam, dg, ng, gram, who):
    """A model record against the reference's means and, exactly, against its own row records."""
    bound = (STOP + gram + 64 * L * 2.0 ** -53) * ng.mean()
    assert mrec[0] == rows and mrec[7] == tol, who
    rk = rrec[:, 2 * L]
    assert mrec[2] == rk.min() and mrec[3] == rk.max() and abs(mrec[1] - rk.mean()) <= 1e-14 * L, (who, mrec[:4], rk)
    assert mrec[5] == rrec[:, 2 * L + 1].max(), who
    ratio = np.where(rrec[:, 2 * L + 3] > 0, rrec[:, 2 * L + 2] / np.where(rrec[:, 2 * L + 3] > 0, rrec[:, 2 * L + 3], 1.0), 0.0)
    assert abs(mrec[6] - ratio.max()) <= 1e-15 * max(ratio.max(), 1e-300) + 1e-300 and mrec[6] <= STOP, (who, mrec[6], ratio.max())
    assert abs(mrec[4] - dg.sum(1).mean()) <= bound, (who, "mean |J|_F^2")
    assert (np.abs(mrec[8:8 + L] - lam.mean(0)) <= bound).all(), (who, "mean lambda")
    assert (np.abs(mrec[8 + L:8 + 2 * L] - dg.mean(0)) <= bound).all(), (who, "mean diag")


@pytest.mark.parametrize("case", LC.CASES, ids=[f"{n}-rows{r}" for n, r in LC.CASES])
def test_row_and_model_records_against_float64(case):
    """Every row and model record of the case against the float64 reference, within the case's own bound.  The tightest is
    ('sig_one_latent', 1), |G|_F within 8 x worst = 8 x 4.09e-17 = 3.27e-16 (2.4 ulp): the kernel is 1.38e-16 away; a slope rounded
    three times instead of once puts it at 4.14e-16 (the comment below TABLE)."""
    name, rows = case
    assert case in TABLE, "run tools/linear_jacobian_reference.py first"
    gram = LC.GRAM_FACTOR * TABLE[case]
    c = _shape(name)
    tol = LC.case_tol(case)
    mrec, rrec = c.call(rows, z=_zdev(LC.case_latents(case)), tol=tol)
    worst = {}
    for r, (lam, dg, rank, ng) in enumerate(_reference(case)):
        _check_rows(c.L, rrec[r], lam, dg, rank, ng, gram, (case, r), worst)
        _check_model(c.L, mrec[r], rrec[r], rows, tol, lam, dg, ng, gram, (case, r))
    print(case, "observed worst", {k: f"{v:.2e}" for k, v in worst.items()}, "max sweeps", mrec[:, 5].max())


@pytest.mark.parametrize("name", [n for n, s in LC.SHAPES.items() if not s["sig"]])
def test_one_decoder_rows_are_the_spectrum_of_the_exact_record(name):
    """One decoder: J = K^T at every z, so the min(D, L) largest lambda of every row are the largest eigenvalues of K^T K the exact
    log-likelihood call leaves in its record (the D x D Gram of the same kernel, another solve), and all rows of a replica agree bitwise."""
    c = _shape(name)
    L, D, rows = c.L, c.D, 37
    k = min(D, L)
    _, rrec = c.call(rows, seeds=[5, 6, 7], steps=[1, 2, 3])
    e = c.eng
    assert e.supports_exact_log_likelihood(2)
    rlen = e.exact_log_likelihood_record_len
    assert rlen == 10 + D                                # [10, 10 + D): the eigenvalues of K^T K, ascending
    out = torch.full((R, rlen), SENT, dtype=torch.float64, device="cuda")
    e.exact_log_likelihood_replicas(c.params, 8, out, kind=2, dd=3, did=3, pad=D - 3, x_seeds=_i64([5, 6, 7]), x_steps=_i32([1, 2, 3]), n=R,
                                    state_stride=c.ss)
    torch.cuda.synchronize()
    ex = out.cpu().numpy()
    for r in range(R):
        assert all(rrec[r, i].tobytes() == rrec[r, 0].tobytes() for i in range(rows)), (name, r)
        ng = rrec[r, 0, 2 * L + 3]
        top = ex[r, 10:10 + D][::-1][:k]
        err = np.abs(rrec[r, 0, :k] - top).max()
        print(name, r, "against the exact record:", err / ng, "bound", 2 * STOP + 64 * 32 * 2.0 ** -53)
        assert err <= (2 * STOP + 64 * 32 * 2.0 ** -53) * ng, (name, r, err, ng)
        _check_self(L, rrec[r], (name, r))


@pytest.mark.parametrize("how", ["Ks=0", "bs=+800", "bs=-800"])
@pytest.mark.parametrize("name", ["sig_odd", "sig_script6"])           # an odd shape; D = 28, the cap: the last head and the last column of J
def test_a_switched_off_second_decoder_is_the_one_decoder_call_bitwise(name, how):
    """g = 0 on every head -- K_s = 0 (b_s generic), or b_s = +-800 (K_s generic: |u| stays above 745, exp(-|u|) is exactly 0) -- leaves
    J = K_d^T: the row records of the one-decoder context with the same K_d, bit for bit, finite everywhere."""
    two = _shape(name)
    one = _engine(dict(D=two.D, L=two.L, sig=False))
    assert one.supports_linear_decoder_jacobian()
    rows = 37
    z = _zdev(LC.case_latents((name, rows)))

    def edit(p):
        if how == "Ks=0":
            p["SigDecoder/FC0/kernel"] = np.zeros_like(p["SigDecoder/FC0/kernel"])
        else:
            p["SigDecoder/FC0/bias"] = np.full_like(p["SigDecoder/FC0/bias"], 800.0 if how == "bs=+800" else -800.0)
    flats2 = two.edited(edit)
    trees = LC.trees_of(name, flats2)
    if how != "Ks=0":
        with np.errstate(over="ignore"):                 # the reference's exp(-u) at u = -800 is inf, its s = 0: only u is read here
            assert min(float(np.abs(LC.jacobian64(p, LC.case_latents((name, rows))[r])[1]).min()) for r, p in enumerate(trees)) > 745.2
    cfg1 = LC.cfg_of(dict(D=two.D, L=two.L, sig=False))
    flats1 = [O.flatten(cfg1, {k: v for k, v in p.items() if not k.startswith("SigDecoder")}, np.float32) for p in trees]
    assert flats1[0].size == one.P
    _, got = two.call(rows, z=z, params=two.stack(two.ss, flats2))
    p1 = torch.full((R, one.P + 3), SENT, dtype=torch.float32, device="cuda")
    for r, f in enumerate(flats1):
        p1[r, :one.P] = torch.as_tensor(f)
    out = torch.full((R, two.os), SENT, dtype=torch.float64, device="cuda")
    ro = torch.full((R, rows, two.rlen), SENT, dtype=torch.float64, device="cuda")
    one.linear_decoder_jacobian_replicas(p1, rows, out, two.ws, z=z, row_out=ro, z_tag=LC.Z_TAG, state_stride=one.P + 3)
    torch.cuda.synchronize()
    want = ro.cpu().numpy()
    assert np.isfinite(got).all() and (got[:, :, 2 * two.L + 3] > 0).all()
    assert got.tobytes() == want.tobytes(), (name, how)


@pytest.mark.parametrize("name,k", [("sig_script6", 5), ("sig_null", 3), ("lin_odd", 7)])
def test_planted_rank(name, k):
    """Rows l >= k of K_d and K_s exactly zero: rank k on every row, diag G exactly 0.0 for l >= k."""
    c = _shape(name)
    rows = 37

    def edit(p):
        for net in ("Decoder", "SigDecoder"):
            if f"{net}/FC0/kernel" in p:
                K = p[f"{net}/FC0/kernel"].copy()
                K[k:] = 0.0
                p[f"{net}/FC0/kernel"] = K
    flats = c.edited(edit)
    z = LC.case_latents((name, rows))
    # the k planted singular values are well above the threshold in the reference
    for r, p in enumerate(LC.trees_of(name, flats)):
        lam = LC.row_records64(LC.jacobian64(p, z[r])[0], LC.RANK_TOL)[0]
        assert (lam[:, k - 1] > 10 * LC.RANK_TOL * lam[:, 0]).all(), (name, r, (lam[:, k - 1] / lam[:, 0]).min())
    mrec, rrec = c.call(rows, z=_zdev(z), params=c.stack(c.ss, flats))
    assert (rrec[:, :, 2 * c.L] == k).all(), rrec[:, :, 2 * c.L]
    assert (rrec[:, :, c.L + k:2 * c.L] == 0.0).all() and (rrec[:, :, c.L:c.L + k] > 0.0).all()
    assert (mrec[:, 1:4] == k).all()
    for r in range(R):
        _check_self(c.L, rrec[r], (name, r))


@pytest.mark.parametrize("name", ["sig_script1", "lin_narrow"])
def test_dead_decoder(name):
    """All decoder kernels zero: G = 0, 0 sweeps, rank 0, zeros, no NaN."""
    c = _shape(name)

    def edit(p):
        for net in ("Decoder", "SigDecoder"):
            if f"{net}/FC0/kernel" in p:
                p[f"{net}/FC0/kernel"] = np.zeros_like(p[f"{net}/FC0/kernel"])
    mrec, rrec = c.call(37, seeds=[5, 6, 7], steps=[1, 2, 3], params=c.stack(c.ss, c.edited(edit)))
    assert np.isfinite(mrec).all() and np.isfinite(rrec).all()
    assert (rrec == 0).all() and (mrec[:, 1:7] == 0).all() and (mrec[:, 8:] == 0).all() and (mrec[:, 0] == 37).all()


@pytest.mark.parametrize("name", ["sig_script1", "sig_odd", "lin_odd"])
def test_bitwise_properties(name):
    rows = 37
    c = _shape(name)
    L = c.L
    seeds, steps = [2 ** 64 - 3, 991, 31337], [3, 2 ** 32 - 1, 2]
    # drawing mode against explicit mode on the z1 vaek_make_batch writes
    drawn_m, drawn = c.call(rows, seeds=seeds, steps=steps)
    z = torch.stack([c.eng.make_batch(2, None, 3, 3, c.D - 3, 0.0, rows, seeds[r], step=steps[r], tag=LC.Z_TAG, want_x=False)[1] for r in range(R)])
    expl_m, expl = c.call(rows, z=z.contiguous())
    assert drawn.tobytes() == expl.tobytes() and drawn_m.tobytes() == expl_m.tobytes()
    for r in range(R):
        _check_self(L, drawn[r], ("drawn", r))
    if c.sig:                                            # the rows differ: the latents are read
        assert drawn[0, 0, :L].tobytes() != drawn[0, 1, :L].tobytes()
    # two runs; row_out = NULL leaves the model record what it is
    again_m, again = c.call(rows, seeds=seeds, steps=steps)
    assert again.tobytes() == drawn.tobytes() and again_m.tobytes() == drawn_m.tobytes()
    alone_m, none = c.call(rows, seeds=seeds, steps=steps, rows_out=False)
    assert none is None and alone_m.tobytes() == drawn_m.tobytes()
    # replica r of n = 3 against n = 1 on its slices; a shared latent set (z_stride = 0) against its copies
    for r in range(R):
        m1, r1 = c.call(rows, seeds=seeds[r:r + 1], steps=steps[r:r + 1], n=1, first=r)
        assert m1[0].tobytes() == drawn_m[r].tobytes() and r1[0].tobytes() == drawn[r].tobytes()
    sh_m, sh = c.call(rows, z=z[1].contiguous())
    cp_m, cp = c.call(rows, z=torch.stack([z[1]] * R).contiguous())
    assert sh.tobytes() == cp.tobytes() and sh_m.tobytes() == cp_m.tobytes() and sh[1].tobytes() == expl[1].tobytes()
    # a row of the 37-row call against the same latents as the two rows of 2-row calls
    for i in (0, 8, 35):
        _, two = c.call(2, z=z[:, [i, i + 1]].contiguous())
        assert two.tobytes() == expl[:, [i, i + 1]].tobytes(), i
    # another parameter stride (a multiple of 4) and an engine of another batch size
    s4 = c.ss + (4 - c.ss % 4)
    assert c.ss % 4 and s4 % 4 == 0
    st_m, st = c.call(rows, z=z.contiguous(), params=c.stack(s4))
    assert st.tobytes() == expl.tobytes() and st_m.tobytes() == expl_m.tobytes()
    other = _shape(name, 37)
    ot_m, ot = c.call(rows, z=z.contiguous(), eng=other.eng)
    assert ot.tobytes() == expl.tobytes() and ot_m.tobytes() == expl_m.tobytes()


def test_the_call_is_capturable_and_profiled():
    c = _shape("sig_script1")
    seeds, steps = [5, 6, 7], [1, 2, 3]
    eager_m, eager = c.call(37, seeds=seeds, steps=steps)
    out = torch.full((R, c.os), SENT, dtype=torch.float64, device="cuda")
    ro = torch.full((R, 37, c.rlen), SENT, dtype=torch.float64, device="cuda")
    sd, st = _i64(seeds), _i32(steps)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.eng.linear_decoder_jacobian_replicas(c.params, 37, out, c.ws, z_seeds=sd, z_steps=st, row_out=ro, z_tag=LC.Z_TAG)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                     # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert out[:, :c.len].cpu().numpy().tobytes() == eager_m.tobytes() and ro.cpu().numpy().tobytes() == eager.tobytes()
    c.eng.profile_begin()
    c.call(37, seeds=seeds, steps=steps)
    rep = c.eng.profile_report()
    assert sorted(rep) == sorted(LABELS) and all(rep[k]["count"] == 1 for k in LABELS), rep


def test_refusals_that_need_a_device():
    from tests import decoder_jacobian_cases as DC
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c = _shape("sig_script1")
    z = _zdev(LC.case_latents(("sig_script1", 37)))
    sd, st = [5, 6, 7], [1, 2, 3]

    def refused(what, **kw):
        out = torch.full((R, c.os), SENT, dtype=torch.float64, device="cuda")
        args = dict(z_seeds=_i64(sd), z_steps=_i32(st), z_tag=LC.Z_TAG)
        args.update(kw)
        rows, ws = args.pop("rows", 37), args.pop("workspace", c.ws)
        o = args.pop("out", out)
        with pytest.raises(VaekError, match="vaek_linear_decoder_jacobian_replicas") as ei:
            c.eng.linear_decoder_jacobian_replicas(c.params, rows, o, ws, **args)
        torch.cuda.synchronize()
        assert ei.value.code == -1 and bool((out == SENT).all()), what

    refused("struct_size", struct_size=8)
    refused("n = 0", n=0)
    refused("n above the cap", n=c.eng.train_loop_max_replicas + 1)
    refused("rows = 0", rows=0)
    refused("rows above the cap", rows=4097)
    refused("no seeds", z_seeds=None)
    refused("no steps", z_steps=None)
    refused("no out", out=None, out_stride=c.os)
    refused("state_stride < P", state_stride=c.P - 1)
    refused("out_stride < record", out_stride=c.len - 1)
    refused("row_out_stride short", row_out=torch.zeros(R, 37, c.rlen, dtype=torch.float64, device="cuda"), row_out_stride=37 * c.rlen - 1)
    refused("z_stride < 0", z=z, z_stride=-1)
    refused("0 < z_stride < rows L", z=z, z_stride=37 * c.L - 1)
    for bad in (-1e-9, 1.0, float("nan")):
        refused("rank_tol", rank_tol=bad)
    refused("tag", z_tag=2 ** 30)
    refused("workspace NULL", workspace=None)
    refused("workspace misaligned", workspace=c.ws.data_ptr() + 8)
    # the row cap: n * rows <= 2^20, here and in the workspace query, which grows with n and rows
    assert c.eng.linear_decoder_jacobian_max_rows == 2 ** 20
    assert c.eng.linear_decoder_jacobian_workspace(256, 4096) == 256 * 4096 * c.rlen * 8      # exactly the cap
    with pytest.raises(VaekError, match="vaek_linear_decoder_jacobian_workspace_bytes.*1052672 rows, at most 1048576"):
        c.eng.linear_decoder_jacobian_workspace(257, 4096)
    big = torch.zeros(257, c.ss, dtype=torch.float32, device="cuda")
    with pytest.raises(VaekError, match="vaek_linear_decoder_jacobian_replicas.*1052672 rows, at most 1048576"):
        c.eng.linear_decoder_jacobian_replicas(big, 4096, torch.zeros(257, c.len, dtype=torch.float64, device="cuda"), c.ws,
                                               z_seeds=_i64([1] * 257), z_steps=_i32([1] * 257))
    assert c.eng.linear_decoder_jacobian_workspace(1, 1) < c.eng.linear_decoder_jacobian_workspace(1, 2) < c.eng.linear_decoder_jacobian_workspace(2, 2)
    # contexts the predicate does not cover: an mlp3 context, two decoders with D = 29, D = 33, bf16; the batch and force_generic do not matter
    s = DC.SHAPES["script1"]
    fence = [Engine(100, s["D"], s["L"], s["enc"], s["dec"], -1.0, True, False), Engine(100, 29, 6, (), (), -1.0, True, True),
             Engine(100, 33, 6, (), (), -1.0, True, False), Engine(100, 7, 33, (), (), -1.0, True, False)]
    for e in fence:
        assert not e.supports_linear_decoder_jacobian()
        with pytest.raises(VaekError, match="vaek_linear_decoder_jacobian_workspace_bytes.*needs a float32 linear VAE"):
            e.linear_decoder_jacobian_workspace(1, 1)
        with pytest.raises(VaekError, match="vaek_linear_decoder_jacobian_replicas.*needs a float32 linear VAE"):
            e.linear_decoder_jacobian_replicas(torch.zeros(1, e.P, device="cuda"), 1, torch.zeros(1, 80, dtype=torch.float64, device="cuda"),
                                               c.ws, z_seeds=_i64([1]), z_steps=_i32([1]))
    for e in (Engine(100, 28, 6, (), (), -1.0, True, True), Engine(4096, 32, 32, (), (), -1.0, False, False),
              Engine(100, 7, 6, (), (), -1.0, True, True, force_generic=True)):
        assert e.supports_linear_decoder_jacobian()


class _Model:
    """What ReplicaJacobianLinear asks of a VAEModel, around real engines."""

    def __init__(self, name, flat, seed, batch=100):
        import types
        s = LC.SHAPES[name]
        engines = {}

        def engine(B, gb=0):
            if B not in engines:
                engines[B] = _shape(name, B).eng
            return engines[B]
        self.model = types.SimpleNamespace(module=types.SimpleNamespace(engine=engine, tunable_decoder_var=True),
                                           flat=torch.as_tensor(flat).cuda())
        self.batch_size, self.print_batch_size = batch, 1000
        self.optimizer = types.SimpleNamespace(global_batch=0)
        self.dataset = types.SimpleNamespace(device_spec=lambda: (2, None, 3, 3, s["D"] - 3, 0.0), key=(seed, 2), _draws=5)
        self.key, self._latent_draws, self.dirname = (3, 4), 9, name


@pytest.mark.parametrize("at", ["prior", "posterior"])
def test_replica_jacobian_linear_against_float64(at):
    """Three two-decoder models, 4 rows each: the class's records against the float64 reference on the latents it used -- the z1
    make_batch draws under its seed, step and tag (prior), the library's own vaek_forward mu of the rows it draws (posterior).  The
    bound's middle term is measured on these latents (gram_longdouble); the rank is compared where the reference leaves the
    threshold free."""
    from vae_training_amd.trainer import ReplicaJacobianLinear
    name, rows, tol = "sig_script1", 4, 1e-4
    c = _shape(name)
    ms = [_Model(name, f, seed) for f, seed in zip(c.flats, (68, 48, 54))]
    jac = ReplicaJacobianLinear(ms, rows=rows, at=at, rank_tol=tol)
    stats = jac.event()
    assert all(m._jacobian_draws == 1 and m.key == (3, 4) and m._latent_draws == 9 and m.dataset._draws == 5 for m in ms)
    trees = LC.trees_of(name)
    for r, (m, st) in enumerate(zip(ms, stats)):
        seed = m.dataset.key[0] ^ m.dataset.key[1]
        eng = _shape(name, rows).eng
        if at == "prior":
            z = eng.make_batch(2, None, 3, 3, c.D - 3, 0.0, rows, seed, step=1, tag=jac.Z_TAG, want_x=False)[1]
        else:
            x, z1, z2 = eng.make_batch(2, None, 3, 3, c.D - 3, 0.0, rows, seed, step=1, tag=jac.X_TAG)
            z = eng.forward(m.model.flat, x, z1, z2, sampling=False)[1]
        z = z.cpu().numpy()
        lam, dg, rank, ng, _ = LC.row_records64(LC.jacobian64(trees[r], z)[0], tol)
        gram = LC.GRAM_FACTOR * float(LC.gram_longdouble(trees[r], z).max())
        bound = (STOP + gram + 64 * c.L * 2.0 ** -53) * ng.mean()
        ratio = lam / lam[:, :1]
        assert not ((ratio >= tol / 2) & (ratio <= 2 * tol)).any(), "a ratio of this event sits on the threshold: pick other seeds"
        assert list(st) == list(jac.KEYS)
        err = max(np.abs(st[jac.KEYS[0]] - lam.mean(0)).max(), np.abs(st[jac.KEYS[2]] - dg.mean(0)).max())
        print(at, r, "error / mean |G|", err / ng.mean(), "bound", bound / ng.mean(), "ranks", rank)
        assert err <= bound
        assert st[jac.KEYS[1]].tolist() == [rank.mean(), rank.min(), rank.max()]
        assert m.jacobian_spectra[-1] is st[jac.KEYS[0]] and len(m.jacobian_ranks) == 1 and len(m.latent_sensitivities) == 1


@pytest.mark.parametrize("sweep", [False, True], ids=["alone", "sweep"])
def test_run_py_writes_the_jacobian_keys(tmp_path, sweep):
    """Line 1 of sigmoid_vae_padding_expts.sh, 30 batches, --linear_decoder_jacobian prior, in a fresh child process, alone and with
    --sweep_dataset_seeds 69,24: the new keys' shapes."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "ljac", "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "", "-ow", "--latent_dim", "6", "--padding_dim", "3",
           "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", "--linear_decoder_jacobian", "prior"]
    names = ["ljac"]
    if sweep:
        cmd += ["--sweep_dataset_seeds", "69,24"]
        names = ["ljac_ds69", "ljac_ds24"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    banner = ("Decoder Jacobian events: 1000 prior latent rows per model, rank threshold 0.0001, one call for 2 models" if sweep else
              "Decoder Jacobian events: 1000 prior latent rows, rank threshold 0.0001")
    assert banner in r.stdout and "(vaek_linear_decoder_jacobian_replicas)" in r.stdout, r.stdout[-1500:]
    assert "Decoder Jacobian Rank (mean) |" in r.stdout, r.stdout[-1500:]
    for nm in names:
        f = dict(np.load(os.path.join(str(tmp_path), "data", nm, "losses.npz"), allow_pickle=True))
        spec, rank, sens = (np.asarray(f[k], dtype=np.float64) for k in ("Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"))
        ev = spec.shape[0]
        assert ev >= 1 and spec.shape == (ev, 6) and rank.shape == (ev, 3) and sens.shape == (ev, 6), (spec.shape, rank.shape, sens.shape)
        assert np.isfinite(spec).all() and (np.diff(spec, axis=1) <= 0).all() and (0 <= rank[:, 1]).all() and (rank[:, 1] <= rank[:, 0]).all() \
            and (rank[:, 0] <= rank[:, 2]).all() and (rank[:, 2] <= 6).all()
        assert abs(spec.sum() - sens.sum()) <= 1e-9 * sens.sum()
