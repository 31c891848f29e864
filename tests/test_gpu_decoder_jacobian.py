"""-m gpu: vaek_mlp3_decoder_jacobian_replicas -- the spectra of the decoder Jacobian J(z) = d Decoder(z) / dz of N three-hidden-layer MLP
VAEs of one shape in one call (csrc/mlp3_jacobian.hip) -- and its callers, trainer.ReplicaJacobianMlp3 and `run.py --decoder_jacobian`.

A row record is [lambda (L, descending), diag G (L), rank, sweeps, off_F, |G|_F] with G = J^T J; a model record [rows, mean / min / max
rank, mean |J|_F^2, max sweeps, max off_F / |G|_F, rank_tol, mean lambda (L), mean diag G (L)].  References:
  - the float64 NumPy reference of tests/decoder_jacobian_cases.py on the cases' explicit latents, every row through row_out:
    |lambda_k - ref| and |diag G - ref| <= GRAM_RTOL |G_ref|_F + 64 L 2^-53 |G_ref|_F (Weyl, plus the Jacobi stop), |G|_F within GRAM_RTOL
    relative, the rank exactly; the model record's means within the same bound with the mean |G_ref|_F, its counts exact;
  - itself: sum lambda = trace G within 1e-12 relative, off_F <= 2^-43 |G|_F, sweeps <= 32, lambda descending, on every row;
  - itself, BITWISE: drawing mode against explicit mode on the z1 vaek_make_batch writes, replica r of n = 3 against n = 1 on its
    slices, two runs, a captured call, engines of different batch sizes, two parameter strides (one not a multiple of 4), a row of a
    37-row call against the same latents as a row of a 2-row call, row_out given or NULL, sentinels between the records.
HOW WELL THE REFERENCE IS DEFINED (tools/decoder_jacobian_reference.py, on the CPU, before any run of the kernel; TABLE below): per
case the worst distance of a float32 forward with sequential k-order accumulation from float64 on a hidden pre-activation (0.4 .. 2.8e-6),
the case's smallest |pre| (every case >= KINK_FACTOR = 8 times its distance: J is piecewise constant in the masks, a flipped mask is no
rounding error) and the relative error of G under the same emulation; GRAM_RTOL = 8 x the worst of those.
tests/test_decoder_jacobian_inputs.py recomputes the table without a GPU.
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
from tests import decoder_jacobian_cases as DC
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
LABELS = ["mlp3_jacobian_tangent", "mlp3_jacobian_solve", "mlp3_jacobian_finalize"]
R = DC.R
# JACOBIAN_TABLE_BEGIN (written by tools/decoder_jacobian_reference.py: per case (dist, min |pre|, gram) of its docstring)
TABLE = {
    ('script1', 1): (6.489e-07, 1.106e-04, 3.395e-07),
    ('script1', 2): (7.416e-07, 2.483e-05, 4.679e-07),
    ('script1', 37): (1.064e-06, 1.235e-05, 7.300e-07),
    ('narrow', 1): (4.056e-07, 8.359e-05, 2.713e-07),
    ('narrow', 2): (4.056e-07, 8.359e-05, 2.713e-07),
    ('narrow', 37): (5.734e-07, 5.912e-05, 4.627e-07),
    ('mixed', 1): (3.970e-07, 2.964e-04, 3.954e-07),
    ('mixed', 2): (6.222e-07, 2.964e-04, 3.954e-07),
    ('mixed', 37): (8.312e-07, 2.402e-05, 3.607e-07),
    ('odd', 1): (4.591e-07, 1.238e-05, 3.039e-07),
    ('odd', 2): (5.819e-07, 1.238e-05, 3.039e-07),
    ('odd', 37): (9.559e-07, 1.088e-04, 3.499e-07),
    ('wide', 1): (1.066e-06, 2.429e-04, 3.507e-07),
    ('wide', 2): (1.066e-06, 4.856e-05, 3.857e-07),
    ('wide', 37): (1.251e-06, 1.866e-05, 3.927e-07),
    ('one_latent', 1): (6.410e-07, 2.134e-05, 6.025e-07),
    ('one_latent', 2): (6.680e-07, 2.134e-05, 6.025e-07),
    ('one_latent', 70): (2.822e-06, 2.394e-05, 1.119e-06),
}
GRAM_WORST = 1.119e-06
# JACOBIAN_TABLE_END
GRAM_RTOL = DC.GRAM_FACTOR * GRAM_WORST
# OBSERVED on one MI355X, all 18 cases x 3 replicas, relative to |G_ref|_F: lambda 8.5e-7, diag G 8.5e-7, |G|_F 8.5e-7 at worst (one_latent, 70
# rows; every L > 1 shape below 4.9e-7), against GRAM_RTOL = 9.0e-6; at most 11 sweeps (odd, L = 20), 9 at L = 32, 0 at L = 1
STOP = 2.0 ** -43


class _Shape:
    """One engine of a shape and its R replicas' parameters in a stack whose stride exceeds P by sentinel floats and is NOT a multiple
    of 4; model records go to a sentinel-filled [n, 2 L + 8 + 3] buffer, row records to a sentinel-filled [n, rows, 2 L + 4] one."""

    def __init__(self, name, batch=100, **ekw):
        from vae_training_amd.engine import Engine
        s = self.s = DC.SHAPES[name]
        self.name, self.L, self.D = name, s["L"], s["D"]
        self.eng = e = Engine(batch, s["D"], s["L"], s["enc"], s["dec"], -1.0, True, False, **ekw)
        assert e.supports_mlp3_decoder_jacobian()
        self.P = e.P
        self.ss = e.P + 5 if (e.P + 5) % 4 else e.P + 6
        self.flats = DC.make_flats(name)
        assert self.flats[0].size == e.P
        self.params = self.stack(self.ss)
        self.len, self.rlen = e.decoder_jacobian_record_len, e.decoder_jacobian_row_record_len
        assert (self.len, self.rlen) == (2 * self.L + 8, 2 * self.L + 4)
        self.os = self.len + 3
        self.ws = torch.empty(e.mlp3_decoder_jacobian_workspace(R, max(DC.ROWS[name])), dtype=torch.uint8, device="cuda")

    def stack(self, stride, flats=None):
        p = torch.full((R, stride), SENT, dtype=torch.float32, device="cuda")
        for r, f in enumerate(self.flats if flats is None else flats):
            p[r, :self.P] = torch.as_tensor(f)
        return p

    def call(self, rows, z=None, seeds=None, steps=None, tol=DC.RANK_TOL, n=R, params=None, rows_out=True, eng=None, first=0, **kw):
        """(model records [n, 2 L + 8], row records [n, rows, 2 L + 4] or None), sentinels checked."""
        params = self.params if params is None else params
        out = torch.full((n, self.os), SENT, dtype=torch.float64, device="cuda")
        ro = torch.full((n, rows, self.rlen), SENT, dtype=torch.float64, device="cuda") if rows_out else None
        (eng or self.eng).mlp3_decoder_jacobian_replicas(
            params[first:first + n], rows, out, self.ws, z_seeds=None if seeds is None else _i64(seeds), z_steps=None if steps is None else _i32(steps),
            z=z, rank_tol=tol, row_out=ro, z_tag=DC.Z_TAG, n=n, state_stride=params.shape[1], **kw)
        torch.cuda.synchronize()
        assert bool((out[:, self.len:] == SENT).all()) and bool((params[:, self.P:] == SENT).all())
        return out[:, :self.len].cpu().numpy(), None if ro is None else ro.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _shape(name, batch=100):
    return _Shape(name, batch)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Per replica (lambda, diag, rank, |G|_F) of the case in float64."""
    z = DC.case_latents(case)
    return [DC.row_records64(DC.jacobian64(p, z[r])[0], DC.case_tol(case))[:4] for r, p in enumerate(DC.trees_of(case[0]))]


def _zdev(z):
    return torch.as_tensor(np.ascontiguousarray(z), dtype=torch.float32).cuda().contiguous()


def _check_rows(L, rec, lam, dg, rank, ng, tol_g, who, worst):
    """Row records [rows, 2 L + 4] of one replica against its float64 reference and against themselves."""
    bound = tol_g * ng + 64 * L * 2.0 ** -53 * ng
    el = np.abs(rec[:, :L] - lam).max(1)
    ed = np.abs(rec[:, L:2 * L] - dg).max(1)
    en = np.abs(rec[:, 2 * L + 3] - ng)
    worst["lambda / |G|"] = max(worst.get("lambda / |G|", 0.0), float((el[ng > 0] / ng[ng > 0]).max(initial=0.0)))
    worst["diag / |G|"] = max(worst.get("diag / |G|", 0.0), float((ed[ng > 0] / ng[ng > 0]).max(initial=0.0)))
    worst["|G| rel"] = max(worst.get("|G| rel", 0.0), float((en[ng > 0] / ng[ng > 0]).max(initial=0.0)))
    assert (el <= bound).all(), (who, "lambda", el.max(), bound.min())
    assert (ed <= bound).all(), (who, "diag", ed.max(), bound.min())
    assert (en <= tol_g * ng).all(), (who, "|G|_F", en.max())
    assert (rec[:, 2 * L] == rank).all(), (who, "rank", rec[:, 2 * L], rank)
    _check_self(L, rec, who)


def _check_self(L, rec, who):
    lam, dg = rec[:, :L], rec[:, L:2 * L]
    sweeps, off, ng = rec[:, 2 * L + 1], rec[:, 2 * L + 2], rec[:, 2 * L + 3]
    assert np.isfinite(rec).all(), who
    assert (np.abs(lam.sum(1) - dg.sum(1)) <= 1e-12 * np.abs(dg.sum(1))).all(), (who, "trace")
    assert (off <= STOP * ng).all() and (sweeps <= 32).all() and (sweeps == np.round(sweeps)).all(), (who, sweeps, off, ng)
    assert (np.diff(lam, axis=1) <= 0).all(), (who, "descending")


def _check_model(L, mrec, rrec, rows, tol, lam, dg, ng, tol_g, who):
    """A model record against the reference's means and, exactly, against its own row records."""
    bound = (tol_g + 64 * L * 2.0 ** -53) * ng.mean()
    assert mrec[0] == rows and mrec[7] == tol, who
    rk = rrec[:, 2 * L]
    assert mrec[2] == rk.min() and mrec[3] == rk.max() and abs(mrec[1] - rk.mean()) <= 1e-14 * L, (who, mrec[:4], rk)
    assert mrec[5] == rrec[:, 2 * L + 1].max(), who
    ratio = np.where(rrec[:, 2 * L + 3] > 0, rrec[:, 2 * L + 2] / np.where(rrec[:, 2 * L + 3] > 0, rrec[:, 2 * L + 3], 1.0), 0.0)
    assert abs(mrec[6] - ratio.max()) <= 1e-15 * max(ratio.max(), 1e-300) + 1e-300 and mrec[6] <= STOP, (who, mrec[6], ratio.max())
    assert abs(mrec[4] - dg.sum(1).mean()) <= bound, (who, "mean |J|_F^2")
    assert (np.abs(mrec[8:8 + L] - lam.mean(0)) <= bound).all(), (who, "mean lambda")
    assert (np.abs(mrec[8 + L:8 + 2 * L] - dg.mean(0)) <= bound).all(), (who, "mean diag")


@pytest.mark.parametrize("case", DC.CASES, ids=[f"{n}-rows{r}" for n, r in DC.CASES])
def test_row_and_model_records_against_float64(case):
    name, rows = case
    assert case in TABLE and GRAM_RTOL > 0, "run tools/decoder_jacobian_reference.py first"
    c = _shape(name)
    tol = DC.case_tol(case)
    mrec, rrec = c.call(rows, z=_zdev(DC.case_latents(case)), tol=tol)
    worst = {}
    for r, (lam, dg, rank, ng) in enumerate(_reference(case)):
        _check_rows(c.L, rrec[r], lam, dg, rank, ng, GRAM_RTOL, (case, r), worst)
        _check_model(c.L, mrec[r], rrec[r], rows, tol, lam, dg, ng, GRAM_RTOL, (case, r))
    print(case, "GRAM_RTOL", GRAM_RTOL, "observed worst", {k: f"{v:.2e}" for k, v in worst.items()}, "max sweeps", mrec[:, 5].max())


def test_degenerate_decoders_and_an_exact_kink():
    """A zero last kernel: J = 0, rank 0, 0 sweeps, no NaN.  An explicit row z = 0 under a zero FC0 bias: every first-layer
    pre-activation is exactly 0, so that row's J is 0 -- and its neighbours' records are what they are without it, bitwise."""
    case = ("script1", 37)
    c = _shape("script1")
    cfg = DC.cfg_of(c.s)
    z = DC.case_latents(case)[0].copy()                   # [37, L], shared by the replicas
    dead, kink = [], []
    for f in c.flats:
        p = O.unflatten(cfg, f.astype(np.float64))
        q = dict(p)
        q["Decoder/FC3/kernel"] = np.zeros_like(p["Decoder/FC3/kernel"])
        dead.append(O.flatten(cfg, q, np.float32))
        q = dict(p)
        q["Decoder/FC0/bias"] = np.zeros_like(p["Decoder/FC0/bias"])
        kink.append(O.flatten(cfg, q, np.float32))
    mrec, rrec = c.call(37, z=_zdev(z), params=c.stack(c.ss, dead))
    assert np.isfinite(mrec).all() and np.isfinite(rrec).all()
    assert (rrec == 0).all() and (mrec[:, 1:7] == 0).all() and (mrec[:, 8:] == 0).all() and (mrec[:, 0] == 37).all()
    pk = c.stack(c.ss, kink)
    base_m, base = c.call(37, z=_zdev(z), params=pk)
    zk = z.copy()
    zk[5] = 0.0
    _, got = c.call(37, z=_zdev(zk), params=pk)
    assert np.isfinite(got).all() and (got[:, 5] == 0).all() and (base[:, 5, :c.L] != 0).any()
    keep = [i for i in range(37) if i != 5]
    assert got[:, keep].tobytes() == base[:, keep].tobytes()
    for r in range(R):
        _check_self(c.L, got[r], ("kink", r))


def test_bitwise_properties():
    name, rows = "script1", 37
    c = _shape(name)
    L = c.L
    seeds, steps = [2 ** 64 - 3, 991, 31337], [3, 2 ** 32 - 1, 2]
    # drawing mode against explicit mode on the z1 vaek_make_batch writes
    drawn_m, drawn = c.call(rows, seeds=seeds, steps=steps)
    z = torch.stack([c.eng.make_batch(2, None, 3, 3, 3, 0.0, rows, seeds[r], step=steps[r], tag=DC.Z_TAG, want_x=False)[1] for r in range(R)])
    expl_m, expl = c.call(rows, z=z.contiguous())
    assert drawn.tobytes() == expl.tobytes() and drawn_m.tobytes() == expl_m.tobytes()
    for r in range(R):
        _check_self(L, drawn[r], ("drawn", r))
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
    # a row does not depend on its place in the tile: rows 0 .. 36 against the same latents as the two rows of 2-row calls
    for i in (0, 8, 9, 35):
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
    # L = 1 across two tile boundaries, and the widest shape (one row a tile)
    for nm, rw in (("one_latent", 70), ("wide", 2)):
        d = _shape(nm)
        a_m, a = d.call(rw, seeds=seeds, steps=steps)
        zz = torch.stack([d.eng.make_batch(2, None, 3, 3, d.D - 3, 0.0, rw, seeds[r], step=steps[r], tag=DC.Z_TAG, want_x=False)[1] for r in range(R)])
        b_m, b = d.call(rw, z=zz.contiguous())
        assert a.tobytes() == b.tobytes() and a_m.tobytes() == b_m.tobytes(), nm


def test_the_call_is_capturable_and_profiled():
    c = _shape("script1")
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
            c.eng.mlp3_decoder_jacobian_replicas(c.params, 37, out, c.ws, z_seeds=sd, z_steps=st, row_out=ro, z_tag=DC.Z_TAG)
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
    from tests import mlp3_cases as MC
    from tests.gpu_util import engine_for
    from vae_training_amd._lib import VaekError
    c = _shape("script1")
    z = _zdev(DC.case_latents(("script1", 37)))
    sd, st = [5, 6, 7], [1, 2, 3]

    def refused(what, **kw):
        out = torch.full((R, c.os), SENT, dtype=torch.float64, device="cuda")
        args = dict(z_seeds=_i64(sd), z_steps=_i32(st), z_tag=DC.Z_TAG)
        args.update(kw)
        rows, ws = args.pop("rows", 37), args.pop("workspace", c.ws)
        o = args.pop("out", out)
        with pytest.raises(VaekError, match="vaek_mlp3_decoder_jacobian_replicas") as ei:
            c.eng.mlp3_decoder_jacobian_replicas(c.params, rows, o, ws, **args)
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
    # the column cap: n * rows * L <= 2^20, here and in the workspace query, which grows with n and rows
    wide = _shape("wide")
    assert wide.eng.mlp3_decoder_jacobian_max_columns == 2 ** 20
    assert wide.eng.mlp3_decoder_jacobian_workspace(8, 4096) == 8 * 4096 * 32 * 32 * 4 + 8 * 4096 * 68 * 8      # exactly the cap
    with pytest.raises(VaekError, match="vaek_mlp3_decoder_jacobian_workspace_bytes.*columns"):
        wide.eng.mlp3_decoder_jacobian_workspace(9, 4096)
    big = torch.zeros(9, wide.ss, dtype=torch.float32, device="cuda")
    with pytest.raises(VaekError, match="vaek_mlp3_decoder_jacobian_replicas.*1179648 columns, at most 1048576"):
        wide.eng.mlp3_decoder_jacobian_replicas(big, 4096, torch.zeros(9, wide.len, dtype=torch.float64, device="cuda"), wide.ws,
                                                z_seeds=_i64([1] * 9), z_steps=_i32([1] * 9))
    assert c.eng.mlp3_decoder_jacobian_workspace(1, 1) < c.eng.mlp3_decoder_jacobian_workspace(1, 2) < c.eng.mlp3_decoder_jacobian_workspace(2, 2)
    # contexts the predicate does not cover; the batch, the world and force_generic do not matter
    for cfg, dk, B, seed, kw in MC.FENCE:
        e = engine_for(cfg, B, **kw)
        covered = e.supports_mlp3_log_likelihood(2)
        assert e.supports_mlp3_decoder_jacobian() == covered, MC.case_id((cfg, dk, B, seed, kw))
        if not covered:
            with pytest.raises(VaekError, match="vaek_mlp3_decoder_jacobian_workspace_bytes.*needs a float32 VAE"):
                e.mlp3_decoder_jacobian_workspace(1, 1)
            with pytest.raises(VaekError, match="vaek_mlp3_decoder_jacobian_replicas.*needs a float32 VAE"):
                e.mlp3_decoder_jacobian_replicas(torch.zeros(1, e.P, device="cuda"), 1, torch.zeros(1, 80, dtype=torch.float64, device="cuda"),
                                                 c.ws, z_seeds=_i64([1]), z_steps=_i32([1]))


class _Model:
    """What ReplicaJacobianMlp3 asks of a VAEModel, around real engines."""

    def __init__(self, name, flat, seed, batch=100):
        import types
        s = DC.SHAPES[name]
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
def test_replica_jacobian_mlp3_against_float64(at):
    """Three models, 4 rows each: the class's records against the float64 reference on the latents it used -- the z1 make_batch draws
    under its seed, step and tag (prior), the library's own vaek_forward mu of the rows it draws (posterior)."""
    from vae_training_amd.trainer import ReplicaJacobianMlp3
    name, rows, tol = "script1", 4, 1e-4
    c = _shape(name)
    # dataset seeds searched on the CPU (rows and latents emulated with oracle/philox.py, mu by the float64 encoder): in both modes every
    # hidden |pre| of every row is >= 2e-4 and no lambda_k / lambda_1 lies in [tol / 4, 4 tol]
    ms = [_Model(name, f, seed) for f, seed in zip(c.flats, (68, 48, 54))]
    jac = ReplicaJacobianMlp3(ms, rows=rows, at=at, rank_tol=tol)
    stats = jac.event()
    assert all(m._jacobian_draws == 1 and m.key == (3, 4) and m._latent_draws == 9 and m.dataset._draws == 5 for m in ms)
    trees = DC.trees_of(name)
    for r, (m, st) in enumerate(zip(ms, stats)):
        seed = m.dataset.key[0] ^ m.dataset.key[1]
        eng = _shape(name, rows).eng
        if at == "prior":
            z = eng.make_batch(2, None, 3, 3, 3, 0.0, rows, seed, step=1, tag=jac.Z_TAG, want_x=False)[1]
        else:
            x, z1, z2 = eng.make_batch(2, None, 3, 3, 3, 0.0, rows, seed, step=1, tag=jac.X_TAG)
            z = eng.forward(m.model.flat, x, z1, z2, sampling=False)[1]
        z = z.cpu().numpy()
        J, pres = DC.jacobian64(trees[r], z)
        lam, dg, rank, ng, _ = DC.row_records64(J, tol)
        min_pre = min(float(np.abs(p).min()) for p in pres)
        worst_dist = max(v[0] for k, v in TABLE.items() if k[0] == name)      # this shape's float32 forward
        print(at, r, "smallest |pre|", min_pre, "ranks", rank)
        assert min_pre >= DC.KINK_FACTOR * worst_dist, "a row of this event sits on a kink: the reference does not define it"
        bound = (GRAM_RTOL + 64 * c.L * 2.0 ** -53) * ng.mean()
        assert list(st) == list(jac.KEYS)
        assert (np.abs(st[jac.KEYS[0]] - lam.mean(0)) <= bound).all() and (np.abs(st[jac.KEYS[2]] - dg.mean(0)) <= bound).all()
        assert st[jac.KEYS[1]].tolist() == [rank.mean(), rank.min(), rank.max()]
        assert m.jacobian_spectra[-1] is st[jac.KEYS[0]] and len(m.jacobian_ranks) == 1 and len(m.latent_sensitivities) == 1


def test_run_py_writes_the_jacobian_keys(tmp_path):
    """Line 1 of sphere_vae_padding_expts.sh, 30 batches, --decoder_jacobian prior, in a fresh child process: the new keys' shapes."""
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "jac", "--dataset", "sphere", "--encoder_layer_sizes", "200|200|200", "--layer_sizes",
           "200|200|200", "-ow", "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30",
           "--decoder_jacobian", "prior"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Decoder Jacobian events: 1000 prior latent rows, rank threshold 0.0001 (vaek_mlp3_decoder_jacobian_replicas)" in r.stdout
    assert "Decoder Jacobian Rank (mean) |" in r.stdout, r.stdout[-1500:]
    f = dict(np.load(os.path.join(str(tmp_path), "data", "jac", "losses.npz"), allow_pickle=True))
    spec, rank, sens = (np.asarray(f[k], dtype=np.float64) for k in ("Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"))
    assert spec.shape == (1, 6) and rank.shape == (1, 3) and sens.shape == (1, 6), (spec.shape, rank.shape, sens.shape)
    assert np.isfinite(spec).all() and (np.diff(spec[0]) <= 0).all() and 0 <= rank[0, 1] <= rank[0, 0] <= rank[0, 2] <= 6
    assert abs(spec.sum() - sens.sum()) <= 1e-9 * sens.sum()
