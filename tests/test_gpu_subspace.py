"""-m gpu: eigenvectors of the covariance spectra and principal angles between two eigenbases (csrc/cov_spectrum.hip) --
vaek_cov_eigen_rows, vaek_eigen_event_replicas, vaek_subspace_angles -- and their callers, trainer.ReplicaSubspace and
`run.py --subspace`.

An eigen record is the spectrum record (bitwise vaek_cov_spectrum_rows') and then V row-major, column k the eigenvector of eigenvalue
k with its largest component positive.  The bounds E1 (orthonormality), E2 (residual), the angle bound against
scipy.linalg.subspace_angles and the Davis-Kahan bound of the planted events are tests/subspace_cases.py's; the input sets are
tests/cov_spectrum_cases.py's; tests/test_subspace_host.py holds a float64 restatement to the same bounds without a GPU."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import cov_spectrum_cases as K
from tests import subspace_cases as Z
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
X_TAG, Z_TAG = 5, 6
ROWS = 257
SAMPLE_EPS = -30.0


@functools.lru_cache(maxsize=None)
def _plain_engine(D):
    from vae_training_amd.engine import Engine
    e = Engine(100, D, 4, (), (), -1.0, False, False)
    assert e.supports_cov_spectrum() and e.cov_eigen_record_len == Z.eigen_len(D) and e.cov_spectrum_record_len == Z.spectrum_len(D)
    return e


def _rows_call(fn, ln, sets, pad_x=3, pad_out=5):
    """The records [n, ln] of float32 sets [n, rows, D] through ONE call of `fn` (cov_eigen_rows or cov_spectrum_rows), with strides
    larger than a set and a record and sentinels in front of, between and behind the records, which must survive."""
    n, rows, D = sets.shape
    xs = torch.full((n, rows * D + pad_x), SENT, dtype=torch.float32, device="cuda")
    xs[:, :rows * D] = torch.as_tensor(sets).reshape(n, rows * D).cuda()
    os_ = ln + pad_out
    buf = torch.full((3 + n * os_,), SENT, dtype=torch.float64, device="cuda")
    fn(xs, rows, buf.data_ptr() + 24, n=n, x_stride=rows * D + pad_x, out_stride=os_)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:3] == SENT), "doubles in front of the first record were written"
    recs = b[3:].reshape(n, os_)
    assert np.all(recs[:, ln:] == SENT), "doubles between two records were written"
    assert not np.any(recs[:, :ln] == SENT)
    return recs[:, :ln].copy()


@pytest.mark.parametrize("D", Z.DIMS)
def test_explicit_sets_eigenvectors(D):
    """Every (rows, variant) at this D: the first D^2 + 2 D + 4 doubles are bitwise vaek_cov_spectrum_rows' record; E1, E2, the sign rule
    and the order hold; set s of the n = 4 call is bitwise the n = 1 call on it; two runs are bitwise equal; sentinels survive."""
    eng = _plain_engine(D)
    ln, sl = Z.eigen_len(D), Z.spectrum_len(D)
    worst = [0.0, 0.0]
    for rows in Z.ROWS:
        sets = K.explicit_sets(D, rows)
        recs = _rows_call(eng.cov_eigen_rows, ln, sets)
        spec = _rows_call(eng.cov_spectrum_rows, sl, sets)
        assert np.array_equal(recs[:, :sl], spec), "the spectrum part is not vaek_cov_spectrum_rows' record"
        assert np.array_equal(recs, _rows_call(eng.cov_eigen_rows, ln, sets, pad_x=0, pad_out=0)), "two runs (and two strides) differ"
        one = _rows_call(eng.cov_eigen_rows, ln, sets[2:3])
        assert np.array_equal(one[0], recs[2]), "set 2 of n = 4 is not the n = 1 call on it"
        for v, rec in zip(K.VARIANTS, recs):
            u1, u2 = Z.check_eigen(f"D {D} rows {rows} {v}", Z.split_eigen_record(rec, D))
            worst = [max(worst[0], u1), max(worst[1], u2)]
    print(f"D {D}: worst E1 {worst[0]:.3f}, worst E2 {worst[1]:.3f} (units of the bounds)")


def _angles_call(eng, Vas, Vbs, ka, kb, pad=3):
    """The angle records [n, kb + 4] of n pairs of hand-made eigen records (V blocks Vas[p], Vbs[p]) through ONE vaek_subspace_angles
    call, padded strides and sentinels everywhere a record is not; a and b must come back unchanged."""
    n, D = len(Vas), Vas[0].shape[0]
    ln, ol = Z.eigen_len(D), kb + 4

    def stack(Vs):
        t = torch.full((n, ln + pad), SENT, dtype=torch.float64, device="cuda")
        t[:, :ln] = torch.as_tensor(np.stack([Z.eigen_record_of_basis(V) for V in Vs])).cuda()
        return t

    a, b = stack(Vas), stack(Vbs)
    a0, b0 = a.clone(), b.clone()
    buf = torch.full((2 + n * (ol + pad),), SENT, dtype=torch.float64, device="cuda")
    eng.subspace_angles(a, b, ka, kb, buf.data_ptr() + 16, n=n, a_stride=ln + pad, b_stride=ln + pad, out_stride=ol + pad)
    torch.cuda.synchronize()
    assert torch.equal(a, a0) and torch.equal(b, b0), "the eigen records were written"
    h = buf.cpu().numpy()
    assert np.all(h[:2] == SENT)
    recs = h[2:].reshape(n, ol + pad)
    assert np.all(recs[:, ol:] == SENT), "doubles between two angle records were written"
    assert not np.any(recs[:, :ol] == SENT)
    return recs[:, :ol].copy()


def test_angles_exact_cases_and_random_bases():
    """U = W: every sin^2 and [kb] are exactly 0; disjoint coordinate subspaces: every sin^2 is exactly 1 and [kb] = kb; random
    orthonormal bases against scipy."""
    for D, k in ((2, 1), (3, 2), (32, 5), (32, 32)):
        eng = _plain_engine(D)
        perm = np.eye(D)[:, np.random.default_rng(D).permutation(D)]
        for V in (np.eye(D), perm):
            r = Z.split_angle_record(_angles_call(eng, [V], [V], k, k)[0], k)
            assert r["sin2"].tolist() == [0.0] * k and r["frob2"] == 0.0 and r["sweeps"] == 0 and r["off"] == 0.0 and r["orth"] == 0.0, (D, k, r)
    for D, ka, kb in ((2, 1, 1), (3, 1, 1), (32, 3, 3), (32, 16, 16), (32, 20, 5)):
        eng = _plain_engine(D)
        flip = np.eye(D)[:, ::-1]                                        # its last kb columns are e_{kb-1} .. e_0: outside U where ka + kb <= D
        r = Z.split_angle_record(_angles_call(eng, [np.eye(D)], [flip], ka, kb)[0], kb)
        assert r["sin2"].tolist() == [1.0] * kb and r["frob2"] == float(kb) and r["sweeps"] == 0, (D, ka, kb, r)
    rng = np.random.default_rng(11)
    for D, ka, kb in ((7, 4, 3), (21, 21, 5), (32, 16, 16), (32, 31, 30)):
        eng = _plain_engine(D)
        Vas = [np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(2)]
        Vbs = [np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(2)]
        recs = _angles_call(eng, Vas, Vbs, ka, kb)
        for p in range(2):
            Z.check_angles(f"random D {D} ka {ka} kb {kb} pair {p}", recs[p], Vas[p], Vbs[p], ka, kb)


@pytest.mark.parametrize("D", Z.ANGLE_DIMS)
def test_angles_of_a_planted_plane_rotation(D):
    """One plane rotation by theta in {1e-3, 0.3, pi/2 - 1e-3}, the three thetas as the three pairs of ONE call, for every (ka, kb) of
    the cases module: against scipy within off_F(G) + 64 D 2^-53; pair p of n = 3 is bitwise the n = 1 call."""
    eng = _plain_engine(D)
    Vas = [np.eye(D)] * 3
    Vbs = [Z.rotated_basis(D, th) for th in Z.THETAS]
    for ka, kb in Z.angle_pairs(D):
        recs = _angles_call(eng, Vas, Vbs, ka, kb)
        assert np.array_equal(recs, _angles_call(eng, Vas, Vbs, ka, kb, pad=0)), "two runs (and two strides) differ"
        for p, th in enumerate(Z.THETAS):
            r = Z.check_angles(f"D {D} theta {th:.4f} ka {ka} kb {kb}", recs[p], Vas[p], Vbs[p], ka, kb)
            one = _angles_call(eng, Vas[p:p + 1], Vbs[p:p + 1], ka, kb)
            assert np.array_equal(one[0], recs[p]), f"pair {p} of n = 3 is not the n = 1 call"
            if (ka, kb) == (1, 1):
                assert abs(r["sin2"][0] - np.sin(th) ** 2) <= Z.angle_bound(D, r["off"]), (D, th, r)


PLANTED = {
    "linear_dd6_did3_pd6": dict(kind=0, D=12, L=8, dd=6, did=3, pad=6, tdv=True, eps=-1.0, k=3),
    "sphere_dd3_pd3": dict(kind=2, D=6, L=6, dd=3, did=3, pad=3, tdv=False, eps=-1.0, k=3),
}
R = 3
PLANTED_THETAS = ((1e-3, 0.3, 1.2), (0.05, 0.5, 1.0), (0.2, 0.7, np.pi / 2 - 1e-3))
PLANTED_SCALES = ((1.5, 1.0, 0.7), (0.8, 1.3, 1.0), (1.0, 0.6, 1.4))


class _PlantedCase:
    """R = 3 linear VAEs whose decoder has k non-zero rows spanning a subspace at known angles to the data's span (the other rows and
    the bias zero, sample_eps = -30, so the generated rows lie in that span up to e^-15), each with its own A, seeds and angles."""

    def __init__(self, name):
        from vae_training_amd.engine import Engine
        s = self.s = PLANTED[name]
        D, L, k = s["D"], s["L"], s["k"]
        self.engines = {b: Engine(b, D, L, (), (), s["eps"], s["tdv"], False) for b in (5, ROWS)}
        self.eng = e = self.engines[ROWS]
        assert e.supports_spectrum_event(s["kind"])
        self.len = e.cov_eigen_record_len
        cfg = O.Config(D, L, (), (), s["eps"], s["tdv"], None)
        rng = np.random.default_rng(5)
        alen = s["dd"] * s["did"] if s["kind"] == 0 else 0
        A = rng.standard_normal((R, alen)).astype(np.float32) if alen else None
        self.A = None if A is None else torch.as_tensor(A).cuda().contiguous()
        self.a_stride = alen
        flats = []
        for r in range(R):
            span = np.zeros((D, k))
            if s["kind"] == 0:
                span[:s["dd"]] = A[r].astype(np.float64).reshape(s["dd"], s["did"])          # the data is (A X^T)^T, zero padding
            else:
                span[:k] = np.eye(k)                                                          # the unit sphere of the first dd coordinates
            full = np.linalg.qr(np.concatenate([span, rng.standard_normal((D, D - k))], axis=1))[0]
            Q, N = full[:, :k], full[:, k:2 * k]
            p = O.init_params(cfg, seed=r)
            p["Decoder/FC0/kernel"] = Z.planted_decoder(Q, N, PLANTED_THETAS[r], PLANTED_SCALES[r], L)
            p["Decoder/FC0/bias"] = np.zeros(D)
            flats.append(O.flatten(cfg, p, np.float32))
        self.P, self.ss, self.os = e.P, e.P + 5, 2 * self.len + 3
        self.params = torch.full((R, self.ss), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :e.P] = torch.as_tensor(np.stack(flats)).cuda()
        self.x_seeds, self.z_seeds = [77, 2 ** 63 + 5, 1000003], [2 ** 64 - 3, 991, 31337]
        self.x_steps, self.z_steps = [1, 4, 2 ** 31 + 7], [3, 2 ** 32 - 1, 2]
        self.tabs = (_i64(self.x_seeds), _i32(self.x_steps), _i64(self.z_seeds), _i32(self.z_steps),
                     torch.full((R,), SAMPLE_EPS, dtype=torch.float32, device="cuda"))

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float64, device="cuda")

    def call(self, out, rs=None, eng=None, rows=ROWS, **kw):
        s = self.s
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, kind=s["kind"], A=None if self.A is None else self.A[sl], dd=s["dd"], did=s["did"],
                 pad=s["pad"], var_added=0.0, x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl],
                 z_steps=self.tabs[3][sl], sample_eps=self.tabs[4][sl], out=out, a_stride=self.a_stride, x_tag=X_TAG, z_tag=Z_TAG)
        a.update(kw)
        (eng or self.eng).eigen_event_replicas(**a)

    def records(self, rs=None, eng=None):
        n = R if rs is None else len(range(*rs.indices(R)))
        out = self.out(n)
        self.call(out, rs=rs, eng=eng)
        torch.cuda.synchronize()
        assert bool((out[:, 2 * self.len:] == SENT).all()), "doubles between two replicas' records were written"
        assert not bool((out[:, :2 * self.len] == SENT).any())
        return out

    def angles(self, out, n=R):
        k = self.s["k"]
        ang = torch.full((n, k + 4), SENT, dtype=torch.float64, device="cuda")
        self.eng.subspace_angles(out, out[:, self.len:], k, k, ang, n=n, a_stride=self.os, b_stride=self.os)
        return ang

    def host_rows(self, r):
        """(fake, real) rows of replica r by the host route on the same draws: vaek_make_batch and vaek_forward."""
        s, e = self.s, self.eng
        Ar = None if self.A is None else self.A[r].clone()
        x = e.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], 0.0, ROWS, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG, want_z=False)[0]
        _, z1, z2 = e.make_batch(0, None, 1, 1, s["D"] - 1, 0.0, ROWS, self.z_seeds[r], step=self.z_steps[r], tag=Z_TAG, want_x=False)
        fake, _ = e.forward(self.params[r, :self.P].contiguous(), None, z1, z2, sampling=True, eps=SAMPLE_EPS, want_mu=False)
        torch.cuda.synchronize()
        return fake.cpu().numpy(), x.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _planted(name):
    return _PlantedCase(name)


@pytest.mark.parametrize("name", list(PLANTED))
def test_fused_event_on_a_planted_subspace(name):
    """The real record is bitwise cov_eigen_rows on vaek_make_batch's x; replica r is bitwise the n = 1 call; the result does not depend
    on ctx.batch (5 and 257); two runs are bitwise equal; E1 / E2 on both sides; the angles against the host route on the same draws
    (vaek_make_batch, vaek_forward, numpy.cov, eigh, scipy.linalg.subspace_angles) within the Davis-Kahan bound the test computes from
    the records themselves, with gap_ref >= 1e-3 lambda_max asserted on both sides of every replica."""
    from scipy.linalg import subspace_angles
    c = _planted(name)
    s, D, k, ln = c.s, c.s["D"], c.s["k"], c.len
    before = c.params.clone()
    a = c.records()
    assert torch.equal(a, c.records()), "two runs differ"
    assert torch.equal(a, c.records(eng=c.engines[5])), "the event depends on ctx.batch"
    ang = c.angles(a)
    torch.cuda.synchronize()
    got, gang = a.cpu().numpy(), ang.cpu().numpy()
    for r in range(R):
        one = c.records(rs=slice(r, r + 1))
        assert torch.equal(one[0], a[r]), f"replica {r} of n = 3 differs from its n = 1 call"
        assert torch.equal(c.angles(one, n=1)[0], ang[r]), f"pair {r} of n = 3 differs from its n = 1 call"
        fake, x = c.host_rows(r)
        real = _rows_call(c.eng.cov_eigen_rows, ln, x[None])[0]
        assert np.array_equal(real, got[r, ln:2 * ln]), f"replica {r}: the real record is not vaek_cov_eigen_rows on make_batch's x"
        assert not x[:, D - s["pad"]:].any()
        sides = [Z.split_eigen_record(got[r, :ln], D), Z.split_eigen_record(real, D)]
        dk, spans = [], []
        for side, rec, rows in (("fake", sides[0], fake), ("real", sides[1], x)):
            Z.check_eigen(f"{name} replica {r} {side} side", rec)
            C_ref = np.cov(rows.astype(np.float64).T, ddof=1).reshape(D, D)
            dk.append(Z.davis_kahan(f"{name} replica {r} {side}", rec["cov"], C_ref, k))
            spans.append(np.linalg.eigh(C_ref)[1][:, D - k:])
        ar = Z.split_angle_record(gang[r], k)
        sin_dev = np.sqrt(np.clip(ar["sin2"], 0.0, 1.0))
        sin_ref = np.sort(np.sin(subspace_angles(spans[0], spans[1])))
        bound = 2.0 * max(dk) + 1e-12
        err = float(np.max(np.abs(sin_dev - sin_ref)))
        planted = float(np.max(np.abs(sin_dev - np.sin(np.sort(PLANTED_THETAS[r])))))
        print(f"{name} replica {r}: |d sin theta| {err:.2e} = {err / bound:.3f} of the Davis-Kahan bound {bound:.2e}; against the planted "
              f"angles {planted:.2e}; angles {np.arcsin(sin_dev)}; sweeps {int(ar['sweeps'])}, off_F {ar['off']:.1e}, orth {ar['orth']:.1e}")
        assert err <= bound, (name, r, err, bound)
        assert abs(ar["frob2"] - np.sum(ar["sin2"])) <= Z.angle_bound(D, ar["off"])
        assert ar["orth"] <= Z.e1_bound(D, max(sides[0]["sweeps"], sides[1]["sweeps"])) * 2
        # float32 rows: each covariance moves by at most about 4 * 2^-24 |C|, and |C| / gap <= 1e3 is asserted above
        assert planted <= 2.0 * 4.0 * 2.0 ** -24 / Z.GAP_MIN, (name, r, planted)
    assert torch.equal(c.params, before), "params were written"


@pytest.mark.parametrize("L", [5, 7])
def test_real_side_equals_make_batch_rows_off_the_square_matrix(L):
    """The first check of test_fused_event_on_a_planted_subspace, bitwise, where the event's own draw of the real rows leaves the line
    the planted cases are on: a 5 x 9 mixing matrix (the A[d * did + k] stride), dataset noise whose normals start at Philox block 3,
    latent streams with L % 4 = 1 and 3."""
    from vae_training_amd.engine import Engine
    n, D, dd, did, pad, var = 3, 7, 5, 9, 2, 0.25
    eng = Engine(ROWS, D, L, (), (), -1.0, True, False)
    assert eng.supports_spectrum_event(0)
    ln = eng.cov_eigen_record_len
    g = torch.Generator().manual_seed(17)
    params = (torch.randn(n, eng.P, generator=g) * 0.3).cuda().contiguous()
    A = torch.randn(n, dd * did, generator=g).cuda().contiguous()
    x_seeds, x_steps = [77, 2 ** 63 + 5, 1000003], [1, 4, 2 ** 31 + 7]
    out = torch.full((n, 2 * ln + 3), SENT, dtype=torch.float64, device="cuda")
    eng.eigen_event_replicas(params=params, rows=ROWS, kind=0, A=A, dd=dd, did=did, pad=pad, var_added=var, x_seeds=_i64(x_seeds),
                             x_steps=_i32(x_steps), z_seeds=_i64([2 ** 64 - 3, 991, 31337]), z_steps=_i32([3, 2 ** 32 - 1, 2]),
                             sample_eps=torch.full((n,), -1.0, dtype=torch.float32, device="cuda"), out=out, a_stride=dd * did,
                             x_tag=X_TAG, z_tag=Z_TAG)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:, 2 * ln:] == SENT) and np.isfinite(got[:, :2 * ln]).all()
    for r in range(n):
        x = eng.make_batch(0, A[r].clone(), dd, did, pad, var, ROWS, x_seeds[r], step=x_steps[r], tag=X_TAG, want_z=False)[0].cpu().numpy()
        assert x[:, dd:].all()                                                   # noise reaches the padding columns
        real = _rows_call(eng.cov_eigen_rows, ln, x[None])[0]
        assert np.array_equal(real, got[r, ln:2 * ln]), f"replica {r}: the real record is not vaek_cov_eigen_rows on make_batch's x"


def test_refusals_leave_the_buffers_untouched():
    """Every refusal of the three entry points returns VAEK_ERR_INVALID with a message naming the function and leaves the sentinel
    buffers unchanged; exactly one profile record per launch, under the new labels."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c = _planted("linear_dd6_did3_pd6")
    eng, D, ln, k = c.eng, 12, c.len, 3
    x = torch.as_tensor(K.explicit_sets(D, 37)).cuda().contiguous()

    def rows_refused(why, e=eng, **kw):
        out = torch.full((4, ln + 2), SENT, dtype=torch.float64, device="cuda")
        a = dict(x=x, rows=37, out=out, n=4, x_stride=37 * D, out_stride=ln + 2)
        a.update(kw)
        with pytest.raises(VaekError) as ei:
            e.cov_eigen_rows(**a)
        assert ei.value.code == -1 and "vaek_cov_eigen_rows" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), why

    rows_refused("x NULL", x=None)
    rows_refused("out NULL", out=None)
    rows_refused("n = 0", n=0)
    rows_refused("n over the cap", n=eng.cov_spectrum_max_sets + 1)
    rows_refused("rows = 1", rows=1)
    rows_refused("rows over the cap", rows=4097)
    rows_refused("x_stride < 0", x_stride=-1)
    rows_refused("0 < x_stride < rows * D", x_stride=37 * D - 1)
    rows_refused("out_stride < the eigen record length", out_stride=ln - 1)
    rows_refused("out_stride = the spectrum record length", out_stride=eng.cov_spectrum_record_len)
    keep = torch.full((4, ln + 2), SENT, dtype=torch.float64, device="cuda")
    rows_refused("out misaligned", out=keep.data_ptr() + 4)
    assert bool((keep == SENT).all())
    wide = Engine(100, 33, 6, (), (), -1.0, True, False)
    rows_refused("data_dim 33", e=wide)

    def event_refused(why, **kw):
        out = c.out()
        before = c.params.clone()
        with pytest.raises(VaekError) as ei:
            c.call(out, **kw)
        assert ei.value.code == -1 and "vaek_eigen_event_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(c.params, before), why

    mlp3 = Engine(100, 12, 8, (200, 200, 200), (200, 200, 200), -1.0, True, False)
    bf16 = Engine(100, 12, 8, (), (), -1.0, True, False, dtype="bf16")
    event_refused("mlp3", eng=mlp3)
    event_refused("bf16", eng=bf16)
    event_refused("struct_size", struct_size=12)
    event_refused("n = 0", n=0)
    event_refused("n over the cap", n=eng.train_loop_max_replicas + 1)
    event_refused("rows = 1", rows=1)
    event_refused("rows over the cap", rows=4097)
    for name in ("x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps"):
        event_refused(name + " NULL", **{name: None})
    event_refused("state_stride < P", state_stride=c.P - 1)
    event_refused("out_stride < two eigen records", out_stride=2 * ln - 1)
    event_refused("out_stride = two spectrum records", out_stride=2 * eng.cov_spectrum_record_len)
    o = c.out()
    with pytest.raises(VaekError) as ei:
        c.call(o.data_ptr() + 4, out_stride=c.os)
    assert ei.value.code == -1 and "aligned" in str(ei.value) and bool((o == SENT).all())
    with pytest.raises(VaekError) as ei:
        c.call(None, out_stride=c.os)
    assert "vaek_eigen_event_replicas" in str(ei.value)
    event_refused("a_stride < 0", a_stride=-1)
    event_refused("A NULL, kind 0", A=None)
    event_refused("did = 17", did=17)
    event_refused("kind 3", kind=3)
    event_refused("x_tag = 2^30", x_tag=2 ** 30)
    event_refused("z_tag = 2^30", z_tag=2 ** 30)
    event_refused("dataset dimension != data_dim", pad=7)

    recs = c.records()
    ol = k + 4

    def angles_refused(why, e=eng, **kw):
        out = torch.full((R, ol + 2), SENT, dtype=torch.float64, device="cuda")
        a = dict(a=recs, b=recs[:, ln:], ka=k, kb=k, out=out, n=R, a_stride=c.os, b_stride=c.os, out_stride=ol + 2)
        a.update(kw)
        before = recs.clone()
        with pytest.raises(VaekError) as ei:
            e.subspace_angles(**a)
        assert ei.value.code == -1 and "vaek_subspace_angles" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(recs, before), why

    angles_refused("a NULL", a=None)
    angles_refused("b NULL", b=None)
    angles_refused("out NULL", out=None)
    angles_refused("n = 0", n=0)
    angles_refused("n over the cap", n=eng.cov_spectrum_max_sets + 1)
    angles_refused("kb = 0", kb=0)
    angles_refused("kb > ka", ka=2, kb=3)
    angles_refused("ka > D", ka=D + 1)
    angles_refused("ka = 0", ka=0, kb=0)
    angles_refused("a_stride below the eigen record", a_stride=ln - 1)
    angles_refused("b_stride below the eigen record", b_stride=ln - 1)
    angles_refused("a_stride = 0", a_stride=0)
    angles_refused("out_stride < kb + 4", out_stride=ol - 1)
    angles_refused("a misaligned", a=recs.data_ptr() + 4)
    angles_refused("b misaligned", b=recs.data_ptr() + 8 * ln + 4)
    keep = torch.full((R, ol + 2), SENT, dtype=torch.float64, device="cuda")
    angles_refused("out misaligned", out=keep.data_ptr() + 4)
    assert bool((keep == SENT).all())
    angles_refused("data_dim 33", e=wide)

    eng.profile_begin(16)
    c.call(c.out())
    eng.cov_eigen_rows(x, 37, torch.empty(4, ln, dtype=torch.float64, device="cuda"))
    c.angles(recs)
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert sorted(rep) == ["cov_eigen_rows", "eigen_event_replicas", "subspace_angles"], rep
    assert all(v["count"] == 1 for v in rep.values()), rep


def test_captured_replay_of_event_and_angles():
    """The event and the angles call on its records, captured into one graph and replayed twice = the eager run, bitwise."""
    c = _planted("sphere_dd3_pd3")
    k = c.s["k"]
    eager = c.records()
    eager_ang = c.angles(eager)
    torch.cuda.synchronize()
    out = c.out()
    ang = torch.full((R, k + 4), SENT, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.call(out)
            c.eng.subspace_angles(out, out[:, c.len:], k, k, ang, n=R, a_stride=c.os, b_stride=c.os)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ang == SENT).all())                       # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(ang, eager_ang)
        out[:, :2 * c.len] = 0.0
        ang.zero_()


def _model(engine, flat, seed, spec, eps, name):
    ds = types.SimpleNamespace(device_spec=lambda: spec, key=(seed, 2))
    opt = types.SimpleNamespace(global_batch=100)
    return types.SimpleNamespace(dataset=ds, batch_size=100, optimizer=opt, key=(3, 4), print_batch_size=1000, current_epsilon=eps,
                                 gt_eigen=[], ht_eigen=[], dirname=name,
                                 model=types.SimpleNamespace(module=types.SimpleNamespace(engine=engine), flat=flat))


def test_replica_subspace_on_three_linear_models_equals_three_single_runs():
    """trainer.ReplicaSubspace on the three planted linear models: ONE eigen_event_replicas call, ONE subspace_angles call; every
    model's four stats are bitwise those of ReplicaSubspace([that model]) under the same counter; k defaults to min(dd, did) = 3."""
    from vae_training_amd.engine import Engine
    from vae_training_amd.trainer import ReplicaSubspace
    c = _planted("linear_dd6_did3_pd6")
    s = c.s
    engines = {}

    def engine(B, gb=0):
        if B not in engines:
            engines[B] = Engine(B, s["D"], s["L"], (), (), s["eps"], s["tdv"], False)
        return engines[B]

    def models():
        return [_model(engine, c.params[r, :c.P].clone(), 69 + r, (0, c.A[r].clone(), s["dd"], s["did"], s["pad"], 0.0), SAMPLE_EPS, f"lin{r}")
                for r in range(R)]

    ms = models()
    sp = ReplicaSubspace(ms, rows=ROWS)
    assert sp.fused and sp.k == 3 and sp.VEC
    sp.eng.profile_begin(16)
    stats = sp.event()
    rep = sp.eng.profile_report()
    assert sorted(rep) == ["eigen_event_replicas", "subspace_angles"] and all(v["count"] == 1 for v in rep.values()), rep
    solo = models()
    for r in range(R):
        one = ReplicaSubspace([solo[r]], rows=ROWS).event()[0]
        assert list(one) == list(stats[r]) == ["learnt eigenvalue", "ground truth eigenvalue", "Principal Angles", "Subspace Distance"]
        for key in one:
            assert np.array_equal(np.asarray(one[key]), np.asarray(stats[r][key])), (r, key)
        want = np.sort(PLANTED_THETAS[r])
        assert np.max(np.abs(np.sin(stats[r]["Principal Angles"]) - np.sin(want))) <= 2.0 * 4.0 * 2.0 ** -24 / Z.GAP_MIN
        assert abs(stats[r]["Subspace Distance"] - np.sqrt(np.sum(np.sin(stats[r]["Principal Angles"]) ** 2))) <= 1e-9
        assert ms[r]._spectrum_draws == 1 and ms[r].key == (3, 4) and len(ms[r].principal_angles) == len(ms[r].ht_eigen) == 1


def test_host_route_on_one_mlp3_model_matches_numpy_and_scipy():
    """ReplicaSubspace on one three-hidden-layer MLP model (sphere rows): make_batch + forward, ONE cov_eigen_rows call with n = 2, one
    angles call; the angles against numpy.cov / eigh / scipy on the stack's own rows within the Davis-Kahan bound."""
    from scipy.linalg import subspace_angles
    from vae_training_amd.engine import Engine
    from vae_training_amd.trainer import ReplicaSubspace
    cfg = O.Config(6, 6, (200, 200, 200), (200, 200, 200), -3.0, True, None)
    engines = {}

    def engine(B, gb=0):
        if B not in engines:
            engines[B] = Engine(B, 6, 6, (200, 200, 200), (200, 200, 200), -3.0, True, False)
        return engines[B]

    flat = torch.as_tensor(O.flatten(cfg, O.init_params(cfg, seed=0), np.float32)).cuda()
    m = _model(engine, flat, 69, (2, None, 3, 3, 3, 0.0), 2.0, "mlp3_69")             # eps = 2: the sampling noise spreads the fake rows
    sp = ReplicaSubspace([m], rows=ROWS)
    assert not sp.fused and sp.k == 3 and sp.eng.step_path == "mlp3"
    sp.eng.profile_begin(16)
    st = sp.event()[0]
    rep = sp.eng.profile_report()
    assert rep["cov_eigen_rows"]["count"] == 1 and rep["subspace_angles"]["count"] == 1, rep
    recs, stack = sp.out.cpu().numpy(), sp.stack.cpu().numpy()
    dk, spans = [], []
    for side in range(2):
        rec = Z.split_eigen_record(recs[side], 6)
        Z.check_eigen(f"mlp3 side {side}", rec)
        K.check_t1(f"mlp3 side {side}", rec, stack[side])
        C_ref = np.cov(stack[side].astype(np.float64).T, ddof=1).reshape(6, 6)
        dk.append(Z.davis_kahan(f"mlp3 side {side}", rec["cov"], C_ref, 3))
        spans.append(np.linalg.eigh(C_ref)[1][:, 3:])
        assert np.array_equal(st[sp.KEYS[side]], rec["eig"])
    sin_ref = np.sort(np.sin(subspace_angles(spans[0], spans[1])))
    bound = 2.0 * max(dk) + 1e-12
    err = float(np.max(np.abs(np.sin(st["Principal Angles"]) - sin_ref)))
    print(f"mlp3 host route: |d sin theta| {err:.2e} = {err / bound:.3f} of the Davis-Kahan bound {bound:.2e}; angles {st['Principal Angles']}")
    assert err <= bound, (err, bound)
    assert m._spectrum_draws == 1 and m.key == (3, 4)


def _run_py(tmp_path, name, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", "sigmoid", "--encoder_layer_sizes", "", "--layer_sizes", "", "-ow",
           "--latent_dim", "6", "--padding_dim", "3", "-dd", "3", "--epsilon", "-3", "-tdv", "--num_batches", "30", *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)


def _losses(tmp_path, name):
    return dict(np.load(os.path.join(str(tmp_path), "data", name, "losses.npz"), allow_pickle=True))


def test_run_py_subspace_in_a_sweep(tmp_path):
    """run.py --subspace auto --eigenvalues --sweep_dataset_seeds 69,24 in a fresh process: losses.npz has the two new keys, and its
    EigenValues is bitwise that of the same run without --subspace; everything else is bitwise the same too."""
    r = _run_py(tmp_path, "sub", "--subspace", "auto", "--eigenvalues", "--sweep_dataset_seeds", "69,24")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Subspace events: the 4 leading eigenvectors of 1000 generated and 1000 real rows per model (vaek_eigen_event_replicas, " \
           "vaek_subspace_angles)" in r.stdout
    p = _run_py(tmp_path, "plain", "--eigenvalues", "--sweep_dataset_seeds", "69,24")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Subspace events" not in p.stdout
    new = {"Subspace Distance", "Principal Angles"}
    for seed in (69, 24):
        got, plain = _losses(tmp_path, f"sub_ds{seed}"), _losses(tmp_path, f"plain_ds{seed}")
        assert new <= set(got) and not new & set(plain) and sorted(set(got) - new) == sorted(plain)
        ang = np.asarray(got["Principal Angles"], dtype=np.float64)
        dist = np.asarray(got["Subspace Distance"], dtype=np.float64)
        assert ang.shape == (1, 4) and dist.shape == (1,), (ang.shape, dist.shape)          # one event (step 0) x k = dd + 1 = 4
        assert np.all(np.diff(ang[0]) >= 0) and np.all(ang >= 0) and np.all(ang <= np.pi / 2)
        assert abs(dist[0] - np.sqrt(np.sum(np.sin(ang[0]) ** 2))) <= 1e-9
        for key in plain:
            a, b = np.asarray(plain[key]), np.asarray(got[key])
            assert a.shape == b.shape and (a.dtype == object or a.tobytes() == b.tobytes()), key
        assert np.asarray(got["EigenValues"], dtype=np.float64).tobytes() == np.asarray(plain["EigenValues"], dtype=np.float64).tobytes()


def test_run_py_subspace_alone_on_one_model(tmp_path):
    """run.py --subspace 2 without --eigenvalues on one model: the two new keys with K = 2 angles per event and no eigenvalue key."""
    r = _run_py(tmp_path, "one", "--subspace", "2")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Subspace events: 1000 generated and 1000 real rows" in r.stdout and "Eigenvalue events" not in r.stdout
    got = _losses(tmp_path, "one")
    ang = np.asarray(got["Principal Angles"], dtype=np.float64)
    dist = np.asarray(got["Subspace Distance"], dtype=np.float64)
    assert ang.shape == (1, 2) and dist.shape == (1,), (ang.shape, dist.shape)
    assert np.all(np.diff(ang[0]) >= 0) and np.all(ang >= 0) and np.all(ang <= np.pi / 2)
    assert abs(dist[0] - np.sqrt(np.sum(np.sin(ang[0]) ** 2))) <= 1e-9
    assert not {"EigenValues", "learnt eigenvalue", "ground truth eigenvalue"} & set(got)
    r = _run_py(tmp_path, "bad", "--subspace", "8")
    assert r.returncode != 0 and "--subspace 8 needs" in r.stderr and "data_dim: 7" in r.stderr, r.stderr[-1500:]
    assert "Batch |" not in r.stdout
