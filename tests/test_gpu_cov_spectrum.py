"""-m gpu: the covariance spectra of csrc/cov_spectrum.hip -- vaek_cov_spectrum_rows (explicit rows), vaek_spectrum_event_replicas
(the fused event of N linear VAEs) -- and their callers, trainer.ReplicaSpectrum and `run.py --eigenvalues`.

A record is D eigenvalues (ascending), D column means, the D x D covariance, then sweeps run, final off_F, |C|_F, rows.  The input
sets and the bounds T1 (C and m against numpy.cov on the identical float32 rows) and T2 (eigenvalues against LAPACK on the DEVICE's
own C) are tests/cov_spectrum_cases.py's; tests/test_cov_spectrum_host.py holds a float64 restatement of the algorithm to the same
bounds on the same sets without a GPU.  The fused event is checked against itself BITWISE (properties (i) .. (iv) of include/vaek.h)
and, on its fake side, against a float64 NumPy decode of the device's own latents:
  T3  |dC_ij| <= 1e-5 max_k(C_kk + m_k^2) (the project's ELBO contract: the decode is float32), and
      |d lambda_k| <= |C_dev - C_oracle|_2 + T2 (Weyl), the norm computed here.
The event shapes are the six of sigmoid_vae_padding_expts.sh (two decoders), two of seed_linpadding_expts.sh (D = 12 and D = 20,
L = 20) and sphere rows on a linear VAE (no epsilon leaf); N = 1, 3 and 5 replicas."""
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
from tests.gpu_util import _i32, _i64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0
X_TAG, Z_TAG = 5, 6
R = 5
T3 = 1e-5
SHAPES = {
    "sigmoid_dd3_pd3": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=7, L=6, dd=3, did=1, pad=3, var=0.0),
    "sigmoid_dd3_pd13": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=17, L=8, dd=3, did=1, pad=13, var=0.0),
    "sigmoid_dd5_pd16": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=22, L=16, dd=5, did=1, pad=16, var=0.0),
    "sigmoid_dd5_pd5": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=11, L=10, dd=5, did=1, pad=5, var=0.0),
    "sigmoid_dd7_pd7": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=15, L=13, dd=7, did=1, pad=7, var=0.0),
    "sigmoid_dd7_pd20": dict(sig=True, tdv=True, eps=-3.0, kind=1, D=28, L=24, dd=7, did=1, pad=20, var=0.0),
    "linear_12": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=12, L=20, dd=3, did=3, pad=9, var=0.0),
    "linear_20": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=20, L=20, dd=3, did=3, pad=17, var=0.0),
    "sphere": dict(sig=False, tdv=False, eps=-1.0, kind=2, D=6, L=6, dd=3, did=3, pad=3, var=0.0),
}
# a mixing matrix that is not square, did > 4 with noise (noise normals from Philox block 3), L % 4 = 1 and 3: property (iii) alone
OFF_SQUARE = {
    "did9_L5": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=7, L=5, dd=5, did=9, pad=2, var=0.25),
    "did9_L7": dict(sig=False, tdv=True, eps=-1.0, kind=0, D=7, L=7, dd=5, did=9, pad=2, var=0.25),
}
EVENT_ROWS = 1000


@functools.lru_cache(maxsize=None)
def _plain_engine(D):
    from vae_training_amd.engine import Engine
    e = Engine(100, D, 4, (), (), -1.0, False, False)
    assert e.supports_cov_spectrum() and e.cov_spectrum_record_len == D * D + 2 * D + 4
    return e


def _rows_call(eng, sets, pad_x=3, pad_out=5):
    """The records [n, len] (float64 NumPy) of float32 sets [n, rows, D] through ONE vaek_cov_spectrum_rows call, with strides larger
    than a set and a record and sentinels in front of, between and behind the records, which must survive."""
    n, rows, D = sets.shape
    ln = eng.cov_spectrum_record_len
    xs = torch.full((n, rows * D + pad_x), SENT, dtype=torch.float32, device="cuda")
    xs[:, :rows * D] = torch.as_tensor(sets).reshape(n, rows * D).cuda()
    os_ = ln + pad_out
    buf = torch.full((3 + n * os_,), SENT, dtype=torch.float64, device="cuda")
    eng.cov_spectrum_rows(xs, rows, buf.data_ptr() + 24, n=n, x_stride=rows * D + pad_x, out_stride=os_)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:3] == SENT), "doubles in front of the first record were written"
    recs = b[3:].reshape(n, os_)
    assert np.all(recs[:, ln:] == SENT), "doubles between two records were written"
    assert not np.any(recs[:, :ln] == SENT)
    return recs[:, :ln].copy()


@pytest.mark.parametrize("D", K.DIMS)
def test_explicit_sets_meet_t1_and_t2(D):
    """Every (rows, variant) at this D: T1, T2, sweeps below the cap; set s of the n = 4 call is bitwise the n = 1 call on it; two runs
    are bitwise equal."""
    eng = _plain_engine(D)
    worst = dict(c=0.0, m=0.0, e=0.0, sweeps=0)
    for rows in K.ROWS:
        sets = K.explicit_sets(D, rows)
        recs = _rows_call(eng, sets)
        assert np.array_equal(recs, _rows_call(eng, sets, pad_x=0, pad_out=0)), "two runs (and two strides) differ"
        one = _rows_call(eng, sets[2:3])
        assert np.array_equal(one[0], recs[2]), "set 2 of n = 4 is not the n = 1 call on it"
        for v, rec, x in zip(K.VARIANTS, recs, sets):
            r = K.split_record(rec, D)
            what = f"D {D} rows {rows} {v}"
            uc, um = K.check_t1(what, r, x)
            sweeps, ue = K.check_t2(what, r)
            worst = dict(c=max(worst["c"], uc), m=max(worst["m"], um), e=max(worst["e"], ue), sweeps=max(worst["sweeps"], sweeps))
            if v == "const":
                assert r["cov"][0, 0] == 0.0 and r["mean"][0] == 3.0, what           # a constant column: exact sums, an exactly-zero variance
    print(f"D {D}: worst T1 C {worst['c']:.3f} m {worst['m']:.3f}, worst T2 {worst['e']:.3f} (units of the bounds), most sweeps {worst['sweeps']}")


@pytest.mark.parametrize("name", list(K.PADDED))
def test_padded_rows_from_make_batch(name):
    """Rows vaek_make_batch writes, with exactly-zero padding columns: T1, T2, and `pad` eigenvalues that are zero up to T2."""
    s = K.PADDED[name]
    eng = _plain_engine(s["D"])
    alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
    A = torch.as_tensor(np.random.default_rng(3).standard_normal(alen), dtype=torch.float32).cuda() if alen else None
    for rows in K.PADDED_ROWS:
        x = eng.make_batch(s["kind"], A, s["dd"], s["did"], s["pad"], s["var"], rows, 1234567, step=3, tag=X_TAG, want_z=False)[0]
        xn = x.cpu().numpy()
        assert xn.shape == (rows, s["D"]) and not xn[:, s["D"] - s["pad"]:].any()
        r = K.split_record(_rows_call(eng, xn[None])[0], s["D"])
        what = f"{name} rows {rows}"
        K.check_t1(what, r, xn)
        K.check_t2(what, r)
        assert np.all(np.abs(r["eig"][:s["pad"]]) <= K.t2_bound(s["D"], r["off"], r["norm"])), (what, r["eig"])
        assert not r["cov"][s["D"] - s["pad"]:].any()


class _EventCase:
    """One engine and R replicas with distinct parameters, seeds (one above 2^63), steps (one above 2^31), sampling eps and dataset
    matrices, in a parameter stack whose stride exceeds P by 5 sentinel floats; records go to a sentinel-filled [R, 2 len + 3] buffer."""

    def __init__(self, name, batch=100):
        from vae_training_amd.engine import Engine
        s = self.s = SHAPES[name] if name in SHAPES else OFF_SQUARE[name]
        self.eng = e = Engine(batch, s["D"], s["L"], (), (), s["eps"], s["tdv"], s["sig"])
        assert e.supports_spectrum_event(s["kind"]) and e.supports_cov_spectrum()
        self.len = e.cov_spectrum_record_len
        assert self.len == s["D"] ** 2 + 2 * s["D"] + 4
        self.cfg = cfg = O.Config(s["D"], s["L"], (), (), s["eps"], s["tdv"], "sigmoid" if s["sig"] else None)
        rng = np.random.default_rng(41)
        alen = {0: s["dd"] * s["did"], 1: s["dd"], 2: 0}[s["kind"]]
        self.A = torch.as_tensor(rng.standard_normal((R, alen)), dtype=torch.float32).cuda().contiguous() if alen else None
        self.a_stride = alen
        self.P, self.ss, self.os = e.P, e.P + 5, 2 * self.len + 3
        flats = []
        for r in range(R):
            p = {k: v + 0.05 * rng.standard_normal(v.shape) for k, v in O.init_params(cfg, seed=r).items()}
            flats.append(O.flatten(cfg, p, np.float32))
        self.params = torch.full((R, self.ss), SENT, dtype=torch.float32, device="cuda")
        self.params[:, :e.P] = torch.as_tensor(np.stack(flats)).cuda()
        self.trees = [O.unflatten(cfg, f.astype(np.float64)) for f in flats]
        self.x_seeds, self.z_seeds = [77, 2 ** 63 + 5, 1000003, 12, 2 ** 64 - 9], [2 ** 64 - 3, 991, 31337, 5, 8]
        self.x_steps, self.z_steps = [1, 4, 2 ** 31 + 7, 9, 2], [3, 2 ** 32 - 1, 2, 1, 77]
        self.sample_eps = [-3.0, -1.0, 0.5, -2.0, 0.0]
        self.tabs = (_i64(self.x_seeds), _i32(self.x_steps), _i64(self.z_seeds), _i32(self.z_steps),
                     torch.tensor(self.sample_eps, dtype=torch.float32, device="cuda"))

    def out(self, n=R):
        return torch.full((n, self.os), SENT, dtype=torch.float64, device="cuda")

    def call(self, out, rows, rs=None, **kw):
        s = self.s
        sl = slice(None) if rs is None else rs
        a = dict(params=self.params[sl], rows=rows, kind=s["kind"], A=None if self.A is None else self.A[sl], dd=s["dd"], did=s["did"],
                 pad=s["pad"], var_added=s["var"], x_seeds=self.tabs[0][sl], x_steps=self.tabs[1][sl], z_seeds=self.tabs[2][sl],
                 z_steps=self.tabs[3][sl], sample_eps=self.tabs[4][sl], out=out, a_stride=self.a_stride, x_tag=X_TAG, z_tag=Z_TAG)
        a.update(kw)
        eng = a.pop("eng", self.eng)
        eng.spectrum_event_replicas(**a)

    def records(self, rows, rs=None, **kw):
        n = R if rs is None else len(range(*rs.indices(R)))
        out = self.out(n)
        self.call(out, rows, rs=rs, **kw)
        torch.cuda.synchronize()
        assert bool((out[:, 2 * self.len:] == SENT).all()), "doubles between two replicas' records were written"
        assert not bool((out[:, :2 * self.len] == SENT).any())
        return out

    def x_rows(self, r, rows):
        s = self.s
        Ar = None if self.A is None else self.A[r].clone()
        return self.eng.make_batch(s["kind"], Ar, s["dd"], s["did"], s["pad"], s["var"], rows, self.x_seeds[r], step=self.x_steps[r], tag=X_TAG,
                                   want_z=False)[0]

    def fake64(self, r, rows):
        """The fake batch of replica r in float64 NumPy from the device's own latents."""
        s, p = self.s, self.trees[r]
        _, z1, z2 = self.eng.make_batch(0, None, 1, 1, s["D"] - 1, 0.0, rows, self.z_seeds[r], step=self.z_steps[r], tag=Z_TAG, want_x=False)
        z1, z2 = z1.cpu().numpy().astype(np.float64), z2.cpu().numpy().astype(np.float64)
        y = z1 @ p["Decoder/FC0/kernel"] + p["Decoder/FC0/bias"]
        if s["sig"]:
            y = y + 1.0 / (1.0 + np.exp(-(z1 @ p["SigDecoder/FC0/kernel"] + p["SigDecoder/FC0/bias"])))
        return y + z2 * np.exp(self.sample_eps[r] / 2.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    return _EventCase(name)


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_event_properties_and_the_fake_side(name):
    """(i) replica r of N = 5 and of N = 3 is bitwise the N = 1 call on its slices; (ii) two runs are bitwise equal; (iii) the REAL
    record is bitwise vaek_cov_spectrum_rows on vaek_make_batch's x; (iv) engines of other batch sizes leave the same bits; T1 / T2 on
    the real side; T3 on the fake side; params and A untouched."""
    from vae_training_amd.engine import Engine
    c = _case(name)
    s, D, ln, rows = c.s, c.s["D"], c.len, EVENT_ROWS
    before, a_before = c.params.clone(), None if c.A is None else c.A.clone()
    a = c.records(rows)
    assert torch.equal(a, c.records(rows)), "(ii) two runs differ"
    three = c.records(rows, rs=slice(0, 3))
    assert torch.equal(three, a[:3]), "(i) N = 3 differs from N = 5"
    for r in range(R):
        one = c.records(rows, rs=slice(r, r + 1))
        assert torch.equal(one[0], a[r]), f"(i) replica {r} of N = 5 differs from its N = 1 call"
    for batch in (5, 4096):
        eng = Engine(batch, D, s["L"], (), (), s["eps"], s["tdv"], s["sig"])
        assert eng.supports_spectrum_event(s["kind"])
        assert torch.equal(c.records(rows, eng=eng), a), f"(iv) batch {batch} differs"
    got = a.cpu().numpy()
    worst_c, worst_e = 0.0, 0.0
    for r in range(R):
        x = c.x_rows(r, rows)
        real = _rows_call(c.eng, x.cpu().numpy()[None])[0]
        assert np.array_equal(real, got[r, ln:2 * ln]), f"(iii) replica {r}: the real record is not vaek_cov_spectrum_rows on make_batch's x"
        rr = K.split_record(real, D)
        K.check_t1(f"{name} real side replica {r}", rr, x.cpu().numpy())
        K.check_t2(f"{name} real side replica {r}", rr)
        assert np.all(np.abs(rr["eig"][:s["pad"]]) <= K.t2_bound(D, rr["off"], rr["norm"]))
        fr = K.split_record(got[r, :ln], D)
        K.check_t2(f"{name} fake side replica {r}", fr)
        f64 = c.fake64(r, rows)
        m, co = f64.mean(axis=0), np.cov(f64.T, ddof=1).reshape(D, D)
        scale = float(np.max(np.diag(co) + m * m))
        ec = float(np.max(np.abs(fr["cov"] - co)))
        ee = float(np.max(np.abs(fr["eig"] - np.linalg.eigvalsh(co))))
        be = float(np.linalg.norm(fr["cov"] - co, 2)) + K.t2_bound(D, fr["off"], fr["norm"])
        print(f"{name} fake side replica {r}: T3 |dC| {ec:.2e} = {ec / (T3 * scale):.3f} of the bound, |d lambda| {ee:.2e} = {ee / be:.3f} of the bound")
        assert ec <= T3 * scale and ee <= be, (name, r, ec, T3 * scale, ee, be)
        assert float(np.max(np.abs(fr["mean"] - m))) <= T3 * np.sqrt(scale)
        worst_c, worst_e = max(worst_c, ec / scale), max(worst_e, ee / be)
    print(f"{name}: worst fake-side |dC| / max(C_kk + m_k^2) {worst_c:.2e} (bound {T3:.0e}), worst |d lambda| {worst_e:.3f} of its bound")
    assert torch.equal(c.params, before), "params were written"
    assert c.A is None or torch.equal(c.A, a_before), "A was written"


@pytest.mark.parametrize("name", list(OFF_SQUARE))
def test_real_side_equals_make_batch_rows_off_the_square_matrix(name):
    """(iii) of test_fused_event_properties_and_the_fake_side, bitwise, at dd = 5, did = 9 with dataset noise: the event's own draw of
    the real rows is vaek_make_batch's."""
    c = _case(name)
    ln, rows = c.len, 257
    got = c.records(rows).cpu().numpy()
    for r in range(R):
        x = c.x_rows(r, rows).cpu().numpy()
        assert x[:, c.s["dd"]:].all()                                            # noise reaches the padding columns
        real = _rows_call(c.eng, x[None])[0]
        assert np.array_equal(real, got[r, ln:2 * ln]), f"replica {r}: the real record is not vaek_cov_spectrum_rows on make_batch's x"


def test_fused_event_at_other_row_counts_and_captured():
    """2, 257 and 4096 rows on one shape: (iii) again, T2 on both sides; a captured call replayed twice = the eager call."""
    c = _case("sigmoid_dd3_pd3")
    D, ln = c.s["D"], c.len
    for rows in (2, 257, 4096):
        got = c.records(rows, rs=slice(0, 3)).cpu().numpy()
        for r in range(3):
            real = _rows_call(c.eng, c.x_rows(r, rows).cpu().numpy()[None])[0]
            assert np.array_equal(real, got[r, ln:2 * ln]), (rows, r)
            K.check_t2(f"rows {rows} real side replica {r}", K.split_record(real, D))
            K.check_t2(f"rows {rows} fake side replica {r}", K.split_record(got[r, :ln], D))
    eager = c.records(257)
    out = c.out()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            c.call(out, 257)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                     # capture does not execute
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        out[:, :2 * ln] = 0.0


def _mlp3_model(engines, flat, seed):
    from vae_training_amd.engine import Engine

    def engine(B, gb=0):
        if B not in engines:
            engines[B] = Engine(B, 6, 6, (200, 200, 200), (200, 200, 200), -3.0, True, False)
        return engines[B]

    ds = types.SimpleNamespace(device_spec=lambda: (2, None, 3, 3, 3, 0.0), key=(seed, 2))
    opt = types.SimpleNamespace(global_batch=100)
    return types.SimpleNamespace(dataset=ds, batch_size=100, optimizer=opt, key=(3, 4), print_batch_size=1000, current_epsilon=-3.0,
                                 gt_eigen=[], ht_eigen=[], dirname=f"mlp3_{seed}",
                                 model=types.SimpleNamespace(module=types.SimpleNamespace(engine=engine), flat=flat))


def test_host_route_on_an_mlp3_sweep_of_two_models():
    """trainer.ReplicaSpectrum on two three-hidden-layer MLP models (sphere rows): no fused event, make_batch + forward per model, ONE
    vaek_cov_spectrum_rows call with n = 4; every record against T1 and T2 on the stack's rows; the real side has `pad` zeros."""
    from vae_training_amd.trainer import ReplicaSpectrum
    cfg = O.Config(6, 6, (200, 200, 200), (200, 200, 200), -3.0, True, None)
    engines = {}
    ms = []
    for r, seed in enumerate((69, 24)):
        flat = torch.as_tensor(O.flatten(cfg, O.init_params(cfg, seed=r), np.float32)).cuda()
        ms.append(_mlp3_model(engines, flat, seed))
    sp = ReplicaSpectrum(ms, rows=257)
    assert not sp.fused and sp.eng.step_path == "mlp3" and not sp.eng.supports_spectrum_event(2)
    sp.eng.profile_begin(16)
    stats = sp.event()
    rep = sp.eng.profile_report()
    assert rep["cov_spectrum_rows"]["count"] == 1, rep
    recs, stack = sp.out.cpu().numpy(), sp.stack.cpu().numpy()
    for r in range(2):
        for side, key in enumerate(sp.KEYS):
            rec = K.split_record(recs[2 * r + side], 6)
            what = f"mlp3 model {r} {key}"
            K.check_t1(what, rec, stack[2 * r + side])
            K.check_t2(what, rec)
            assert np.array_equal(stats[r][key], rec["eig"]) and np.array_equal((ms[r].ht_eigen, ms[r].gt_eigen)[side][-1], rec["eig"])
        real = K.split_record(recs[2 * r + 1], 6)
        assert np.all(np.abs(real["eig"][:3]) <= K.t2_bound(6, real["off"], real["norm"])) and real["eig"][3] > 0.1
        assert not stack[2 * r + 1][:, 3:].any() and np.allclose(np.linalg.norm(stack[2 * r + 1][:, :3], axis=1), 1.0, atol=1e-5)
    assert not np.array_equal(recs[0], recs[2]) and ms[0]._spectrum_draws == 1 and ms[0].key == (3, 4)


def test_arguments_predicates_and_profile_labels():
    """Every refusal of include/vaek.h returns VAEK_ERR_INVALID with a message naming the function and leaves the sentinel buffers
    unchanged; the predicates; exactly one profile record per launch."""
    from vae_training_amd._lib import VaekError
    from vae_training_amd.engine import Engine
    c, lin, sph = _case("sigmoid_dd3_pd3"), _case("linear_12"), _case("sphere")
    eng = c.eng
    D, ln = 7, c.len
    x = torch.as_tensor(K.explicit_sets(7, 37)).cuda().contiguous()                  # [4, 37, 7]

    def rows_refused(why, e=eng, **kw):
        out = torch.full((4, ln + 2), SENT, dtype=torch.float64, device="cuda")
        a = dict(x=x, rows=37, out=out, n=4, x_stride=37 * 7, out_stride=ln + 2)
        a.update(kw)
        with pytest.raises(VaekError) as ei:
            e.cov_spectrum_rows(**a)
        assert ei.value.code == -1 and "vaek_cov_spectrum_rows" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), why
        return out

    rows_refused("x NULL", x=None)
    rows_refused("out NULL", out=None)
    rows_refused("n = 0", n=0)
    rows_refused("n over the cap", n=eng.cov_spectrum_max_sets + 1)
    rows_refused("rows = 1", rows=1)
    rows_refused("rows = 0", rows=0)
    rows_refused("rows over the cap", rows=4097)
    rows_refused("x_stride < 0", x_stride=-1)
    rows_refused("0 < x_stride < rows * D", x_stride=37 * 7 - 1)
    rows_refused("out_stride < the record length", out_stride=ln - 1)
    keep = torch.full((4, ln + 2), SENT, dtype=torch.float64, device="cuda")
    rows_refused("out misaligned", out=keep.data_ptr() + 4)
    assert bool((keep == SENT).all())
    wide = Engine(100, 33, 6, (), (), -1.0, True, False)
    assert not wide.supports_cov_spectrum() and not wide.supports_spectrum_event(0)
    rows_refused("data_dim 33", e=wide)
    assert eng.cov_spectrum_max_sets == 2 * eng.train_loop_max_replicas and eng.cov_spectrum_max_sweeps == 32
    # any architecture, dtype and batch with data_dim <= 32 takes explicit rows; the fused event is the linear VAEs'
    mlp3 = Engine(100, 6, 6, (200, 200, 200), (200, 200, 200), -1.0, False, False)
    mlp1 = Engine(100, 7, 6, (64,), (64,), -1.0, True, True)
    bf16 = Engine(100, 7, 6, (), (), -1.0, True, True, dtype="bf16")
    for e in (mlp3, mlp1, bf16):
        assert e.supports_cov_spectrum()
    assert Engine(100, 32, 32, (), (), -1.0, True, False).supports_spectrum_event(0)
    assert Engine(100, 28, 32, (), (), -1.0, True, True).supports_spectrum_event(1)
    assert not Engine(100, 29, 6, (), (), -1.0, True, True).supports_spectrum_event(1)        # two decoders: D <= 28
    assert not Engine(100, 6, 33, (), (), -1.0, True, False).supports_spectrum_event(0)       # L > 32
    assert not eng.supports_spectrum_event(3) and not eng.supports_spectrum_event(-1)
    shared = _rows_call(eng, K.explicit_sets(7, 37)[:1])
    out = torch.full((3, ln), SENT, dtype=torch.float64, device="cuda")
    eng.cov_spectrum_rows(x[0], 37, out, n=3, x_stride=0)                                # x_stride 0: one set shared by all
    torch.cuda.synchronize()
    assert all(np.array_equal(out[k].cpu().numpy(), shared[0]) for k in range(3))

    def refused(why, e, **kw):
        out = e.out()
        before = e.params.clone()
        with pytest.raises(VaekError) as ei:
            e.call(out, kw.pop("rows", 37), **kw)
        assert ei.value.code == -1 and "vaek_spectrum_event_replicas" in str(ei.value), (why, ei.value)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and torch.equal(e.params, before), why

    for why, e2, kind in (("mlp3", mlp3, 2), ("one hidden layer", mlp1, 1), ("bf16", bf16, 1)):
        assert not e2.supports_spectrum_event(kind), why
        refused(why, sph if kind == 2 else c, eng=e2)
    refused("struct_size", c, struct_size=12)
    refused("n = 0", c, n=0)
    refused("n over the cap", c, n=eng.train_loop_max_replicas + 1)
    refused("rows = 1", c, rows=1)
    refused("rows over the cap", c, rows=4097)
    for name in ("x_seeds", "x_steps", "z_seeds", "z_steps", "sample_eps"):
        refused(name + " NULL", c, **{name: None})
    with pytest.raises(VaekError) as ei:
        c.call(None, 37, out_stride=c.os)
    assert ei.value.code == -1 and "vaek_spectrum_event_replicas" in str(ei.value)
    refused("state_stride < P", c, state_stride=c.P - 1)
    refused("out_stride < two records", c, out_stride=2 * ln - 1)
    o = c.out()
    with pytest.raises(VaekError) as ei:
        c.call(o.data_ptr() + 4, 37, out_stride=c.os)
    assert ei.value.code == -1 and "aligned" in str(ei.value) and bool((o == SENT).all())
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
    # kind 2 needs no A; a shared A (a_stride 0) is legal; exactly one profile record per launch
    sph.call(sph.out(), 37, A=None)
    eng.profile_begin(16)
    c.call(c.out(), 37, a_stride=0, A=c.A[0].clone())
    c.call(c.out(), 4096)
    eng.cov_spectrum_rows(x, 37, torch.empty(4, ln, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert sorted(rep) == ["cov_spectrum_rows", "spectrum_event_replicas"], rep
    assert rep["spectrum_event_replicas"]["count"] == 2 and rep["cov_spectrum_rows"]["count"] == 1, rep


def _run_py(tmp_path, name, dataset, layers, latent, pad, dd, eps, *extra, batches="300"):
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), name, "--dataset", dataset, "--encoder_layer_sizes", layers, "--layer_sizes", layers,
           "-ow", "--latent_dim", latent, "--padding_dim", pad, "-dd", dd, "--epsilon", eps, "-tdv", "--num_batches", batches, *extra]
    return subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)


def _losses(tmp_path, name):
    return dict(np.load(os.path.join(str(tmp_path), "data", name, "losses.npz"), allow_pickle=True))


LINES = {
    "sigmoid": ("sigmoid", "", "6", "3", "3", "-3", 7, 3, ()),
    "linear": ("linear_gaussian", "", "20", "9", "3", "-1", 12, 9, ("-ds", "2", "-lr", "1e-3")),
    "sphere": ("sphere", "200|200|200", "6", "3", "3", "-3", 6, 3, ()),
}


@pytest.mark.parametrize("script", list(LINES))
def test_run_py_eigenvalues_on_line_1_of_each_script(tmp_path, script):
    """300 batches of line 1 of sigmoid_vae_padding_expts.sh, seed_linpadding_expts.sh and sphere_vae_padding_expts.sh (the host route)
    with --eigenvalues: EigenValues = (learnt, ground truth) with one entry of D values per n_print event; the real side has `pad`
    eigenvalues that are zero up to T2's scale; the same run without the flag has no new key and is otherwise bitwise the same."""
    dataset, layers, latent, pad, dd, eps, D, npad, extra = LINES[script]
    r = _run_py(tmp_path, "ev", dataset, layers, latent, pad, dd, eps, "--eigenvalues", *extra)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Eigenvalue events: 1000 generated and 1000 real rows" in r.stdout
    got = _losses(tmp_path, "ev")
    ev = np.asarray(got["EigenValues"], dtype=np.float64)
    assert ev.shape == (2, 1, D), ev.shape                               # (learnt, ground truth) x one event (step 0) x D
    assert np.all(np.diff(ev, axis=-1) >= 0) and np.isfinite(ev).all()
    for k, key in enumerate(("learnt eigenvalue", "ground truth eigenvalue")):
        assert np.array_equal(np.asarray(got[key], dtype=np.float64).reshape(1, D), ev[k]), key
    gt = ev[1, 0]
    assert np.all(np.abs(gt[:npad]) <= 64 * D * 2.0 ** -53 * np.linalg.norm(gt) + 2.0 ** -43 * np.linalg.norm(gt)), gt
    assert np.all(gt[npad:] > 1e-3), gt
    assert np.all(ev[0, 0][npad:] > 1e-3), ev[0, 0]                      # an untrained decoder spreads variance over every direction
    p = _run_py(tmp_path, "plain", dataset, layers, latent, pad, dd, eps, *extra)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Eigenvalue events" not in p.stdout
    plain = _losses(tmp_path, "plain")
    new = {"EigenValues", "learnt eigenvalue", "ground truth eigenvalue"}
    assert sorted(k for k in got if k not in new) == sorted(plain) and not new & set(plain)
    for k in plain:
        a, b = np.asarray(plain[k]), np.asarray(got[k])
        assert a.shape == b.shape and (a.dtype == object or a.tobytes() == b.tobytes()), k


def test_run_py_eigenvalues_in_a_sweep_and_the_refusal(tmp_path):
    """--sweep_dataset_seeds with --fused_stats and --log_likelihood_samples: one fused spectrum call for both models; a 33-column
    dataset is refused before any step."""
    r = _run_py(tmp_path, "sw", "sigmoid", "", "6", "3", "3", "-3", "--eigenvalues", "--sweep_dataset_seeds", "69,24", "--fused_stats",
                "--log_likelihood_samples", "8", batches="30")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Eigenvalue events: 1000 generated and 1000 real rows per model (vaek_spectrum_event_replicas)" in r.stdout
    evs = [np.asarray(_losses(tmp_path, f"sw_ds{seed}")["EigenValues"], dtype=np.float64) for seed in (69, 24)]
    assert all(e.shape == (2, 1, 7) for e in evs) and not np.array_equal(evs[0], evs[1])
    r = _run_py(tmp_path, "wide", "sphere", "", "6", "30", "3", "-3", "--eigenvalues", batches="30")
    assert r.returncode != 0 and "--eigenvalues needs data_dim <= 32" in r.stderr and "data_dim: 33" in r.stderr, r.stderr[-1500:]
    assert "Batch |" not in r.stdout
