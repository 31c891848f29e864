"""The input sets and the bounds of the covariance-spectrum tests, NumPy only: tests/test_gpu_cov_spectrum.py runs the kernels on
them, tests/test_cov_spectrum_host.py and tools/cov_spectrum_reference.py the float64 restatement of the algorithm.

EXPLICIT SETS, per (D, rows) four variants of float32 rows:
  mixed    correlated Gaussian rows g M + b with a random D x D map M and a mean b of the rows' own scale
  iso      standard normal rows: clustered eigenvalues
  const    mixed with column 0 replaced by the constant 3 (an exactly-zero row and column of C)
  bigmean  rows whose mean is 100 standard deviations: the cancellation in S2 - rows m m^T
D = 1, 2, 3 (odd: padded to even), 7, 21 (a second 16-column block, odd), 28, 32 (both blocks full); rows = 2, 3, 5 (the fewest a
ddof = 1 covariance has; less than one k-step, just over one), 17 (rank-deficient at D = 32), 33, 255, 256, 257 (around one tile),
1000 (the print batch), 4096 (the cap: 16 tiles).  Rows < D make every such set rank-deficient.
PADDED SETS: sphere, linear_gaussian and sigmoid rows with exactly-zero padding columns.  The GPU test draws them with
vaek_make_batch; the host test draws the same shapes from the oracle's datasets (the device rows need the GPU; the zero columns, the
distribution and the ranks are the same).

BOUNDS (the issue's):
  T1  C and m against numpy.cov in float64 on the identical float32 rows: |dC_ij| <= 1e-11 max_k(C_kk + m_k^2) and
      |dm_k| <= 1e-11 sqrt(max_k(C_kk + m_k^2)).  The summation bound is rows 2^-53 = 4.6e-13 at 4096 rows; the factor of about 20
      covers the differing order.
  T2  eigenvalues against numpy.linalg.eigvalsh of the SAME C: |d lambda_k| <= off_F(reported) + 64 D 2^-53 |C|_F: Weyl's bound on the
      residual plus both solvers' backward error; sweeps below the cap, off_F <= 2^-43 |C|_F, eigenvalues ascending."""
import numpy as np

DIMS = (1, 2, 3, 7, 21, 28, 32)
ROWS = (2, 3, 5, 17, 33, 255, 256, 257, 1000, 4096)
VARIANTS = ("mixed", "iso", "const", "bigmean")
MAX_SWEEPS = 32
STOP = 2.0 ** -43
T1 = 1e-11

# name -> dataset kind (0 linear_gaussian, 1 sigmoid, 2 sphere), D, dd, did, pad, var_added
PADDED = {
    "sphere_dd3_pd3": dict(kind=2, D=6, dd=3, did=3, pad=3, var=0.0),
    "sphere_dd5_pd16": dict(kind=2, D=21, dd=5, did=5, pad=16, var=0.0),
    "linear_dd3_pd9": dict(kind=0, D=12, dd=3, did=3, pad=9, var=0.0),
    "linear_dd3_pd17": dict(kind=0, D=20, dd=3, did=3, pad=17, var=0.0),
    "sigmoid_dd3_pd3": dict(kind=1, D=7, dd=3, did=1, pad=3, var=0.0),
    "sigmoid_dd7_pd20": dict(kind=1, D=28, dd=7, did=1, pad=20, var=0.0),
}
PADDED_ROWS = (5, 257, 1000)
KIND_NAME = {0: "linear_gaussian", 1: "sigmoid", 2: "sphere"}


def explicit_sets(D, rows):
    """float32 [len(VARIANTS), rows, D], the same for every caller."""
    rng = np.random.default_rng(1000 * D + rows)
    g = rng.standard_normal((rows, D))
    mixed = g @ (rng.standard_normal((D, D)) / np.sqrt(D)) + rng.standard_normal(D)
    iso = rng.standard_normal((rows, D))
    const = mixed.copy()
    const[:, 0] = 3.0
    bigmean = rng.standard_normal((rows, D)) * 0.5 + 50.0 * np.where(np.arange(D) % 2 == 0, 1.0, -1.0)
    return np.stack([mixed, iso, const, bigmean]).astype(np.float32)


def host_padded_rows(name, rows):
    """The padded set `name` from the oracle's dataset of that kind (float32 [rows, D])."""
    from oracle import elbo_oracle as O
    s = PADDED[name]
    _, sampler = O.make_dataset(KIND_NAME[s["kind"]], seed=11, dd=s["dd"], did=s["did"], pad=s["pad"], var_added=s["var"])
    x = np.asarray(sampler(np.random.default_rng(5), rows), np.float32)
    assert x.shape == (rows, s["D"]) and not x[:, s["D"] - s["pad"]:].any()
    return x


def all_host_sets():
    """(name, float32 rows) of every input set of the GPU file, the padded ones drawn on the host."""
    for D in DIMS:
        for rows in ROWS:
            for v, x in zip(VARIANTS, explicit_sets(D, rows)):
                yield f"D{D}_rows{rows}_{v}", x
    for name in PADDED:
        for rows in PADDED_ROWS:
            yield f"{name}_rows{rows}", host_padded_rows(name, rows)


def split_record(rec, D):
    """A record of D^2 + 2 D + 4 doubles as a dict."""
    rec = np.asarray(rec, np.float64)
    assert rec.shape == (D * D + 2 * D + 4,)
    t = 2 * D + D * D
    return {"eig": rec[:D], "mean": rec[D:2 * D], "cov": rec[2 * D:t].reshape(D, D), "sweeps": rec[t], "off": rec[t + 1], "norm": rec[t + 2],
            "rows": rec[t + 3]}


def t2_bound(D, off, norm):
    return off + 64.0 * D * 2.0 ** -53 * norm


def check_t1(what, r, x32):
    """T1 on a record dict `r` against numpy.cov of the identical float32 rows.  Returns the two errors in the unit of their bounds."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    D = x.shape[1]
    m = x.mean(axis=0)
    c = np.cov(x.T, ddof=1).reshape(D, D)
    scale = float(np.max(np.diag(c) + m * m))
    ec, em = float(np.max(np.abs(r["cov"] - c))), float(np.max(np.abs(r["mean"] - m)))
    uc = ec / (T1 * scale) if scale > 0 else (0.0 if ec == 0 else np.inf)
    um = em / (T1 * np.sqrt(scale)) if scale > 0 else (0.0 if em == 0 else np.inf)
    print(f"{what}: T1 |dC| {ec:.2e} = {uc:.3f} of the bound, |dm| {em:.2e} = {um:.3f} of the bound")
    assert np.array_equal(r["cov"], r["cov"].T), f"{what}: C is not exactly symmetric"
    assert r["rows"] == x.shape[0], what
    assert uc <= 1.0 and um <= 1.0, (what, uc, um)
    return uc, um


def check_t2(what, r):
    """T2 on a record dict `r` against numpy.linalg.eigvalsh of its own C.  Returns (sweeps, error in the unit of the bound)."""
    D = r["cov"].shape[0]
    ref = np.linalg.eigvalsh(r["cov"])
    bound = t2_bound(D, r["off"], r["norm"])
    err = float(np.max(np.abs(r["eig"] - ref)))
    unit = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
    print(f"{what}: T2 sweeps {int(r['sweeps'])}, off_F / |C|_F {r['off'] / r['norm'] if r['norm'] > 0 else 0.0:.1e}, |d lambda| {err:.2e} = {unit:.3f} of the bound")
    assert r["sweeps"] == int(r["sweeps"]) and 0 <= r["sweeps"] < MAX_SWEEPS, (what, r["sweeps"])
    assert r["off"] <= STOP * r["norm"], (what, r["off"], r["norm"])
    assert abs(r["norm"] - np.sqrt(np.sum(r["cov"] ** 2))) <= 1e-14 * r["norm"], what
    assert np.all(np.diff(r["eig"]) >= 0), (what, "not ascending")
    assert unit <= 1.0, (what, err, bound)
    return int(r["sweeps"]), unit
