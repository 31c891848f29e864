"""NumPy float64 restatement of csrc/cov_spectrum.hip, from the CPU ALONE (no GPU, no kernel): the same moments, covariance,
round-robin ordering, rotation formula, direct off-diagonal norm, stop rule and sweep cap.  tests/test_cov_spectrum_host.py holds it
to numpy.linalg.eigvalsh on every input set of tests/test_gpu_cov_spectrum.py (the sets are tests/cov_spectrum_cases.py's), so a case
that cannot converge below the cap is found here and not on the GPU.

    python tools/cov_spectrum_reference.py        # per case: sweeps, off_F / |C|_F, eigenvalue error in the unit of the T2 bound

It is a restatement of the algorithm, not of the instruction stream: the order of the row sum inside a four-row matrix-core step and
fused multiply-adds differ, so it agrees with the device within the test's bounds, not bitwise."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SWEEPS = 32                    # kSpectrumMaxSweeps
TOL = 2.0 ** -43                   # off_F <= TOL * |C|_F stops the solve
HUGE_THETA = 1e150                 # above it theta is not squared: t = 1 / (2 theta)


def covariance(x32):
    """(m, C) of float32 rows [rows, D] as the kernel forms them: float64 sums of exact products, C = (S2 - rows m m^T) / (rows - 1),
    the upper triangle mirrored."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    n = x.shape[0]
    s1, s2 = x.sum(axis=0), x.T @ x
    m = s1 / n
    c = (s2 - n * np.outer(m, m)) / (n - 1.0)
    c = np.triu(c) + np.triu(c, 1).T
    return m, c


def round_pairs(de, rnd):
    """The de / 2 disjoint (p, q) of round `rnd` of a sweep: index de - 1 stays, the others turn."""
    n1 = de - 1
    return [(rnd, n1)] + [((rnd + k) % n1, (rnd - k + n1) % n1) for k in range(1, de // 2)]


def rotation(app, aqq, apq):
    """(c, s) that zero a_pq; (1, 0) where a_pq == 0; safe where theta overflows."""
    if apq == 0.0:
        return 1.0, 0.0
    with np.errstate(over="ignore", divide="ignore"):
        theta = np.float64(aqq - app) / np.float64(2.0 * apq)
    ath = abs(theta)
    t = 0.5 / theta if ath > HUGE_THETA else np.copysign(1.0, theta) / (ath + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    return c, t * c


def off_norm(a):
    return float(np.sqrt(2.0 * np.sum(np.triu(a, 1) ** 2)))


def jacobi_eigenvalues(c, max_sweeps=MAX_SWEEPS):
    """(eigenvalues ascending, sweeps run, final off_F, |C|_F) of a symmetric D x D matrix."""
    d = c.shape[0]
    de = d + (d & 1)
    a = np.zeros((de, de))
    a[:d, :d] = c
    norm_c = float(np.sqrt(np.sum(a * a)))
    sweeps = 0
    while True:
        off = off_norm(a)
        if off <= TOL * norm_c or sweeps == max_sweeps:
            break
        for rnd in range(de - 1):
            cs, sn, mate = np.ones(de), np.zeros(de), np.arange(de)
            for p, q in round_pairs(de, rnd):
                co, si = rotation(a[p, p], a[q, q], a[p, q])
                cs[p] = cs[q] = co
                sn[p], sn[q] = -si, si                       # new column i = c col_i + s_i col_mate(i)
                mate[p], mate[q] = q, p
            b = cs[:, None] * (cs[None, :] * a + sn[None, :] * a[:, mate]) + sn[:, None] * (cs[None, :] * a[mate, :] + sn[None, :] * a[mate][:, mate])
            a = np.triu(b) + np.triu(b, 1).T                 # computed for i <= j, mirrored
        sweeps += 1
    eig = np.sort(np.diag(a)[:d], kind="stable")
    return eig, sweeps, off, norm_c


def record(x32):
    """The kernel's record of one set as a dict."""
    m, c = covariance(x32)
    eig, sweeps, off, norm_c = jacobi_eigenvalues(c)
    return {"eig": eig, "mean": m, "cov": c, "sweeps": sweeps, "off": off, "norm": norm_c, "rows": x32.shape[0]}


def t2_bound(d, off, norm_c):
    """T2 of the tests: Weyl's bound on the residual plus both solvers' backward error."""
    return off + 64.0 * d * 2.0 ** -53 * norm_c


def main():
    from tests import cov_spectrum_cases as K
    worst_sweeps, worst_err = 0, 0.0
    for name, x in K.all_host_sets():
        r = record(x)
        ref = np.linalg.eigvalsh(r["cov"])
        err = float(np.max(np.abs(r["eig"] - ref)))
        unit = err / t2_bound(x.shape[1], r["off"], r["norm"]) if r["norm"] > 0 else 0.0
        rel = r["off"] / r["norm"] if r["norm"] > 0 else 0.0
        lam = float(np.max(np.abs(ref))) or 1.0
        print(f"{name:34s} sweeps {r['sweeps']:2d}  off/|C| {rel:.1e}  err/lam_max {err / lam:.1e}  err/T2 {unit:.2f}")
        worst_sweeps, worst_err = max(worst_sweeps, r["sweeps"]), max(worst_err, err / lam)
    print(f"most sweeps {worst_sweeps} of {MAX_SWEEPS}; worst error {worst_err:.1e} lambda_max")


if __name__ == "__main__":
    main()
