"""The cases and the bounds of the eigenvector and principal-angle tests, NumPy only: tests/test_gpu_subspace.py runs the kernels on
them, tests/test_subspace_host.py and tools/cov_eigen_reference.py the float64 restatement.  The explicit input sets are
tests/cov_spectrum_cases.py's (imported, not copied).

BOUNDS on an eigen record (V = the record's eigenvectors, C, lambda, sweeps, off_F, |C|_F its own):
  E1  orthonormality: max |V^T V - I| <= K1 D (sweeps + 1) 2^-53.
  E2  residual: |C V - V diag(lambda)|_F <= off_F + K2 D 2^-53 |C|_F.
K1 and K2 are powers of two fixed from the float64 restatement's worst case over cov_spectrum_cases.all_host_sets() (the device
differs from the restatement only in fused multiply-adds and summation order; a factor of 4 covers that):
  K1 = 4.    The restatement's worst E1 is 1.0 in the unit D (sweeps + 1) 2^-53 (2 ulp, on D2_rows255_mixed): 1/4 of the bound.
  K2 = 256.  The restatement's worst E2 is 0.64 of off_F + 64 D 2^-53 |C|_F (on D7_rows255_bigmean), hence four times 64.  The stop
             rule's off_F dominates that case and does not grow with K2, so at K2 = 256 the same case stands at 0.305 of the bound,
             not at 0.16: the tighter of the two readings of "a factor of 4" is kept.
  (measured with tools/cov_eigen_reference.py, a plain accumulation of V, on the CPU.)
SIGN RULE: every column's component of largest magnitude is positive, a tie goes to the lowest row.  ORDER: column k belongs to
eigenvalue k, ascending (E2 pairs them; the Rayleigh quotient is checked too).

ANGLES on hand-made records (no solve involved: orthonormal bases written into caller-owned eigen records), against
scipy.linalg.subspace_angles on the same matrices: |sin^2_dev - sin^2_scipy| <= off_F(G) + 64 D 2^-53, and |[kb] - sum sin^2| <= the
same bound.  PLANTED EVENTS against the host route on the same draws (Davis-Kahan, each side's subspace moves by at most
|C_dev - C_ref|_2 / gap_ref and the two sides add): |d sin theta_i| <= 2 max_side(|C_dev - C_ref|_2 / gap_ref) + 1e-12, gap_ref =
lambda_k - lambda_{k+1} of the reference C, and every case has gap_ref >= 1e-3 lambda_max (asserted, never skipped on)."""
import numpy as np

from tests import cov_spectrum_cases as K

K1 = 4.0
K2 = 256.0
DIMS = (1, 2, 3, 7, 21, 32)
ROWS = (2, 5, 257)
THETAS = (1e-3, 0.3, np.pi / 2 - 1e-3)
ANGLE_DIMS = (2, 3, 32)
GAP_MIN = 1e-3


def spectrum_len(D):
    return D * D + 2 * D + 4


def eigen_len(D):
    return 2 * D * D + 2 * D + 4


def split_eigen_record(rec, D):
    """An eigen record of 2 D^2 + 2 D + 4 doubles as a dict: cov_spectrum_cases.split_record's keys and "vec"."""
    rec = np.asarray(rec, np.float64)
    assert rec.shape == (eigen_len(D),)
    r = K.split_record(rec[:spectrum_len(D)], D)
    r["vec"] = rec[spectrum_len(D):].reshape(D, D)
    return r


def split_angle_record(rec, kb):
    rec = np.asarray(rec, np.float64)
    assert rec.shape == (kb + 4,)
    return {"sin2": rec[:kb], "frob2": rec[kb], "sweeps": rec[kb + 1], "off": rec[kb + 2], "orth": rec[kb + 3]}


def e1_bound(D, sweeps):
    return K1 * D * (sweeps + 1) * 2.0 ** -53


def e2_bound(D, off, norm):
    return off + K2 * D * 2.0 ** -53 * norm


def check_eigen(what, r):
    """E1, E2, the sign rule and the order on a record dict `r`.  Returns (E1, E2) in the units of their bounds."""
    V, C, lam = r["vec"], r["cov"], r["eig"]
    D = V.shape[0]
    g1 = float(np.max(np.abs(V.T @ V - np.eye(D))))
    g2 = float(np.sqrt(np.sum((C @ V - V * lam[None, :]) ** 2)))
    b1, b2 = e1_bound(D, r["sweeps"]), e2_bound(D, r["off"], r["norm"])
    u1, u2 = g1 / b1, (g2 / b2 if b2 > 0 else (0.0 if g2 == 0 else np.inf))
    print(f"{what}: E1 {g1:.2e} = {u1:.3f} of the bound, E2 {g2:.2e} = {u2:.3f} of the bound (sweeps {int(r['sweeps'])})")
    assert np.isfinite(V).all(), what
    assert u1 <= 1.0, (what, "E1", g1, b1)
    assert u2 <= 1.0, (what, "E2", g2, b2)
    assert np.all(np.diff(lam) >= 0), (what, "eigenvalues not ascending")
    for k in range(D):
        i = int(np.argmax(np.abs(V[:, k])))                          # the first of equal magnitudes: the lowest row
        assert V[i, k] > 0.0, (what, "sign rule", k, V[:, k])
        assert abs(V[:, k] @ C @ V[:, k] - lam[k]) <= b2 + b1 * r["norm"], (what, "column", k, "is not eigenvalue", k)
    return u1, u2


def angle_bound(D, off):
    return off + 64.0 * D * 2.0 ** -53


def eigen_record_of_basis(V):
    """An eigen record whose V block is the orthonormal D x D matrix `V`; the spectrum part is zero (the angles call reads V only)."""
    V = np.asarray(V, np.float64)
    D = V.shape[0]
    rec = np.zeros(eigen_len(D))
    rec[spectrum_len(D):] = V.reshape(-1)
    return rec


def rotated_basis(D, theta):
    """I with the plane (0, D - 1) turned by theta: column D - 1 = cos e_{D-1} + sin e_0, column 0 = cos e_0 - sin e_{D-1}."""
    V = np.eye(D)
    c, s = np.cos(theta), np.sin(theta)
    V[D - 1, D - 1], V[0, D - 1] = c, s
    V[0, 0], V[D - 1, 0] = c, -s
    return V


def angle_pairs(D):
    """The (ka, kb) of the planted-rotation cases at this D, where valid."""
    want = [(1, 1), (2, 1), (D, D), ((D + 1) // 2, 1)]
    return sorted({(ka, kb) for ka, kb in want if 1 <= kb <= ka <= D})


def scipy_sin2(Va, Vb, ka, kb):
    """sin^2 of the principal angles between the last ka columns of Va and the last kb of Vb, ascending."""
    from scipy.linalg import subspace_angles
    D = Va.shape[0]
    th = subspace_angles(Va[:, D - ka:], Vb[:, D - kb:])
    return np.sort(np.sin(th) ** 2)


def check_angles(what, rec, Va, Vb, ka, kb):
    """The angle record `rec` (kb + 4 doubles) against scipy on the same bases."""
    D = Va.shape[0]
    r = split_angle_record(rec, kb)
    ref = scipy_sin2(Va, Vb, ka, kb)
    bound = angle_bound(D, r["off"])
    err = float(np.max(np.abs(r["sin2"] - ref)))
    ferr = abs(r["frob2"] - float(np.sum(r["sin2"])))
    print(f"{what}: |d sin^2| {err:.2e} = {err / bound:.3f} of the bound, |[kb] - sum| {ferr:.2e} = {ferr / bound:.3f} of the bound, "
          f"sweeps {int(r['sweeps'])}, off_F {r['off']:.1e}")
    assert np.all(np.diff(r["sin2"]) >= 0), (what, "not ascending")
    assert r["sweeps"] == int(r["sweeps"]) and 0 <= r["sweeps"] < K.MAX_SWEEPS, (what, r["sweeps"])
    assert err <= bound, (what, err, bound, r["sin2"], ref)
    assert ferr <= bound, (what, ferr, bound)
    assert r["orth"] <= 64.0 * D * 2.0 ** -53, (what, "the hand-made bases are orthonormal", r["orth"])
    return r


def planted_decoder(Q, N, thetas, scales, L):
    """Decoder kernel [L, D] with k non-zero rows: row i = scales[i] (cos theta_i q_i + sin theta_i n_i), q_i the columns of Q (an
    orthonormal basis of the data's span), n_i those of N (orthonormal, orthogonal to Q): the principal angles between the rows' span
    and the data's span are exactly `thetas`."""
    D, k = Q.shape
    W = np.zeros((L, D))
    for i in range(k):
        W[i] = scales[i] * (np.cos(thetas[i]) * Q[:, i] + np.sin(thetas[i]) * N[:, i])
    return W


def davis_kahan(what, C_dev, C_ref, k):
    """|C_dev - C_ref|_2 / gap_ref of one side; asserts the gap condition."""
    lam = np.linalg.eigvalsh(C_ref)
    D = lam.shape[0]
    gap = lam[D - k] - (lam[D - k - 1] if k < D else 0.0)
    assert gap >= GAP_MIN * lam[-1], (what, "gap", gap, lam)
    return float(np.linalg.norm(C_dev - C_ref, 2)) / gap
