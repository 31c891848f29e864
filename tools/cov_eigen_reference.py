"""NumPy float64 restatement of the eigenvector half of csrc/cov_spectrum.hip, from the CPU ALONE (no GPU, no kernel): the Jacobi solve
of tools/cov_spectrum_reference.py (imported, not copied: the same covariance, ordering, rotation, off-norm, stop rule and cap) with
the rotations accumulated into V (V starts as I; each round V <- V J, new column i = c_i V[:, i] + s_i V[:, mate(i)]), the columns in
the eigenvalues' order (counting ranks, ties by index), the sign rule (the component of largest magnitude is positive, a tie goes to
the lowest row), and vaek_subspace_angles: M = U^T W, R = W - U M formed explicitly, G = R^T R, G's eigenvalues by the same solve.
V never feeds back into the matrix, so sweeps and eigenvalues are those of cov_spectrum_reference.record.

    python tools/cov_eigen_reference.py        # per case: sweeps, E1 and E2 in the units of their bounds (tests/subspace_cases.py)

It is a restatement of the algorithm, not of the instruction stream: summation order and fused multiply-adds differ, so it agrees
with the device within the tests' bounds, not bitwise."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("cov_spectrum_reference", os.path.join(ROOT, "tools", "cov_spectrum_reference.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


def jacobi_eigen(c, max_sweeps=S.MAX_SWEEPS):
    """(eigenvalues ascending, V with column k the eigenvector of eigenvalue k, sweeps run, final off_F, |C|_F) of a symmetric D x D
    matrix: cov_spectrum_reference.jacobi_eigenvalues with V <- V J in every round."""
    d = c.shape[0]
    de = d + (d & 1)
    a = np.zeros((de, de))
    a[:d, :d] = c
    v = np.eye(de)
    norm_c = float(np.sqrt(np.sum(a * a)))
    sweeps = 0
    while True:
        off = S.off_norm(a)
        if off <= S.TOL * norm_c or sweeps == max_sweeps:
            break
        for rnd in range(de - 1):
            cs, sn, mate = np.ones(de), np.zeros(de), np.arange(de)
            for p, q in S.round_pairs(de, rnd):
                co, si = S.rotation(a[p, p], a[q, q], a[p, q])
                cs[p] = cs[q] = co
                sn[p], sn[q] = -si, si
                mate[p], mate[q] = q, p
            b = cs[:, None] * (cs[None, :] * a + sn[None, :] * a[:, mate]) + sn[:, None] * (cs[None, :] * a[mate, :] + sn[None, :] * a[mate][:, mate])
            a = np.triu(b) + np.triu(b, 1).T
            v = cs[None, :] * v + sn[None, :] * v[:, mate]
        sweeps += 1
    diag = np.diag(a)[:d]
    order = np.argsort(diag, kind="stable")                    # the counting ranks: ties by index
    vec = v[:d][:, order]
    return diag[order], fix_signs(vec), sweeps, off, norm_c


def fix_signs(v):
    """Every column's component of largest magnitude positive; a tie goes to the lowest row (numpy.argmax takes the first)."""
    v = np.array(v, np.float64)
    for k in range(v.shape[1]):
        i = int(np.argmax(np.abs(v[:, k])))
        if v[i, k] < 0.0:
            v[:, k] = -v[:, k]
    return v


def record(x32):
    """The eigen record of one set as a dict: cov_spectrum_reference.record's keys and "vec"."""
    m, c = S.covariance(x32)
    eig, vec, sweeps, off, norm_c = jacobi_eigen(c)
    return {"eig": eig, "mean": m, "cov": c, "sweeps": sweeps, "off": off, "norm": norm_c, "rows": x32.shape[0], "vec": vec}


def subspace_record(va, vb, ka, kb):
    """vaek_subspace_angles' record as a dict from two eigenvector matrices (columns in ascending eigenvalue order)."""
    d = va.shape[0]
    assert 1 <= kb <= ka <= d
    u, w = va[:, d - ka:], vb[:, d - kb:]
    m = u.T @ w
    r = w - u @ m                                              # explicit: I - M^T M would lose the small angles
    g = r.T @ r
    g = np.triu(g) + np.triu(g, 1).T
    sin2, sweeps, off, _ = S.jacobi_eigenvalues(g)
    orth = max(float(np.max(np.abs(u.T @ u - np.eye(ka)))), float(np.max(np.abs(w.T @ w - np.eye(kb)))))
    return {"sin2": sin2, "frob2": float(np.sum(r * r)), "sweeps": sweeps, "off": off, "orth": orth}


def angles(sin2):
    """Principal angles in radians, ascending, as trainer.ReplicaSubspace reports them."""
    return np.arcsin(np.sqrt(np.clip(sin2, 0.0, 1.0)))


def e1(r):
    """max |V^T V - I| of a record dict."""
    d = r["vec"].shape[0]
    return float(np.max(np.abs(r["vec"].T @ r["vec"] - np.eye(d))))


def e2(r):
    """|C V - V diag(lambda)|_F on the record's own C and lambda."""
    return float(np.sqrt(np.sum((r["cov"] @ r["vec"] - r["vec"] * r["eig"][None, :]) ** 2)))


def main():
    from tests import cov_spectrum_cases as K
    from tests import subspace_cases as Z
    worst1, worst2 = (0.0, ""), (0.0, "")
    for name, x in K.all_host_sets():
        r = record(x)
        d = x.shape[1]
        u1 = e1(r) / Z.e1_bound(d, r["sweeps"])
        b2 = Z.e2_bound(d, r["off"], r["norm"])
        u2 = e2(r) / b2 if b2 > 0 else 0.0
        print(f"{name:34s} sweeps {r['sweeps']:2d}  E1 {u1:.3f}  E2 {u2:.3f}  (units of the bounds)")
        worst1, worst2 = max(worst1, (u1, name)), max(worst2, (u2, name))
    print(f"worst E1 {worst1[0]:.3f} of its bound on {worst1[1]}; worst E2 {worst2[0]:.3f} of its bound on {worst2[1]}")


if __name__ == "__main__":
    main()
