"""NumPy float64 restatement of vaek_exact_log_likelihood_replicas (csrc/exact_loglik.inc), from the CPU ALONE (no GPU, no kernel): a
one-decoder linear VAE is a linear-Gaussian latent-variable model, p(x) = N(b_d, K^T K + e^{eps} I), so log p(x), the ELBO of the
diagonal-Gaussian encoder and their difference KL(q(z|x) || p(z|x)) are closed forms.  G = K^T K is solved by the Jacobi routine of
tools/cov_eigen_reference.py (imported, not copied: the device's ordering, rotation, off-norm, 2^-43 stop and 32-sweep cap), the
eigenvalues are clamped at 0 where s_i = max(lambda_i, 0) + e^{eps} is formed -- the one place that uses G being PSD -- and the
formulae are the header's.

An INDEPENDENT evaluation checks it: mpmath at 60 digits (Cholesky of K^T K + e^{eps} I, a triangular solve, the log-determinant from
the factor's diagonal; the ELBO term by term); where mpmath is absent, scipy.stats.multivariate_normal.logpdf, for eps >= -8 only.

    python tools/exact_log_likelihood_reference.py     # per case: sweeps and the worst errors in units of the bounds of tests/exact_loglik_cases.py

It is a restatement of the algorithm, not of the instruction stream: summation order and fused multiply-adds differ, so it agrees
with the device within the tests' bounds, not bitwise."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("cov_eigen_reference", os.path.join(ROOT, "tools", "cov_eigen_reference.py"))
_E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_E)
jacobi_eigen = _E.jacobi_eigen

KE, BE, KD, BD, LV = "Encoder/FC0/kernel", "Encoder/FC0/bias", "Decoder/FC0/kernel", "Decoder/FC0/bias", "epsilon_p"
LOG2PI = float(np.log(2.0 * np.pi))
HEAD = 10
MP_DIGITS = 60

try:
    import mpmath as mp
except ImportError:                                            # the scipy route below, eps >= -8
    mp = None


def gram(k):
    """K^T K, the upper triangle computed and mirrored (float64 products of float32 values are exact)."""
    g = k.T @ k
    return np.triu(g) + np.triu(g, 1).T


def evaluate(p, eps, x):
    """The device's evaluation as a dict: per-row "logp", "elbo", "gap", "quad", "M" (the sum of the magnitudes of the ELBO's terms),
    and the model's "eig" (ascending, unclamped), "logdet", "sweeps", "off", "norm", "cond", "T"."""
    k, bd, e, be, lv = p[KD], p[BD], p[KE], p[BE], p[LV]
    d = k.shape[1]
    eig, vec, sweeps, off, norm = jacobi_eigen(gram(k))
    s = np.maximum(eig, 0.0) + np.exp(eps)
    logdet = float(np.sum(np.log(s)))
    t = float(np.sum(np.exp(lv) * np.sum(k * k, axis=1)))
    y = (x - bd) @ vec
    quad = np.sum(y * y / s, axis=1)
    logp = -0.5 * (quad + logdet + d * LOG2PI)
    mu = x @ e + be
    r = mu @ k + bd - x
    rsq = np.sum(r * r, axis=1)
    musq = np.sum(mu * mu, axis=1)
    elbo = -0.5 * (np.exp(-eps) * (rsq + t) + d * (eps + LOG2PI)) - 0.5 * (np.sum(np.exp(lv) - 1.0 - lv) + musq)
    mag = 0.5 * (np.exp(-eps) * (rsq + t) + d * abs(eps) + d * LOG2PI) + 0.5 * (np.sum(np.exp(lv) + 1.0 + np.abs(lv)) + musq)
    cond = (off + 64.0 * d * 2.0 ** -53 * norm) * np.exp(-eps)
    return {"logp": logp, "elbo": elbo, "gap": logp - elbo, "quad": quad, "M": mag, "eig": eig, "logdet": logdet, "sweeps": sweeps,
            "off": off, "norm": norm, "cond": cond, "T": t}


def record(p, eps, x):
    """The record of 10 + D doubles the device stores for these rows."""
    r = evaluate(p, eps, x)
    head = [r["logp"].mean(), r["elbo"].mean(), r["gap"].mean(), eps, r["logdet"], r["sweeps"], r["off"], r["norm"], r["cond"], x.shape[0]]
    return np.concatenate([np.array(head, np.float64), r["eig"]])


def _mpv(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, np.float64).ravel()]


def high_precision(p, eps, x):
    """(log p(x_i), ELBO(x_i), logdet) of every row, independent of the restatement: 60-digit mpmath, Cholesky of K^T K + e^{eps} I.
    Returned as float64 arrays of the correctly rounded values (and the gap, rounded after the subtraction)."""
    if mp is None:
        return _scipy_route(p, eps, x)
    mp.mp.dps = MP_DIGITS
    k, bd, e, be, lv = p[KD], p[BD], p[KE], p[BE], p[LV]
    l_dim, d = k.shape
    km = [[mp.mpf(float(k[l, j])) for j in range(d)] for l in range(l_dim)]
    em = [[mp.mpf(float(e[i, l])) for l in range(l_dim)] for i in range(d)]
    bdm, bem, lvm = _mpv(bd), _mpv(be), _mpv(lv)
    epsm = mp.mpf(float(eps))
    evar = mp.exp(epsm)
    c = mp.matrix(d, d)
    for i in range(d):
        for j in range(i, d):
            v = mp.fsum(km[l][i] * km[l][j] for l in range(l_dim))
            c[i, j] = c[j, i] = v
        c[i, i] += evar
    ch = mp.cholesky(c)
    logdet = 2 * mp.fsum(mp.log(ch[i, i]) for i in range(d))
    log2pi = mp.log(2 * mp.pi)
    t = mp.fsum(mp.exp(lvm[l]) * mp.fsum(km[l][j] ** 2 for j in range(d)) for l in range(l_dim))
    klc = mp.fsum(mp.exp(v) - 1 - v for v in lvm)
    logp, elbo, gap = [], [], []
    for row in np.asarray(x, np.float64):
        xm = _mpv(row)
        y = []
        for i in range(d):                                     # forward substitution: ch y = x - b_d
            y.append((xm[i] - bdm[i] - mp.fsum(ch[i, j] * y[j] for j in range(i))) / ch[i, i])
        quad = mp.fsum(v * v for v in y)
        lp = -(quad + logdet + d * log2pi) / 2
        mu = [bem[l] + mp.fsum(xm[i] * em[i][l] for i in range(d)) for l in range(l_dim)]
        r = [bdm[j] - xm[j] + mp.fsum(mu[l] * km[l][j] for l in range(l_dim)) for j in range(d)]
        el = -(mp.exp(-epsm) * (mp.fsum(v * v for v in r) + t) + d * (epsm + log2pi)) / 2 - (klc + mp.fsum(v * v for v in mu)) / 2
        logp.append(float(lp))
        elbo.append(float(el))
        gap.append(float(lp - el))
    return np.array(logp), np.array(elbo), np.array(gap), float(logdet)


def _scipy_route(p, eps, x):
    if eps < -8.0:
        raise RuntimeError("without mpmath the independent evaluation is scipy's float64 logpdf, which is only trusted for eps >= -8")
    from scipy.stats import multivariate_normal
    k, bd = p[KD], p[BD]
    d = k.shape[1]
    cov = gram(k) + np.exp(eps) * np.eye(d)
    logp = np.atleast_1d(multivariate_normal.logpdf(x, mean=bd, cov=cov))
    r = evaluate(p, eps, x)                                    # no independent ELBO on this route: the formulae again
    return logp, r["elbo"], logp - r["elbo"], float(np.linalg.slogdet(cov)[1])


def main():
    from tests import exact_loglik_cases as K
    rows = 24
    worst = {"logp": (0.0, ""), "elbo": (0.0, ""), "logdet": (0.0, "")}
    for name, d, l_dim, eps_cli in K.all_cases() + K.all_cases(ill=True):
        p, _, _, eps = K.make_model(d, l_dim, eps_cli)
        x = K.make_rows(p, eps, rows)
        r = evaluate(p, eps, x)
        lp, el, _, ld = high_precision(p, eps, x)
        b1 = K.logp_bound(d, r["quad"], r["logdet"], r["off"], r["norm"], eps)
        u1 = float(np.max(np.abs(r["logp"] - lp) / b1))
        u2 = float(np.max(np.abs(r["elbo"] - el) / K.elbo_bound(r["M"])))
        u3 = abs(r["logdet"] - ld) / K.logdet_bound(d, r["logdet"], r["off"], r["norm"], eps)
        print(f"{name:18s} sweeps {r['sweeps']:2d}  cond {r['cond']:.2e}  |d log p| {np.max(np.abs(r['logp'] - lp)):.2e} = {u1:.4f}  "
              f"|d ELBO| {np.max(np.abs(r['elbo'] - el)):.2e} = {u2:.4f}  |d logdet| = {u3:.4f}  min gap {np.min(r['gap']):.3e}  (units of the bounds)")
        for key, u in (("logp", u1), ("elbo", u2), ("logdet", u3)):
            worst[key] = max(worst[key], (u, name))
    for key, (u, name) in worst.items():
        print(f"worst {key}: {u:.4f} of its bound on {name}")


if __name__ == "__main__":
    main()
