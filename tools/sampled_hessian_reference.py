"""NumPy float64 restatement of vaek_sampled_elbo_hvp_replicas and vaek_sampled_elbo_hessian_lanczos_replicas
(csrc/sampled_hessian.hip), from the CPU ALONE (no GPU, no kernel): the sample-average negated ELBO f_K of a linear VAE with one or
two decoders on fixed rows and fixed latent samples, its gradient and Hessian-vector products by the explicit formulas of
include/vaek.h (forward over reverse, written out).  The Lanczos run is tools/elbo_hessian_reference.py's `lanczos` on this hvp.

theta is the flat parameter vector in the library's leaf order -- E [D][L], b_e [L], K [L][D], b_d [D], with two decoders K_s [L][D],
b_s [D], then epsilon_p [L] and, under tunable_eps, epsilon [1] -- holding float32 values; x is [rows][D] and xi [rows][K][L], float32
values too.  Everything is float64.  Column q = i K + k is (row i, sample k).

MAGNITUDE IMAGES.  Model(..., mag=True) evaluates the same formulas with every operand replaced by its absolute value and every
subtraction by an addition; sigma, sigma' and sigma'' enter as the absolute values of their computed (true) results, the exponentials
as themselves.  A rounding bound for a value computed in another summation order is a small multiple of n u times its magnitude image.

An INDEPENDENT evaluation checks the formulas: torch float64 autograd of f_K written from its definition (torch_f).

    python tools/sampled_hessian_reference.py     # per case of tests/sampled_hessian_cases.py: f, gradient and H v against autograd"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2PI = float(np.log(2.0 * np.pi))
RECORD_LEN = 142


def param_count(D, L, tdv, sig):
    return D * L + L + (2 if sig else 1) * (L * D + D) + L + (1 if tdv else 0)


def offsets(D, L, sig):
    """Flat offsets of b_e, K, b_d, K_s, b_s, epsilon_p, epsilon (K_s and b_s empty with one decoder)."""
    o_be = D * L
    o_k = o_be + L
    o_bd = o_k + L * D
    o_ks = o_bd + D
    o_bs = o_ks + (L * D if sig else 0)
    o_p = o_bs + (D if sig else 0)
    return o_be, o_k, o_bd, o_ks, o_bs, o_p, o_p + L


def _sigmoid(u):
    return 1.0 / (1.0 + np.exp(-u))


class Model:
    """f_K, its gradient and H v of one model on one set of rows and samples; mag: the magnitude image of each."""

    def __init__(self, theta, x, xi, D, L, eps_cli, tdv, sig, mag=False):
        theta = np.asarray(theta, np.float64)
        assert theta.shape == (param_count(D, L, tdv, sig),)
        x, xi = np.asarray(x, np.float64), np.asarray(xi, np.float64)
        self.rows, self.K_samples = xi.shape[0], xi.shape[1]
        assert x.shape == (self.rows, D) and xi.shape[2] == L
        self.D, self.L, self.tdv, self.sig, self.mag, self.P = D, L, tdv, sig, mag, theta.size
        self.o = o_be, o_k, o_bd, o_ks, o_bs, o_p, o_c = offsets(D, L, sig)
        N = self.N = self.rows * self.K_samples
        X = np.repeat(x, self.K_samples, axis=0)                        # [N, D]: column q = i K + k
        XI = xi.reshape(N, L)
        E, be = theta[:o_be].reshape(D, L), theta[o_be:o_k]
        Kd, bd = theta[o_k:o_bd].reshape(L, D), theta[o_bd:o_ks]
        Ks = theta[o_ks:o_bs].reshape(L, D) if sig else np.zeros((L, D))
        bs = theta[o_bs:o_p] if sig else np.zeros(D)
        self.p = theta[o_p:o_p + L]
        c = theta[o_c] if tdv else 1.0
        self.eps = float(c) * float(eps_cli)                            # float64 product: f_K is a smooth function of c
        self.a = np.exp(-self.eps)
        self.w, self.sd = np.exp(self.p), np.exp(0.5 * self.p)
        self.c0, self.c1 = self.a / N, 1.0 / N
        # the true sigmoid and its derivatives: the magnitude image takes their absolute values, not those of a magnitude pass
        if sig:
            s_true = X @ E + be + self.sd * XI
            sgm = _sigmoid(s_true @ Ks + bs)
            sp = sgm * (1.0 - sgm)
            spp = sp * (1.0 - 2.0 * sgm)
        else:
            sgm = sp = spp = np.zeros((N, D))
        ab = np.abs if mag else (lambda v: v)
        self.sgn = 1.0 if mag else -1.0                                 # the sign a subtraction carries
        self.eps_cli = ab(float(eps_cli))
        self.X, self.XI, self.E, self.be, self.Kd, self.bd, self.Ks, self.bs = (ab(v) for v in (X, XI, E, be, Kd, bd, Ks, bs))
        self.sgm, self.sp, self.spp = ab(sgm), ab(sp), ab(spp)
        self.mu = self.X @ self.E + self.be
        self.s = self.mu + self.sd * self.XI
        self.r = self.s @ self.Kd + self.bd + self.sgm + self.sgn * self.X
        self.gy = self.c0 * self.r
        self.ga = self.gy * self.sp
        self.gs = self.gy @ self.Kd.T + self.ga @ self.Ks.T
        self.gmu = self.gs + self.c1 * self.mu
        self.aQ = float(np.sum(self.c0 * self.r * self.r))

    def f(self):
        sgn = self.sgn
        kl = np.sum(self.w + sgn * 1.0 + sgn * (np.abs(self.p) if self.mag else self.p))
        eps = abs(self.eps) if self.mag else self.eps
        return float(np.sum(self.c1 * 0.5 * self.mu * self.mu) + 0.5 * kl + 0.5 * self.aQ + 0.5 * self.D * (eps + LOG2PI))

    def grad(self):
        o_be, o_k, o_bd, o_ks, o_bs, o_p, o_c = self.o
        g = np.zeros(self.P)
        g[:o_be] = (self.X.T @ self.gmu).ravel()
        g[o_be:o_k] = self.gmu.sum(axis=0)
        g[o_k:o_bd] = (self.s.T @ self.gy).ravel()
        g[o_bd:o_ks] = self.gy.sum(axis=0)
        if self.sig:
            g[o_ks:o_bs] = (self.s.T @ self.ga).ravel()
            g[o_bs:o_p] = self.ga.sum(axis=0)
        g[o_p:o_p + self.L] = 0.5 * (self.w + self.sgn * 1.0) + np.sum(self.gs * (0.5 * self.sd * self.XI), axis=0)
        if self.tdv:
            g[o_c] = self.eps_cli * (0.5 * self.D + self.sgn * 0.5 * self.aQ)
        return g

    def _hvp1(self, v):
        o_be, o_k, o_bd, o_ks, o_bs, o_p, o_c = self.o
        D, L, sgn = self.D, self.L, self.sgn
        dE, dbe = v[:o_be].reshape(D, L), v[o_be:o_k]
        dK, dbd = v[o_k:o_bd].reshape(L, D), v[o_bd:o_ks]
        dKs = v[o_ks:o_bs].reshape(L, D) if self.sig else np.zeros((L, D))
        dbs = v[o_bs:o_p] if self.sig else np.zeros(D)
        dp = v[o_p:o_p + L]
        deps = self.eps_cli * v[o_c] if self.tdv else 0.0
        hx = 0.5 * self.sd * self.XI
        dmu = self.X @ dE + dbe
        ds = dmu + dp * hx
        dy = ds @ self.Kd + self.s @ dK + dbd
        du = ds @ self.Ks + self.s @ dKs + dbs
        dr = dy + self.sp * du
        dgy = self.c0 * (dr + sgn * deps * self.r)
        dga = dgy * self.sp + self.gy * self.spp * du
        dgs = dgy @ self.Kd.T + self.gy @ dK.T + dga @ self.Ks.T + self.ga @ dKs.T
        dgmu = dgs + self.c1 * dmu
        out = np.zeros(self.P)
        out[:o_be] = (self.X.T @ dgmu).ravel()
        out[o_be:o_k] = dgmu.sum(axis=0)
        out[o_k:o_bd] = (ds.T @ self.gy + self.s.T @ dgy).ravel()
        out[o_bd:o_ks] = dgy.sum(axis=0)
        if self.sig:
            out[o_ks:o_bs] = (ds.T @ self.ga + self.s.T @ dga).ravel()
            out[o_bs:o_p] = dga.sum(axis=0)
        out[o_p:o_p + L] = 0.5 * self.w * dp + np.sum(dgs * hx + self.gs * (0.5 * dp * hx), axis=0)
        if self.tdv:
            out[o_c] = self.eps_cli * float(np.sum(self.c0 * self.r * (0.5 * deps * self.r + sgn * dr)))
        return out

    def hvp(self, v):
        """H v for v [P] or [n, P]."""
        v = np.asarray(v, np.float64)
        V = np.abs(v.reshape(-1, self.P)) if self.mag else v.reshape(-1, self.P)
        out = np.stack([self._hvp1(row) for row in V])
        return out[0] if v.ndim == 1 else out

    def hessian(self):
        """H as a matrix: P products with unit vectors."""
        return self.hvp(np.eye(self.P))


# ---- the independent evaluation: torch float64 autograd of f_K written from its definition ----------------------------------------------
def torch_f(theta, x, xi, D, L, eps_cli, tdv, sig):
    """f_K(theta) as a torch scalar; x [rows, D], xi [rows, K, L]."""
    import torch
    o_be, o_k, o_bd, o_ks, o_bs, o_p, o_c = offsets(D, L, sig)
    E, be = theta[:o_be].reshape(D, L), theta[o_be:o_k]
    Kd, bd, p = theta[o_k:o_bd].reshape(L, D), theta[o_bd:o_ks], theta[o_p:o_p + L]
    eps = theta[o_c] * eps_cli if tdv else torch.as_tensor(float(eps_cli), dtype=theta.dtype)
    mu = x @ E + be                                                     # [rows, L]
    z = mu[:, None, :] + torch.exp(0.5 * p) * xi                        # [rows, K, L]
    y = z @ Kd + bd
    if sig:
        y = y + torch.sigmoid(z @ theta[o_ks:o_bs].reshape(L, D) + theta[o_bs:o_p])
    Q = torch.mean(torch.sum((y - x[:, None, :]) ** 2, dim=2))
    return (torch.mean(0.5 * torch.sum(mu * mu, dim=1)) + 0.5 * torch.sum(torch.exp(p) - 1.0 - p) + 0.5 * torch.exp(-eps) * Q
            + 0.5 * D * (eps + LOG2PI))


def autograd(theta, x, xi, D, L, eps_cli, tdv, sig, V=None, dense=False):
    """(f_K, gradient [P], H V^T as [n, P] or None, dense H or None) by torch float64 autograd, as NumPy arrays."""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    xt, xit = t64(x), t64(xi)
    fn = lambda t: torch_f(t, xt, xit, D, L, eps_cli, tdv, sig)
    th = t64(theta).requires_grad_(True)
    val = fn(th)
    g, = torch.autograd.grad(val, th)
    hv = None
    if V is not None:
        hv = np.stack([torch.autograd.functional.hvp(fn, th.detach(), t64(v))[1].numpy() for v in np.asarray(V, np.float64)])
    H = None
    if dense:
        H = torch.autograd.functional.hessian(fn, th.detach(), vectorize=True)
        H = (0.5 * (H + H.T)).numpy()
    return float(val.detach()), g.numpy(), hv, H


def main():
    sys.path.insert(0, ROOT)
    from tests import sampled_hessian_cases as K
    for case in K.CASES:
        rows = case.rows[0]
        theta, x, xi = K.make_theta(case), K.make_rows(case, rows), K.make_samples(case, rows)
        args = (case.D, case.L, case.eps_cli, case.tdv, case.sig)
        m, mg = Model(theta, x, xi, *args), Model(theta, x, xi, *args, mag=True)
        V = K.directions(case)
        f, g, hv, _ = autograd(theta, x, xi, *args, V=V)
        worst = max(K.worst_ratio(m.f() - f, K.value_bound(case, rows, mg.f())),
                    K.worst_ratio(m.grad() - g, K.value_bound(case, rows, mg.grad())),
                    K.worst_ratio(m.hvp(V) - hv, K.value_bound(case, rows, mg.hvp(V))))
        print(f"{case.name}: P {m.P}  columns {m.N}  f_K {m.f():.12e}  |grad| {np.linalg.norm(m.grad()):.6e}  "
              f"worst |restatement - autograd| / bound {worst:.3e}")


if __name__ == "__main__":
    main()
