"""NumPy float64 restatement of vaek_elbo_hvp_replicas and vaek_elbo_hessian_lanczos_replicas (csrc/elbo_hessian.hip), from the CPU
ALONE (no GPU, no kernel): the negated exact mean ELBO f of a one-decoder linear VAE, its gradient, Hessian-vector products and the
Lanczos run with full reorthogonalisation, by the formulas of include/vaek.h.

theta is the flat parameter vector in the library's leaf order -- E [D][L], b_e [L], K [L][D], b_d [D], epsilon_p [L] and, under
tunable_eps, epsilon [1] -- holding float32 values; x is [rows][D], float32 values too.  Everything is float64.

MAGNITUDE IMAGES.  Model(..., mag=True) evaluates the same formulas with every operand replaced by its absolute value and every
subtraction by an addition: f, the gradient and H v come out as the sums of the magnitudes of their terms.  A rounding bound for a
value computed in another summation order is a small multiple of n u times its magnitude image (a running-error bound), which is what
the tests state theirs against; it stays meaningful where the value itself cancels to zero.

An INDEPENDENT evaluation checks the formulas: torch float64 autograd of f written row by row from the ELBO's definition (mu = x E +
b_e, r = mu K + b_d - x, ...), never through S.

    python tools/elbo_hessian_reference.py     # per case of tests/elbo_hessian_cases.py: HVP and gradient against autograd, the Lanczos bounds

It is a restatement of the algorithm, not of the instruction stream: summation order and fused multiply-adds differ, and late Lanczos
coefficients are legitimately sensitive to that, so alpha and beta are not comparable element by element with the device's; the Ritz
values and their residual bounds are."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2PI = float(np.log(2.0 * np.pi))
HEAD, MAX_STEPS = 12, 32
RECORD_LEN = HEAD + 4 * MAX_STEPS
BREAKDOWN = 2.0 ** -40


def param_count(D, L, tdv):
    return 2 * D * L + 2 * L + D + (1 if tdv else 0)


def offsets(D, L):
    """Flat offsets of b_e (U = [E; b_e] starts at 0), K, b_d, epsilon_p, epsilon."""
    off_wd = (D + 1) * L
    off_bd = off_wd + L * D
    return D * L, off_wd, off_bd, off_bd + D, off_bd + D + L


def moments(x):
    """S = (1 / rows) sum [x; 1][x; 1]^T, (D + 1) x (D + 1)."""
    x1 = np.concatenate([np.asarray(x, np.float64), np.ones((x.shape[0], 1))], axis=1)
    return x1.T @ x1 / x.shape[0]


class Model:
    """f, gradient and H v of one model on one set of rows; mag: the magnitude image of each."""

    def __init__(self, theta, x, D, L, eps_cli, tdv, mag=False):
        theta = np.asarray(theta, np.float64)
        assert theta.shape == (param_count(D, L, tdv),)
        self.D, self.L, self.tdv, self.mag, self.P = D, L, tdv, mag, theta.size
        _, self.o_k, self.o_bd, self.o_p, self.o_c = offsets(D, L)
        ab = np.abs if mag else (lambda v: v)
        self.sg = 1.0 if mag else -1.0                                  # the sign a subtraction carries
        x = np.asarray(x, np.float64)
        self.rows = x.shape[0]
        self.S = moments(ab(x))
        self.U = ab(theta[:self.o_k].reshape(D + 1, L))
        self.K = ab(theta[self.o_k:self.o_bd].reshape(L, D))
        bd = ab(theta[self.o_bd:self.o_p])
        self.p = theta[self.o_p:self.o_p + L]
        c = theta[self.o_c] if tdv else 1.0
        self.eps_cli = ab(float(eps_cli))
        self.eps = float(c) * float(eps_cli)                            # float64 product: f is a smooth function of c
        self.a = np.exp(-self.eps)
        self.w = np.exp(self.p)
        C = np.concatenate([self.sg * np.eye(D), bd[None, :]], axis=0)
        self.R = self.U @ self.K + C
        self.k2 = np.sum(self.K * self.K, axis=1)
        self.SR = self.S @ self.R
        self.Q = float(np.sum(self.R * self.SR) + np.sum(self.w * self.k2))
        self.G = self.a * self.SR

    def f(self):
        sg, D = self.sg, self.D
        kl = np.sum(self.w + sg * 1.0 + sg * (np.abs(self.p) if self.mag else self.p))
        eps = abs(self.eps) if self.mag else self.eps
        return float(0.5 * np.sum(self.U * (self.S @ self.U)) + 0.5 * kl + 0.5 * self.a * self.Q + 0.5 * D * (eps + LOG2PI))

    def grad(self):
        sg, a, w = self.sg, self.a, self.w
        g = np.zeros(self.P)
        g[:self.o_k] = (self.S @ self.U + self.G @ self.K.T).ravel()
        g[self.o_k:self.o_bd] = (self.U.T @ self.G + a * w[:, None] * self.K).ravel()
        g[self.o_bd:self.o_p] = self.G[self.D]
        g[self.o_p:self.o_p + self.L] = 0.5 * (w + sg * 1.0) + 0.5 * a * w * self.k2
        if self.tdv:
            g[self.o_c] = self.eps_cli * (0.5 * self.D + sg * 0.5 * a * self.Q)
        return g

    def hvp(self, v):
        """H v for v [P] or [n, P]."""
        v = np.asarray(v, np.float64)
        one = v.ndim == 1
        V = np.abs(v.reshape(-1, self.P)) if self.mag else v.reshape(-1, self.P)
        n, D, L, sg, a, w = V.shape[0], self.D, self.L, self.sg, self.a, self.w
        dU = V[:, :self.o_k].reshape(n, D + 1, L)
        dK = V[:, self.o_k:self.o_bd].reshape(n, L, D)
        dbd = V[:, self.o_bd:self.o_p]
        dp = V[:, self.o_p:self.o_p + L]
        deps = (self.eps_cli * V[:, self.o_c] if self.tdv else np.zeros(n))[:, None, None]
        dw = w * dp
        dC = np.zeros((n, D + 1, D))
        dC[:, D, :] = dbd
        dR = dU @ self.K + self.U @ dK + dC
        dG = a * (self.S @ dR) + sg * deps * self.G
        kdk = np.sum(self.K * dK, axis=2)
        out = np.zeros((n, self.P))
        out[:, :self.o_k] = (self.S @ dU + dG @ self.K.T + self.G @ dK.transpose(0, 2, 1)).reshape(n, -1)
        hk = (dU.transpose(0, 2, 1) @ self.G + self.U.T @ dG + a * w[None, :, None] * dK + a * dw[:, :, None] * self.K
              + sg * deps * a * w[None, :, None] * self.K)
        out[:, self.o_k:self.o_bd] = hk.reshape(n, -1)
        out[:, self.o_bd:self.o_p] = dG[:, D, :]
        d1 = deps[:, :, 0]
        out[:, self.o_p:self.o_p + L] = 0.5 * dw + 0.5 * a * dw * self.k2 + a * w * kdk + sg * 0.5 * d1 * a * w * self.k2
        if self.tdv:
            dQ = 2.0 * np.sum(self.SR * dR, axis=(1, 2)) + np.sum(dw * self.k2 + 2.0 * w * kdk, axis=1)
            out[:, self.o_c] = self.eps_cli * (0.5 * d1[:, 0] * a * self.Q + sg * 0.5 * a * dQ)
        return out[0] if one else out

    def hessian(self):
        """H as a matrix: P products with unit vectors, 256 at a time."""
        H = np.zeros((self.P, self.P))
        eye = np.eye(self.P)
        for lo in range(0, self.P, 256):
            H[lo:lo + 256] = self.hvp(eye[lo:lo + 256])
        return H


def lanczos(hvp, v0, steps):
    """The device's run: full reorthogonalisation (classical Gram-Schmidt twice), the breakdown rule, T solved by eigh.  Returns a dict:
    k, alpha [k], beta [k] (beta[k - 1] = beta_k), theta [k] ascending, rho [k], omega, basis [k, P], norm_t."""
    v0 = np.asarray(v0, np.float64)
    P = v0.size
    n0 = float(np.sqrt(np.sum(v0 * v0)))
    kmax = min(int(steps), P) if (n0 > 0.0 and np.isfinite(n0)) else 0
    basis, alpha, beta = np.zeros((max(kmax, 1), P)), [], []
    k, scale = 0, 0.0
    if kmax:
        basis[0] = v0 / n0
    for j in range(kmax):
        w = hvp(basis[j])
        al = 0.0
        for _ in range(2):
            c = basis[:j + 1] @ w
            w = w - c @ basis[:j + 1]
            al += c[j]
        be = float(np.sqrt(np.sum(w * w)))
        alpha.append(al)
        beta.append(be)
        k = j + 1
        scale = max(scale, abs(al))
        if be <= BREAKDOWN * scale or k == kmax:
            break
        scale = max(scale, be)
        basis[k] = w / be
    alpha, beta, basis = np.array(alpha), np.array(beta), basis[:k]
    res = dict(k=k, alpha=alpha, beta=beta, basis=basis, omega=0.0, theta=np.zeros(0), rho=np.zeros(0), norm_t=0.0)
    if k:
        T = tridiagonal(alpha, beta)
        theta, s = np.linalg.eigh(T)
        res.update(theta=theta, rho=np.abs(beta[k - 1] * s[k - 1]), norm_t=float(np.sqrt(np.sum(T * T))))
        if k > 1:
            g = basis @ basis.T
            res["omega"] = float(np.max(np.abs(g[np.triu_indices(k, 1)])))
    return res


def tridiagonal(alpha, beta):
    """T of a run's alpha_1 .. alpha_k and beta_1 .. beta_{k-1} (beta_k is the residual, not an entry)."""
    k = len(alpha)
    return np.diag(np.asarray(alpha, np.float64)) + np.diag(np.asarray(beta, np.float64)[:k - 1], 1) + np.diag(np.asarray(beta, np.float64)[:k - 1], -1)


def record(model, run):
    """The 140-double record of vaek_elbo_hessian_lanczos_replicas (sweeps and off_F, which are the device solve's, as 0)."""
    rec = np.zeros(RECORD_LEN)
    k = run["k"]
    rec[0], rec[1], rec[2] = model.f(), float(np.sqrt(np.sum(model.grad() ** 2))), k
    rec[3] = run["beta"][k - 1] if k else 0.0
    rec[6], rec[7], rec[8], rec[11] = run["norm_t"], model.rows, model.eps, run["omega"]
    if k:
        rec[9], rec[10] = run["theta"][-1], run["theta"][0]
        for i, key in enumerate(("theta", "rho", "alpha", "beta")):
            rec[HEAD + i * MAX_STEPS:HEAD + i * MAX_STEPS + k] = run[key]
    return rec


# ---- the independent evaluation: torch float64 autograd of f written row by row ---------------------------------------------------------
def torch_f(theta, x, D, L, eps_cli, tdv):
    """f(theta) as a torch scalar: minus the mean over rows of the ELBO of include/vaek.h, never through S."""
    import torch
    _, o_k, o_bd, o_p, o_c = offsets(D, L)
    E, be = theta[:D * L].reshape(D, L), theta[D * L:o_k]
    K, bd, p = theta[o_k:o_bd].reshape(L, D), theta[o_bd:o_p], theta[o_p:o_p + L]
    eps = theta[o_c] * eps_cli if tdv else torch.as_tensor(float(eps_cli), dtype=theta.dtype)
    mu = x @ E + be
    r = mu @ K + bd - x
    T = torch.sum(torch.exp(p) * torch.sum(K * K, dim=1))
    elbo = (-0.5 * (torch.exp(-eps) * (torch.sum(r * r, dim=1) + T) + D * (eps + LOG2PI))
            - 0.5 * torch.sum(torch.exp(p)[None, :] + mu * mu - 1.0 - p[None, :], dim=1))
    return -torch.mean(elbo)


def autograd(theta, x, D, L, eps_cli, tdv):
    """(f, gradient [P], Hessian [P, P]) by torch float64 autograd, as NumPy arrays."""
    import torch
    th = torch.tensor(np.asarray(theta, np.float64), dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
    fn = lambda t: torch_f(t, xt, D, L, eps_cli, tdv)
    val = fn(th)
    g, = torch.autograd.grad(val, th)
    H = torch.autograd.functional.hessian(fn, th.detach(), vectorize=True)
    H = 0.5 * (H + H.T)
    return float(val.detach()), g.numpy(), H.numpy()


def main():
    sys.path.insert(0, ROOT)
    from tests import elbo_hessian_cases as K
    for case in K.CASES:
        theta, x = K.make_theta(case), K.make_rows(case, case.rows[0])
        m = Model(theta, x, case.D, case.L, case.eps_cli, case.tdv)
        f, g, H = autograd(theta, x, case.D, case.L, case.eps_cli, case.tdv)
        V = K.directions(case)
        hv, scale = m.hvp(V), np.max(np.abs(H @ V.T))
        lam = np.linalg.eigvalsh(H)
        norm_h = max(abs(lam[0]), abs(lam[-1]))
        run = lanczos(m.hvp, K.start_vector(case), case.steps[-1])
        gap = np.array([np.min(np.abs(lam - th)) for th in run["theta"]])
        print(f"{case.name}: P {m.P}  |f - autograd| {abs(m.f() - f):.2e}  grad {np.max(np.abs(m.grad() - g)):.2e}  "
              f"max|Hv - H_autograd v| / max|H v| {np.max(np.abs(hv - V @ H)) / scale:.2e}  k {run['k']}  omega {run['omega']:.2e}  "
              f"theta_max {run['theta'][-1]:.6e} (lambda_max {lam[-1]:.6e}, rho {run['rho'][-1]:.1e})  theta_min {run['theta'][0]:.6e} "
              f"(lambda_min {lam[0]:.6e})  worst (gap - rho) / |H| {np.max(gap - run['rho']) / norm_h:.2e}")


if __name__ == "__main__":
    main()
