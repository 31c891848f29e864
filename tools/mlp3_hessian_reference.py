"""NumPy float64 restatement of vaek_mlp3_sampled_elbo_hvp_replicas and vaek_mlp3_sampled_elbo_hessian_lanczos_replicas
(csrc/mlp3_hessian.hip), from the CPU ALONE (no GPU, no kernel): the sample-average negated ELBO f_K of a three-hidden-layer MLP VAE on
fixed rows and fixed latent samples, its gradient and Hessian-vector products by the explicit formulas of include/vaek.h (forward over
reverse through the two four-Dense relu stacks, written out).  The Lanczos run is tools/elbo_hessian_reference.py's `lanczos` on this hvp.

theta is the flat parameter vector in the library's leaf order -- Encoder FC0 kernel [D][h0], bias, .. FC3, Decoder FC0 .. FC3,
epsilon_p [L] and, under tunable_eps, epsilon [1] -- holding float32 values; x is [rows][D] and xi [rows][K][L], float32 values too.
Everything is float64.  Column q = i K + k is (row i, sample k).  A unit is live iff its float64 pre-activation is > 0.

MAGNITUDE IMAGES.  Model(..., mag=True) evaluates the same formulas with every operand replaced by its absolute value and every
subtraction by an addition; the relu masks are those of the TRUE pass (kept, not recomputed), the exponentials enter as themselves.  A
rounding bound for a value computed in another summation order is a small multiple of n u times its magnitude image.

An INDEPENDENT evaluation checks the formulas: torch float64 autograd of f_K written from its definition (torch_f).

    python tools/mlp3_hessian_reference.py     # per shape of tests/mlp3_hessian_cases.py: f, gradient and H v against autograd, the
                                               # smallest |pre-activation|, and the CPU Lanczos run of the breakdown case"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2PI = float(np.log(2.0 * np.pi))
RECORD_LEN = 142


def layer_sizes(D, L, enc, dec):
    """The eight Dense layers as (n_in, n_out): the encoder's four, then the decoder's."""
    e, d = [D] + list(enc) + [L], [L] + list(dec) + [D]
    return [(e[i], e[i + 1]) for i in range(4)] + [(d[i], d[i + 1]) for i in range(4)]


def layer_offsets(D, L, enc, dec):
    """Flat offset of every layer's kernel (its bias follows), then of epsilon_p."""
    offs, o = [], 0
    for n_in, n_out in layer_sizes(D, L, enc, dec):
        offs.append(o)
        o += (n_in + 1) * n_out
    return offs, o


def param_count(D, L, enc, dec, tdv):
    return layer_offsets(D, L, enc, dec)[1] + L + (1 if tdv else 0)


def _split(vec, D, L, enc, dec):
    """[(W, b)] * 8 views of a flat vector."""
    offs, _ = layer_offsets(D, L, enc, dec)
    out = []
    for (n_in, n_out), o in zip(layer_sizes(D, L, enc, dec), offs):
        out.append((vec[o:o + n_in * n_out].reshape(n_in, n_out), vec[o + n_in * n_out:o + (n_in + 1) * n_out]))
    return out


class Model:
    """f_K, its gradient and H v of one model on one set of rows and samples; mag: the magnitude image of each."""

    def __init__(self, theta, x, xi, D, L, enc, dec, eps_cli, tdv, mag=False):
        theta = np.asarray(theta, np.float64)
        self.shape = (D, L, tuple(enc), tuple(dec))
        assert theta.shape == (param_count(*self.shape, tdv),)
        x, xi = np.asarray(x, np.float64), np.asarray(xi, np.float64)
        self.rows, self.K_samples = xi.shape[0], xi.shape[1]
        assert x.shape == (self.rows, D) and xi.shape[2] == L
        self.D, self.L, self.tdv, self.mag, self.P = D, L, tdv, mag, theta.size
        self.o_p = layer_offsets(*self.shape)[1]
        self.o_c = self.o_p + L
        N = self.N = self.rows * self.K_samples
        X = np.repeat(x, self.K_samples, axis=0)                        # [N, D]: column q = i K + k
        XI = xi.reshape(N, L)
        self.p = theta[self.o_p:self.o_p + L]
        c = theta[self.o_c] if tdv else 1.0
        self.eps = float(c) * float(eps_cli)
        self.w, self.sd = np.exp(self.p), np.exp(0.5 * self.p)
        self.c0, self.c1 = np.exp(-self.eps) / N, 1.0 / N
        layers = _split(theta, *self.shape)
        # the TRUE pass: its masks are the function's, and the magnitude image keeps them
        self.masks, self.pres = [None] * 8, []
        h = X
        for i in range(8):
            if i == 4:
                h = h + self.sd * XI
            a = h @ layers[i][0] + layers[i][1]
            if i % 4 < 3:
                self.pres.append(a)
                self.masks[i] = a > 0.0
                h = np.where(self.masks[i], a, 0.0)
            else:
                h = a
        ab = np.abs if mag else (lambda v: v)
        self.sgn = 1.0 if mag else -1.0                                 # the sign a subtraction carries
        self.eps_cli = ab(float(eps_cli))
        self.X, self.XI = ab(X), ab(XI)
        self.layers = [(ab(W), ab(b)) for W, b in layers]
        self.hx = 0.5 * self.sd * self.XI
        # forward with the kept masks: acts[i] = the input of layer i
        self.acts = [None] * 8
        h = self.X
        for i in range(8):
            if i == 4:
                self.mu = h
                h = h + self.sd * self.XI
            self.acts[i] = h
            a = h @ self.layers[i][0] + self.layers[i][1]
            h = a * self.masks[i] if self.masks[i] is not None else a
        self.r = h + self.sgn * self.X
        self.aQ = float(np.sum(self.c0 * self.r * self.r))
        # backward: ga[i] = the masked gradient at layer i's output
        self.ga = [None] * 8
        g = self.c0 * self.r
        for i in range(7, -1, -1):
            if i == 3:
                self.gs = g
                g = g + self.c1 * self.mu
            if self.masks[i] is not None:
                g = g * self.masks[i]
            self.ga[i] = g
            g = g @ self.layers[i][0].T

    def min_abs_pre(self):
        return min(float(np.min(np.abs(a))) for a in self.pres)

    def f(self):
        sgn = self.sgn
        kl = np.sum(self.w + sgn * 1.0 + sgn * (np.abs(self.p) if self.mag else self.p))
        eps = abs(self.eps) if self.mag else self.eps
        return float(np.sum(self.c1 * 0.5 * self.mu * self.mu) + 0.5 * kl + 0.5 * self.aQ + 0.5 * self.D * (eps + LOG2PI))

    def _pack(self, pairs, p_leaf, c_leaf):
        out = np.zeros(self.P)
        for (dW, db), (W, b) in zip(pairs, _split(out, *self.shape)):
            W[...] = dW
            b[...] = db
        out[self.o_p:self.o_p + self.L] = p_leaf
        if self.tdv:
            out[self.o_c] = c_leaf
        return out

    def grad(self):
        pairs = [(self.acts[i].T @ self.ga[i], self.ga[i].sum(axis=0)) for i in range(8)]
        p_leaf = 0.5 * (self.w + self.sgn * 1.0) + np.sum(self.gs * self.hx, axis=0)
        return self._pack(pairs, p_leaf, self.eps_cli * (0.5 * self.D + self.sgn * 0.5 * self.aQ))

    def _hvp1(self, v):
        sgn, L = self.sgn, self.L
        dl = _split(v, *self.shape)
        dp = v[self.o_p:self.o_p + L]
        deps = self.eps_cli * v[self.o_c] if self.tdv else 0.0
        # tangent forward
        dacts = [None] * 8
        dh = np.zeros_like(self.X)
        for i in range(8):
            if i == 4:
                dmu = dh
                dh = dh + dp * self.hx
            dacts[i] = dh
            da = dh @ self.layers[i][0] + self.acts[i] @ dl[i][0] + dl[i][1]
            dh = da * self.masks[i] if self.masks[i] is not None else da
        dr = dh
        # tangent backward
        dga = [None] * 8
        dg = self.c0 * (dr + sgn * deps * self.r)
        for i in range(7, -1, -1):
            if i == 3:
                dgs = dg
                dg = dg + self.c1 * dmu
            if self.masks[i] is not None:
                dg = dg * self.masks[i]
            dga[i] = dg
            dg = dg @ self.layers[i][0].T + self.ga[i] @ dl[i][0].T
        pairs = [(dacts[i].T @ self.ga[i] + self.acts[i].T @ dga[i], dga[i].sum(axis=0)) for i in range(8)]
        p_leaf = 0.5 * self.w * dp + np.sum(dgs * self.hx + self.gs * (0.5 * dp * self.hx), axis=0)
        c_leaf = self.eps_cli * float(np.sum(self.c0 * self.r * (0.5 * deps * self.r + sgn * dr)))
        return self._pack(pairs, p_leaf, c_leaf)

    def hvp(self, v):
        """H v for v [P] or [n, P]."""
        v = np.asarray(v, np.float64)
        V = np.abs(v.reshape(-1, self.P)) if self.mag else v.reshape(-1, self.P)
        out = np.stack([self._hvp1(row) for row in V])
        return out[0] if v.ndim == 1 else out


def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lanczos(hvp, v0, steps):
    """The device's run on the restated H v: tools/elbo_hessian_reference.lanczos (full reorthogonalisation, classical Gram-Schmidt
    twice, the breakdown rule)."""
    return _sibling("elbo_hessian_reference").lanczos(hvp, v0, steps)


# ---- the independent evaluation: torch float64 autograd of f_K written from its definition ----------------------------------------------
def torch_f(theta, x, xi, D, L, enc, dec, eps_cli, tdv):
    """f_K(theta) as a torch scalar; x [rows, D], xi [rows, K, L]."""
    import torch
    offs, o_p = layer_offsets(D, L, enc, dec)
    sizes = layer_sizes(D, L, enc, dec)

    def stack(h, first):
        for i in range(first, first + 4):
            n_in, n_out = sizes[i]
            W = theta[offs[i]:offs[i] + n_in * n_out].reshape(n_in, n_out)
            h = h @ W + theta[offs[i] + n_in * n_out:offs[i] + (n_in + 1) * n_out]
            if i % 4 < 3:
                h = torch.relu(h)
        return h

    p = theta[o_p:o_p + L]
    eps = theta[o_p + L] * eps_cli if tdv else torch.as_tensor(float(eps_cli), dtype=theta.dtype)
    mu = stack(x, 0)                                                    # [rows, L]
    z = mu[:, None, :] + torch.exp(0.5 * p) * xi                        # [rows, K, L]
    y = stack(z, 4)
    Q = torch.mean(torch.sum((y - x[:, None, :]) ** 2, dim=2))
    return (torch.mean(0.5 * torch.sum(mu * mu, dim=1)) + 0.5 * torch.sum(torch.exp(p) - 1.0 - p) + 0.5 * torch.exp(-eps) * Q
            + 0.5 * D * (eps + LOG2PI))


def autograd(theta, x, xi, D, L, enc, dec, eps_cli, tdv, V=None):
    """(f_K, gradient [P], H V^T as [n, P] or None) by torch float64 autograd, as NumPy arrays."""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    xt, xit = t64(x), t64(xi)
    fn = lambda t: torch_f(t, xt, xit, D, L, enc, dec, eps_cli, tdv)
    th = t64(theta).requires_grad_(True)
    val = fn(th)
    g, = torch.autograd.grad(val, th)
    hv = None
    if V is not None:
        hv = np.stack([torch.autograd.functional.hvp(fn, th.detach(), t64(v))[1].numpy() for v in np.asarray(V, np.float64)])
    return float(val.detach()), g.numpy(), hv


def main():
    sys.path.insert(0, ROOT)
    from tests import mlp3_hessian_cases as K
    for name in K.SHAPES:
        for rows, samples in K.ROWS_K:
            case = (name, rows, samples)
            theta, x, xi = K.make_theta(name), K.make_rows(case), K.make_samples(case)
            m, mg = K.model(case), K.model(case, mag=True)
            V = K.directions(name)
            f, g, hv = autograd(theta, x, xi, *K.model_args(name), V=V)
            worst = max(K.worst_ratio(m.f() - f, K.value_bound(case, mg.f())), K.worst_ratio(m.grad() - g, K.value_bound(case, mg.grad())),
                        K.worst_ratio(m.hvp(V) - hv, K.value_bound(case, mg.hvp(V))))
            print(f"{name} rows {rows} K {samples}: P {m.P}  f_K {m.f():.12e}  |grad| {np.linalg.norm(m.grad()):.6e}  min |pre| "
                  f"{min(K.model(case, r).min_abs_pre() for r in range(K.R)):.2e}  worst |restatement - autograd| / bound {worst:.3e}")
    case = K.BREAKDOWN_CASE
    run = lanczos(K.model(case).hvp, K.start_vector(case[0]), 32)
    print(f"{case} from a random start: k {run['k']}  beta_k {run['beta'][-1]:.3e}  theta_max {run['theta'][-1]:.6e}")
    run = lanczos(K.model(case).hvp, K.breakdown_start(case), 32)
    print(f"{case} from breakdown_start (dead Decoder/FC1 units): k {run['k']}  alpha {run['alpha']}  beta {run['beta']}")


if __name__ == "__main__":
    main()
