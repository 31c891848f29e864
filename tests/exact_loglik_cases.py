"""The cases and the bounds of the exact log-likelihood tests, NumPy only: tests/test_gpu_exact_log_likelihood.py runs
vaek_exact_log_likelihood_replicas on them, tests/test_exact_log_likelihood_host.py and tools/exact_log_likelihood_reference.py the
float64 restatement against a 60-digit evaluation.

MODELS.  A parameter tree has oracle/elbo_oracle.py's leaf names; every leaf is float32-representable (what the device reads).
(D, L) in SHAPES: (3, 2) and (7, 7) odd D (the Jacobi padding index), (12, 20) L > D, (20, 4) D > L, (32, 32) the largest
instantiation.  The decoder kernel K [L][D] has its rows beyond the first `kept(L)` = min(3, L - 1) scaled by 1e-3 (collapsed
latents: K^T K is numerically rank-deficient) and, where D > 4, its last three columns zero (padding: K^T K is exactly singular and
the model variance there is e^{eps} alone).  epsilon_p = -2 + 0.3 N(0, 1); the shapes of TDV carry a tunable epsilon leaf.
eps in EPS = (-0.8, -8, -20), and EPS_ILL = -30 for the one ill-conditioned case the GPU test only reports on.  Under -tdv the leaf
is 1 + 0.05 N(0, 1) and eps_cli the listed value, so eps = float32(leaf * eps_cli) as the device forms it.
ROWS.  x = z K + b_d + e^{eps / 2} noise rounded to float32, z ~ N(0, I_L): rows near the model's manifold, so quad stays O(D).  Row
i does not depend on the row count; ROWS = (1, 5, 257, 1000) are prefixes of one set of MAX_ROWS.

BOUNDS (off_F, |G|_F, quad, logdet: the evaluation's own, G = K^T K, u = 2^-53):
  log p(x):  |d| <= (quad + D) (off_F + 64 D u |G|_F) e^{-eps} + 64 D u (quad + |logdet| + D)
             the first term: an eigenvalue of G is known to off_F + 64 D u |G|_F (DESIGN 3.16's bound), so s_i = lambda_i + e^{eps}
             to that relative to e^{eps} at worst, which moves quad by quad times it and logdet by D times it; the second: the
             rounding of the D-term sums themselves.
  ELBO(x):   |d| <= 2^-40 M, M the sum of the magnitudes of the ELBO's terms: about 100 float64 terms, a margin of about 100 over n u.
  gap(x) >= -(the two bounds).
  logdet:    |d| <= D * conditioning + 64 D u |logdet|, conditioning = (off_F + 64 D u |G|_F) e^{-eps} (record slot 8).
  eigenvalues against LAPACK: off_F + 64 D u |G|_F."""
import numpy as np

U = 2.0 ** -53
SHAPES = ((3, 2), (7, 7), (12, 20), (20, 4), (32, 32))
TDV = ((12, 20), (32, 32))
EPS = (-0.8, -8.0, -20.0)
EPS_ILL = -30.0
ROWS = (1, 5, 257, 1000)
MAX_ROWS = 1000
KE, BE, KD, BD, LV, EP = ("Encoder/FC0/kernel", "Encoder/FC0/bias", "Decoder/FC0/kernel", "Decoder/FC0/bias", "epsilon_p", "epsilon")


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def kept(L):
    return min(3, L - 1)


def make_model(D, L, eps_cli, seed=0):
    """(tree of float64 arrays holding float32 values, tdv, eps_cli, eps as the device forms it)."""
    rng = np.random.default_rng(1000 * D + 10 * L + seed)
    k = rng.standard_normal((L, D)) * 0.8
    k[kept(L):] *= 1e-3
    if D > 4:
        k[:, D - 3:] = 0.0
    p = {KE: _f32(0.3 * rng.standard_normal((D, L)) / np.sqrt(D)), BE: _f32(0.1 * rng.standard_normal(L)), KD: _f32(k),
         BD: _f32(0.2 * rng.standard_normal(D)), LV: _f32(-2.0 + 0.3 * rng.standard_normal(L))}
    tdv = (D, L) in TDV
    if tdv:
        p[EP] = _f32(1.0 + 0.05 * rng.standard_normal(1))
        eps = float(np.float32(p[EP][0]) * np.float32(eps_cli))
    else:
        eps = float(np.float32(eps_cli))
    return p, tdv, float(eps_cli), eps


def make_rows(p, eps, rows=MAX_ROWS, seed=0):
    """[rows, D] float64 holding float32 values: z K + b_d + e^{eps / 2} noise."""
    L, D = p[KD].shape
    rng = np.random.default_rng(77 + seed)
    z = rng.standard_normal((rows, L))
    return _f32(z @ p[KD] + p[BD] + np.exp(eps / 2) * rng.standard_normal((rows, D)))


def exact_posterior_model(D=8, L=3, eps_cli=-0.8, seed=0):
    """A model whose encoder IS the posterior, up to the float32 rounding of its leaves: the decoder kernel has orthogonal rows of
    norms sigma_l, so p(z | x) = N((x - b_d) E, diag(1 / (1 + sigma_l^2 e^{-eps}))) with E = K^T diag(e^{-eps} / (1 + sigma_l^2
    e^{-eps})): b_e = -b_d E, epsilon_p = -log(1 + sigma_l^2 e^{-eps}).  Its gap is 0 up to that rounding."""
    rng = np.random.default_rng(5 + seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, L)))
    sigma = np.linspace(0.5, 1.5, L)
    k = _f32(sigma[:, None] * q.T)
    eps = float(np.float32(eps_cli))
    s2 = np.sum(k * k, axis=1)
    w = np.exp(-eps) / (1.0 + s2 * np.exp(-eps))
    bd = _f32(0.2 * rng.standard_normal(D))
    e = k.T * w[None, :]
    p = {KE: _f32(e), BE: _f32(-bd @ e), KD: k, BD: bd, LV: _f32(-np.log1p(s2 * np.exp(-eps)))}
    return p, False, float(eps_cli), eps


def all_cases(ill=False):
    """(name, D, L, eps_cli) of every case; ill: the eps = -30 case alone."""
    if ill:
        return [("D12_L20_eps-30", 12, 20, EPS_ILL)]
    return [(f"D{D}_L{L}_eps{e:g}", D, L, e) for (D, L) in SHAPES for e in EPS]


def eig_bound(D, off, norm):
    return off + 64.0 * D * U * norm


def conditioning(D, off, norm, eps):
    return eig_bound(D, off, norm) * np.exp(-eps)


def logp_bound(D, quad, logdet, off, norm, eps):
    return (quad + D) * conditioning(D, off, norm, eps) + 64.0 * D * U * (quad + abs(logdet) + D)


def elbo_bound(M):
    return 2.0 ** -40 * M


def logdet_bound(D, logdet, off, norm, eps):
    return D * conditioning(D, off, norm, eps) + 64.0 * D * U * abs(logdet)
