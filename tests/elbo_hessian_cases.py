"""The cases and the bounds of the ELBO-Hessian tests, NumPy only: tests/test_gpu_elbo_hessian.py runs vaek_elbo_hvp_replicas and
vaek_elbo_hessian_lanczos_replicas on them, tests/test_elbo_hessian_host.py the float64 restatement (tools/elbo_hessian_reference.py)
against torch autograd.

MODELS.  theta is the flat parameter vector in the library's leaf order (E [D][L], b_e [L], K [L][D], b_d [D], epsilon_p [L] and, under
tunable_eps, epsilon [1]): N(0, 0.3^2) rounded to float32, epsilon = 1 (so eps = eps_cli exactly, in float32 and in float64).
ROWS.  x = z A rounded to float32, z ~ N(0, I_dd), A [dd][dd] ~ N(0, 1): a rank-dd linear map, then `pad` zero columns, D = dd + pad.
Row i does not depend on the row count: every row count is a prefix of one set.

  D / L    tunable_eps  eps_cli  rows       steps      what it covers
  2 / 1    no           -1       5          32         P = 8 < steps, no epsilon leaf
  3 / 2    yes          -3       7 and 1    5 and 32   rows not a tile multiple; odd steps (odd Jacobi size); breakdown below P = 20
  13 / 5   yes          -3       300        32         odd D
  12 / 20  yes          -1       1000       32         P = 533, the script shape
  32 / 32  yes          -3       300        32         P = 2145, every image at its largest

BOUNDS (u = 2^-53).
  an element of H v, of the gradient, and f:  |device - restatement| <= 64 (rows + 2 D + L) u M, M that value's MAGNITUDE IMAGE (the
      restatement with every operand replaced by its absolute value and every subtraction by an addition).  A running-error bound: the
      longest chain behind a value adds rows terms (the moments), then D + 1 and L and D + 1 terms (S dR, dU K, U^T dG), and both sides
      round, so n u M with n = rows + 2 D + L covers one side and the factor 64 the other side, fma against separate rounding, the two
      exponentials and the division by rows.
  a Ritz value theta_i, i < k:  min_j |lambda_j - theta_i| <= rho_i + (64 P u + k omega) |H|_2: rho_i is the exact-arithmetic residual
      bound; a computed H v is off by at most about P u |H| |v|, and a basis that is orthonormal only to omega turns the Rayleigh-Ritz
      argument's V^T V = I into I + O(k omega).
  omega <= 2^-40: twice-applied Gram-Schmidt leaves O(u) times a modest factor; 2^-40 is 8000 u."""
import collections

import numpy as np

U = 2.0 ** -53
OMEGA_MAX = 2.0 ** -40

Case = collections.namedtuple("Case", "name D L tdv eps_cli rows steps dd pad seed")
CASES = (
    Case("D2_L1", 2, 1, False, -1.0, (5,), (32,), 2, 0, 1),
    Case("D3_L2", 3, 2, True, -3.0, (7, 1), (5, 32), 2, 1, 2),
    Case("D13_L5", 13, 5, True, -3.0, (300,), (32,), 10, 3, 3),
    Case("D12_L20", 12, 20, True, -1.0, (1000,), (32,), 3, 9, 4),
    Case("D32_L32", 32, 32, True, -3.0, (300,), (32,), 16, 16, 5),
)
BY_NAME = {c.name: c for c in CASES}
MAX_ROWS = 1000


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def param_count(c):
    return 2 * c.D * c.L + 2 * c.L + c.D + (1 if c.tdv else 0)


def make_theta(c, replica=0):
    """[P] float64 holding float32 values."""
    rng = np.random.default_rng(100 * c.seed + replica)
    th = _f32(0.3 * rng.standard_normal(param_count(c)))
    if c.tdv:
        th[-1] = 1.0
    return th


def make_map(c, replica=0):
    """A [dd][dd] float64 holding float32 values: the dataset's linear map (vaek_make_batch's A for kind 0, did = dd)."""
    return _f32(np.random.default_rng(7000 + 100 * c.seed + replica).standard_normal((c.dd, c.dd)))


def make_rows(c, rows, replica=0):
    """[rows, D] float64 holding float32 values: the first `rows` of the case's set."""
    rng = np.random.default_rng(9000 + 100 * c.seed + replica)
    z = rng.standard_normal((MAX_ROWS, c.dd))
    x = np.zeros((MAX_ROWS, c.D))
    x[:, :c.dd] = _f32(z @ make_map(c, replica))
    return x[:rows]


def first_elements(c):
    """The flat index of the first element of every leaf."""
    D, L = c.D, c.L
    off_wd = (D + 1) * L
    off_bd = off_wd + L * D
    return [0, D * L, off_wd, off_bd, off_bd + D] + ([off_bd + D + L] if c.tdv else [])


def directions(c):
    """[3 + leaves, P]: three random directions, then the unit vector of each leaf's first element."""
    P = param_count(c)
    rng = np.random.default_rng(500 + c.seed)
    first = first_elements(c)
    V = np.zeros((3 + len(first), P))
    V[:3] = rng.standard_normal((3, P))
    for i, e in enumerate(first):
        V[3 + i, e] = 1.0
    return V


def start_vector(c, replica=0):
    return np.random.default_rng(300 + 10 * c.seed + replica).standard_normal(param_count(c))


def value_bound(c, rows, mag):
    """The bound on |device - restatement| of a value whose magnitude image is `mag`."""
    return 64.0 * (rows + 2 * c.D + c.L) * U * mag


def ritz_slack(P, k, omega, norm_h):
    return (64.0 * P * U + k * omega) * norm_h
