"""The cases and the bounds of the sampled-ELBO-Hessian tests, NumPy only: tests/test_gpu_sampled_hessian.py runs
vaek_sampled_elbo_hvp_replicas and vaek_sampled_elbo_hessian_lanczos_replicas on them, tests/test_sampled_hessian_host.py the float64
restatement (tools/sampled_hessian_reference.py) against torch autograd and, on the sigma-point cases, against the exact restatement.

MODELS.  theta is the flat parameter vector in the library's leaf order (E [D][L], b_e [L], K [L][D], b_d [D], with two decoders K_s
[L][D], b_s [D], then epsilon_p [L] and, under tunable_eps, epsilon [1]): N(0, 0.3^2) rounded to float32, epsilon = 1.
ROWS.  As tests/elbo_hessian_cases.make_rows: x = z A rounded to float32, z ~ N(0, I_dd), then -- two-decoder cases -- the sigmoid
dataset's column sigmoid(z . a), then `pad` zero columns.  Row i does not depend on the row count.
SAMPLES.  xi [rows][K][L], float32 values.  Sigma-point cases: K = 2 L, sample 2 l is +sqrt(L) e_l and sample 2 l + 1 its negative, for
every row (mean 0, second moment I: f_K = f of the exact call identically in theta; L in {1, 4, 16} keeps sqrt(L) exact in float32).
Else N(0, 1); sample k of row i does not depend on the row count.

  name      D / L    decoders  tdv  rows     K               steps     what it covers
  D2_L1     2 / 1    1         no   5        2 (+-1)         32        P = 8 < steps, sigma points
  D4_L2s    4 / 2    2         yes  7 and 1  3               5 and 32  odd K, odd Jacobi size, breakdown below P, one row
  D5_L4     5 / 4    1         yes  7        8 (+-2 e_l)     32        sigma points, columns below one tile
  D13_L5s   13 / 5   2         yes  300      5               32        odd D, 1500 columns: not a tile multiple
  D32_L16   32 / 16  1         yes  40       32 (+-4 e_l)    32        widest one-decoder image, sigma points
  D28_L32s  28 / 32  2         yes  64       8               32        P = 2809, every image at its largest
  D28_L24s  28 / 24  2         yes  1000     8               32        sigmoid_dd7_pd20_ld_24, the script shape; many tiles

BOUNDS (u = 2^-53).
  an element of H v, of the gradient, and f_K:  |device - restatement| <= 64 (rows K + 2 D + 2 L) u M, M that value's MAGNITUDE IMAGE
      (the restatement with every operand replaced by its absolute value and every subtraction by an addition; sigma, sigma', sigma''
      as the absolute values of their computed results).  The running-error form of tests/elbo_hessian_cases.py: the longest chain
      behind a value adds rows K terms (the columns of a replica), then the inner products of the passes (D, L, L and D terms), and
      both sides round, so n u M with n = rows K + 2 D + 2 L covers one side and the factor 64, carried over from that file, the other
      side, fma against separate rounding, the exponentials, the sigmoid's division and the division by rows K.
      tests/test_sampled_hessian_host.py holds the restatement against torch float64 autograd -- honest float64 in another operation
      order -- under this very bound: the worst |restatement - autograd| / bound over every case, direction and element measured
      there is 3.4e-3 (an element of H v at D32_L16), i.e. about 290x room where 8x is asked, so the factor stays 64.
  Ritz values and omega: ritz_slack and OMEGA_MAX of tests/elbo_hessian_cases.py, as they stand."""
import collections

import numpy as np

U = 2.0 ** -53
OMEGA_MAX = 2.0 ** -40

Case = collections.namedtuple("Case", "name D L sig tdv eps_cli rows K sigma steps dd pad seed")
CASES = (
    Case("D2_L1", 2, 1, False, False, -1.0, (5,), 2, True, (32,), 2, 0, 1),
    Case("D4_L2s", 4, 2, True, True, -3.0, (7, 1), 3, False, (5, 32), 2, 1, 2),
    Case("D5_L4", 5, 4, False, True, -3.0, (7,), 8, True, (32,), 3, 2, 3),
    Case("D13_L5s", 13, 5, True, True, -3.0, (300,), 5, False, (32,), 7, 5, 4),
    Case("D32_L16", 32, 16, False, True, -3.0, (40,), 32, True, (32,), 16, 16, 5),
    Case("D28_L32s", 28, 32, True, True, -3.0, (64,), 8, False, (32,), 7, 20, 6),
    Case("D28_L24s", 28, 24, True, True, -3.0, (1000,), 8, False, (32,), 7, 20, 7),
)
BY_NAME = {c.name: c for c in CASES}
SIGMA_CASES = tuple(c for c in CASES if c.sigma)
DENSE_CASES = CASES[:4]                                                 # P <= 600: the dense reference H is assembled from the restatement
MAX_ROWS = 1000


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def param_count(c):
    return c.D * c.L + c.L + (2 if c.sig else 1) * (c.L * c.D + c.D) + c.L + (1 if c.tdv else 0)


def make_theta(c, replica=0):
    """[P] float64 holding float32 values."""
    rng = np.random.default_rng(100 * c.seed + replica)
    th = _f32(0.3 * rng.standard_normal(param_count(c)))
    if c.tdv:
        th[-1] = 1.0
    return th


def make_rows(c, rows, replica=0):
    """[rows, D] float64 holding float32 values: the first `rows` of the case's set."""
    rng = np.random.default_rng(9000 + 100 * c.seed + replica)
    z = rng.standard_normal((MAX_ROWS, c.dd))
    A = _f32(np.random.default_rng(7000 + 100 * c.seed + replica).standard_normal((c.dd, c.dd)))
    x = np.zeros((MAX_ROWS, c.D))
    x[:, :c.dd] = _f32(z @ A)
    if c.sig:
        a = np.random.default_rng(8000 + 100 * c.seed + replica).standard_normal(c.dd)
        x[:, c.dd] = _f32(1.0 / (1.0 + np.exp(-(z @ a))))
    assert c.dd + (1 if c.sig else 0) + c.pad == c.D
    return x[:rows]


def make_samples(c, rows, replica=0):
    """[rows, K, L] float64 holding float32 values."""
    if c.sigma:
        assert c.K == 2 * c.L
        one = np.zeros((c.K, c.L))
        for l in range(c.L):
            one[2 * l, l], one[2 * l + 1, l] = np.sqrt(c.L), -np.sqrt(c.L)
        assert np.array_equal(one, _f32(one))
        return np.broadcast_to(one, (rows, c.K, c.L)).copy()
    rng = np.random.default_rng(6000 + 100 * c.seed + replica)
    return _f32(rng.standard_normal((MAX_ROWS, c.K, c.L)))[:rows]


def first_elements(c):
    """The flat index of the first element of every leaf."""
    D, L = c.D, c.L
    first = [0, D * L, D * L + L, D * L + L + L * D]
    off = first[-1] + D
    if c.sig:
        first += [off, off + L * D]
        off += L * D + D
    return first + [off] + ([off + L] if c.tdv else [])


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
    return 64.0 * (rows * c.K + 2 * c.D + 2 * c.L) * U * mag


def exact_value_bound(c, rows, mag):
    """tests/elbo_hessian_cases.value_bound for the exact call on the same rows."""
    return 64.0 * (rows + 2 * c.D + c.L) * U * mag


def worst_ratio(diff, bound):
    """max |diff| / bound over the elements; an element whose bound is 0 must agree exactly (inf otherwise)."""
    diff, bound = np.abs(np.asarray(diff, np.float64)).ravel(), np.asarray(bound, np.float64).ravel()
    ratio = np.where(bound > 0.0, diff / np.where(bound > 0.0, bound, 1.0), np.where(diff > 0.0, np.inf, 0.0))
    return float(np.max(ratio))


def ritz_slack(P, k, omega, norm_h):
    return (64.0 * P * U + k * omega) * norm_h
