"""The cases and the bounds of the MLP sampled-ELBO-Hessian tests: tests/test_gpu_mlp3_hessian.py runs
vaek_mlp3_sampled_elbo_hvp_replicas and vaek_mlp3_sampled_elbo_hessian_lanczos_replicas on them, tests/test_mlp3_hessian_host.py holds
the float64 restatement (tools/mlp3_hessian_reference.py) to torch autograd and to the oracle, tests/test_mlp3_hessian_inputs.py proves
the inputs usable.

SHAPES.  The smallest that can still go wrong (tests/decoder_jacobian_cases.SHAPES): narrow 64.64.64 (D 7, L 6), mixed (enc 64.256.100,
dec 130.72.200; D 9, L 5), odd 66.201.130 (D 12, L 20), script1 200.200.200 (D = L = 6), wide 256.256.256 (D = L = 32, P = 296 545), and
narrow_notdv: narrow without tunable_eps (no epsilon leaf).  A CASE is (shape, rows, K) with (rows, K) from ROWS_K: (1, 1) one column,
(5, 3) 15 columns = a partial second tile of 8, (37, 2) 74 columns, (9, 1) two tiles, the second nearly empty.
PARAMETERS.  The recipe of tests/decoder_jacobian_cases.make_flats, R = 3 replicas a shape, float32 values, eps_cli = -1.
ROWS AND SAMPLES.  x [rows][D] = 0.5 N(0, 1) and xi [rows][K][L] = N(0, 1), rounded to float32, from the case's seed (SEEDS, else
DEFAULT_SEED) and the replica; row i and its samples do not depend on the row count.  tests/test_mlp3_hessian_inputs.py requires the
smallest |pre-activation| of the float64 reference over every hidden unit, column and replica of a case to be >= MIN_PRE = 1e-9: two
float64 evaluations in different summation orders differ by ~1e-13 there, so they agree on every relu mask.  A case that fails gets
another seed in SEEDS.

BOUNDS (u = 2^-53).
  an element of H v, of the gradient, and f_K:  |device - restatement| <= 64 n_chain u M with M that value's MAGNITUDE IMAGE (the
      restatement with every operand replaced by its absolute value and every subtraction by an addition, the masks kept) and
      n_chain = 2 rows K + sum_layers (n_in + n_out) + 2 D + 2 L: the running-error form of tests/sampled_hessian_cases.py with this
      function's chain -- the contraction over the replica's columns (twice: the tangent launch adds two products a column), then the
      inner products of every Dense layer forward and backward, then the head's.  The factor 64 is that file's.
      tests/test_mlp3_hessian_host.py holds the restatement to torch float64 autograd under this very bound and prints the worst ratio.
  Ritz values and omega: ritz_slack and OMEGA_MAX of tests/sampled_hessian_cases.py, as they stand."""
import functools
import importlib.util
import os

import numpy as np

from tests import decoder_jacobian_cases as DJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
OMEGA_MAX = 2.0 ** -40
MIN_PRE = 1e-9
R = 3
EPS_CLI = -1.0
X_TAG, Z_TAG, V_TAG = 14, 15, 16
BASES = ("narrow", "mixed", "odd", "script1", "wide")
SHAPES = {name: dict(DJ.SHAPES[name], tdv=True) for name in BASES}
SHAPES["narrow_notdv"] = dict(DJ.SHAPES["narrow"], tdv=False)
ROWS_K = ((1, 1), (5, 3), (37, 2), (9, 1))
CASES = tuple((name, rows, samples) for name in SHAPES for rows, samples in ROWS_K)
MAX_ROWS, MAX_K = 37, 3
DEFAULT_SEED = 4242
SEEDS = {}                                       # case -> seed, for a case whose default seed puts a pre-activation within MIN_PRE of 0
# the drawing-mode streams of the R replicas: distinct seeds and steps, one step 2^32 - 1
X_SEEDS, X_STEPS = [77, 2 ** 63 + 5, 1000003], [1, 2 ** 32 - 1, 2 ** 31 + 7]
Z_SEEDS, Z_STEPS = [91, 2 ** 63 + 17, 424243], [3, 2 ** 31 + 9, 2 ** 32 - 1]
# Lanczos: (case, steps)
LANCZOS_CASES = ((("narrow", 37, 2), 32), (("script1", 37, 1), 32), (("odd", 5, 3), 7), (("wide", 5, 1), 8))
# every (shape, rows, K) a test evaluates: tests/test_mlp3_hessian_inputs.py holds each to MIN_PRE
ALL_CASES = CASES + tuple(c for c, _ in LANCZOS_CASES if c not in CASES)
# The breakdown case.  One column of `narrow` from a RANDOM start does not break down within 32 steps (the CPU Lanczos run of
# tools/mlp3_hessian_reference.py reaches k = 32 with beta_32 = 4.6: one column still reaches every live unit of eight layers, a few
# hundred directions), so the case that does is the same column from breakdown_start: a vector supported on the incoming weights and
# biases of the Decoder/FC1 units that are DEAD in that column.  H v0 = 0 there exactly (the mask zeroes the unit's tangent and its
# gradient), so alpha_1 = beta_1 = 0 and the run ends at k = 1 < steps (tests/test_mlp3_hessian_inputs.py holds the CPU run to that).
BREAKDOWN_CASE = ("narrow", 1, 1)
# the workspace of csrc/mlp3_hessian.hip, in doubles
WS_HEAD, WS_TAIL, WS_STATE, WS_CHUNK, WS_STEPS, WS_PAIR_PITCH, WS_COLS = 8, 40, 192, 2048, 32, 512, 8


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def ref():
    spec = importlib.util.spec_from_file_location("mlp3_hessian_reference", os.path.join(ROOT, "tools", "mlp3_hessian_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def base_of(name):
    return "narrow" if name == "narrow_notdv" else name


def layer_sizes(name):
    s = SHAPES[name]
    e, d = [s["D"]] + list(s["enc"]) + [s["L"]], [s["L"]] + list(s["dec"]) + [s["D"]]
    return [(e[i], e[i + 1]) for i in range(4)] + [(d[i], d[i + 1]) for i in range(4)]


def param_count(name):
    s = SHAPES[name]
    return sum((a + 1) * b for a, b in layer_sizes(name)) + s["L"] + (1 if s["tdv"] else 0)


def model_args(name):
    s = SHAPES[name]
    return s["D"], s["L"], s["enc"], s["dec"], EPS_CLI, s["tdv"]


def oracle_cfg(name):
    s = SHAPES[name]
    return DJ.cfg_of(s, tdv=s["tdv"], eps=EPS_CLI)


@functools.lru_cache(maxsize=None)
def _flats(base):
    return DJ.make_flats(base)


def make_theta(name, replica=0):
    """[P] float64 holding float32 values; without tunable_eps the epsilon leaf (the last element) is cut."""
    flat = _flats(base_of(name))[replica].astype(np.float64)
    return flat if SHAPES[name]["tdv"] else flat[:-1].copy()


def case_seed(case):
    return SEEDS.get(case, DEFAULT_SEED)


def make_rows(case, replica=0):
    """[rows, D] float64 holding float32 values."""
    name, rows, _ = case
    rng = np.random.default_rng([case_seed(case), 1, replica])
    return _f32(0.5 * rng.standard_normal((MAX_ROWS, SHAPES[name]["D"])))[:rows]


def make_samples(case, replica=0):
    """[rows, K, L] float64 holding float32 values."""
    name, rows, samples = case
    rng = np.random.default_rng([case_seed(case), 2, replica])
    return _f32(rng.standard_normal((MAX_ROWS, MAX_K, SHAPES[name]["L"])))[:rows, :samples]


@functools.lru_cache(maxsize=None)
def model(case, replica=0, mag=False):
    """The restatement (or its magnitude image) of replica `replica` of a case; computed once and left unchanged."""
    name = case[0]
    return ref().Model(make_theta(name, replica), make_rows(case, replica), make_samples(case, replica), *model_args(name), mag=mag)


def leaf_offset(name, leaf):
    """Flat offset of a named leaf (oracle names)."""
    o = 0
    for n, shape in oracle_cfg(name).leaves():
        if n == leaf:
            return o
        o += int(np.prod(shape))
    raise KeyError(leaf)


@functools.lru_cache(maxsize=None)
def directions(name):
    """[3, P]: a dense random direction, one unit vector inside Decoder/FC1/kernel, one supported on epsilon_p and epsilon only."""
    P, s = param_count(name), SHAPES[name]
    rng = np.random.default_rng(500 + len(name))
    V = np.zeros((3, P))
    V[0] = rng.standard_normal(P)
    n_in, n_out = layer_sizes(name)[5]
    V[1, leaf_offset(name, "Decoder/FC1/kernel") + (n_in // 2) * n_out + n_out // 3] = 1.0
    tail = s["L"] + (1 if s["tdv"] else 0)
    V[2, P - tail:] = rng.standard_normal(tail)
    return V


def start_vector(name, replica=0):
    return np.random.default_rng([300, len(name), replica]).standard_normal(param_count(name))


def breakdown_start(case, replica=0):
    """[P]: N(0, 1) on the kernel columns and biases of the Decoder/FC1 units dead in every column of the case, 0 elsewhere."""
    name = case[0]
    dead = ~np.any(model(case, replica).masks[5], axis=0)
    assert dead.any()
    n_in, n_out = layer_sizes(name)[5]
    o = leaf_offset(name, "Decoder/FC1/kernel")
    block = np.zeros((n_in + 1, n_out))
    block[:, dead] = np.random.default_rng([301, replica]).standard_normal((n_in + 1, int(dead.sum())))
    v = np.zeros(param_count(name))
    v[o:o + (n_in + 1) * n_out] = block.ravel()
    return v


def n_chain(case):
    name, rows, samples = case
    s = SHAPES[name]
    return 2 * rows * samples + sum(a + b for a, b in layer_sizes(name)) + 2 * s["D"] + 2 * s["L"]


def value_bound(case, mag):
    """The bound on |device - restatement| of a value whose magnitude image is `mag`."""
    return 64.0 * n_chain(case) * U * mag


def worst_ratio(diff, bound):
    """max |diff| / bound over the elements; an element whose bound is 0 must agree exactly (inf otherwise)."""
    diff, bound = np.abs(np.asarray(diff, np.float64)).ravel(), np.asarray(bound, np.float64).ravel()
    ratio = np.where(bound > 0.0, diff / np.where(bound > 0.0, bound, 1.0), np.where(diff > 0.0, np.inf, 0.0))
    return float(np.max(ratio))


def ritz_slack(P, k, omega, norm_h):
    return (64.0 * P * U + k * omega) * norm_h


def workspace_doubles(name, rows, samples):
    """Doubles of ONE replica's workspace block: head, gradient, tail partials, Lanczos state, w, two dot tables, the norms, the Gram
    partials, then per layer h, g_a, dh, dg_a as [unit][column pitch]."""
    P = param_count(name)
    tiles = (rows * samples + WS_COLS - 1) // WS_COLS
    chunks = (P + WS_CHUNK - 1) // WS_CHUNK
    even = lambda v: (v + 1) & ~1
    head = WS_HEAD + even(P) + tiles * WS_TAIL + WS_STATE + even(P) + 2 * chunks * WS_STEPS + even(chunks) + chunks * WS_PAIR_PITCH
    return head + 2 * sum(a + b for a, b in layer_sizes(name)) * tiles * WS_COLS


def workspace_bytes(name, n, rows, samples):
    return 8 * n * workspace_doubles(name, rows, samples)
