"""Shared cases and float64 reference of the decoder Jacobian spectra of linear VAEs (csrc/linear_jacobian.hip): what
tests/test_gpu_linear_jacobian.py runs on the GPU, what tests/test_linear_jacobian_inputs.py first proves usable on the CPU, and what
tools/linear_jacobian_reference.py measures.  NumPy only.

PARAMETERS: the recipe of tests/decoder_jacobian_cases.make_flats -- lecun-normal kernels (oracle.init_params) perturbed by 0.02 N(0, 1),
biases 0.1 N(0, 1), epsilon_p = -2 + 0.3 N(0, 1), epsilon = 1 + 0.05 N(0, 1) under -tdv, eps_cli = -1 --, except that the second
decoder's kernel K_s and bias b_s are N(0, 1): u = z K_s + b_s then has a standard deviation of about sqrt(L + 1), so its D entries
per row reach both the linear part of the sigmoid (|u| < 1) and its flat part (|u| > 4).  R = 3 replicas a shape.
LATENTS: decoder_jacobian_cases.z1_64 -- the z1 block rule of include/vaek.h through oracle/philox.py, rounded to float32 -- so the
reference and the kernel see the same bits.  A case's seed comes from SEEDS, its rank threshold from RANK_TOLS, else RANK_TOL (both
searched by tools/linear_jacobian_reference.py --search: no reference ratio lambda_k / lambda_1 inside [tol / 2, 2 tol]).
REFERENCE (float64), read against networks.py:73-83: x_hat = z K_d + b_d [+ sigmoid(z K_s + b_s)], so
  u = z @ K_s + b_s,  s = 1 / (1 + exp(-u)),  J[d][l] = K_d[l][d] + s_d (1 - s_d) K_s[l][d],  G = J^T J,  numpy.linalg.eigvalsh
(the two products as explicit loops of elementwise operations, so the figures do not depend on the machine's BLAS)
-- the textbook s (1 - s), not the kernel's e / (1 + e)^2 form: the two agree to a few ulp where neither head is saturated, which is
what GRAM_FACTOR leaves room for.  gram_longdouble evaluates G a second time in numpy.longdouble: how well float64 defines it."""
import numpy as np

from oracle import elbo_oracle as O
from tests import decoder_jacobian_cases as DC

R = DC.R
Z_TAG = DC.Z_TAG
RANK_TOL = DC.RANK_TOL
GRAM_FACTOR = DC.GRAM_FACTOR
Z_STEPS = DC.Z_STEPS
SHAPES = {
    "sig_script1": dict(D=7, L=6, sig=True),                  # sigmoid_vae_padding_expts.sh line 1
    "sig_script6": dict(D=28, L=24, sig=True),                # line 6: the D cap of two decoders
    "sig_null": dict(D=5, L=32, sig=True),                    # L > D: 27 null directions, the largest L
    "sig_one_latent": dict(D=9, L=1, sig=True),               # the Jacobi order is padded to 2
    "sig_odd": dict(D=11, L=13, sig=True),
    "lin_odd": dict(D=12, L=20, sig=False),
    "lin_wide": dict(D=32, L=32, sig=False),
    "lin_narrow": dict(D=32, L=3, sig=False),
}
ROWS = {name: (1, 2, 37) for name in SHAPES}
ROWS["sig_script1"] = (1, 2, 37, 257)         # 257 rows: the finalize tree crosses its 256-row tile
CASES = [(name, rows) for name in SHAPES for rows in ROWS[name]]
DEFAULT_SEED = 31337
# SEARCH_BEGIN (written by tools/linear_jacobian_reference.py --search)
SEEDS = {
}
RANK_TOLS = {
    ('sig_odd', 37): 1e-05,
    ('lin_wide', 1): 1e-05,
    ('lin_wide', 2): 1e-05,
    ('lin_wide', 37): 1e-05,
}
# SEARCH_END


def case_seed(case):
    return SEEDS.get(case, DEFAULT_SEED)


def case_tol(case):
    return RANK_TOLS.get(case, RANK_TOL)


def case_seeds(case, seed=None):
    return [(case_seed(case) if seed is None else seed) + 1000003 * r for r in range(R)]


def cfg_of(s, tdv=True, eps=-1.0):
    return O.Config(s["D"], s["L"], (), (), eps, tdv, "sigmoid" if s["sig"] else "linear_gaussian")


def make_flats(name):
    """The R float32 parameter vectors of shape `name`."""
    cfg = cfg_of(SHAPES[name])
    rng = np.random.default_rng(29)
    flats = []
    for r in range(R):
        p = {}
        for k, v in O.init_params(cfg, seed=r).items():
            if k.startswith("SigDecoder"):
                p[k] = rng.standard_normal(v.shape)
            elif k.endswith("kernel"):
                p[k] = v + 0.02 * rng.standard_normal(v.shape)
            elif k.endswith("bias"):
                p[k] = 0.1 * rng.standard_normal(v.shape)
            elif k == "epsilon_p":
                p[k] = -2.0 + 0.3 * rng.standard_normal(v.shape)
            else:
                p[k] = 1.0 + 0.05 * rng.standard_normal(v.shape)
        flats.append(O.flatten(cfg, p, np.float32))
    return flats


def trees_of(name, flats=None):
    cfg = cfg_of(SHAPES[name])
    return [O.unflatten(cfg, np.asarray(f).astype(np.float64)) for f in (make_flats(name) if flats is None else flats)]


def case_latents(case, seed=None):
    """[R, rows, L] float32: the explicit latents of the case."""
    name, rows = case
    L = SHAPES[name]["L"]
    return np.stack([DC.z1_64(sd, st, Z_TAG, rows, L) for sd, st in zip(case_seeds(case, seed), Z_STEPS)]).astype(np.float32)


def jacobian(p, z, dtype=np.float64):
    """J [rows, D, L] on latents z [rows, L] in `dtype`, and u [rows, D] (None with one decoder)."""
    z = np.asarray(z, dtype)
    Kd = np.asarray(p["Decoder/FC0/kernel"], dtype)                        # [L, D]
    J = np.broadcast_to(Kd.T, (z.shape[0],) + Kd.T.shape).copy()
    if "SigDecoder/FC0/kernel" not in p:
        return J, None
    Ks = np.asarray(p["SigDecoder/FC0/kernel"], dtype)
    u = np.broadcast_to(np.asarray(p["SigDecoder/FC0/bias"], dtype), (z.shape[0], Ks.shape[1])).copy()
    for l in range(Ks.shape[0]):                                           # z @ K_s + b_s without BLAS: the same figures on every machine
        u = u + z[:, l, None] * Ks[l][None]
    one = dtype(1.0)
    s = one / (one + np.exp(-u))
    return J + (s * (one - s))[:, :, None] * Ks.T[None], u


def jacobian64(p, z):
    return jacobian(p, z, np.float64)


def gram(J):
    """G = J^T J [rows, L, L] of J [rows, D, L] in J's dtype, each entry a sum over d in d order of elementwise products: the same
    figures whatever BLAS the machine has."""
    G = np.zeros((J.shape[0], J.shape[2], J.shape[2]), J.dtype)
    for d in range(J.shape[1]):
        G = G + J[:, d, :, None] * J[:, d, None, :]
    return G


def row_records64(J, tol):
    """decoder_jacobian_cases.row_records64 on gram(J): (lambda descending [rows, L], diag G [rows, L], rank [rows], |G|_F [rows], G)."""
    G = gram(J)
    lam = np.linalg.eigvalsh(G)[:, ::-1]
    top = lam[:, :1]
    rank = np.where(top[:, 0] > 0.0, (lam > tol * top).sum(1), 0)
    return lam, np.diagonal(G, axis1=1, axis2=2).copy(), rank, np.sqrt(np.square(G).sum((1, 2))), G


def gram_longdouble(p, z):
    """Per row |G_64 - G_ld|_F / |G_64|_F: G = J^T J evaluated in float64 against the same formula in numpy.longdouble."""
    J64, _ = jacobian(p, z, np.float64)
    Jld, _ = jacobian(p, z, np.longdouble)
    G64, Gld = gram(J64), gram(Jld)
    err = np.sqrt(np.square((G64.astype(np.longdouble) - Gld)).sum((1, 2))).astype(np.float64)
    ng = np.sqrt(np.square(G64).sum((1, 2)))
    return np.where(ng > 0, err / np.where(ng > 0, ng, 1.0), 0.0)


def ratios64(case, seed=None):
    """Every lambda_k / lambda_1, k >= 2, of the case's float64 reference, sorted (rows whose lambda_1 is 0 left out)."""
    z = case_latents(case, seed)
    out = []
    for r, p in enumerate(trees_of(case[0])):
        lam = row_records64(jacobian64(p, z[r])[0], RANK_TOL)[0]
        lam = lam[lam[:, 0] > 0]
        out.append((lam[:, 1:] / lam[:, :1]).ravel())
    return np.sort(np.concatenate(out))


def measure(case, seed=None, tol=None):
    """The figures of one case: dict(gram: worst |G_64 - G_ld|_F / |G|_F over rows and replicas, ratio_hit: whether some
    lambda_k / lambda_1 lies in [tol / 2, 2 tol], u_min / u_max: the smallest and largest |u| (two decoders; else None))."""
    tol = case_tol(case) if tol is None else tol
    z = case_latents(case, seed)
    gram, hit, us = 0.0, False, []
    for r, p in enumerate(trees_of(case[0])):
        J, u = jacobian64(p, z[r])
        gram = max(gram, float(gram_longdouble(p, z[r]).max()))
        lam = row_records64(J, tol)[0]
        ratio = lam / np.where(lam[:, :1] > 0, lam[:, :1], 1.0)
        hit = hit or bool(((ratio >= tol / 2) & (ratio <= 2 * tol)).any())
        if u is not None:
            us.append(np.abs(u).ravel())
    us = np.concatenate(us) if us else None
    return dict(gram=gram, ratio_hit=hit, u_min=None if us is None else float(us.min()), u_max=None if us is None else float(us.max()))
