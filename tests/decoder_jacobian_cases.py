"""Shared cases and float64 reference of the decoder Jacobian spectra (csrc/mlp3_jacobian.hip): what tests/test_gpu_decoder_jacobian.py
runs on the GPU, what tests/test_decoder_jacobian_inputs.py first proves usable on the CPU, and what tools/decoder_jacobian_reference.py
measures.  NumPy only.

PARAMETERS: the recipe of tests/test_gpu_mlp3_log_likelihood.py -- lecun-normal kernels (oracle.init_params) perturbed by 0.02 N(0, 1),
biases 0.1 N(0, 1), epsilon_p = -2 + 0.3 N(0, 1), epsilon = 1 + 0.05 N(0, 1) under -tdv, eps_cli = -1 --, R = 3 replicas a shape.
LATENTS: row i of replica r of a case is the float32 rounding of the normals oracle/philox.py gives for the z1 block rule of
include/vaek.h (blocks q < ceil(L / 4) of the latent stream of row i under (seed, step, tag); the first L normals).  The GPU test hands
them to the call as explicit rows, so the reference and the kernel see the same bits.  A case's seed comes from SEEDS (searched by
tools/decoder_jacobian_reference.py --search so that no hidden pre-activation of any row is within KINK_FACTOR float32 errors of 0)
and its rank threshold from RANK_TOLS, else RANK_TOL.
REFERENCE (float64): forward through oracle.fcn_forward's arithmetic (h @ kernel + bias, relu), masks pre > 0, J by the masked
products, G = J^T J, numpy.linalg.eigvalsh."""
import numpy as np

from oracle import elbo_oracle as O
from oracle import philox as PH

R = 3
Z_TAG = 8
RANK_TOL = 1e-4
KINK_FACTOR = 8          # smallest |pre| >= 8 x the float32 forward's distance: the order inside an MFMA k-step is not the emulation's
GRAM_FACTOR = 8
H200 = (200, 200, 200)
SHAPES = {
    "script1": dict(enc=H200, dec=H200, D=6, L=6),                                   # sphere_vae_padding_expts.sh line 1
    "narrow": dict(enc=(64, 64, 64), dec=(64, 64, 64), D=7, L=6),
    "mixed": dict(enc=(64, 256, 100), dec=(130, 72, 200), D=9, L=5),
    "odd": dict(enc=(66, 201, 130), dec=(66, 201, 130), D=12, L=20),
    "wide": dict(enc=(256, 256, 256), dec=(256, 256, 256), D=32, L=32),
    "one_latent": dict(enc=H200, dec=H200, D=6, L=1),
}
# rows: a single row, a full tile and a partial last tile of 64 // (L + 1) rows for every shape
ROWS = {name: (1, 2, 37) for name in SHAPES}
ROWS["one_latent"] = (1, 2, 70)               # 32 rows a tile: 70 crosses two tile boundaries
CASES = [(name, rows) for name in SHAPES for rows in ROWS[name]]
Z_STEPS = [3, 2 ** 32 - 1, 2]
# the seed of replica r of a case is SEEDS[case] + 1000003 r
DEFAULT_SEED = 31337
SEEDS = {
    ('mixed', 37): 31338,
    ('odd', 37): 31339,
    ('wide', 1): 31338,
    ('wide', 2): 31338,
    ('one_latent', 70): 31349,
}
# 111 rows of 32 eigenvalues leave no threshold of the usual size free: ('wide', 37) takes the middle of the widest gap of its ratios.
# That is below float32's 2^-24, and still well defined: G is formed in float64 from the float32 J, so a small eigenvalue moves by
# 2 sigma_k |dJ|, not by |dJ| sigma_1
RANK_TOLS = {
    ('script1', 2): 1e-05,
    ('script1', 37): 1e-05,
    ('narrow', 37): 1e-05,
    ('wide', 1): 1e-05,
    ('wide', 2): 4.1e-06,
    ('wide', 37): 4.3e-08,
}


def case_seed(case):
    return SEEDS.get(case, DEFAULT_SEED)


def case_tol(case):
    return RANK_TOLS.get(case, RANK_TOL)


def cfg_of(s, tdv=True, eps=-1.0):
    return O.Config(s["D"], s["L"], s["enc"], s["dec"], eps, tdv, None)


def make_flats(name):
    """The R float32 parameter vectors of shape `name`."""
    cfg = cfg_of(SHAPES[name])
    rng = np.random.default_rng(23)
    flats = []
    for r in range(R):
        p = {}
        for k, v in O.init_params(cfg, seed=r).items():
            if k.endswith("kernel"):
                p[k] = v + 0.02 * rng.standard_normal(v.shape)
            elif k.endswith("bias"):
                p[k] = 0.1 * rng.standard_normal(v.shape)
            elif k == "epsilon_p":
                p[k] = -2.0 + 0.3 * rng.standard_normal(v.shape)
            else:
                p[k] = 1.0 + 0.05 * rng.standard_normal(v.shape)
        flats.append(O.flatten(cfg, p, np.float32))
    return flats


def trees_of(name):
    cfg = cfg_of(SHAPES[name])
    return [O.unflatten(cfg, f.astype(np.float64)) for f in make_flats(name)]


def z1_64(seed, step, tag, rows, L):
    """[rows, L] float64 normals: the z1 vaek_make_batch draws -- blocks q < ceil(L / 4) of the latent stream of row i (counter (row,
    block, step, tag + 2^30), key = the seed's two words), the first L of the 4 ceil(L / 4) normals."""
    nlb = (L + 3) // 4
    ctr = np.zeros((rows, nlb, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(rows, dtype=np.uint32)[:, None]
    ctr[..., 1] = np.arange(nlb, dtype=np.uint32)[None, :]
    ctr[..., 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32(tag + 2 ** 30)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return PH.normals_from_bits(PH.philox4x32(ctr, key)).reshape(rows, nlb * 4)[:, :L]


def case_seeds(case):
    return [case_seed(case) + 1000003 * r for r in range(R)]


def case_latents(case):
    """[R, rows, L] float32: the explicit latents of the case."""
    name, rows = case
    L = SHAPES[name]["L"]
    return np.stack([z1_64(sd, st, Z_TAG, rows, L) for sd, st in zip(case_seeds(case), Z_STEPS)]).astype(np.float32)


def decoder_layers(p):
    return [(p[f"Decoder/FC{i}/kernel"], p[f"Decoder/FC{i}/bias"]) for i in range(4)]


def jacobian64(p, z):
    """Float64 reference on latents z [rows, L]: (J [rows, D, L], pres: the three hidden pre-activations [rows, H_i])."""
    z = np.asarray(z, np.float64)
    layers = decoder_layers(p)
    h = z
    T = np.broadcast_to(np.eye(z.shape[1]), (z.shape[0], z.shape[1], z.shape[1])).copy()      # [rows, l, unit]: d h / d z_l
    pres = []
    for i, (W, b) in enumerate(layers):
        pre = h @ W + b
        T = T @ W
        if i < 3:
            pres.append(pre)
            live = pre > 0.0
            h = np.maximum(pre, 0.0)
            T = T * live[:, None, :]
        else:
            h = pre
    return np.swapaxes(T, 1, 2), pres


def row_records64(J, tol):
    """Per row of J [rows, D, L]: (lambda descending [rows, L], diag G [rows, L], rank [rows], |G|_F [rows], G)."""
    G = np.swapaxes(J, 1, 2) @ J
    lam = np.linalg.eigvalsh(G)[:, ::-1]
    top = lam[:, :1]
    rank = np.where(top[:, 0] > 0.0, (lam > tol * top).sum(1), 0)
    return lam, np.diagonal(G, axis1=1, axis2=2).copy(), rank, np.sqrt(np.square(G).sum((1, 2))), G


def dense32_seq(x, W, b):
    """Float32 x @ W (+ b) with one accumulator per output walked over k in k order: the emulation of a Dense layer's sum."""
    x = np.asarray(x, np.float32)
    W = np.asarray(W, np.float32)
    acc = np.zeros((x.shape[0], W.shape[1]), np.float32)
    for k in range(W.shape[0]):
        acc = acc + x[:, k:k + 1] * W[k][None, :]
    return acc if b is None else acc + np.asarray(b, np.float32)[None, :]


def jacobian32(p, z):
    """The float32 emulation: (J32 [rows, D, L] float32, pres32), masks from the float32 pre-activations."""
    z = np.asarray(z, np.float32)
    rows, L = z.shape
    h = z
    T = np.broadcast_to(np.eye(L, dtype=np.float32), (rows, L, L)).reshape(rows * L, L).copy()
    pres = []
    for i, (W, b) in enumerate(decoder_layers(p)):
        pre = dense32_seq(h, W, b)
        T = dense32_seq(T, W, None)
        if i < 3:
            pres.append(pre)
            live = pre > 0.0
            h = np.where(live, pre, np.float32(0.0))
            T = (T.reshape(rows, L, -1) * live[:, None, :]).reshape(rows * L, -1)
        else:
            h = pre
    return np.swapaxes(T.reshape(rows, L, -1), 1, 2), pres


def ratios64(case, seed=None):
    """Every lambda_k / lambda_1, k >= 2, of the case's float64 reference, sorted (rows whose lambda_1 is 0 left out)."""
    name, rows = case
    L = SHAPES[name]["L"]
    seeds = case_seeds(case) if seed is None else [seed + 1000003 * r for r in range(R)]
    out = []
    for r, p in enumerate(trees_of(name)):
        lam = row_records64(jacobian64(p, z1_64(seeds[r], Z_STEPS[r], Z_TAG, rows, L).astype(np.float32))[0], RANK_TOL)[0]
        lam = lam[lam[:, 0] > 0]
        out.append((lam[:, 1:] / lam[:, :1]).ravel())
    return np.sort(np.concatenate(out))


def measure(case, seed=None, tol=None):
    """The figures of one case from the float64 reference and the float32 emulation: dict(dist: worst |pre32 - pre64| over the hidden
    pre-activations, min_pre: smallest |pre64|, gram: worst |G32 - G64|_F / |G64|_F over rows and replicas, ratio_hit: whether some
    lambda_k / lambda_1 lies in [tol / 2, 2 tol])."""
    name, rows = case
    L = SHAPES[name]["L"]
    tol = case_tol(case) if tol is None else tol
    seeds = case_seeds(case) if seed is None else [seed + 1000003 * r for r in range(R)]
    dist = gram = 0.0
    min_pre = np.inf
    hit = False
    for r, p in enumerate(trees_of(name)):
        z = z1_64(seeds[r], Z_STEPS[r], Z_TAG, rows, L).astype(np.float32)
        J64, pres64 = jacobian64(p, z)
        J32, pres32 = jacobian32(p, z)
        for a, b in zip(pres32, pres64):
            dist = max(dist, float(np.abs(a.astype(np.float64) - b).max()))
            min_pre = min(min_pre, float(np.abs(b).min()))
        lam, _, _, ng, G64 = row_records64(J64, tol)
        J32 = J32.astype(np.float64)
        G32 = np.swapaxes(J32, 1, 2) @ J32
        err = np.sqrt(np.square(G32 - G64).sum((1, 2)))
        gram = max(gram, float((err[ng > 0] / ng[ng > 0]).max()) if (ng > 0).any() else 0.0)
        ratio = lam / np.where(lam[:, :1] > 0, lam[:, :1], 1.0)
        hit = hit or bool(((ratio >= tol / 2) & (ratio <= 2 * tol)).any())
    return dict(dist=dist, min_pre=min_pre, gram=gram, ratio_hit=hit)
