"""The cases and the bounds of the batch-generator conformance tests, NumPy only: tests/test_gpu_rng_conformance.py runs
vaek_make_batch and vaek_rng_fill on them, tests/test_rng_host.py a float32 emulation of csrc/rng_dev.h -- the proof that the
reference alone stays inside the bounds.

REFERENCES (oracle/philox.py).  normals_from_bits is the IDEAL Box-Muller: float64 on the exact 24-bit integer.  The kernel forms
u1 = ((float)(w >> 8) + 0.5f) 2^-24 in float32: from w >> 8 = 2^23 on the sum is a tie and rounds to even (down for even values, up
for odd ones: half of all pairs carry a u1 that is off by 2^-25), and w >> 8 = 2^24 - 1 gave u1 = 1, r = 0 until normals4 clamped
u1 to 0x1.fffffep-1f.  So kernel and ideal reference differ BY DESIGN in the tail, by up
to 2^-13 / sqrt(2 m) at 1 - u1 = m 2^-24 (1.2e-4 at m = 1/2), and a tolerance between them says nothing about the kernel.  The
KERNEL-UNIFORM reference, normals_kernel_uniform, is Box-Muller in float64 on the kernel's own float32 uniforms; what is left
between it and the device is v_log, v_sqrt, v_sin, v_cos and three float32 products.

CASES.  rows = 257 (two 256-thread blocks, the second ragged); A is float32 N(0, 1) from the case's own generator.
linear_gaussian (dd, did, pad, var), L cycling through (20, 5, 6, 7, 1, 32) so that L % 4 takes all four values; sigmoid (dd, pad);
sphere (dd, pad): the tables below.  They hold a mixing matrix that is not square (the A[d * did + k] stride), did > 4 with noise
(the noise block offset (did + 3) / 4 is 2, 3 and 4), dd > 4 (dataset blocks 1 .. 3), dd = 1 and 16, a sigmoid column that opens
a new 4-column piece (dd = 4, D = 5), D = 32, and the L % 4 = 3 latent split.  Counter edges, on at least one case of every kind:
row0 = 2^32 - 100 (the row index wraps inside the batch), step = 2^32 - 1, tag = 0x3FFFFFFF (the largest; the latents' tag + 2^30
is then 0x7FFFFFFF), seed = 0xFEDCBA9876543210.

BOUNDS, per element, none left out.  eps_n bounds one device normal against the kernel-uniform reference; n, nu are the reference
normals (batch_reference's deps), sigma = sqrt(var).
  z1, z2:           eps_n.
  linear_gaussian:  eps_n (sum_k |A_dk| + sigma) + c 2^-24 (sum_k |A_dk n_k| + sigma |nu|), c = did + 2: did + 1 fused
                    multiply-adds, each rounding a partial sum of at most the bracket to 2^-25 relative, and sigma = sqrtf(var)
                    itself (var and the root round: 1.5 * 2^-25) -- about twice what they can add up to.  Rows of A beyond dd are
                    zero, so a padding column is sigma nu within the same formula, and exactly 0.0 at var = 0.
  sigmoid:          data columns eps_n (they are the normals); the sigmoid column 1/4 (eps_n sum |a_d| + c 2^-24 sum |a_d n_d|)
                    + 4 * 2^-24, c = dd + 2 (sigmoid' <= 1/4; expf, the sum and the quotient are the last term); padding exactly 0.
  sphere:           data columns 2 sqrt(dd) eps_n / |g| + 2^-22 (g + e over |g + e| moves by at most 2 |e| / |g|, |e| <=
                    sqrt(dd) eps_n; the sum of squares, root, quotient and product are the 2^-22); padding exactly 0; the row's
                    norm is 1 within sqrt(dd) 2^-22.

EPS_N is MEASURED: profiles/rng_conformance.txt holds the largest |device - kernel-uniform reference| over the 3 * 2^22 normals
of tests/test_gpu_rng_conformance.py's vaek_rng_fill calls, and EPS_N is twice it -- the hardware's log and sin / cos error
depends on the argument and 2^23 pairs do not see the worst one.  EPS_FLOOR = 6.1e-7 is what the reference itself needs: the
largest error of a float32 Box-Muller with correctly rounded transcendentals (emulate_normals) against the kernel-uniform reference
over 2^23 normals.  tests/test_rng_host.py holds the emulation of every case to the bounds at eps_n = EPS_FLOOR."""
import numpy as np

from oracle import philox as P

ROWS = 257
EPS_FLOOR = 6.1e-7
EPS_N = 2 * 7.392e-7                            # twice the measured maximum: profiles/rng_conformance.txt
KIND = {"linear_gaussian": 0, "sigmoid": 1, "sphere": 2}
L_CYCLE = (20, 5, 6, 7, 1, 32)
LINEAR = ((1, 1, 0, 0.0), (3, 3, 9, 0.04), (3, 2, 28, 0.25), (2, 5, 3, 0.25), (5, 9, 0, 1e-4), (4, 4, 4, 0.5), (16, 1, 7, 0.0),
          (16, 16, 0, 0.01), (8, 16, 24, 0.25))
SIGMOID = ((1, 0), (3, 3), (4, 0), (7, 20), (16, 0), (15, 16))
SPHERE = ((1, 0), (2, 3), (3, 3), (4, 0), (5, 16), (16, 16))
PLAIN = dict(row0=1000, step=12, tag=5, seed=99)
ROW0_EDGE, STEP_EDGE, TAG_EDGE, SEED_EDGE = 2 ** 32 - 100, 2 ** 32 - 1, 0x3FFFFFFF, 0xFEDCBA9876543210
ALL_EDGES = dict(row0=ROW0_EDGE, step=STEP_EDGE, tag=TAG_EDGE, seed=SEED_EDGE)
# the counters of case i of a kind: every edge at once on the second, one edge each on the next four, none elsewhere
_EDGES = (PLAIN, ALL_EDGES, dict(PLAIN, row0=ROW0_EDGE), dict(PLAIN, step=STEP_EDGE), dict(PLAIN, tag=TAG_EDGE), dict(PLAIN, seed=SEED_EDGE))
# the three (seed, step, tag) of the raw-normal test (vaek_rng_fill's counter is (block lo, block hi, step, tag): any 32-bit tag)
FILL_TRIPLES = ((0x123456789ABCDEF, 17, 3), (SEED_EDGE, STEP_EDGE, TAG_EDGE), (77, 0, 0xFFFFFFFF))
FILL_BIG, FILL_SMALL = 1 << 22, (1, 2, 3, 5, 4099)
# key (77, 0), step 0, tag 0, block 0: rows whose first (word 0) or second (word 2) pair has w >> 8 = 2^24 - 1
TAIL_SEED = 77
TAIL_ROWS = ((3895978, 0, (0xffffff91, 0xf8312a72, 0xae3a358b, 0x00ea8479)), (6405805, 0, (0xffffff74, None, None, None)),
             (22116046, 2, (None, None, 0xffffff6b, None)))


def _case(kind, i, dd, did, pad, var, L):
    D = dd + pad + (1 if kind == "sigmoid" else 0)
    c = dict(kind=KIND[kind], kind_name=kind, dd=dd, did=did, pad=pad, var=var, L=L, D=D, rows=ROWS, **_EDGES[i % len(_EDGES)])
    c["name"] = f"{kind}_dd{dd}_did{did}_pad{pad}_var{var:g}_L{L}" + ("_edges" if c["row0"] == ROW0_EDGE and c["step"] == STEP_EDGE else "")
    return c


def all_cases():
    out = [_case("linear_gaussian", i, dd, did, pad, var, L_CYCLE[i % len(L_CYCLE)]) for i, (dd, did, pad, var) in enumerate(LINEAR)]
    out += [_case("sigmoid", i, dd, 1, pad, 0.0, L_CYCLE[(i + 2) % len(L_CYCLE)]) for i, (dd, pad) in enumerate(SIGMOID)]
    out += [_case("sphere", i, dd, 1, pad, 0.0, L_CYCLE[(i + 3) % len(L_CYCLE)]) for i, (dd, pad) in enumerate(SPHERE)]
    return out


CASES = all_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))


def make_A(c):
    """The case's dataset parameter, float32: [dd, did] (linear_gaussian), [dd] (sigmoid), None (sphere)."""
    rng = np.random.default_rng(100 * c["dd"] + c["did"] + 10000 * c["kind"])
    if c["kind"] == 0:
        return rng.standard_normal((c["dd"], c["did"])).astype(np.float32)
    return rng.standard_normal(c["dd"]).astype(np.float32) if c["kind"] == 1 else None


def reference(c, normals=P.normals_kernel_uniform):
    """batch_reference of the case: (x, z1, z2, deps)."""
    return P.batch_reference(c["kind"], make_A(c), c["dd"], c["did"], c["pad"], c["var"], c["rows"], c["row0"], c["seed"], c["step"],
                             c["tag"], c["L"], c["D"], normals=normals)


# ---- rng_dev.h in NumPy float32: the same operations in the same order, transcendentals correctly rounded ----------------------------
_F = np.float32


def _fma(a, b, c):          # float32 fused multiply-add: the product is exact in float64
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(_F)


def emulate_normals(bits):
    """normals4: r = sqrt(-2 ln 2 * log2(u1)), (r cos, r sin) of u2 revolutions."""
    u1, u2 = P.kernel_uniforms(bits)
    r = np.sqrt(_F(-1.3862943611198906) * np.log2(u1.astype(np.float64)).astype(_F))
    t = 2 * np.pi * u2.astype(np.float64)
    out = np.empty(np.asarray(bits).shape, dtype=_F)
    out[..., 0::2] = r * np.cos(t).astype(_F)
    out[..., 1::2] = r * np.sin(t).astype(_F)
    return out


def emulate_batch(c):
    """make_batch_items of the case in float32: (x, z1, z2)."""
    k, dd, did, D, L, rows = c["kind"], c["dd"], c["did"], c["D"], c["L"], c["rows"]
    A = make_A(c)

    def draw(tag, q0, count):
        nblk = (count + 3) // 4
        return emulate_normals(P.stream_bits(c["seed"], c["step"], tag, c["row0"], rows, q0, nblk)).reshape(rows, 4 * nblk)[:, :count]
    nrm = draw(c["tag"], 0, did if k == 0 else dd)
    x = np.zeros((rows, D), dtype=_F)
    if k == 0:
        for d in range(dd):
            v = np.zeros(rows, dtype=_F)
            for j in range(did):
                v = _fma(A[d, j], nrm[:, j], v)
            x[:, d] = v
        if c["var"] > 0:
            x = _fma(np.sqrt(_F(c["var"])), draw(c["tag"], P.noise_block_offset(did), D), x)
    elif k == 1:
        dot = np.zeros(rows, dtype=_F)
        for d in range(dd):
            dot = _fma(nrm[:, d], A[d], dot)
        x[:, :dd] = nrm
        x[:, dd] = _F(1) / (_F(1) + np.exp(-dot.astype(np.float64)).astype(_F))
    else:
        nsq = np.zeros(rows, dtype=_F)
        for d in range(dd):
            nsq = _fma(nrm[:, d], nrm[:, d], nsq)
        x[:, :dd] = nrm * (_F(1) / np.sqrt(nsq))[:, None]
    z = draw((c["tag"] + 0x40000000) & 0xFFFFFFFF, 0, L + D)
    return x, z[:, :L].copy(), z[:, L:].copy()


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def x_bound(c, deps, eps_n):
    """[rows, D]: the bound on every element of x; 0 where the element is exactly 0.0."""
    k, dd, did, D = c["kind"], c["dd"], c["did"], c["D"]
    n, nu = deps["n"], deps["nu"]
    A = make_A(c)
    b = np.zeros((n.shape[0], D))
    if k == 0:
        A = np.abs(A.astype(np.float64))
        sigma = float(np.sqrt(c["var"])) if c["var"] > 0 else 0.0
        b[:, :dd] = eps_n * A.sum(axis=1)[None, :] + (did + 2) * 2.0 ** -24 * (np.abs(n) @ A.T)
        if sigma > 0:
            b += eps_n * sigma + (did + 2) * 2.0 ** -24 * sigma * np.abs(nu)
    elif k == 1:
        a = np.abs(A.astype(np.float64))
        b[:, :dd] = eps_n
        b[:, dd] = 0.25 * (eps_n * a.sum() + (dd + 2) * 2.0 ** -24 * (np.abs(n) @ a)) + 4 * 2.0 ** -24
    else:
        b[:, :dd] = (2 * np.sqrt(dd) * eps_n / np.linalg.norm(n, axis=1) + 2.0 ** -22)[:, None]
    return b


def _ratio(err, bound):
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    r = np.where(err == 0, 0.0, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.inf))
    return float(np.max(np.where(np.isfinite(err), r, np.inf)))


def worst_ratios(c, ref, got, eps_n):
    """error / bound, the largest over EVERY element, of got = (x, z1, z2) against ref = reference(c): {"x", "z1", "z2"} and, for a
    sphere, "norm".  A non-finite element, or a nonzero one where the bound is 0, gives inf.  All are <= 1 when the case passes."""
    x, z1, z2, deps = ref
    gx, gz1, gz2 = (np.asarray(a, np.float64) for a in got)
    assert gx.shape == x.shape and gz1.shape == z1.shape and gz2.shape == z2.shape
    out = {"x": _ratio(np.abs(gx - x), x_bound(c, deps, eps_n)), "z1": _ratio(np.abs(gz1 - z1), eps_n), "z2": _ratio(np.abs(gz2 - z2), eps_n)}
    if c["kind"] == 2:
        out["norm"] = _ratio(np.abs(np.linalg.norm(gx[:, :c["dd"]], axis=1) - 1.0), np.sqrt(c["dd"]) * 2.0 ** -22)
    return out
