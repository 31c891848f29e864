"""Float64 references for the linear-moment launch (csrc/linear_moments.hip, linear_moments_dev.h), role by role, and the ctypes image
of vaek_debug_lin's argument struct.  Needs no GPU: the functions take and return torch tensors on any device.

The moment image.  A batch's sufficient statistic is M = U^T U with U = [z1 (L) | x (D) | z2 (D) | 1], NF = L + 2 D + 1 features in
NB = 3 or 4 blocks of 16.  The streamers and reducers leave the UPPER BLOCK TRIANGLE, block (b1, b2), b1 <= b2, at index
lin_blk = b1 NB - b1 (b1 - 1) / 2 + (b2 - b1), each block in the MFMA accumulator layout: element (i, j) of a block at
((i >> 2) * 16 + j) * 4 + (i & 3)  (lin_img_coords / lin_m_index).  A diagonal block holds both of its halves.

Bounds.
  streamers + reducers   exact integers (exact_batch): bitwise.  wide_batch: |got - M[i, j]| <= (n_add + 1) 2^-24 Mabs[i, j],
                         n_add = T / CW + CW: a multiplying wave chains the T / CW rows it takes of a tile (CW = 8 waves in the
                         launch-per-step form, 4 in the persistent one) in float32, the CW images are then added in float32
                         (T / CW + CW - 1 roundings; the + 1 of the bound covers a product rounded by itself).  Everything behind
                         the tile is float64.
  updaters               |got - ref| <= k 2^-24 mag, mag = the sum of the absolute values of the terms of the output as the comment
                         block above LinUpd forms it (every matrix by its absolute value, every difference as a sum), k = the
                         float32 roundings on the output's path (roundings()):
                             every output     inv_bt = (float)(1 / Bt), the final cast                         2
                             d logvar         each of its two terms meets ONE of inv_bt / rows_over_bt         2
                             d epsilon        + rows = (float)rows                                             3
                             dkl              + rows                                                           3
                             mse, loss        + rows, + the float constant log 2 pi                            4
                         The float64 arithmetic in between (and the matrix-core updater's own e^x and 1 / x, good to 1e-16)
                         adds nothing at this scale."""
import ctypes as C
import math

import torch

from tests import dense16_ref as R

D64 = torch.float64
LOG2PI = math.log(2.0 * math.pi)
U24 = 2.0 ** -24


# ---- vaek_debug_lin (csrc/linear_moments.hip) ---------------------------------------------------------------------------------
PLAN_FIELDS = ("ok", "NB", "NO", "T", "ntiles", "persist", "which_step", "which_persist", "n_stream", "n_reduce")


class LinDebugArgs(C.Structure):
    _fields_ = [("plan", C.c_int32 * 10), ("n", C.c_int32), ("reserved", C.c_int32), ("xs", C.c_void_p), ("z1s", C.c_void_p),
                ("z2s", C.c_void_p), ("step_dev", C.c_void_p), ("M_out", C.c_void_p)]


def bind(lib):
    fn = lib.vaek_debug_lin
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LinDebugArgs), C.c_void_p, C.c_void_p]
    return fn


# ---- the packed image -----------------------------------------------------------------------------------------------------------
def n_blocks(D, L):
    return 3 if (L + 2 * D + 1 + 15) // 16 <= 3 else 4


def image_len(NB):
    return NB * (NB + 1) // 2 * 256


def lin_blk(NB, b1, b2):
    return b1 * NB - b1 * (b1 - 1) // 2 + (b2 - b1)


def _coords(NB, device="cpu"):
    """Per image element e: (row, col) of the 16 NB x 16 NB matrix, and whether e lies in a diagonal block (lin_img_coords)."""
    e = torch.arange(image_len(NB), device=device)
    blk, ln = e >> 8, (e >> 2) & 63
    i, j = ((ln >> 4) << 2) + (e & 3), ln & 15
    b1 = torch.zeros_like(blk)
    b2 = torch.zeros_like(blk)
    for a in range(NB):
        for b in range(a, NB):
            hit = blk == lin_blk(NB, a, b)
            b1[hit], b2[hit] = a, b
    return 16 * b1 + i, 16 * b2 + j, b1 == b2


def m_index(NB, r, c):
    """lin_m_index: where element (r, c) of the symmetric matrix is read from."""
    br, bc = r >> 4, c >> 4
    b1, b2, i, j = (br, bc, r & 15, c & 15) if br <= bc else (bc, br, c & 15, r & 15)
    return lin_blk(NB, b1, b2) * 256 + (((i >> 2) * 16 + j) << 2) + (i & 3)


def pack(M, NB):
    """M [..., nf, nf] (nf <= 16 NB; symmetric) -> the image [..., NO]: unused features are zero."""
    n = 16 * NB
    full = torch.zeros(M.shape[:-2] + (n, n), dtype=M.dtype, device=M.device)
    full[..., :M.shape[-2], :M.shape[-1]] = M
    r, c, _ = _coords(NB, M.device)
    return full[..., r, c].contiguous()


def unpack(img, NB):
    """The image [..., NO] -> the 16 NB x 16 NB matrix the updaters read: the stored block triangle and its mirror below (a diagonal
    block as it is stored)."""
    n = 16 * NB
    r, c, diag = _coords(NB, img.device)
    out = torch.zeros(img.shape[:-1] + (n, n), dtype=img.dtype, device=img.device)
    off = ~diag
    out[..., c[off], r[off]] = img[..., off]
    out[..., r, c] = img
    return out


def cells(D, L, NB, device="cpu"):
    """Three boolean masks over the image that partition it: cells of real features (both < L + 2 D + 1; of a diagonal block the upper
    half with the diagonal), the mirrored (lower) half of the diagonal blocks, and the cells that must be exactly zero."""
    nf = L + 2 * D + 1
    r, c, diag = _coords(NB, device)
    live = (r < nf) & (c < nf)
    mirror = live & diag & (r > c)
    return live & ~mirror, mirror, ~live


# ---- batches --------------------------------------------------------------------------------------------------------------------
def _gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) & (2 ** 63 - 1))
    return g


def exact_batch(B, D, L, seed, device="cpu"):
    """x [B, D], z1 [B, L], z2 [B, D] float32 holding integers in [-7, 7], no column constant (B >= 2): every product is at most 49
    and every sum of at most 512 rows below 2^24, so float32 chains in any order are exact."""
    g = _gen(seed, device)
    out = []
    for cols in (D, L, D):
        t = torch.randint(-7, 8, (B, cols), generator=g, device=device)
        if B >= 2:
            const = (t == t[:1]).all(0)
            t[0, const] = torch.where(t[0, const] < 7, t[0, const] + 1, t[0, const] - 1)
        out.append(t.to(torch.float32))
    return out[0], out[1], out[2]


def wide_batch(B, D, L, seed, device="cpu"):
    """The same shapes with full 24-bit mantissas, random signs and magnitudes 10^U(-2, 1)."""
    g = _gen(seed, device)
    out = []
    for cols in (D, L, D):
        u = torch.rand(B, cols, generator=g, device=device, dtype=D64) * 3.0 - 2.0
        s = torch.randint(0, 2, (B, cols), generator=g, device=device).to(D64) * 2.0 - 1.0
        out.append((s * 10.0 ** u).to(torch.float32))
    return out[0], out[1], out[2]


def features(x, z1, z2):
    """U = [z1 | x | z2 | 1] in float64."""
    one = torch.ones(x.shape[0], 1, dtype=D64, device=x.device)
    return torch.cat([z1.to(D64), x.to(D64), z2.to(D64), one], 1)


def moments(x, z1, z2):
    """(M, Mabs) = (U^T U, |U|^T |U|), float64 [NF, NF]."""
    u = features(x, z1, z2)
    return u.t() @ u, u.abs().t() @ u.abs()


def n_add(T, cw):
    """float32 additions on the longest chain of one cell of a tile's image: the T / cw rows a multiplying wave takes, plus the cw
    images combined."""
    return T // cw + cw


def check_moments(img, M, Mabs, D, L, NB, nadd=None, what=""):
    """The image(s) a kernel left, [..., NO], against (M, Mabs) [..., NF, NF].  nadd None: the real cells bitwise M (exact integers);
    else within (nadd + 1) 2^-24 Mabs.  Always: the diagonal blocks bitwise symmetric, the cells of unused features == 0.  Returns
    the largest error-to-bound ratio."""
    assert img.dtype == D64 and img.shape[-1] == image_len(NB) and img.shape[:-1] == M.shape[:-2], (what, img.dtype, img.shape, M.shape)
    assert torch.isfinite(img).all(), f"{what}: non-finite moment image"
    real, mirror, zero = cells(D, L, NB, img.device)
    nz = int((img[..., zero] != 0).sum())
    assert nz == 0, f"{what}: {nz} cells of unused features are not exactly 0"
    full = unpack(img, NB)
    r, c, diag = _coords(NB, img.device)
    asym = int((full[..., r[diag], c[diag]] != full[..., c[diag], r[diag]]).sum())
    assert asym == 0, f"{what}: {asym} cells of the diagonal blocks differ from their mirror image"
    want, wabs = pack(M, NB), pack(Mabs, NB)
    live = real | mirror
    err = (img - want).abs()
    bound = torch.zeros_like(err) if nadd is None else (nadd + 1) * U24 * wabs
    bad = (err > bound) & live
    if bad.any():
        over = torch.where(live, err - bound, torch.full_like(err, -1.0))
        idx = tuple(int(v) for v in torch.unravel_index(torch.argmax(over), over.shape))
        e = idx[-1]
        rule = "differ from the exact integer moments" if nadd is None else f"are outside ({nadd} + 1) 2^-24 Mabs"
        raise AssertionError(f"{what}: {int(bad.sum())} cells {rule}; worst at {idx} (row {int(r[e])}, col {int(c[e])}): "
                             f"got {float(img[idx])!r} want {float(want[idx])!r} Mabs {float(wabs[idx])!r}")
    if nadd is None:
        return 0.0
    return float((err[..., live] / bound[..., live].clamp(min=1e-300)).max())


# ---- the updaters: the algebra of the comment block above LinUpd, float64, with term magnitudes ---------------------------------
def _t(a, device="cpu"):
    return torch.as_tensor(a, dtype=D64, device=device)


def step_ref(cfg, p, M, rows, Bt, eps_cli=None, p1_latents=None):
    """Loss terms and gradients of one step from (parameters, M).  p: the oracle's parameter tree (values float32-representable);
    M [NF, NF] float64; rows: the samples M sums over; Bt: the divisor of the batch mean.  Returns {"loss" | "dkl" | "mse": (value,
    mag), "grad": (ref [P], mag [P])} in the flat leaf order, mag = the sum of the absolute values of the terms.
    p1_latents: a defect for the mutation tests -- P1 = R M formed from the first p1_latents latents only."""
    D, L = cfg.D, cfg.L
    dev = M.device
    cli = float(cfg.epsilon if eps_cli is None else eps_cli)
    We, be = _t(p["Encoder/FC0/kernel"], dev), _t(p["Encoder/FC0/bias"], dev)        # [D, L], [L]
    Wd, bd = _t(p["Decoder/FC0/kernel"], dev), _t(p["Decoder/FC0/bias"], dev)        # [L, D], [D]
    lv = _t(p["epsilon_p"], dev)
    eps = float(_t(p["epsilon"]).reshape(-1)[0]) * cli if cfg.tdv else cli
    sigma, inv_var = math.exp(0.5 * eps), math.exp(-eps)
    s, elv = torch.exp(0.5 * lv), torch.exp(lv)
    nf, fone = L + 2 * D + 1, L + 2 * D
    zs, xs, z2s = slice(0, L), slice(L, L + D), slice(L + D, L + 2 * D)
    M = M.to(D64)
    Ma = M.abs()
    assert M.shape == (nf, nf), (M.shape, nf)
    # S = E + [diag(s) | 0 | 0 | 0], E = [0 | We^T | 0 | be]
    E = torch.zeros(L, nf, dtype=D64, device=dev)
    E[:, xs], E[:, fone] = We.t(), be
    S = E.clone()
    S[:, zs] += torch.diag(s)
    SM, SMa = S @ M, S.abs() @ Ma
    Q, Qa = SM - s[:, None] * M[zs], SMa + s[:, None] * Ma[zs]                      # Q = E M, as the kernels form it
    Wd1, SM1, SMa1 = Wd, SM, SMa
    if p1_latents is not None:
        Wd1, SM1, SMa1 = Wd[:p1_latents], SM[:p1_latents], SMa[:p1_latents]
    P1 = Wd1.t() @ SM1 - M[xs] + sigma * M[z2s] + bd[:, None] * M[fone][None, :]    # [D, NF]
    P1a = Wd1.abs().t() @ SMa1 + Ma[xs] + sigma * Ma[z2s] + bd.abs()[:, None] * Ma[fone][None, :]
    G, Ga = Wd @ P1, Wd.abs() @ P1a                                                  # [L, NF]
    dwd, dwda = S @ P1.t(), S.abs() @ P1a.t()                                        # [L, D]
    dd = torch.arange(D, device=dev)
    ssq = (Wd * dwd).sum() + (-P1[dd, L + dd] + sigma * P1[dd, L + D + dd] + bd * P1[:, fone]).sum()
    ssqa = (Wd.abs() * dwda).sum() + (P1a[dd, L + dd] + sigma * P1a[dd, L + D + dd] + bd.abs() * P1a[:, fone]).sum()
    musq = (We.t() * Q[:, xs]).sum() + (be * Q[:, fone]).sum()
    musqa = (We.abs().t() * Qa[:, xs]).sum() + (be.abs() * Qa[:, fone]).sum()
    z2r, z2ra = P1[dd, L + D + dd].sum(), P1a[dd, L + D + dd].sum()
    inv_bt = 1.0 / float(Bt)
    c0 = inv_var * inv_bt
    rows = float(rows)
    ll = torch.arange(L, device=dev)
    g = [((c0 * G[:, xs] + Q[:, xs] * inv_bt).t(), (c0 * Ga[:, xs] + Qa[:, xs] * inv_bt).t()),           # dWe [D, L]
         (c0 * G[:, fone] + Q[:, fone] * inv_bt, c0 * Ga[:, fone] + Qa[:, fone] * inv_bt),               # dbe
         (c0 * dwd, c0 * dwda), (c0 * P1[:, fone], c0 * P1a[:, fone]),                                   # dWd, dbd
         (0.5 * s * c0 * G[ll, ll] - 0.5 * (1.0 - elv) * rows * inv_bt, 0.5 * s * c0 * Ga[ll, ll] + 0.5 * (1.0 + elv) * rows * inv_bt)]
    if cfg.tdv:
        g.append(((cli * (-0.5 * ssq * inv_var + 0.5 * rows * D + 0.5 * sigma * z2r * inv_var) * inv_bt).reshape(1),
                  (abs(cli) * (0.5 * ssqa * inv_var + 0.5 * rows * D + 0.5 * sigma * z2ra * inv_var) * inv_bt).reshape(1)))
    dkl = (0.5 * musq - 0.5 * rows * (1.0 + lv - elv).sum()) * inv_bt
    dkla = (0.5 * musqa + 0.5 * rows * (1.0 + lv.abs() + elv).sum()) * inv_bt
    mse = (0.5 * ssq * inv_var + 0.5 * rows * D * (LOG2PI + eps)) * inv_bt
    msea = (0.5 * ssqa * inv_var + 0.5 * rows * D * (LOG2PI + abs(eps))) * inv_bt
    return {"loss": (dkl + mse, dkla + msea), "dkl": (dkl, dkla), "mse": (mse, msea),
            "grad": (torch.cat([a.reshape(-1) for a, _ in g]), torch.cat([b.reshape(-1) for _, b in g]))}


def roundings(cfg, device="cpu"):
    """k per output of the updaters' [P + 3] (gradients, loss, dkl, mse): the float32 roundings on its path (module docstring)."""
    P = 2 * cfg.D * cfg.L + 2 * cfg.L + cfg.D + (1 if cfg.tdv else 0)
    k = torch.full((P + 3,), 2.0, dtype=D64, device=device)
    if cfg.tdv:
        k[P - 1] = 3.0
    k[P], k[P + 1], k[P + 2] = 4.0, 3.0, 4.0
    return k


def step_vectors(ref, device=None):
    """step_ref's result as the kernels lay it out: (ref [P + 3], mag [P + 3]) -- gradients, loss, dkl, mse."""
    g, ga = ref["grad"]
    tail = [ref[n] for n in ("loss", "dkl", "mse")]
    r = torch.cat([g, torch.stack([a.reshape(()) for a, _ in tail])])
    m = torch.cat([ga, torch.stack([b.reshape(()) for _, b in tail])])
    return (r, m) if device is None else (r.to(device), m.to(device))


def check_step(got, cfg, ref, what=""):
    """got: the updater's float32 [P + 4] (gradients, loss, dkl, mse, 0) against step_ref's result: every element within k 2^-24 mag,
    the last slot exactly 0.  Returns the largest error-to-bound ratio."""
    r, m = step_vectors(ref, got.device)
    assert got.numel() == r.numel() + 1, (what, got.numel(), r.numel())
    assert float(got[-1]) == 0.0, f"{what}: grads[P + 3] is {float(got[-1])!r}, not 0"
    return R.check_f32(got[:-1], r, roundings(cfg, got.device) * m, tol=U24, what=what)
