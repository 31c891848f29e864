"""Float64 references for the kernels of the step's tail (csrc/elbo.hip: elbo, elbo_reduce, reparam_bwd, finalize, bulk_finalize,
adam, out4, add_noise, sum_slabs_inplace), reached one launcher at a time through vaek_debug_tail (csrc/debug_tail.hip), and the
ctypes image of that entry's argument struct.  Needs no GPU: the functions take torch tensors on any device.

The bounds follow tests/dense16_ref.py: per output |got - ref| <= F32_TOL * mag, mag = the sum of the absolute values of the terms
that make the output (a difference 1 - s counts as 1 + s).  Where an output is a function of an inexact input (the update of Adam
from m), the input's magnitude is carried through in place of its value.

  d_lin   = r e^-eps inv_bt, r = y_lin (+ sg) + e^(eps/2) z2 - x      mag = (|y_lin| + sg + |e^(eps/2) z2| + |x|) e^-eps inv_bt
  d_sig   = d_lin sg (1 - sg)                                          mag = mag(d_lin) sg (1 + sg)
  partial = {sum mse, sum mu^2, sum d eps, 0} per split                dense16_ref.elbo_sums' bounds over the split's own rows,
                                                                       F32_TOL * sum mu^2
  dmu     = d + mu inv_bt; partial[s][l] = sum_rows d z1               mag = |d| + |mu| inv_bt; sum |d z1|
  d_logvar_e = 1/2 e^(lv/2) S - 1/2 (1 - e^lv) rows/bt                 mag = 1/2 e^(lv/2) S|.| + 1/2 (1 + e^lv) rows/bt
  d eps   = eps_cli (sum deps + 1/2 rows D) inv_bt                     the same with absolute values
  dkl     = (1/2 sum mu^2 - 1/2 rows sum_l (1 + lv - e^lv)) inv_bt     mag = (1/2 sum mu^2 + 1/2 rows sum_l (1 + |lv| + e^lv)) inv_bt
  mse     = (sum + 1/2 rows D (log 2 pi + eps)) inv_bt                 the same with absolute values
  Adam    m' = b1 m + (1 - b1) g, v' = b2 v + (1 - b2) g^2             mag = |b1 m| + |(1 - b1) g|; v' itself
          p' = p - lr (m' / bc1) / (sqrt(v' / bc2) + 1e-8)             |got - ref| <= 2^-24 |ref| + F32_TOL * lr (mag(m') / bc1) / (...)

On the parameter bound: it is relative to the UPDATE, not to |p| (which would hide the update), plus the one rounding the
stored parameter carries; and the update is as inexact as m' is, so where b1 m and (1 - b1) g cancel its magnitude is taken from
mag(m') -- with |m'| in its place one element in thirty of a random state is outside F32_TOL from float32 rounding alone."""
import ctypes as C
import math

import torch

from tests import dense16_ref as R

F32_TOL, D64, f64 = R.F32_TOL, R.D64, R.f64
LOG2PI = math.log(2.0 * math.pi)
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8

# ---- vaek_debug_tail (csrc/debug_tail.hip) ------------------------------------------------------------------------------------
TAIL_OPS = ["elbo", "elbo_reduce", "reparam_bwd", "finalize", "out4", "add_noise", "sum_slabs_inplace", "sum_slabs"]
TAIL_OP = {n: i for i, n in enumerate(TAIL_OPS)}
_PTRS = ["x", "y_lin", "y_sig", "z2", "mu", "eps_param", "d_lin", "d_sig", "partial", "step_dev", "part", "dsamp", "z1", "slabs", "epart",
         "rpart", "params", "grads", "params_rw", "m", "v", "loss_hist", "lv", "out", "scratch"]


class TailArgs(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("rows", "D", "L", "S", "rows_per_split", "bm", "nbx", "want_deps", "Se", "fuse", "nseg", "reserved")] +
                [("seg_end", C.c_int32 * 32), ("seg_S", C.c_int32 * 32)] +
                [(n, C.c_int64) for n in ("P", "off_epsp", "off_eps", "hi", "lo", "slab_stride", "n", "loss_hist_cap")] +
                [(n, C.c_float) for n in ("eps_cli", "inv_bt", "rows_over_bt", "rows_f", "lr", "reserved_f")] +
                [(n, C.c_void_p) for n in _PTRS] + [("scratch_bytes", C.c_int64)])


def bind(lib):
    fn = lib.vaek_debug_tail
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(TailArgs), C.c_void_p]
    return fn


def tail_args(**kw):
    """TailArgs from keywords: tensors become their addresses, seg_end / seg_S take lists."""
    a = TailArgs()
    for k, val in kw.items():
        if k in ("seg_end", "seg_S"):
            for i, e in enumerate(val):
                getattr(a, k)[i] = int(e)
        elif isinstance(val, torch.Tensor):
            assert val.is_contiguous()
            setattr(a, k, val.data_ptr())
        else:
            setattr(a, k, val)
    return a


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def f32(v):
    """A Python number as the float32 the library receives."""
    return float(torch.tensor(v, dtype=torch.float32))


def eps_of(eps_param, eps_cli):
    """eps = eps_param * eps_cli formed as ONE float32 product (the kernels' first line), or eps_cli alone."""
    if eps_param is None:
        return f32(eps_cli)
    return float(torch.tensor(float(eps_param), dtype=torch.float32) * torch.tensor(eps_cli, dtype=torch.float32))


def n_splits(rows, rps):
    return (rows + rps - 1) // rps


def split_sums(v, rps):
    """v [rows, ...] float64 -> [S, ...]: the sum over each split's own rows (split s owns rows [s rps, (s + 1) rps))."""
    rows = v.shape[0]
    idx = torch.arange(rows, device=v.device) // rps
    out = torch.zeros((n_splits(rows, rps),) + tuple(v.shape[1:]), dtype=D64, device=v.device)
    return out.index_add_(0, idx, v)


def ratio_of(got, ref, bound, what=""):
    """Elementwise |got - ref| <= bound (a tensor of bounds, not tol * mag).  Returns the largest ratio."""
    return R.check_f32(got, ref, bound, tol=1.0, what=what)


# ---- elbo / elbo_reduce -------------------------------------------------------------------------------------------------------
def elbo_elements(x, y_lin, y_sig, z2, eps, inv_bt):
    """Returns (y, mag, (d_lin, mag), (d_sig, mag) or None): y = y_lin (+ sigmoid(y_sig)) with its magnitude, the two gradients."""
    y, mag = f64(y_lin), f64(y_lin).abs()
    sg = None
    if y_sig is not None:
        sg = torch.sigmoid(f64(y_sig))
        y, mag = y + sg, mag + sg
    d_lin, m_lin = R.elbo(y, mag, x, z2, eps, inv_bt)
    d_sig = None if sg is None else (d_lin * sg * (1.0 - sg), m_lin * sg * (1.0 + sg))
    return y, mag, (d_lin, m_lin), d_sig


def elbo_row_sums(y, mag, x, z2, eps, tol=F32_TOL):
    """dense16_ref.elbo_sums row by row: (mse, deps, bound_mse, bound_deps), each [rows] (the same formulas, summed over columns only)."""
    e = torch.tensor(float(eps), dtype=D64)
    sig, inv_var = float(torch.exp(0.5 * e)), float(torch.exp(-e))
    z, xd = f64(z2), f64(x)
    sz = sig * z
    rr = y + sz - xd
    m = mag + sz.abs() + xd.abs()
    q = 0.5 * rr * rr * inv_var
    b_q = inv_var * (rr.abs() * m + 0.5 * rr * rr)
    b_d = b_q + 0.5 * float(torch.exp(-0.5 * e)) * z.abs() * (m + rr.abs())
    return q.sum(1), (-q + 0.5 * sig * z * rr * inv_var).sum(1), tol * b_q.sum(1), tol * b_d.sum(1)


def elbo_partials(y, mag, x, z2, mu, eps, rps):
    """partial[S][3] = {sum mse, sum mu^2, sum d eps} over each split's own rows, and its bounds [S][3]."""
    mse, deps, b_mse, b_deps = elbo_row_sums(y, mag, x, z2, eps)
    musq = (f64(mu) ** 2).sum(1)
    ref = torch.stack([split_sums(mse, rps), split_sums(musq, rps), split_sums(deps, rps)], 1)
    bound = torch.stack([split_sums(b_mse, rps), F32_TOL * split_sums(musq, rps), split_sums(b_deps, rps)], 1)
    return ref, bound


def tile_partials(part, bm, nbx, mu, rows, rps):
    """elbo_reduce: split s sums the pairs of the tile rows it owns.  part [tile rows, nbx, 2] -> (ref [S][3], bound [S][3])."""
    p = f64(part)[:(rows + bm - 1) // bm]
    per_row = rps // bm
    musq = split_sums((f64(mu) ** 2).sum(1), rps)
    ref = torch.stack([split_sums(p[..., 0].sum(1), per_row), musq, split_sums(p[..., 1].sum(1), per_row)], 1)
    bound = F32_TOL * torch.stack([split_sums(p[..., 0].abs().sum(1), per_row), musq, split_sums(p[..., 1].abs().sum(1), per_row)], 1)
    return ref, bound


def check_partials(partial, ref, bound, what=""):
    """partial [S][4] against (ref, bound) [S][3]: every split by itself, the float64 totals, and partial[s][3] == 0 exactly."""
    p = f64(partial).reshape(-1, 4)
    assert p.shape[0] == ref.shape[0], (what, p.shape, ref.shape)
    assert torch.isfinite(p).all(), f"{what}: non-finite partial"
    assert int((p[:, 3] != 0).sum()) == 0, f"{what}: partial[s][3] is not exactly 0"
    r = ratio_of(p[:, :3], ref, bound, what=what + " per split")
    return max(r, ratio_of(p[:, :3].sum(0), ref.sum(0), bound.sum(0), what=what + " totals"))


# ---- reparam_bwd --------------------------------------------------------------------------------------------------------------
def reparam_bwd(d, mu, z1, inv_bt, rps):
    """Returns ((dmu, mag), (partial [S][L], mag))."""
    d, mu, z1 = f64(d), f64(mu), f64(z1)
    return (d + mu * inv_bt, d.abs() + mu.abs() * inv_bt), (split_sums(d * z1, rps), split_sums((d * z1).abs(), rps))


def d_logvar(s, s_mag, lv, rows_over_bt):
    """d logvar_e from the summed partials: (ref, mag)."""
    lv = f64(lv)
    h, e = 0.5 * torch.exp(0.5 * lv), torch.exp(lv)
    return h * s - 0.5 * (1.0 - e) * rows_over_bt, h * s_mag + 0.5 * (1.0 + e) * rows_over_bt


# ---- finalize / out4 ----------------------------------------------------------------------------------------------------------
def loss_terms(epart, lv, eps, rows, D, inv_bt):
    """From epart [Se][4] (float32 partials as the kernel reads them): {name: (ref, mag)} for loss, dkl, mse and deps = (sum d eps +
    1/2 rows D) inv_bt."""
    e, lv = f64(epart).reshape(-1, 4), f64(lv)
    s_mse, s_musq, s_deps = e[:, 0].sum(), e[:, 1].sum(), e[:, 2].sum()
    dkl = (0.5 * s_musq - 0.5 * rows * (1.0 + lv - torch.exp(lv)).sum()) * inv_bt
    m_dkl = (0.5 * s_musq + 0.5 * rows * (1.0 + lv.abs() + torch.exp(lv)).sum()) * inv_bt
    c = 0.5 * rows * D
    mse = (s_mse + c * (LOG2PI + eps)) * inv_bt
    m_mse = (e[:, 0].abs().sum() + c * (LOG2PI + abs(eps))) * inv_bt
    deps = (s_deps + c) * inv_bt
    m_deps = (e[:, 2].abs().sum() + c) * inv_bt
    return {"loss": (dkl + mse, m_dkl + m_mse), "dkl": (dkl, m_dkl), "mse": (mse, m_mse), "deps": (deps, m_deps)}


def finalize(slabs, segs, S, epart, rpart, params, off_epsp, off_eps, L, D, eps_cli, rows_over_bt, inv_bt, rows):
    """grads[P + 4] of the finalisation: (ref, mag).  slabs [>= max S, stride]; segs = [(end, slab count)] ascending, outputs behind
    the last end up to off_epsp take S slabs."""
    P = off_epsp + L + (1 if off_eps >= 0 else 0)
    dev = slabs.device
    ref, mag = torch.zeros(P + 4, dtype=D64, device=dev), torch.zeros(P + 4, dtype=D64, device=dev)
    start = 0
    for end, cnt in list(segs) + [(off_epsp, S)]:
        if end > start:
            blk = f64(slabs[:cnt, start:end])
            ref[start:end], mag[start:end] = blk.sum(0), blk.abs().sum(0)
        start = max(start, end)
    lv = params[off_epsp:off_epsp + L]
    rp = f64(rpart).reshape(-1, L)
    ref[off_epsp:off_epsp + L], mag[off_epsp:off_epsp + L] = d_logvar(rp.sum(0), rp.abs().sum(0), lv, rows_over_bt)
    eps = eps_of(float(params[off_eps]) if off_eps >= 0 else None, eps_cli)
    t = loss_terms(epart, lv, eps, rows, D, inv_bt)
    if off_eps >= 0:
        ref[off_eps], mag[off_eps] = f32(eps_cli) * t["deps"][0], abs(f32(eps_cli)) * t["deps"][1]
    for k, name in enumerate(("loss", "dkl", "mse")):
        ref[P + k], mag[P + k] = t[name]
    return ref, mag


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def adam(p, m, v, g, t, lr, grad_scale=1.0):
    """One step from the float32 state (p, m, v) and gradient g at step t >= 1.  Returns ((m', mag), (v', mag), (p', update mag)):
    1 - beta formed in double, bias corrections 1 - beta^t in float64."""
    p, m, v, g = f64(p), f64(m), f64(v), f64(g) * grad_scale
    m1, mm = B1 * m + (1.0 - B1) * g, (B1 * m).abs() + ((1.0 - B1) * g).abs()
    v1 = B2 * v + (1.0 - B2) * g * g
    bc1, bc2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    den = torch.sqrt(v1 / bc2) + ADAM_EPS
    return (m1, mm), (v1, v1), (p - lr * (m1 / bc1) / den, lr * (mm / bc1) / den)


def check_param(got, ref, upd_mag, what=""):
    """|got - ref| <= 2^-24 |ref| + F32_TOL * (magnitude of the update).  Returns, as dense16_ref.check_bf16 does for a rounded output,
    the largest ratio of the error beyond the stored parameter's own rounding (half a float32 ulp of ref, which an element at the
    bottom of its binade uses up entirely) to the update's part of the bound."""
    got, ref, upd_mag = f64(got), f64(ref), f64(upd_mag)
    ratio_of(got, ref, 2.0 ** -24 * ref.abs() + F32_TOL * upd_mag, what=what)
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 25)
    excess = ((got - ref).abs() - half_ulp).clamp(min=0)
    return float((excess / (F32_TOL * upd_mag).clamp(min=1e-300)).max()) if got.numel() else 0.0


def check_adam(got_p, got_m, got_v, p, m, v, g, t, lr, grad_scale=1.0, what=""):
    """The state after one step against the float64 step from (p, m, v).  Returns the ratios (m, v, p)."""
    (m1, mm), (v1, mv), (p1, um) = adam(p, m, v, g, t, lr, grad_scale)
    return (R.check_f32(got_m, m1, mm, what=what + " m"), R.check_f32(got_v, v1, mv, what=what + " v"),
            check_param(got_p, p1, um, what=what + " p"))


# ---- add_noise / sum_slabs ----------------------------------------------------------------------------------------------------
def add_noise(y_lin, y_sig, z2, eps):
    sz = math.exp(0.5 * eps) * f64(z2)
    y, mag = f64(y_lin) + sz, f64(y_lin).abs() + sz.abs()
    if y_sig is not None:
        sg = torch.sigmoid(f64(y_sig))
        y, mag = y + sg, mag + sg
    return y, mag


def sum_slabs(slabs, S, n):
    blk = f64(slabs[:S, :n])
    return blk.sum(0), blk.abs().sum(0)
