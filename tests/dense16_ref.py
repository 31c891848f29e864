"""Float64 references for the bf16 Dense launchers (vaek_debug_dense16, csrc/debug_dense16.hip), rounded where each kernel
rounds, and the comparison that holds a kernel's output to them.  Needs no GPU: the functions take torch tensors on any device.

Where each kernel rounds (read from the kernel sources; "bf16(.)" = round-to-nearest-even of the float32 value):

=====================================================  ==============================================  ========================
launcher (file)                                        operands as the MFMA / ALU sees them            output
=====================================================  ==============================================  ========================
dense_fwd_bf16, dense_fwd_reparam_bf16,                bf16(x), bf16(W), bf16(dY) when staged into     f32; relu mask of dx
dense_bwd_dx_bf16, dense_bwd_dw_bf16 (gemm_bf16.hip)   LDS; bias, z1, exp(lv/2) in f32; dw's ones      from the f32 x_post
                                                       column exact (db = sum bf16(dY))                (none if x_post null)
hs_fwd, hs_dx (gemm_bf16s.hip)                         bf16 activations / dY as stored; W / W^T        bf16(f32 result); dx
                                                       through cvt_weights = bf16(W); bias f32         mask from the bf16
                                                                                                       x_post > 0
hs_dw (gemm_bf16s.hip)                                 bf16 X and dY as stored; db from the ones-MFMA  f32 slabs
sk_first_fwd (gemm_skinny16.hip)                       f32 x and W, fmaf chain in f32                  bf16(relu(.))
sk_last_fwd{,_reparam,_elbo}, sk_first_dx              bf16 A as stored, W through sk_prep = bf16(W)   f32
sk_last_bwd (both forms)                               bf16 h as stored, f32 dy, f32 W                 dh = bf16(dy W^T) * (h
                                                                                                       > 0); G f32
sk_first_bwd (both forms)                              f32 x, bf16 dY as stored                        f32
dense_fwd_out16, dense_fwd{,_reparam,_elbo}_in16,      exact f32 arithmetic on the values as stored    bf16(.) where named
dense_bwd_dx_{out,in}16, dense_bwd_dw_{x,dy}16         (the bf16 side converted exactly); dx_out16:    out16 / dx_out16, f32
(gemm_f32.hip)                                         mask from the bf16 x_post, accumulates the old  otherwise
                                                       bf16 value before its one rounding
=====================================================  ==============================================  ========================

dx_out16's accumulate form adds the old bf16 output in f32 before the single rounding; the step does not use it, but the
launcher offers it and the tests hold it too.

Bounds (check_f32 / check_bf16): per element |got - ref| <= tol * mag with mag = (|A| . |B| + |bias| + |every epilogue addend|),
the absolute operands taken after the kernel's bf16 rounding; tol = F32_TOL.  A bf16 output additionally may differ from bf16(ref)
by at most one bf16 ulp in at most BF16_OFF_FRACTION of its elements (an element whose f32 error bound exceeds one bf16 ulp of
its value, a cancellation, is held by the first bound alone), and masked elements must be exactly 0."""
import torch

F32_TOL = 4e-6
BF16_OFF_FRACTION = 0.005
D64 = torch.float64


def bf16(t):
    """float32 values -> bf16 (round to nearest even), returned as float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(D64)


def bf16_trunc(t):
    """float32 values -> bf16 by truncation (what a wrong epilogue would do), returned as float64."""
    u = t.to(torch.float32).contiguous().view(torch.int32) & -65536
    return u.view(torch.float32).to(D64)


def round_bf16_exact(t):
    """float64 -> the nearest bf16 value (ties to even), without a detour through float32 (no double rounding): float64 keeps 52
    fraction bits, bf16 7, so round away the low 45 bits of the float64 pattern (integer arithmetic: exact on every device)."""
    u = t.to(D64).contiguous().view(torch.int64)
    lsb = (u >> 45) & 1
    u = (u + ((1 << 44) - 1) + lsb) & ~((1 << 45) - 1)
    return u.view(D64)


def _bf16_key(t):
    """bf16 values (float64) -> integers in value order, adjacent bf16 values one apart."""
    b = (t.to(torch.float32).contiguous().view(torch.int32) >> 16).to(torch.int64)
    mag = b & 0x7FFF
    return torch.where(b < 0, -mag, mag)


def f64(t):
    return t.to(D64)


def linear(a, w, b=None):
    """y = a @ w (+ b) in float64, and its magnitude |a| @ |w| (+ |b|)."""
    y = a @ w
    mag = a.abs() @ w.abs()
    if b is not None:
        y = y + b
        mag = mag + b.abs()
    return y, mag


def forward(x, w, b, relu=False, round_x=False, round_w=False):
    """Dense forward: relu(x W + b).  Returns (ref, mag, zero_mask): zero_mask marks the outputs relu forces to 0 (strictly
    negative pre-activations; a pre-activation within the bound of 0 is left free)."""
    a = bf16(x) if round_x else f64(x)
    wv = bf16(w) if round_w else f64(w)
    y, mag = linear(a, wv, f64(b) if b is not None else None)
    zero = None
    if relu:
        zero = y < -F32_TOL * mag
        y = y.clamp(min=0.0)
    return y, mag, zero


def reparam(mu, mag, z1, lv):
    """samples = mu + exp(lv / 2) z1 (f32 epilogue): ref and magnitude."""
    s = torch.exp(0.5 * f64(lv)) * f64(z1)
    return mu + s, mag + s.abs()


def elbo(y, mag, xdata, z2, eps, inv_bt):
    """dL/dx_hat of the ELBO epilogue: (y + exp(eps / 2) z2 - x) exp(-eps) inv_bt, eps = eps_param * eps_cli already multiplied
    out.  Returns (ref, mag)."""
    sz = torch.exp(torch.tensor(0.5 * eps, dtype=D64)) * f64(z2)
    scale = float(torch.exp(torch.tensor(-eps, dtype=D64))) * inv_bt
    r = y + sz - f64(xdata)
    return r * scale, (mag + sz.abs() + f64(xdata).abs()) * scale


def backward_dx(dy, w, x_post=None, acc=None, round_dy=False, round_w=False):
    """dX = (dY W^T) * (x_post > 0) (+ acc).  Returns (ref, mag, zero_mask)."""
    d = bf16(dy) if round_dy else f64(dy)
    wv = bf16(w) if round_w else f64(w)
    y, mag = linear(d, wv.t())
    zero = None
    if x_post is not None:
        keep = f64(x_post) > 0
        y = torch.where(keep, y, torch.zeros_like(y))
        mag = torch.where(keep, mag, torch.zeros_like(mag))
        zero = ~keep
    if acc is not None:
        y = y + f64(acc)
        mag = mag + f64(acc).abs()
        zero = None
    return y, mag, zero


def backward_dw(x, dy, round_x=False, round_dy=False):
    """[X | 1]^T dY as the flat-gradient image [(n_in + 1), n_out].  Returns (ref, mag)."""
    a = bf16(x) if round_x else f64(x)
    d = bf16(dy) if round_dy else f64(dy)
    a1 = torch.cat([a, torch.ones(a.shape[0], 1, dtype=D64, device=a.device)], dim=1)
    return a1.t() @ d, a1.abs().t() @ d.abs()


def check_f32(got, ref, mag, zero=None, tol=F32_TOL, what=""):
    """|got - ref| <= tol * mag everywhere, exactly 0 where `zero` is set.  Returns the largest error-to-bound ratio."""
    got, ref, mag = f64(got), f64(ref), f64(mag)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    if zero is not None and zero.any():
        nz = (got[zero] != 0).sum()
        assert int(nz) == 0, f"{what}: {int(nz)} relu-masked elements are not exactly 0"
    err = (got - ref).abs()
    bound = tol * mag
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err - bound).flatten()))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside {tol:g} * mag; worst at {idx}: "
                             f"got {float(got[idx])!r} ref {float(ref[idx])!r} mag {float(mag[idx])!r}")
    return float((err / bound.clamp(min=1e-300)).max()) if got.numel() else 0.0


def check_bf16(got, ref, mag, zero=None, tol=F32_TOL, what=""):
    """A bf16 output: within 2^-8 |ref| + tol * mag everywhere; equal to bf16(ref) but for at most BF16_OFF_FRACTION of the elements,
    those one bf16 ulp away; exactly 0 where `zero` is set.  Returns the largest ratio of the error beyond half a bf16 ulp of ref
    to tol * mag."""
    got, ref, mag = f64(got), f64(ref), f64(mag)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    if zero is not None and zero.any():
        nz = (got[zero] != 0).sum()
        assert int(nz) == 0, f"{what}: {int(nz)} relu-masked elements are not exactly 0"
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + tol * mag
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err - bound).flatten()))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside 2^-8 |ref| + {tol:g} * mag; worst at {idx}: "
                             f"got {float(got[idx])!r} ref {float(ref[idx])!r}")
    r16 = round_bf16_exact(ref)
    off = got != r16
    n_off = int(off.sum())
    assert n_off <= BF16_OFF_FRACTION * got.numel(), f"{what}: {n_off} of {got.numel()} elements differ from bf16(ref)"
    # one ulp at most -- where the f32 arithmetic can decide the rounding at all: an output that cancels to below its own f32
    # error (tol * mag over one bf16 ulp of ref) is held by the bound above alone
    decided = off & (ref != 0) & (tol * mag < torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 8))
    if decided.any():
        steps = (_bf16_key(got[decided]) - _bf16_key(r16[decided])).abs()
        assert int(steps.max()) == 1, f"{what}: an element is {int(steps.max())} bf16 ulps from bf16(ref)"
    # reported: the error beyond the output's own rounding (half a bf16 ulp of ref) over the f32 part of the bound
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 9).abs()
    excess = (err - half_ulp).clamp(min=0)
    return float((excess / (tol * mag).clamp(min=1e-300)).max()) if got.numel() else 0.0
