"""Float64 references for the Dense launchers (vaek_debug_dense16, csrc/debug_dense16.hip), rounded where each kernel
rounds (the all-f32 kernels of gemm_f32.hip, tests/test_gpu_dense32.py: nowhere), and the comparison that holds a kernel's output to
them.  Needs no GPU: the functions take torch tensors on any device.

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
its value, a cancellation, is held by the first bound alone), and masked elements must be exactly 0.

ELBO epilogues also leave one {mse, d eps} pair per output tile; elbo_sums gives the float64 totals over the real rows x columns and
bounds that carry each element's own bound through the two sums, check_sums holds the tile pairs to them.  guarded / check_guard put
an output between two bands of one NaN bit pattern and look for a store outside it (or an element nobody stored)."""
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


def elbo_sums(y, mag, xdata, z2, eps, tol=F32_TOL):
    """The two sums of the ELBO epilogue over the real rows x columns, rr = y + exp(eps / 2) z2 - x:
    mse = sum rr^2 exp(-eps) / 2, deps = sum (-rr^2 exp(-eps) / 2 + exp(eps / 2) z2 rr exp(-eps) / 2).
    Returns ((mse, deps), (bound_mse, bound_deps)) as float64 numbers.  An element's rr is known to tol * m, m = the magnitude elbo()
    uses for rr before scaling; d(rr^2 / 2) = |rr| d rr, and the products' own roundings add tol * (their value)."""
    e = torch.tensor(float(eps), dtype=D64)
    sig, inv_var = float(torch.exp(0.5 * e)), float(torch.exp(-e))
    z, x = f64(z2), f64(xdata)
    sz = sig * z
    rr = y + sz - x
    m = mag + sz.abs() + x.abs()
    q = 0.5 * rr * rr * inv_var
    mse = q.sum()
    deps = (-q + 0.5 * sig * z * rr * inv_var).sum()
    b_q = inv_var * (rr.abs() * m + 0.5 * rr * rr)
    b_mse = tol * b_q.sum()
    b_deps = tol * (b_q + 0.5 * float(torch.exp(-0.5 * e)) * z.abs() * (m + rr.abs())).sum()
    return (float(mse), float(deps)), (float(b_mse), float(b_deps))


def check_sums(parts, ref, bound, what=""):
    """parts: the {mse, d eps} pairs of every tile, flat.  Their float64 totals are within `bound` of `ref`.  Returns the larger
    error-to-bound ratio."""
    p = f64(parts).reshape(-1, 2)
    assert p.numel() > 0, f"{what}: no tile pairs"
    assert torch.isfinite(p).all(), f"{what}: non-finite tile sums"
    ratio = 0.0
    for name, got, r, b in zip(("mse", "d eps"), p.sum(dim=0).tolist(), ref, bound):
        assert abs(got - r) <= b, f"{what}: {name} sum {got!r} is not within {b!r} of {r!r} ({p.shape[0]} tiles)"
        ratio = max(ratio, abs(got - r) / max(b, 1e-300))
    return ratio


GUARD = 256                  # floats kept on each side of a guarded output
GUARD_FILL = 0x7FC5A5A5      # one quiet-NaN bit pattern no kernel here produces


def guarded(numel, device, lead=0):
    """A float32 buffer of GUARD + lead + numel + GUARD elements, every one GUARD_FILL.  Returns (buffer, view): the view is the
    `numel` floats that start GUARD + lead floats in (lead: 0-3 floats off the buffer's 16-byte alignment)."""
    buf = torch.full((2 * GUARD + lead + numel,), GUARD_FILL, dtype=torch.int32, device=device).view(torch.float32)
    return buf, buf[GUARD + lead:GUARD + lead + numel]


def check_guard(buf, view, written=None, prefilled=False, what=""):
    """The GUARD floats before and after `view` (made by guarded()) still hold the fill bit for bit, and no element of the view does.
    written: only the first `written` elements of the view are to be stored; the rest must still hold the fill.  prefilled: the caller put values into the view before the call (an accumulating op),
    so only the bands are looked at."""
    bits = buf.view(torch.int32)
    n = view.numel()
    start = view.storage_offset() - buf.storage_offset()
    assert 0 <= start - GUARD and start + n + GUARD <= bits.numel(), (what, start, n, bits.numel())
    w = n if written is None else written
    assert 0 <= w <= n, (what, w, n)
    before = int((bits[start - GUARD:start] != GUARD_FILL).sum())
    after = int((bits[start + n:start + n + GUARD] != GUARD_FILL).sum())
    assert before == 0, f"{what}: {before} floats stored in front of the output"
    assert after == 0, f"{what}: {after} floats stored behind the output"
    if prefilled:
        return
    left = int((bits[start:start + w] == GUARD_FILL).sum())
    assert left == 0, f"{what}: {left} of {w} output elements were never stored"
    stray = int((bits[start + w:start + n] != GUARD_FILL).sum())
    assert stray == 0, f"{what}: {stray} elements stored past the {w} expected"
