"""The comparison of tests/test_gpu_dense16.py and tests/test_gpu_dense32.py has power: references with the bugs tiled kernels tend to have must FAIL it, while
a float32 emulation of a correct kernel passes.  Also: vaek_debug_dense16 refuses shapes the step never sends before it launches
anything (no GPU needed: the checks run on the host)."""
import ctypes as C

import pytest
import torch

from tests import dense16_ref as R

torch.manual_seed(0)


def _x(rows, n):
    return R.bf16(torch.relu(torch.randn(rows, n) + 0.4)).float()


def _layer(n_in, n_out):
    return torch.randn(n_in, n_out) * n_in ** -0.5, torch.randn(n_out) * 0.3


def _fails(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def test_f32_emulation_passes():
    """Positive control: the kernels' own arithmetic (float32 accumulation of the bf16-rounded operands) is inside the bound."""
    x, (w, b) = _x(2049, 512), _layer(512, 257)
    got = (R.bf16(x).float() @ R.bf16(w).float() + b).double()
    ref, mag, _ = R.forward(x, w, b, round_x=True, round_w=True)
    assert R.check_f32(got, ref, mag) < 1.0
    xa, dy = torch.cat([_x(4097, 96), torch.ones(4097, 1)], 1), torch.randn(4097, 64)
    ref, mag = R.backward_dw(xa[:, :-1], dy)
    assert R.check_f32((xa.t() @ dy).double(), ref, mag) < 1.0
    y, mag, zero = R.forward(x, w, b, relu=True, round_w=True)
    assert R.check_bf16(torch.relu(x @ R.bf16(w).float() + b).bfloat16(), y, mag, zero=zero) < 1.0


def test_mutated_references_fail():
    # the last row dropped from a dW sum at 4 097 rows
    x, dy = _x(4097, 64), torch.randn(4097, 96)
    got = R.backward_dw(x, dy)[0].float()
    ref, mag = R.backward_dw(x[:-1], dy[:-1])
    assert R.check_f32(got, *R.backward_dw(x, dy)) < 1.0
    _fails(R.check_f32, got, ref, mag)
    # one k index dropped
    x, (w, b) = _x(129, 512), _layer(512, 257)
    ok, mag, _ = R.forward(x, w, b, round_w=True)
    got = ok.float()
    xm = x.clone()
    xm[:, 300] = 0
    ref, mag_m, _ = R.forward(xm, w, b, round_w=True)
    _fails(R.check_f32, got, ref, mag_m)
    # one column of the last tile (columns 256.. of 257) shifted
    ref = ok.clone()
    ref[:, 255:257] = ok[:, 254:256]
    _fails(R.check_f32, got, ref, mag)
    # the bias off by one column
    ref, mag_m, _ = R.forward(x, w, torch.roll(b, 1), round_w=True)
    _fails(R.check_f32, got, ref, mag_m)
    # truncation instead of round-to-nearest-even in a bf16 output
    _fails(R.check_bf16, R.bf16_trunc(got), ok, mag)
    assert R.check_bf16(R.bf16(got), ok, mag) < 1.0


def _g(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _elbo_f32(h, w, b, xd, z2, eps, tile=64, rows=None, cols=None):
    """The ELBO epilogue's tile pairs as a float32 kernel makes them: every product and sum in float32, one pair per tile x tile
    block of the real rows x columns (rows / cols: index lists, to leave an element out or take one twice)."""
    f = torch.float32
    y = h.to(f) @ w.to(f) + b.to(f)
    sig, inv_var = torch.exp(torch.tensor(0.5 * eps, dtype=f)), torch.exp(torch.tensor(-eps, dtype=f))
    rr = (y + sig * z2.to(f)) - xd.to(f)
    q = rr * rr * inv_var
    mse, deps = 0.5 * q, -0.5 * q + 0.5 * sig * z2.to(f) * rr * inv_var
    if rows is not None:
        mse, deps = mse[rows], deps[rows]
    if cols is not None:
        mse, deps = mse[:, cols], deps[:, cols]
    parts = []
    for r0 in range(0, mse.shape[0], tile):
        for c0 in range(0, mse.shape[1], tile):
            parts += [mse[r0:r0 + tile, c0:c0 + tile].sum(), deps[r0:r0 + tile, c0:c0 + tile].sum()]
    return torch.stack(parts)


def test_f32_kernels_emulation_passes():
    """Positive control for the all-f32 kernels: operands and accumulation in float32 stay inside the unrounded float64 reference's
    bound at the longest reductions of tests/test_gpu_dense32.py."""
    g = _g(1)
    x, w, b = torch.randn(257, 4096, generator=g), torch.randn(4096, 20, generator=g) / 64, torch.randn(20, generator=g) * 0.3
    ref, mag, _ = R.forward(x, w, b)
    assert R.check_f32(x @ w + b, ref, mag) < 1.0
    x, dy = torch.randn(4097, 96, generator=g), torch.randn(4097, 64, generator=g)
    ref, mag = R.backward_dw(x, dy)
    assert R.check_f32(torch.cat([x, torch.ones(4097, 1)], 1).t() @ dy, ref, mag) < 1.0
    h, w, b = torch.randn(4097, 64, generator=g), torch.randn(64, 33, generator=g) / 8, torch.randn(33, generator=g) * 0.3
    xd, z2 = torch.randn(4097, 33, generator=g), torch.randn(4097, 33, generator=g)
    y, mag, _ = R.forward(h, w, b)
    for eps in (-2.25, -2.0):
        sums, bounds = R.elbo_sums(y, mag, xd, z2, eps)
        assert R.check_sums(_elbo_f32(h, w, b, xd, z2, eps), sums, bounds) < 1.0


def test_mutated_f32_references_fail():
    g = _g(2)
    # ELBO tile sums at (4097, 64, 33): one ragged row left out; one padded column counted (value = bias, z2 = x = 0)
    rows, K, N, eps = 4097, 64, 33, -2.0
    h, w, b = torch.randn(rows, K, generator=g), torch.randn(K, N, generator=g) / 8, torch.randn(N, generator=g) * 0.3
    xd, z2 = torch.randn(rows, N, generator=g), torch.randn(rows, N, generator=g)
    y, mag, _ = R.forward(h, w, b)
    sums, bounds = R.elbo_sums(y, mag, xd, z2, eps)
    assert R.check_sums(_elbo_f32(h, w, b, xd, z2, eps), sums, bounds) < 1.0
    _fails(R.check_sums, _elbo_f32(h, w, b, xd, z2, eps, rows=list(range(rows - 1))), sums, bounds)
    pad = lambda t, v: torch.cat([t, torch.full((t.shape[0], 1), v)], 1)
    _fails(R.check_sums, _elbo_f32(pad(h, 0.0)[:, :K], pad(w, 0.0), torch.cat([b, b[-1:]]), pad(xd, 0.0), pad(z2, 0.0), eps), sums, bounds)
    # dW|db: the ones row one index off (the bias gradient lands on the last kernel row, the bias row stays empty)
    x, dy = torch.randn(129, 65, generator=g), torch.randn(129, 65, generator=g)
    ref, mag = R.backward_dw(x, dy)
    got = ref.float()
    assert R.check_f32(got, ref, mag) < 1.0
    bad = got.clone()
    bad[64], bad[65] = got[65], 0.0
    _fails(R.check_f32, bad, ref, mag)
    # forward at K = 130: the last k of the ragged k-tile dropped
    x, w, b = torch.randn(129, 130, generator=g), torch.randn(130, 65, generator=g) / 11, torch.randn(65, generator=g) * 0.3
    ref, mag, _ = R.forward(x, w, b)
    got = (x @ w + b)
    assert R.check_f32(got, ref, mag) < 1.0
    _fails(R.check_f32, x[:, :129] @ w[:129] + b, ref, mag)
    # the two rows on either side of the last full tile swapped
    bad = got.clone()
    bad[[127, 128]] = got[[128, 127]]
    _fails(R.check_f32, bad, ref, mag)


def test_guard_bands_see_one_float():
    for lead in (0, 1, 3):
        def fresh():
            buf, v = R.guarded(100, "cpu", lead)
            v.copy_(torch.arange(100.0))
            return buf, v
        buf, v = fresh()
        assert v.numel() == 100 and buf.numel() == 2 * R.GUARD + lead + 100 and v.data_ptr() == buf.data_ptr() + 4 * (R.GUARD + lead)
        R.check_guard(buf, v)
        for i in (R.GUARD + lead - 1, R.GUARD + lead - R.GUARD, R.GUARD + lead + 100, R.GUARD + lead + 100 + R.GUARD - 1):
            buf, v = fresh()
            buf[i] = 0.0                                   # one float in front of / behind the output
            _fails(R.check_guard, buf, v)
            _fails(R.check_guard, buf, v, prefilled=True)
        buf, v = R.guarded(100, "cpu", lead)
        v[:99] = 1.0                                       # one element nobody stored
        _fails(R.check_guard, buf, v)
        R.check_guard(buf, v, written=99)
        v[99] = float("nan")                               # another NaN is a stored value, not the fill
        R.check_guard(buf, v)
        _fails(R.check_guard, buf, v, written=99)          # stored past what the kernel is to write


def test_debug_entry_validates_before_launching():
    from vae_training_amd import _lib
    lib = _lib.load()
    fields = [("rows", C.c_int32), ("n_in", C.c_int32), ("n_out", C.c_int32), ("relu", C.c_int32), ("accumulate", C.c_int32),
              ("S", C.c_int32), ("rows_per_split", C.c_int32), ("form", C.c_int32)] + \
             [(n, C.c_void_p) for n in ("x", "w", "b", "dy", "x_post", "z1", "lv", "xdata", "z2", "eps_param")] + \
             [("eps_cli", C.c_float), ("inv_bt", C.c_float)] + [(n, C.c_void_p) for n in ("out", "out2", "dwb", "scratch")] + \
             [("scratch_bytes", C.c_int64)]
    Args = type("Args", (C.Structure,), {"_fields_": fields})
    fn = lib.vaek_debug_dense16
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Args), C.c_void_p]
    p = 4096          # a non-null address nothing reads: every call below stops before a launch
    hs_fwd, hs_dw, sk_last_bwd, fwd_out16 = 4, 6, 12, 14
    for op, kw in [(hs_fwd, dict(rows=64, n_in=200, n_out=256)), (hs_dw, dict(rows=200, n_in=256, n_out=256, S=4, rows_per_split=50)),
                   (sk_last_bwd, dict(rows=64, n_in=512, n_out=17, S=1)), (fwd_out16, dict(rows=64, n_in=6, n_out=512)),
                   (99, dict(rows=64, n_in=64, n_out=64))]:
        a = Args(x=p, w=p, b=p, dy=p, x_post=p, out=p, dwb=p, **kw)
        assert fn(None, op, C.byref(a), None) == -1, (op, kw)
    a = Args(rows=64, n_in=256, n_out=256, x=p, w=p, b=p, out=p)
    assert fn(None, hs_fwd, C.byref(a), None) == 0 and a.scratch_bytes >= 2 * 256 * 256 * 2
    a.scratch, a.scratch_bytes = 256 * p, 64
    assert fn(None, hs_fwd, C.byref(a), None) == -4
    # the f32_* ops (tests/test_gpu_dense32.py), appended behind the existing ones
    dense_fwd_bf16, f32_fwd, f32_fwd_reparam, f32_fwd_elbo, f32_dx, f32_dw = 0, 22, 23, 24, 25, 26
    every = dict(x=p, w=p, b=p, dy=p, x_post=p, z1=p, lv=p, xdata=p, z2=p, out=p, out2=p, dwb=p)
    shape = dict(rows=200, n_in=33, n_out=231)
    # a layer the bf16 kind does not take is refused there and accepted here, at any width
    assert fn(None, dense_fwd_bf16, C.byref(Args(**every, **shape)), None) == -1
    for op, kw in [(f32_fwd, dict(relu=1)), (f32_fwd_reparam, {}), (f32_fwd_elbo, {}), (f32_dx, dict(relu=1, accumulate=1)),
                   (f32_dw, dict(S=4, rows_per_split=64))]:
        a = Args(**every, **shape, **kw)
        assert fn(None, op, C.byref(a), None) == 0 and a.scratch_bytes >= 0 and a.form == -1, (op, kw)
    for op, kw in [(f32_fwd_reparam, dict(relu=1)), (f32_fwd_elbo, dict(relu=1)), (f32_fwd, dict(accumulate=1)),
                   (f32_dw, dict(accumulate=1, S=4, rows_per_split=64)), (f32_dw, dict(S=4, rows_per_split=50)),
                   (f32_dw, dict(S=0, rows_per_split=64)), (f32_dw, dict(S=3, rows_per_split=64)), (f32_dw, dict(S=5, rows_per_split=64)),
                   (f32_dw, dict(S=2, rows_per_split=128 + 32)), (27, {})]:
        assert fn(None, op, C.byref(Args(**every, **shape, **kw)), None) == -1, (op, kw)
    a = Args(**every, **shape)
    a.xdata = None
    assert fn(None, f32_fwd_elbo, C.byref(a), None) == -1
    # scratch: S slabs at the 64-float pitch for dW|db; one {mse, d eps} pair per 32 x 32 block for the ELBO epilogue
    a = Args(**every, **shape, S=4, rows_per_split=64)
    assert fn(None, f32_dw, C.byref(a), None) == 0 and a.scratch_bytes >= 4 * 34 * 231 * 4
    a.scratch, a.scratch_bytes = 256 * p, 64
    assert fn(None, f32_dw, C.byref(a), None) == -4
    a = Args(**every, **shape)
    assert fn(None, f32_fwd_elbo, C.byref(a), None) == 0 and a.scratch_bytes >= 2 * 7 * 8 * 4
