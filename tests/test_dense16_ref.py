"""The comparison of tests/test_gpu_dense16.py has power: references with the bugs tiled kernels tend to have must FAIL it, while
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
