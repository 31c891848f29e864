"""-m gpu: every all-f32 Dense kernel of gemm_f32.hip, one call at a time, element by element against the float64 reference of
tests/dense16_ref.py (no operand rounding; bound F32_TOL x the element's own magnitude).  The calls go through the f32_* ops of
vaek_debug_dense16 (csrc/debug_dense16.hip): the train step's own dense_fwd / dense_dx / dense_dw with Kind::F32.

What launch() (gemm_f32.hip) picks, with M x N the output and K the reduction (forward: rows x n_out over n_in; dX: rows x n_in over
n_out; dW|db: (n_in + 1) x n_out over rows, in S batch splits):
  N <= 32 -> 128 x 32 tiles (32-deep k-tiles, two in flight except for dW|db); else M <= 32 -> 32 x 128; else 128 x 128 when M, N,
  K >= 128 and tiles x splits >= 512; else 64 x 64 (16-deep k-tiles).
The reparameterisation forward and the unmasked dX take the streaming kernel (label *_ts) when N <= 32, K >= 1024, K % 128 == 0,
M >= 2048 and A (for dX also W) is 16-byte aligned.  Every case asserts the profiler label of the kernel it means to reach.

Each output lies between two guard bands of one NaN bit pattern (dense16_ref.guarded): a store outside the output, or an element
nobody stored, fails the case.  Inputs can start 1-3 floats off their buffer's alignment (the kernels' scalar fetch branch: a
layer's kernel sits at any float offset of the flat parameter vector)."""
import ctypes as C

import pytest
import torch

from tests import dense16_ref as R
from tests import test_gpu_dense16 as T16
from tests.gpu_util import engine_for
from oracle import elbo_oracle as O

pytestmark = pytest.mark.gpu

OP, Args, seed, randn, layer, splits, ROWS = T16.OP, T16.Args, T16.seed, T16.randn, T16.layer, T16.splits, T16.ROWS
f32_tile, TILE_DIMS = T16.f32_tile, T16.TILE_DIMS

# every label the calls of this file hold to the reference
DENSE32 = {"gemm_f32_fwd", "gemm_f32_fwd_128x128", "gemm_f32_fwd_reparam", "gemm_f32_fwd_reparam_ts", "gemm_f32_fwd_elbo",
           "gemm_f32_dx", "gemm_f32_dx_128x128", "gemm_f32_dx_ts", "gemm_f32_dw", "gemm_f32_dw_128x128", "sum_slabs"}
# what else a layer-by-layer f32 step runs: the elementwise ELBO / reparameterisation passes and the finalisation (per call and per
# output: tests/test_gpu_elbo_tail.py, which also runs these models with Adam, in eval and in forward)
NOT_DENSE32 = {"elbo", "elbo_reduce", "reparam_bwd", "finalize", "bulk_finalize"}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    T16.dump_ratios()


@pytest.fixture(scope="module")
def eng():
    cfg = O.Config(6, 6, (64, 64), (64, 64), -3.0, True, "sphere")
    e = engine_for(cfg, 64)
    fn = e.lib.vaek_debug_dense16
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Args), C.c_void_p]
    return e


def note(fam, ratio):
    T16.RATIOS[fam] = max(T16.RATIOS.get(fam, 0.0), ratio)


def call(eng, op, rows, n_in, n_out, expect, relu=0, accumulate=0, S=0, rps=0, eps_cli=0.0, inv_bt=0.0, **t):
    """One vaek_debug_dense16 call; the only main kernel it ran carries the label `expect`."""
    a = Args(rows=rows, n_in=n_in, n_out=n_out, relu=relu, accumulate=accumulate, S=S, rows_per_split=rps, eps_cli=eps_cli,
             inv_bt=inv_bt)
    for k, v in t.items():
        setattr(a, k, T16._p(v))
    lib = eng.lib
    assert lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), None) == 0, lib.vaek_last_error()
    scratch = torch.empty(max(a.scratch_bytes, 256), dtype=torch.uint8, device="cuda")
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    eng.profile_begin(16)
    rc = lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert rc == 0, lib.vaek_last_error()
    assert set(rep) - {"sum_slabs"} == {expect}, (op, rows, n_in, n_out, expect, sorted(rep))
    assert set(rep) <= DENSE32, (op, sorted(rep))


def shifted(t, off):
    """The same values in a view that starts `off` floats into a 16-byte aligned buffer."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 4 * off
    return v


def output(shape, lead=0, init=None):
    """A guarded output: (buffer, view of `shape`)."""
    n = 1
    for s in shape:
        n *= s
    buf, v = R.guarded(n, "cuda", lead)
    if init is not None:
        v.copy_(init.reshape(-1))
    return buf, v.view(shape)


def ts_ok(M, N, K, aligned):
    return N <= 32 and K >= 1024 and K % 128 == 0 and M >= 2048 and aligned


def big(tile):
    return "_128x128" if tile == "128x128" else ""


# ---- one case per op: inputs and reference made once, then one call per entry of `offs` (argument name -> float offset) ----------
NO_OFF = ({},)


def fwd_case(eng, rows, K, N, offs=NO_OFF, want_tile=None):
    seed("f32fwd", rows, K, N)
    x = randn(rows, K)
    w, b = layer(K, N)
    tile = f32_tile(rows, N, K)
    assert want_tile in (None, tile), (tile, want_tile)
    refs = [R.forward(x, w, b, relu=bool(relu)) for relu in (0, 1)]
    for off in offs:
        o = lambda k: off.get(k, 0)
        xs, ws, bs = shifted(x, o("x")), shifted(w, o("w")), shifted(b, o("b"))
        for relu in (0, 1):
            what = f"f32_fwd {rows}x{K}x{N} relu={relu} off={off}"
            buf, y = output((rows, N), o("out"))
            call(eng, "f32_fwd", rows, K, N, "gemm_f32_fwd" + big(tile), relu=relu, x=xs, w=ws, b=bs, out=y)
            R.check_guard(buf, y, what=what)
            ref, mag, zero = refs[relu]
            note(f"f32 {tile} fwd", R.check_f32(y, ref, mag, zero=zero, what=what))


def reparam_case(eng, rows, K, N, offs=NO_OFF, want_ts=None):
    seed("f32rp", rows, K, N)
    x = randn(rows, K)
    w, b = layer(K, N)
    z1, lv = randn(rows, N), randn(N, scale=0.5)
    tile = f32_tile(rows, N, K)
    ref, mag, _ = R.forward(x, w, b)
    rs, ms = R.reparam(ref, mag, z1, lv)
    for off in offs:
        o = lambda k: off.get(k, 0)
        ts = ts_ok(rows, N, K, o("x") == 0)
        assert want_ts in (None, ts), (rows, K, N, off)
        xs, ws, bs, zs, ls = shifted(x, o("x")), shifted(w, o("w")), shifted(b, o("b")), shifted(z1, o("z1")), shifted(lv, o("lv"))
        what = f"f32_fwd_reparam {rows}x{K}x{N} off={off} ts={ts}"
        outs = []
        for _ in range(2 if ts else 1):
            bm, mu = output((rows, N), o("out"))
            bs2, smp = output((rows, N), o("out2"))
            call(eng, "f32_fwd_reparam", rows, K, N, "gemm_f32_fwd_reparam" + ("_ts" if ts else ""), x=xs, w=ws, b=bs, z1=zs, lv=ls,
                 out=mu, out2=smp)
            R.check_guard(bm, mu, what=what + " mu")
            R.check_guard(bs2, smp, what=what + " samples")
            fam = "f32 ts fwd_reparam" if ts else f"f32 {tile} fwd_reparam"
            note(fam, R.check_f32(mu, ref, mag, what=what + " mu"))
            note(fam, R.check_f32(smp, rs, ms, what=what + " samples"))
            outs.append((mu, smp))
        if ts:      # fixed summation order: the same bits from two calls
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), what


def elbo_case(eng, rows, K, N, offs=NO_OFF):
    seed("f32elbo", rows, K, N)
    h = randn(rows, K)
    w, b = layer(K, N)
    xd, z2 = randn(rows, N), randn(rows, N)
    tile = f32_tile(rows, N, K)
    bm, bn = TILE_DIMS[tile]
    full = 2 * ((rows + 31) // 32) * ((N + 31) // 32)           # what the caller provides
    written = 2 * ((rows + bm - 1) // bm) * ((N + bn - 1) // bn)   # what this tile shape writes
    ref, mag, _ = R.forward(h, w, b)
    inv_bt = float(torch.tensor(1.0 / 777.0, dtype=torch.float32))
    epsp = torch.tensor([0.75], device="cuda")
    # eps = eps_param * eps_cli (one f32 product), and eps_cli alone
    variants = [(epsp, -3.0, float(torch.tensor(0.75, dtype=torch.float32) * torch.tensor(-3.0, dtype=torch.float32))),
                (None, -2.0, -2.0)]
    for ep, cli, eps in variants:
        re, me = R.elbo(ref, mag, xd, z2, eps, inv_bt)
        sums, bounds = R.elbo_sums(ref, mag, xd, z2, eps)
        for off in offs:
            o = lambda k: off.get(k, 0)
            what = f"f32_fwd_elbo {rows}x{K}x{N} eps={eps} off={off}"
            bd, dout = output((rows, N), o("out"))
            bp, parts = output((full,), 0)
            call(eng, "f32_fwd_elbo", rows, K, N, "gemm_f32_fwd_elbo", x=shifted(h, o("x")), w=shifted(w, o("w")), b=shifted(b, o("b")),
                 xdata=shifted(xd, o("xdata")), z2=shifted(z2, o("z2")), eps_param=ep, eps_cli=cli, inv_bt=inv_bt, out=dout, out2=parts)
            R.check_guard(bd, dout, what=what + " d_out")
            R.check_guard(bp, parts, written=written, what=what + " tile sums")
            note(f"f32 {tile} fwd_elbo", R.check_f32(dout, re, me, what=what + " d_out"))
            note("f32 elbo sums", R.check_sums(parts[:written], sums, bounds, what=what))


def dx_case(eng, rows, K, N, offs=NO_OFF, want_ts=None, variants=None, want_tile=None):
    """dX [rows, N] = dY [rows, K] W^T, W [n_in = N, n_out = K]."""
    seed("f32dx", rows, K, N)
    dy = randn(rows, K)
    w, _ = layer(N, K)
    x_post = torch.relu(randn(rows, N))
    acc0 = randn(rows, N)
    tile = f32_tile(rows, N, K)
    assert want_tile in (None, tile), (tile, want_tile)
    # (relu, x_post given, accumulate): the step's hidden dX, its first-layer dX plain and added, relu set without a mask source
    for relu, with_mask, acc in variants or ((1, True, 0), (0, False, 0), (0, False, 1), (1, False, 0), (1, True, 1)):
        masked = bool(relu and with_mask)
        ref, mag, zero = R.backward_dx(dy, w, x_post if masked else None, acc0 if acc else None)
        for off in offs:
            o = lambda k: off.get(k, 0)
            ts = not masked and ts_ok(rows, N, K, o("dy") == 0 and o("w") == 0)
            assert want_ts in (None, ts), (rows, K, N, off, masked)
            what = f"f32_dx {rows}x{K}x{N} relu={relu} mask={with_mask} acc={acc} off={off} ts={ts}"
            ds, ws, ps = shifted(dy, o("dy")), shifted(w, o("w")), shifted(x_post, o("x_post")) if with_mask else None
            outs = []
            for _ in range(2 if ts else 1):
                buf, dx = output((rows, N), o("out"), init=acc0 if acc else None)
                call(eng, "f32_dx", rows, N, K, "gemm_f32_dx" + ("_ts" if ts else big(tile)), relu=relu, accumulate=acc, dy=ds, w=ws,
                     x_post=ps, out=dx)
                R.check_guard(buf, dx, prefilled=bool(acc), what=what)
                note("f32 ts dx" if ts else f"f32 {tile} dx", R.check_f32(dx, ref, mag, zero=zero, what=what))
                outs.append(dx)
            if ts:
                assert torch.equal(outs[0], outs[1]), what


def dw_case(eng, n_in, n_out, rows, S, rps, offs=NO_OFF, want_tile=None):
    seed("f32dw", n_in, n_out, rows, S, rps)
    x, dy = randn(rows, n_in), randn(rows, n_out)
    tile = f32_tile(n_in + 1, n_out, rows, S)
    assert want_tile in (None, tile), (tile, want_tile)
    ref, mag = R.backward_dw(x, dy)
    for off in offs:
        o = lambda k: off.get(k, 0)
        what = f"f32_dw {n_in}->{n_out} rows={rows} S={S} rows_per_split={rps} off={off}"
        buf, dwb = output((n_in + 1, n_out))
        call(eng, "f32_dw", rows, n_in, n_out, "gemm_f32_dw" + big(tile), S=S, rps=rps, x=shifted(x, o("x")), dy=shifted(dy, o("dy")),
             dwb=dwb)
        R.check_guard(buf, dwb, what=what)
        note(f"f32 {tile} dw", R.check_f32(dwb, ref, mag, what=what))


# ---- shapes: (rows, K, N) = the GEMM's M, reduction and N for forward / dX; for dW|db a layer K -> N at `rows` --------------------
K_EDGES = [1, 31, 32, 33, 63, 64, 65, 97, 130, 2048]     # 128 x 32: zero, one and two sets of k-tiles in flight, ragged last k-tile
T128x32 = ([(r, 200, 20) for r in ROWS] + [(r, k, 20) for r in (129, 257) for k in K_EDGES] +
           [(r, 130, n) for r in (129, 257) for n in (1, 31, 32)])
T32x128 = [(r, 130, n) for r in (1, 31, 32, 33) for n in (33, 128, 129, 200)]      # rows = 33: the first on the 64 x 64 tile
GRID64 = [33, 63, 64, 65, 129, 200, 257]
T64x64 = ([(129, 130, n) for n in GRID64] + [(r, 130, 65) for r in GRID64 if r != 129] +
          [(129, k, 65) for k in (1, 15, 16, 17, 31, 33)])
T128x128 = [(16384, 128, 512), (16385, 160, 512), (21761, 130, 257), (65536, 128, 128)]
JUST_OUTSIDE = [(16256, 128, 512), (16385, 127, 512), (65536, 128, 127)]           # 508 tiles; K < 128; N < 128
TILED = T128x32 + T32x128 + T64x64


def _expect(rows, K, N):
    return ("128x128" if (rows, K, N) in T128x128 else "64x64" if (rows, K, N) in JUST_OUTSIDE else
            "128x32" if (rows, K, N) in T128x32 else None)


@pytest.mark.parametrize("rows,K,N", TILED + T128x128 + JUST_OUTSIDE)
def test_f32_forward(eng, rows, K, N):
    fwd_case(eng, rows, K, N, want_tile=_expect(rows, K, N))


@pytest.mark.parametrize("rows,K,N", TILED + T128x128[:2])
def test_f32_forward_reparam(eng, rows, K, N):
    reparam_case(eng, rows, K, N, want_ts=False)


@pytest.mark.parametrize("rows,K,N", TILED + [(4097, 64, 33), (257, 130, 257), (16385, 160, 512)])
def test_f32_forward_elbo(eng, rows, K, N):
    """dL/dx_hat element by element and the {mse, d eps} tile sums, rows and n_out off every tile grid."""
    elbo_case(eng, rows, K, N)


@pytest.mark.parametrize("rows,K,N", TILED + T128x128 + JUST_OUTSIDE)
def test_f32_dx(eng, rows, K, N):
    dx_case(eng, rows, K, N, want_ts=False, want_tile=_expect(rows, K, N))


# dW|db: M = n_in + 1.  (n_in, n_out, rows)
DW_128x32 = [(200, 20, r) for r in ROWS] + [(k, 20, r) for r in (129, 257) for k in K_EDGES] + [(130, n, r) for r in (129, 257)
                                                                                                for n in (1, 31, 32)]
DW_32x128 = [(a, b, 257) for a in (1, 6, 30, 31, 32) for b in (33, 64, 200, 512)]         # n_in = 32: the first on the 64 x 64 tile
DW_64x64 = [(m - 1, n, 130) for m in GRID64 for n in GRID64] + [(64, 65, r) for r in (1, 15, 16, 17, 31, 33)]


@pytest.mark.parametrize("mode", ["one", "many"])
@pytest.mark.parametrize("n_in,n_out,rows", DW_128x32 + DW_32x128 + DW_64x64)
def test_f32_dw(eng, n_in, n_out, rows, mode):
    S, rps = splits(rows, mode)
    want = "128x32" if n_out <= 32 else "32x128" if n_in + 1 <= 32 else "64x64"
    dw_case(eng, n_in, n_out, rows, S, rps, want_tile=want)


# (n_in, n_out, rows, S, rows_per_split): the last split of (512, 512, 1627) is 27 rows, shorter than one k-tile
@pytest.mark.parametrize("n_in,n_out,rows,S,rps,tile", [(127, 128, 32768, 512, 64, "128x128"), (128, 128, 16384, 256, 64, "128x128"),
                                                         (512, 512, 1627, 26, 64, "128x128"), (512, 512, 1600, 25, 64, "64x64")])
def test_f32_dw_128x128(eng, n_in, n_out, rows, S, rps, tile):
    dw_case(eng, n_in, n_out, rows, S, rps, want_tile=tile)


# the appended ones row [X | 1]^T: on each lane of a float4 unit (n_in % 4), alone in a tile row (n_in a multiple of the tile height)
@pytest.mark.parametrize("split", ["one", "many", "last_is_one_row"])
@pytest.mark.parametrize("rows", [129, 4097])
@pytest.mark.parametrize("n_in", [63, 64, 65, 66, 67, 127, 128, 129])
def test_f32_dw_ones_row(eng, n_in, rows, split):
    S, rps = splits(rows, split) if split != "last_is_one_row" else {129: (3, 64), 4097: (5, 1024)}[rows]
    if split == "last_is_one_row":
        assert rows - (S - 1) * rps == 1
    dw_case(eng, n_in, 65, rows, S, rps, want_tile="64x64")


# ---- the streaming form and its predicate: both sides of every condition against the same reference -----------------------------
TS = sorted({(m, 1152, 20) for m in (2048, 2049, 2079)} | {(2049, k, 20) for k in (1024, 1152, 4096)} |
            {(2049, 1152, n) for n in (1, 7, 20, 31, 32)})
NOT_TS = [(2047, 1152, 20), (2049, 896, 20), (2049, 1088, 20), (2049, 1152, 33)]


@pytest.mark.parametrize("rows,K,N", TS)
def test_f32_streaming_form(eng, rows, K, N):
    reparam_case(eng, rows, K, N, want_ts=True)
    dx_case(eng, rows, K, N, want_ts=True, variants=((0, False, 0), (0, False, 1), (1, False, 0)))


@pytest.mark.parametrize("rows,K,N", NOT_TS)
def test_f32_tiled_kernel_takes_over_outside_the_streaming_predicate(eng, rows, K, N):
    reparam_case(eng, rows, K, N, want_ts=False)
    dx_case(eng, rows, K, N, want_ts=False, variants=((0, False, 0), (0, False, 1)))


def test_f32_tiled_kernel_takes_over_for_unaligned_or_masked_operands(eng):
    rows, K, N = 2049, 1152, 20
    reparam_case(eng, rows, K, N, offs=({"x": 1},), want_ts=False)
    dx_case(eng, rows, K, N, offs=({"dy": 1}, {"w": 1}), want_ts=False, variants=((0, False, 0), (0, False, 1)))
    dx_case(eng, rows, K, N, want_ts=False, variants=((1, True, 0), (1, True, 1)))


# ---- alignment: each tensor in turn 1, 2 and 3 floats off, same reference, same bound -------------------------------------------
ALIGN_SHAPES = [(129, 130, 65), (129, 132, 20), (16385, 160, 512)]


def one_at_a_time(names, off):
    return tuple({n: off} for n in names)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("rows,K,N", ALIGN_SHAPES)
def test_f32_forward_unaligned(eng, rows, K, N, off):
    fwd_case(eng, rows, K, N, offs=one_at_a_time(("x", "w", "b", "out"), off))
    reparam_case(eng, rows, K, N, offs=one_at_a_time(("x", "w", "b", "z1", "lv", "out", "out2"), off))
    elbo_case(eng, rows, K, N, offs=one_at_a_time(("x", "w", "b", "xdata", "z2", "out"), off))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("rows,K,N", ALIGN_SHAPES)
def test_f32_dx_unaligned(eng, rows, K, N, off):
    dx_case(eng, rows, K, N, offs=one_at_a_time(("dy", "w", "x_post", "out"), off), variants=((1, True, 0), (0, False, 1)))


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("n_in,n_out,rows,S,rps", [(130, 65, 129, 3, 64), (132, 20, 129, 1, 192), (512, 512, 1627, 26, 64)])
def test_f32_dw_unaligned(eng, n_in, n_out, rows, S, rps, off):
    dw_case(eng, n_in, n_out, rows, S, rps, offs=one_at_a_time(("x", "dy"), off))


# ---- validation on the device side: the f32 ops refuse what their launch functions do not offer ---------------------------------
def test_f32_ops_refuse_bad_arguments(eng):
    lib = eng.lib
    dummy = torch.zeros(16, device="cuda")
    cases = [("f32_fwd_reparam", dict(rows=64, n_in=20, n_out=6, relu=1)),                    # no relu switch on an epilogue op
             ("f32_fwd", dict(rows=64, n_in=20, n_out=6, accumulate=1)),                       # forward does not accumulate
             ("f32_dw", dict(rows=200, n_in=20, n_out=6, S=4, rows_per_split=50)),             # split not a multiple of 64
             ("f32_dw", dict(rows=200, n_in=20, n_out=6, S=1, rows_per_split=128))]            # S != ceil(rows / rows_per_split)
    for op, kw in cases:
        a = Args(**kw)
        for f in ("x", "w", "b", "dy", "x_post", "z1", "lv", "out", "out2", "dwb"):
            setattr(a, f, dummy.data_ptr())
        assert lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), None) == -1, (op, kw)


# ---- routing: every kernel a layer-by-layer f32 step runs is one this file holds to the reference (or listed as not Dense) ------
# (hidden, B, D, L, dataset)
ROUTING = [((33,), 300, 6, 6, "sphere"), ((200, 200), 500, 6, 6, "sphere"), ((64, 48, 64, 32), 333, 6, 6, "sphere"),
           ((96,), 515, 7, 6, "sigmoid"), ((512, 512, 512), 65536, 6, 6, "sphere"), ((), 4096, 4096, 20, "linear_gaussian")]


@pytest.mark.parametrize("hidden,B,D,L,ds", ROUTING)
def test_f32_step_kernels_are_all_covered(hidden, B, D, L, ds):
    cfg = O.Config(D, L, hidden, hidden, -3.0, True, ds)
    eng = engine_for(cfg, B, force_generic=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    params = torch.randn(eng.P, generator=g, device="cuda") * 0.05
    grads = eng.new_flat(eng.grad_len)
    x, z1, z2 = (torch.randn(B, n, generator=g, device="cuda") for n in (D, L, D))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.profile_begin(512)
    eng.grads_only(params, grads, step, x, z1, z2)
    torch.cuda.synchronize()
    labels = set(eng.profile_report())
    assert torch.isfinite(grads).all()
    print(f"{hidden} B={B} D={D} L={L} {ds}: {sorted(labels)}")
    assert labels <= DENSE32 | NOT_DENSE32, sorted(labels - DENSE32 - NOT_DENSE32)
    if hidden == (512, 512, 512):
        assert {"gemm_f32_fwd_128x128", "gemm_f32_dx_128x128", "gemm_f32_dw_128x128"} <= labels, sorted(labels)
    if D == 4096:
        assert {"gemm_f32_fwd_reparam_ts", "gemm_f32_dx_ts"} <= labels, sorted(labels)
