"""-m gpu: every Dense launcher of dtype = VAEK_BF16, one call at a time, against a float64 reference that rounds where the kernel
rounds (tests/dense16_ref.py).  The calls go through vaek_debug_dense16 (csrc/debug_dense16.hip): the train step's own launchers,
weights through the step's prep kernels, dW|db slabs summed into the flat-gradient layout.  Shapes are the ones tiled kernels get
wrong: 1, 15-17, 127-129, 2 049 and 4 097 rows, widths of 64, 192, 512 (128- and 256-wide tiles) and 2 048, 200 and 257 off the
64 grid for gemm_bf16.hip, skinny d of 1, 6-9 and 16, both forms of the skinny backward kernels, ragged batch splits."""
import ctypes as C
import json
import os
import zlib

import pytest
import torch

from tests import dense16_ref as R
from tests.gpu_util import engine_for
from oracle import elbo_oracle as O

pytestmark = pytest.mark.gpu

OPS = ["dense_fwd_bf16", "dense_fwd_reparam_bf16", "dense_dx_bf16", "dense_dw_bf16",
       "hs_fwd", "hs_dx", "hs_dw",
       "sk_first_fwd", "sk_last_fwd", "sk_last_fwd_reparam", "sk_last_fwd_elbo", "sk_first_dx", "sk_last_bwd", "sk_first_bwd",
       "fwd_out16", "fwd_in16", "fwd_reparam_in16", "fwd_elbo_in16", "dx_out16", "dx_in16", "dw_x16", "dw_dy16",
       "f32_fwd", "f32_fwd_reparam", "f32_fwd_elbo", "f32_dx", "f32_dw"]          # the f32_* ops: tests/test_gpu_dense32.py
OP = {n: i for i, n in enumerate(OPS)}
# the profiler label each op's main kernel carries (gemm_f32.hip names its tile shape, not its storage types)
LABEL = {"dense_fwd_bf16": "gemm_bf16_fwd", "dense_fwd_reparam_bf16": "gemm_bf16_fwd_reparam", "dense_dx_bf16": "gemm_bf16_dx",
         "dense_dw_bf16": "gemm_bf16_dw", "hs_fwd": "gemm_bf16s_fwd", "hs_dx": "gemm_bf16s_dx", "hs_dw": "gemm_bf16s_dw",
         "sk_first_fwd": "sk16_first_fwd", "sk_last_fwd": "sk16_last_fwd", "sk_last_fwd_reparam": "sk16_last_fwd_reparam",
         "sk_last_fwd_elbo": "sk16_last_fwd_elbo", "sk_first_dx": "sk16_first_dx", "sk_last_bwd": "sk16_last_bwd",
         "sk_first_bwd": "sk16_first_bwd", "fwd_out16": "gemm_f32_fwd", "fwd_in16": "gemm_f32_fwd",
         "fwd_reparam_in16": "gemm_f32_fwd_reparam", "fwd_elbo_in16": "gemm_f32_fwd_elbo", "dx_out16": "gemm_f32_dx",
         "dx_in16": "gemm_f32_dx", "dw_x16": "gemm_f32_dw", "dw_dy16": "gemm_f32_dw"}
# every kernel label the calls of this file hold to the reference: the main kernels, the weight prep and the slab reductions
COVERED = set(LABEL.values()) | {"cvt_weights_bf16", "sk16_prep", "sk16_partials_reduce", "sum_slabs"}
# what else a dtype = bf16 step runs: the elementwise ELBO / reparameterisation passes and the finalisation (per call and per output:
# tests/test_gpu_elbo_tail.py; whole models: tests/test_gpu_bf16.py), and the all-f32 kernels of f32-storage layers whose plain label is not already in COVERED (per call
# and per element: tests/test_gpu_dense32.py)
NOT_DENSE16 = {"elbo", "elbo_reduce", "reparam_bwd", "finalize", "bulk_finalize", "gemm_f32_fwd_reparam_ts", "gemm_f32_dx_ts",
               "gemm_f32_fwd_128x128", "gemm_f32_dx_128x128", "gemm_f32_dw_128x128"}

ROWS = [1, 15, 16, 17, 127, 128, 129, 2049, 4097]
BIG = 65536          # the one C3-height case per op family


class Args(C.Structure):
    _fields_ = [("rows", C.c_int32), ("n_in", C.c_int32), ("n_out", C.c_int32), ("relu", C.c_int32), ("accumulate", C.c_int32),
                ("S", C.c_int32), ("rows_per_split", C.c_int32), ("form", C.c_int32),
                ("x", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p), ("dy", C.c_void_p), ("x_post", C.c_void_p),
                ("z1", C.c_void_p), ("lv", C.c_void_p), ("xdata", C.c_void_p), ("z2", C.c_void_p), ("eps_param", C.c_void_p),
                ("eps_cli", C.c_float), ("inv_bt", C.c_float),
                ("out", C.c_void_p), ("out2", C.c_void_p), ("dwb", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


RATIOS = {}          # op family -> largest error-to-bound ratio seen (written to $VAEK_DENSE16_RATIOS if set); the f32 families of
                     # tests/test_gpu_dense32.py land in the same dictionary and the same file


def family(op):
    return ("gemm_bf16" if op.startswith("dense_") else "gemm_bf16s" if op.startswith("hs_") else
            "sk_last_bwd" if op == "sk_last_bwd" else "sk_first_bwd" if op == "sk_first_bwd" else
            "skinny16" if op.startswith("sk_") else "gemm_f32 bf16 forms")


def note(op, ratio):
    f = family(op)
    RATIOS[f] = max(RATIOS.get(f, 0.0), ratio)


def dump_ratios():
    path = os.environ.get("VAEK_DENSE16_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    dump_ratios()


# gemm_f32.hip's launch(): the output tile of an M x N product over K in `splits` batch splits (the 128 x 128 shape exists for the
# all-f32 instantiations only)
TILE_DIMS = {"128x32": (128, 32), "32x128": (32, 128), "128x128": (128, 128), "64x64": (64, 64)}


def f32_tile(M, N, K, splits=1, all_f32=True):
    if N <= 32:
        return "128x32"
    if M <= 32:
        return "32x128"
    if all_f32 and min(M, N, K) >= 128 and ((M + 127) // 128) * ((N + 127) // 128) * splits >= 512:
        return "128x128"
    return "64x64"


def elbo_parts(rows, n_out):
    """The caller's buffer for the {mse, d eps} tile pairs of an ELBO op (all NaN), as vaek_dense16_args::out2 sizes it."""
    return torch.full((2 * ((rows + 31) // 32) * ((n_out + 31) // 32),), float("nan"), device="cuda")


def check_parts(parts, tiles, ref, mag, xdata, z2, eps, what):
    """The first 2 * tiles floats were written, nothing behind them; their totals against the float64 sums."""
    assert not torch.isnan(parts[:2 * tiles]).any() and torch.isnan(parts[2 * tiles:]).all(), what
    sums, bounds = R.elbo_sums(ref, mag, xdata, z2, eps)
    RATIOS["elbo sums bf16 forms"] = max(RATIOS.get("elbo sums bf16 forms", 0.0), R.check_sums(parts[:2 * tiles], sums, bounds, what=what))


@pytest.fixture(scope="module")
def eng():
    cfg = O.Config(6, 6, (64, 64), (64, 64), -3.0, True, "sphere")
    e = engine_for(cfg, 64, dtype="bf16")
    fn = e.lib.vaek_debug_dense16
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Args), C.c_void_p]
    return e


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return t.data_ptr()


def run(eng, op, rows, n_in, n_out, relu=0, accumulate=0, S=0, rps=0, eps_cli=0.0, inv_bt=0.0, **t):
    """One vaek_debug_dense16 call; returns (form, profiler labels)."""
    a = Args(rows=rows, n_in=n_in, n_out=n_out, relu=relu, accumulate=accumulate, S=S, rows_per_split=rps, eps_cli=eps_cli,
             inv_bt=inv_bt)
    for k, v in t.items():
        setattr(a, k, _p(v))
    lib = eng.lib
    assert lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), None) == 0, lib.vaek_last_error()
    scratch = torch.empty(max(a.scratch_bytes, 256), dtype=torch.uint8, device="cuda")
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel()
    eng.profile_begin(16)
    rc = lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rep = eng.profile_report()
    assert rc == 0, lib.vaek_last_error()
    assert LABEL[op] in rep, (op, sorted(rep))
    assert set(rep) <= COVERED, (op, sorted(rep))
    return a.form, rep


_gen = []          # the module's generator, made on first use (collection must not need a GPU)


def seed(*key):
    if not _gen:
        _gen.append(torch.Generator(device="cuda"))
    _gen[0].manual_seed(zlib.crc32(repr(key).encode()))


def randn(*shape, scale=1.0):
    return torch.randn(*shape, generator=_gen[0], device="cuda", dtype=torch.float32) * scale


def layer(n_in, n_out):
    return randn(n_in, n_out, scale=n_in ** -0.5), randn(n_out, scale=0.3)


def act16(rows, n):
    """A relu'd bf16 activation, about a third of it exact zeros."""
    return torch.relu(randn(rows, n) + 0.4).to(torch.bfloat16)


def splits(rows, mode):
    """(S, rows_per_split): one split, or 64-row multiples with a short last split where rows allow."""
    if mode == "one":
        rps = (rows + 63) // 64 * 64
    else:
        rps = max(64, ((rows + 2) // 3 + 63) // 64 * 64)
    return (rows + rps - 1) // rps, rps


# ---- gemm_bf16.hip: f32 storage, operands rounded to bf16 when staged ---------------------------------------------------------
GB_SHAPES = [(r, 200, 257) for r in ROWS] + [(129, a, b) for a, b in ((64, 64), (192, 512), (512, 512), (2048, 512), (512, 2048),
                                                                      (257, 200))] + [(BIG, 512, 512)]


@pytest.mark.parametrize("rows,n_in,n_out", GB_SHAPES)
def test_gemm_bf16_forward(eng, rows, n_in, n_out):
    seed("gbf", rows, n_in, n_out)
    x = randn(rows, n_in)
    w, b = layer(n_in, n_out)
    for relu in (0, 1):
        y = torch.full((rows, n_out), float("nan"), device="cuda")
        run(eng, "dense_fwd_bf16", rows, n_in, n_out, relu=relu, x=x, w=w, b=b, out=y)
        ref, mag, zero = R.forward(x, w, b, relu=bool(relu), round_x=True, round_w=True)
        note("dense_fwd_bf16", R.check_f32(y, ref, mag, zero=zero, what=f"gemm_bf16_fwd relu={relu}"))
    z1, lv = randn(rows, n_out), randn(n_out, scale=0.5)
    mu, smp = (torch.full((rows, n_out), float("nan"), device="cuda") for _ in range(2))
    run(eng, "dense_fwd_reparam_bf16", rows, n_in, n_out, x=x, w=w, b=b, z1=z1, lv=lv, out=mu, out2=smp)
    ref, mag, _ = R.forward(x, w, b, round_x=True, round_w=True)
    note("dense_fwd_bf16", R.check_f32(mu, ref, mag, what="gemm_bf16_fwd_reparam mu"))
    rs, ms = R.reparam(ref, mag, z1, lv)
    note("dense_fwd_bf16", R.check_f32(smp, rs, ms, what="gemm_bf16_fwd_reparam samples"))


@pytest.mark.parametrize("rows,n_in,n_out", GB_SHAPES)
def test_gemm_bf16_dx(eng, rows, n_in, n_out):
    seed("gbdx", rows, n_in, n_out)
    dy = randn(rows, n_out)
    w, _ = layer(n_in, n_out)
    x_post = torch.relu(randn(rows, n_in))
    acc0 = randn(rows, n_in)
    # (relu, x_post given, accumulate): the step's hidden dX, its first-layer dX, and relu set without a mask source
    for relu, with_mask, acc in ((1, True, 0), (0, False, 1), (1, False, 0), (1, True, 1)):
        dx = acc0.clone() if acc else torch.full((rows, n_in), float("nan"), device="cuda")
        run(eng, "dense_dx_bf16", rows, n_in, n_out, relu=relu, accumulate=acc, dy=dy, w=w, x_post=x_post if with_mask else None,
            out=dx)
        ref, mag, zero = R.backward_dx(dy, w, x_post if (relu and with_mask) else None, acc0 if acc else None,
                                       round_dy=True, round_w=True)
        note("dense_dx_bf16", R.check_f32(dx, ref, mag, zero=zero, what=f"gemm_bf16_dx relu={relu} mask={with_mask} acc={acc}"))


@pytest.mark.parametrize("mode", ["one", "many"])
@pytest.mark.parametrize("rows,n_in,n_out", GB_SHAPES)
def test_gemm_bf16_dw(eng, rows, n_in, n_out, mode):
    seed("gbdw", rows, n_in, n_out, mode)
    x, dy = torch.relu(randn(rows, n_in)), randn(rows, n_out)
    S, rps = splits(rows, mode)
    dwb = torch.full(((n_in + 1), n_out), float("nan"), device="cuda")
    run(eng, "dense_dw_bf16", rows, n_in, n_out, S=S, rps=rps, x=x, dy=dy, dwb=dwb)
    ref, mag = R.backward_dw(x, dy, round_x=True, round_dy=True)
    note("dense_dw_bf16", R.check_f32(dwb, ref, mag, what=f"gemm_bf16_dw S={S}"))


# ---- gemm_bf16s.hip: bf16 storage ---------------------------------------------------------------------------------------------
HS_SHAPES = [(r, 192, 512) for r in ROWS] + [(129, a, b) for a, b in ((64, 64), (512, 192), (512, 512), (2048, 512), (512, 2048),
                                                                      (64, 2048))] + [(BIG, 512, 512)]


def hs_forward_check(eng, rows, n_in, n_out, relu, what):
    x = act16(rows, n_in)
    w, b = layer(n_in, n_out)
    y = torch.full((rows, n_out), float("nan"), device="cuda").to(torch.bfloat16)
    run(eng, "hs_fwd", rows, n_in, n_out, relu=relu, x=x, w=w, b=b, out=y)
    ref, mag, zero = R.forward(x, w, b, relu=bool(relu), round_w=True)
    note("hs_fwd", R.check_bf16(y, ref, mag, zero=zero, what=what))


def hs_dx_check(eng, rows, n_in, n_out, what):
    dy = randn(rows, n_out).to(torch.bfloat16)
    w, _ = layer(n_in, n_out)
    x_post = act16(rows, n_in)
    dx = torch.full((rows, n_in), float("nan"), device="cuda").to(torch.bfloat16)
    run(eng, "hs_dx", rows, n_in, n_out, dy=dy, w=w, x_post=x_post, out=dx)
    ref, mag, zero = R.backward_dx(dy, w, x_post, round_w=True)
    note("hs_dx", R.check_bf16(dx, ref, mag, zero=zero, what=what))


def hs_dw_check(eng, rows, n_in, n_out, S, rps, what):
    x, dy = act16(rows, n_in), randn(rows, n_out).to(torch.bfloat16)
    dwb = torch.full(((n_in + 1), n_out), float("nan"), device="cuda")
    run(eng, "hs_dw", rows, n_in, n_out, S=S, rps=rps, x=x, dy=dy, dwb=dwb)
    ref, mag = R.backward_dw(x, dy)
    note("hs_dw", R.check_f32(dwb, ref, mag, what=what))


@pytest.mark.parametrize("rows,n_in,n_out", HS_SHAPES)
def test_hs_forward_and_dx(eng, rows, n_in, n_out):
    seed("hs", rows, n_in, n_out)
    for relu in (0, 1):
        hs_forward_check(eng, rows, n_in, n_out, relu, f"gemm_bf16s_fwd relu={relu}")
    hs_dx_check(eng, rows, n_in, n_out, "gemm_bf16s_dx")


@pytest.mark.parametrize("mode", ["one", "many"])
@pytest.mark.parametrize("rows,n_in,n_out", HS_SHAPES)
def test_hs_dw(eng, rows, n_in, n_out, mode):
    seed("hsdw", rows, n_in, n_out, mode)
    S, rps = splits(rows, mode)
    hs_dw_check(eng, rows, n_in, n_out, S, rps, f"gemm_bf16s_dw S={S} rows_per_split={rps}")


def test_hs_every_variant_against_reference(eng):
    """Each NT (forward, dX) and TN (dW|db) tile / ring variant at one ragged shape, against the reference itself."""
    lib = eng.lib
    n_nt, n_tn = C.c_int(), C.c_int()
    assert lib.vaek_debug_hs_variant(-1, -1, C.byref(n_nt), C.byref(n_tn)) == 0
    rows, n_in, n_out = 1000, 256, 512
    try:
        for nt in range(n_nt.value):
            assert lib.vaek_debug_hs_variant(nt, -1, None, None) == 0
            seed("nt", nt)
            hs_forward_check(eng, rows, n_in, n_out, 1, f"gemm_bf16s_fwd NT variant {nt}")
            hs_dx_check(eng, rows, n_out, n_in, f"gemm_bf16s_dx NT variant {nt}")
        assert lib.vaek_debug_hs_variant(-2, -1, None, None) == 0
        for tn in range(n_tn.value):
            assert lib.vaek_debug_hs_variant(-1, tn, None, None) == 0
            seed("tn", tn)
            hs_dw_check(eng, rows, n_in, n_out, 4, 256, f"gemm_bf16s_dw TN variant {tn}")
    finally:
        lib.vaek_debug_hs_variant(-2, -2, None, None)


# ---- gemm_skinny16.hip: the skinny first / last layers of a bf16-storage stack (1 <= d <= 16) ----------------------------------
# (rows, d, H)
SK_SHAPES = ([(r, 7, 512) for r in ROWS] + [(129, d, 512) for d in (1, 6, 8, 9, 16)] + [(2049, 6, H) for H in (64, 192, 2048)] +
             [(BIG, 6, 512)])


@pytest.mark.parametrize("rows,d,H", SK_SHAPES)
def test_sk_first_fwd(eng, rows, d, H):
    seed("skff", rows, d, H)
    x = randn(rows, d)
    w, b = layer(d, H)
    for relu in (0, 1):
        y = torch.full((rows, H), float("nan"), device="cuda").to(torch.bfloat16)
        run(eng, "sk_first_fwd", rows, d, H, relu=relu, x=x, w=w, b=b, out=y)
        ref, mag, zero = R.forward(x, w, b, relu=bool(relu))
        note("sk_first_fwd", R.check_bf16(y, ref, mag, zero=zero, what=f"sk16_first_fwd relu={relu}"))


@pytest.mark.parametrize("rows,d,H", SK_SHAPES)
def test_sk_last_fwd(eng, rows, d, H):
    seed("sklf", rows, d, H)
    h = act16(rows, H)
    w, b = layer(H, d)
    y = torch.full((rows, d), float("nan"), device="cuda")
    run(eng, "sk_last_fwd", rows, H, d, x=h, w=w, b=b, out=y)
    ref, mag, _ = R.forward(h, w, b, round_w=True)
    note("sk_last_fwd", R.check_f32(y, ref, mag, what="sk16_last_fwd"))
    z1, lv = randn(rows, d), randn(d, scale=0.5)
    mu, smp = (torch.full((rows, d), float("nan"), device="cuda") for _ in range(2))
    run(eng, "sk_last_fwd_reparam", rows, H, d, x=h, w=w, b=b, z1=z1, lv=lv, out=mu, out2=smp)
    note("sk_last_fwd", R.check_f32(mu, ref, mag, what="sk16_last_fwd_reparam mu"))
    rs, ms = R.reparam(ref, mag, z1, lv)
    note("sk_last_fwd", R.check_f32(smp, rs, ms, what="sk16_last_fwd_reparam samples"))
    # ELBO epilogue: d_out = dL/dx_hat element by element, and its {mse, d eps} tile sums (they feed the loss)
    xd, z2 = randn(rows, d), randn(rows, d)
    epsp = torch.tensor([0.75], device="cuda")
    eps = float(torch.tensor(0.75, dtype=torch.float32) * torch.tensor(-3.0, dtype=torch.float32))
    inv_bt = float(torch.tensor(1.0 / 3000.0, dtype=torch.float32))
    dout = torch.full((rows, d), float("nan"), device="cuda")
    parts = elbo_parts(rows, d)
    run(eng, "sk_last_fwd_elbo", rows, H, d, x=h, w=w, b=b, xdata=xd, z2=z2, eps_param=epsp, eps_cli=-3.0, inv_bt=inv_bt, out=dout,
        out2=parts)
    re, me = R.elbo(ref, mag, xd, z2, eps, inv_bt)
    note("sk_last_fwd", R.check_f32(dout, re, me, what="sk16_last_fwd_elbo d_out"))
    check_parts(parts, (rows + 127) // 128, ref, mag, xd, z2, eps, "sk16_last_fwd_elbo tile sums")      # one pair per 128 rows


@pytest.mark.parametrize("rows,d,H", SK_SHAPES)
def test_sk_first_dx(eng, rows, d, H):
    seed("skdx", rows, d, H)
    dy = randn(rows, H).to(torch.bfloat16)
    w, _ = layer(d, H)
    acc0 = randn(rows, d)
    for acc in (0, 1):
        dx = acc0.clone() if acc else torch.full((rows, d), float("nan"), device="cuda")
        run(eng, "sk_first_dx", rows, d, H, accumulate=acc, dy=dy, w=w, out=dx)
        ref, mag, _ = R.backward_dx(dy, w, acc=acc0 if acc else None, round_w=True)
        note("sk_first_dx", R.check_f32(dx, ref, mag, what=f"sk16_first_dx acc={acc}"))


# (rows, d, H, S, form): the matrix-core form needs H = 512, d <= 8 and rows_per_wg = ceil(rows / (64 S)) a multiple of 16
SK_BWD = ([(r, 7, 512, 1, "lane") for r in ROWS] + [(129, d, 512, 1, "lane") for d in (1, 6, 8, 9, 16)] +
          [(2049, 6, H, 2, "lane") for H in (64, 192, 2048)] +
          [(4096, d, 512, 1, "mfma") for d in (1, 6, 7, 8)] + [(2048, 8, 512, 2, "mfma"), (3072, 6, 512, 3, "mfma")] +
          [(4096, 9, 512, 1, "lane"), (4096, 8, 256, 1, "lane"), (4097, 8, 512, 1, "lane"), (1280, 6, 512, 4, "lane")] +
          [(100, 6, 512, 2, "lane"), (700, 16, 192, 8, "lane")] +            # S * 64 workgroups outnumber the rows
          # the matrix-core form at a ragged tail: the last rows' workgroup ends in a partial 16-row block (1000: 8 rows, 1002: 10,
          # 1004: 12, 2040: 8) or has only some of its blocks (2000: one of two), and the workgroups behind it are empty
          [(1000, 8, 512, 1, "mfma"), (1002, 6, 512, 1, "mfma"), (1004, 7, 512, 1, "mfma"), (2000, 6, 512, 1, "mfma"),
           (2040, 6, 512, 2, "mfma"), (1000, 1, 512, 1, "mfma")] +
          [(BIG, 6, 512, 8, "mfma")])
# The matrix-core form once read the tail of dy / x through one 16-byte piece clamped to the tensor's last 16 bytes: with
# rows * d not a multiple of 4 the last rows of a workgroup saw shifted values.  Those shapes run the per-lane form now.
SK_BWD_NAMED = [pytest.param(1001, 7, 512, 1, "lane", id="mfma_tail_rows_times_d_not_multiple_of_4"),
                pytest.param(4093, 6, 512, 1, "lane", id="mfma_tail_odd_rows_d6")]


@pytest.mark.parametrize("rows,d,H,S,form", SK_BWD + SK_BWD_NAMED)
def test_sk_last_bwd(eng, rows, d, H, S, form):
    seed("sklb", rows, d, H, S)
    h = act16(rows, H)
    dy = randn(rows, d)
    w, _ = layer(H, d)
    dh = torch.full((rows, H), float("nan"), device="cuda").to(torch.bfloat16)
    dwb = torch.full(((H + 1), d), float("nan"), device="cuda")
    got_form, _ = run(eng, "sk_last_bwd", rows, H, d, S=S, x=h, dy=dy, w=w, out=dh, dwb=dwb)
    ref, mag, zero = R.backward_dx(dy, w, h)
    note("sk_last_bwd", R.check_bf16(dh, ref, mag, zero=zero, what=f"sk16_last_bwd dh (form {got_form})"))
    ref, mag = R.backward_dw(h, dy)
    note("sk_last_bwd", R.check_f32(dwb, ref, mag, what=f"sk16_last_bwd dW|db (form {got_form}, S={S})"))
    assert got_form == (1 if form == "mfma" else 0), (got_form, form)


@pytest.mark.parametrize("rows,d,H,S,form", SK_BWD + SK_BWD_NAMED)
def test_sk_first_bwd(eng, rows, d, H, S, form):
    seed("skfb", rows, d, H, S)
    x = randn(rows, d)
    dy = randn(rows, H).to(torch.bfloat16)
    dwb = torch.full(((d + 1), H), float("nan"), device="cuda")
    w, _ = layer(d, H)
    got_form, _ = run(eng, "sk_first_bwd", rows, d, H, S=S, x=x, dy=dy, w=w, dwb=dwb)
    ref, mag = R.backward_dw(x, dy)
    note("sk_first_bwd", R.check_f32(dwb, ref, mag, what=f"sk16_first_bwd dW|db (form {got_form}, S={S})"))
    assert got_form == (1 if form == "mfma" else 0), (got_form, form)


# ---- gemm_f32.hip: the first / last layer of a bf16-storage stack the skinny kernels do not take (d > 16) ----------------------
F16_SHAPES = [(r, 20, 512) for r in ROWS] + [(129, d, H) for d, H in ((17, 64), (20, 192), (32, 2048), (64, 512))] + [(BIG, 20, 512)]


@pytest.mark.parametrize("rows,d,H", F16_SHAPES)
def test_f32_out16_in16_forward(eng, rows, d, H):
    seed("f16f", rows, d, H)
    x = randn(rows, d)
    w0, b0 = layer(d, H)
    for relu in (0, 1):
        y = torch.full((rows, H), float("nan"), device="cuda").to(torch.bfloat16)
        run(eng, "fwd_out16", rows, d, H, relu=relu, x=x, w=w0, b=b0, out=y)
        ref, mag, zero = R.forward(x, w0, b0, relu=bool(relu))
        note("fwd_out16", R.check_bf16(y, ref, mag, zero=zero, what=f"dense_fwd_out16 relu={relu}"))
    h = act16(rows, H)
    w, b = layer(H, d)
    y = torch.full((rows, d), float("nan"), device="cuda")
    run(eng, "fwd_in16", rows, H, d, x=h, w=w, b=b, out=y)
    ref, mag, _ = R.forward(h, w, b)
    note("fwd_in16", R.check_f32(y, ref, mag, what="dense_fwd_in16"))
    z1, lv = randn(rows, d), randn(d, scale=0.5)
    mu, smp = (torch.full((rows, d), float("nan"), device="cuda") for _ in range(2))
    run(eng, "fwd_reparam_in16", rows, H, d, x=h, w=w, b=b, z1=z1, lv=lv, out=mu, out2=smp)
    note("fwd_in16", R.check_f32(mu, ref, mag, what="dense_fwd_reparam_in16 mu"))
    rs, ms = R.reparam(ref, mag, z1, lv)
    note("fwd_in16", R.check_f32(smp, rs, ms, what="dense_fwd_reparam_in16 samples"))
    xd, z2 = randn(rows, d), randn(rows, d)
    inv_bt = float(torch.tensor(1.0 / 777.0, dtype=torch.float32))
    dout = torch.full((rows, d), float("nan"), device="cuda")
    parts = elbo_parts(rows, d)
    run(eng, "fwd_elbo_in16", rows, H, d, x=h, w=w, b=b, xdata=xd, z2=z2, eps_cli=-2.0, inv_bt=inv_bt, out=dout, out2=parts)
    re, me = R.elbo(ref, mag, xd, z2, -2.0, inv_bt)
    note("fwd_in16", R.check_f32(dout, re, me, what="dense_fwd_elbo_in16 d_out"))
    bm, bn = TILE_DIMS[f32_tile(rows, d, H, all_f32=False)]
    check_parts(parts, ((rows + bm - 1) // bm) * ((d + bn - 1) // bn), ref, mag, xd, z2, -2.0, "dense_fwd_elbo_in16 tile sums")


@pytest.mark.parametrize("rows,d,H", F16_SHAPES)
def test_f32_dx16(eng, rows, d, H):
    seed("f16dx", rows, d, H)
    dy = randn(rows, d)
    w, _ = layer(H, d)
    x_post = act16(rows, H)
    old = randn(rows, H).to(torch.bfloat16)
    for acc in (0, 1):
        dx = old.clone() if acc else torch.full((rows, H), float("nan"), device="cuda").to(torch.bfloat16)
        run(eng, "dx_out16", rows, H, d, accumulate=acc, dy=dy, w=w, x_post=x_post, out=dx)
        ref, mag, zero = R.backward_dx(dy, w, x_post, old if acc else None)
        note("dx_out16", R.check_bf16(dx, ref, mag, zero=zero, what=f"dense_bwd_dx_out16 acc={acc}"))
    dyh = randn(rows, H).to(torch.bfloat16)
    w0, _ = layer(d, H)
    acc0 = randn(rows, d)
    for acc in (0, 1):
        dx = acc0.clone() if acc else torch.full((rows, d), float("nan"), device="cuda")
        run(eng, "dx_in16", rows, d, H, accumulate=acc, dy=dyh, w=w0, out=dx)
        ref, mag, _ = R.backward_dx(dyh, w0, acc=acc0 if acc else None)
        note("dx_in16", R.check_f32(dx, ref, mag, what=f"dense_bwd_dx_in16 acc={acc}"))


@pytest.mark.parametrize("mode", ["one", "many"])
@pytest.mark.parametrize("rows,d,H", F16_SHAPES)
def test_f32_dw16(eng, rows, d, H, mode):
    seed("f16dw", rows, d, H, mode)
    S, rps = splits(rows, mode)
    h, dy = act16(rows, H), randn(rows, d)
    dwb = torch.full(((H + 1), d), float("nan"), device="cuda")
    run(eng, "dw_x16", rows, H, d, S=S, rps=rps, x=h, dy=dy, dwb=dwb)
    ref, mag = R.backward_dw(h, dy)
    note("dw_x16", R.check_f32(dwb, ref, mag, what=f"dense_bwd_dw_x16 S={S}"))
    x, dyh = randn(rows, d), randn(rows, H).to(torch.bfloat16)
    dwb = torch.full(((d + 1), H), float("nan"), device="cuda")
    run(eng, "dw_dy16", rows, d, H, S=S, rps=rps, x=x, dy=dyh, dwb=dwb)
    ref, mag = R.backward_dw(x, dyh)
    note("dw_dy16", R.check_f32(dwb, ref, mag, what=f"dense_bwd_dw_dy16 S={S}"))


# ---- refusals: shapes the step never sends are refused before anything launches ----------------------------------------------
def test_out_of_predicate_shapes_are_refused(eng):
    lib = eng.lib
    cases = [("hs_fwd", dict(rows=64, n_in=200, n_out=256)),                  # hidden width off the 64 grid
             ("hs_dw", dict(rows=200, n_in=256, n_out=256, S=4, rows_per_split=50)),     # split not a multiple of 64
             ("hs_dw", dict(rows=200, n_in=256, n_out=256, S=1, rows_per_split=128)),    # S != ceil(rows / rows_per_split)
             ("sk_last_bwd", dict(rows=64, n_in=512, n_out=17, S=1)),         # d > 16
             ("sk_first_fwd", dict(rows=64, n_in=6, n_out=4096)),             # H > 2048
             ("fwd_out16", dict(rows=64, n_in=6, n_out=512)),                 # the skinny kernels take this layer
             ("dense_fwd_bf16", dict(rows=64, n_in=32, n_out=512))]           # gemm_bf16 layers are >= 64 wide on both sides
    dummy = torch.zeros(16, device="cuda")
    for op, kw in cases:
        a = Args(**kw)
        for f in ("x", "w", "b", "dy", "x_post", "out", "dwb"):
            setattr(a, f, dummy.data_ptr())
        assert lib.vaek_debug_dense16(eng.h, OP[op], C.byref(a), None) == -1, (op, kw)
    a = Args(rows=64, n_in=256, n_out=256, x=dummy.data_ptr(), w=dummy.data_ptr(), b=dummy.data_ptr(), out=dummy.data_ptr())
    assert lib.vaek_debug_dense16(eng.h, OP["hs_fwd"], C.byref(a), None) == 0 and a.scratch_bytes > 0
    a.scratch, a.scratch_bytes = dummy.data_ptr(), 64                          # too small: refused, nothing launched
    assert lib.vaek_debug_dense16(eng.h, OP["hs_fwd"], C.byref(a), None) == -4


# ---- routing: every kernel a dtype = bf16 step runs is one this file holds to the reference (or listed as not a Dense kernel) ----
# test_gpu_bf16.py's models, C3's widths, and a first layer with d > 16 (the gemm_f32.hip bf16-stored forms)
ROUTING = ([(hidden, B, ds) for hidden, B in (((128,), 700), ((256, 128), 1000), ((192, 64, 192), 333), ((200, 200), 500),
                                              ((128, 128), 64 * 9 + 1), ((512, 512), 2048), ((512, 512), 2000))
            for ds in ("sphere", "sigmoid")] +
           [((512, 512, 512), 65536, "sphere"), ((512, 512, 512), 4096, "d20")])


@pytest.mark.parametrize("hidden,B,ds", ROUTING)
def test_bf16_step_kernels_are_all_covered(hidden, B, ds):
    D = {"sphere": 6, "sigmoid": 7, "d20": 20}[ds]
    cfg = O.Config(D, 6, hidden, hidden, -3.0, True, "sigmoid" if ds == "sigmoid" else "sphere")
    eng = engine_for(cfg, B, dtype="bf16")
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    params = torch.randn(eng.P, generator=g, device="cuda") * 0.05
    grads = eng.new_flat(eng.grad_len)
    x, z1, z2 = (torch.randn(B, n, generator=g, device="cuda") for n in (D, 6, D))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    eng.profile_begin(512)
    eng.grads_only(params, grads, step, x, z1, z2)
    torch.cuda.synchronize()
    labels = set(eng.profile_report())
    assert torch.isfinite(grads).all()
    print(f"{hidden} B={B} {ds}: {sorted(labels)}")
    assert labels <= COVERED | NOT_DENSE16, sorted(labels - COVERED - NOT_DENSE16)
    if hidden == (512, 512, 512) and ds == "sphere":       # C3: its whole bf16 Dense path is covered per call
        assert {"gemm_bf16s_fwd", "gemm_bf16s_dx", "gemm_bf16s_dw", "sk16_first_fwd", "sk16_last_bwd", "sk16_first_bwd"} <= labels
    if ds == "d20":                                         # the encoder's 20 -> 512 and the decoder's 512 -> 20 layers
        assert {"gemm_f32_fwd", "gemm_f32_fwd_elbo", "gemm_f32_dw"} <= labels
