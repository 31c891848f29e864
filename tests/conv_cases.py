"""The convolution kernels' forms, the cases that pin each of them, and their references -- CPU only (NumPy and torch on the CPU).

Three things live here, shared by tests/test_conv_cases_host.py (no GPU), tests/test_gpu_conv_forms.py and tests/test_gpu_conv.py:

* the per-call REFERENCES: torch float64 with stride 2 / padding 1, the operands rounded to bf16 exactly where the form that runs
  rounds them (both operands in the bf16 GEMM forms, neither in the one-channel streaming forms, the one operand read from its
  bf16 copy in the lean streaming variants), then relu, then [mask > 0];
* form(): a plain restatement of the dispatch of vaek_conv2d_forward / _transpose_forward / _weight_grad (csrc/conv_bf16.hip),
  conv_fwd_fast / conv_wgrad_fast and launch_hs_conv / launch_hs_conv_dw (csrc/gemm_bf16s.hip): which kernel runs, how it tiles
  the problem, whether it decodes pixels by shifts or divisions.  The host test pins it to the library's workspace queries, the GPU
  test to the lean calls the library accepts and refuses;
* CASES: one entry per (form, edge), the smallest shape that reaches the edge, each with the reason it is there.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

BOUND_BF16 = 2e-6        # bf16 GEMM forms: same products, float32 accumulation in another order (test_conv_vae_loss_and_every_gradient_leaf)
BOUND_F32 = 1e-5         # streaming one-channel forms: the project's float32 contract


# ---- references ---------------------------------------------------------------------------------------------------------------
def rb(t):
    return t.to(torch.bfloat16).to(torch.float64)


def ident(t):
    return t


def nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def oihw(t):
    return t.double().cpu().permute(3, 2, 0, 1)


def rel(a, b):
    """max-abs difference of a from the reference b, in units of b's max-abs."""
    return float((a.double().cpu() - b).abs().max() / (b.abs().max() + 1e-30))


def finish(ref, relu, mask):
    ref = ref.permute(0, 2, 3, 1)
    ref = torch.relu(ref) if relu else ref
    return ref if mask is None else ref * (mask.cpu() > 0)


def streams(op, c_in, c_out):
    """Does a FLOAT32 call of this shape run in an exact-f32 streaming kernel (no operand is rounded)?  op: forward / transposed /
    kernel gradient."""
    if op == "transposed":
        return c_out == 1 and c_in % 4 == 0 and c_in <= 256
    return c_in == 1 and 256 % c_out == 0


def ref_forward(x, w, bias=None, relu=False, mask=None, round_x=True, round_w=True):
    """x [B, H, W, Cin], w [4, 4, Cin, Cout] -> [B, H/2, W/2, Cout], float64."""
    rx, rw = (rb if round_x else ident), (rb if round_w else ident)
    ref = F.conv2d(rx(nchw(x)), rw(oihw(w)), None if bias is None else bias.double().cpu(), stride=2, padding=1)
    return finish(ref, relu, mask)


def ref_transpose(y, w, bias=None, relu=False, mask=None, round_y=True, round_w=True):
    """y [B, h, w, Cin], w [4, 4, Cout, Cin] -> [B, 2 h, 2 w, Cout], float64."""
    ry, rw = (rb if round_y else ident), (rb if round_w else ident)
    ref = F.conv_transpose2d(ry(nchw(y)), rw(oihw(w)), None if bias is None else bias.double().cpu(), stride=2, padding=1)
    return finish(ref, relu, mask)


def ref_weight_grad(x, dy, round_x=True, round_dy=True):
    """x [B, H, W, Cin], dy [B, H/2, W/2, Cout] -> (dw [4, 4, Cin, Cout], db [Cout]) float64; db is the column sum of dy as the form
    reads it (a ones row of the same bf16 product in the bf16 forms)."""
    rx, rd = (rb if round_x else ident), (rb if round_dy else ident)
    dw = torch.nn.grad.conv2d_weight(rx(nchw(x)), (dy.shape[3], x.shape[3], 4, 4), rd(nchw(dy)), stride=2, padding=1).permute(2, 3, 1, 0)
    return dw, rd(dy.double().cpu()).sum(dim=(0, 1, 2))


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------
def _pow2(n):
    return n > 0 and (n & (n - 1)) == 0


def _up(v, q=256):
    return (v + q - 1) // q * q


def _cdiv(a, b):
    return (a + b - 1) // b


def thin_channels_ok(c):
    return 1 <= c <= 256 and 256 % c == 0


def thin_groups_ok(c):
    return c % 8 == 0 and c <= 256 and 256 % c == 0


def fwd_fast_ok(transposed, B, H, W, c_in, c_out):
    """conv_fwd_fast: the LDS-DMA shapes of the forward (H, W: its input) / transposed forward (H, W: its input grid)."""
    in_px = B * H * W
    M = in_px if transposed else in_px // 4
    return _pow2(c_in) and c_in >= (16 if transposed else 8) and c_out % 32 == 0 and M >= 1


def forward_workspace_bytes(transposed, B, H, W, c_in, c_out):
    """vaek_conv2d_forward_workspace: [256 B | x bf16 | kernel bf16], 0 where the LDS-DMA shapes do not hold."""
    if not fwd_fast_ok(transposed, B, H, W, c_in, c_out):
        return 0
    return 256 + _up(B * H * W * c_in * 2) + _up(16 * c_in * c_out * 2)


def wgrad_fast(B, H, W, c_in, c_out):
    """conv_wgrad_fast: (ok, splits, rows per split)."""
    Ho, Wo = H // 2, W // 2
    hw, pixels = Ho * Wo, B * Ho * Wo
    if not (c_in % 8 == 0 and c_out % 8 == 0 and _pow2(hw) and _pow2(Wo) and pixels >= 64):
        return False, 0, 0
    tiles = _cdiv(16 * c_in, 128) * _cdiv(c_out, 128)
    S = min(max(1, 1024 // tiles), max(1, pixels // 512))
    rps = _up(_cdiv(pixels, S), 64)
    return True, _cdiv(pixels, rps), rps


def wgrad_splits(pixels, M, N):
    """conv_wgrad_splits of the register-staged kernel gradient."""
    tiles = _cdiv(M, 128) * _cdiv(N, 128)
    return min(min(max(1, 1024 // tiles), max(1, pixels // 256)), 4096)


def weight_grad_workspace_bytes(B, H, W, c_in, c_out):
    """vaek_conv2d_weight_grad_workspace."""
    pixels, M = B * (H // 2) * (W // 2), 16 * c_in + 1
    ok, S, _ = wgrad_fast(B, H, W, c_in, c_out)
    if ok:
        nbytes = 256 + _up(B * H * W * c_in * 2) + _up(pixels * c_out * 2) + S * M * c_out * 4
    else:
        nbytes = wgrad_splits(pixels, M, c_out) * M * c_out * 4
    if c_in == 1 and thin_channels_ok(c_out):
        nbytes = max(nbytes, (2048 + 1) * 17 * c_out * 4)
    return nbytes


@dataclass(frozen=True)
class Form:
    name: str                    # the kernel family that runs; "error" where the library refuses the call (VAEK_ERR_INVALID)
    decode: str = ""             # "shift" / "div": how a flat pixel index becomes (image, row, column); "" where there is one way only
    variants: tuple = ()         # compile-time / lean variants in effect: x16, m16, dy16, out16 (epilogue), out16cvt (a pass), no32
    facts: dict = field(default_factory=dict, compare=False)

    @property
    def key(self):
        return self.name + ("/" + self.decode if self.decode else "")

    @property
    def streaming(self):
        return "thin" in self.name

    @property
    def bound(self):
        return BOUND_F32 if self.streaming else BOUND_BF16

    @property
    def rounding(self):
        """(round the gathered tensor, round the other operand) in the reference of this form."""
        if not self.streaming:
            return True, True
        return "x16" in self.variants, "dy16" in self.variants


ERROR = Form("error")
LEAN_FLAGS = ("x16only", "mask16", "no32", "dy16only")


def _gemm_facts(M, N, K, BM, BN, BK, **more):
    d = dict(rows=M, row_tiles=_cdiv(M, BM), rows_in_last_tile=M - (_cdiv(M, BM) - 1) * BM, col_tiles=_cdiv(N, BN),
             cols_in_last_tile=N - (_cdiv(N, BN) - 1) * BN, k_tiles=_cdiv(K, BK), BM=BM, BN=BN)
    d.update(more)
    return d


def _lds_conv(prefix, M, c_out, K, shift, variants):
    BN = 128 if c_out % 128 == 0 else 64 if c_out % 64 == 0 else 32       # launch_hs_conv: the 32-column tile takes 256 rows
    return Form(f"{prefix}_lds_bn{BN}", "shift" if shift else "div", variants, _gemm_facts(M, c_out, K, 256 if BN == 32 else 128, BN, 64))


def form(op, B, H, W, c_in, c_out, off=(), lean=(), fast=True, masked=False, want16=False):
    """The form one call takes.  op: "fwd" (x [B, H, W, c_in]), "tfwd" (input [B, H, W, c_in] -> [B, 2 H, 2 W, c_out]) or "wgrad"
    (x [B, H, W, c_in], dy c_out channels).  off: the float32 tensors that are NOT 16-byte aligned, of x (the gathered tensor), w,
    out, mask, bias, dy.  lean: x16only (the float32 gathered tensor is NULL beside its bf16 copy; wgrad: both tensors), dy16only
    (wgrad: only dy is NULL), mask16 (the relu mask is the bf16 copy of its source), no32 (no float32 result).  fast: a workspace
    is given.  masked: a relu mask is given.  want16: a bf16 result is asked for."""
    lean, off = frozenset(lean), frozenset(off)
    assert lean <= set(LEAN_FLAGS) and off <= {"x", "w", "out", "mask", "bias", "dy"}
    masked = masked or "mask16" in lean
    al = lambda n: n not in off
    x_al = al("x") or "x16only" in lean                    # (a NULL pointer counts as aligned)
    out_al = al("out") or "no32" in lean
    mask_al = not masked or "mask16" in lean or al("mask")
    v = lambda *names: tuple(n for n in names if n)
    if op == "fwd":
        assert H % 2 == 0 and W % 2 == 0
        Ho, Wo = H // 2, W // 2
        hw, M = Ho * Wo, B * Ho * Wo
        shift = _pow2(hw) and _pow2(Wo)
        is_lean = bool(lean & {"x16only", "mask16", "no32"})
        thin = c_in == 1 and thin_channels_ok(c_out)
        fast_ok = fwd_fast_ok(False, B, H, W, c_in, c_out)
        if is_lean and not thin:
            if not (fast_ok and fast and x_al and al("w") and out_al and al("bias")):
                return ERROR
            return _lds_conv("fwd", M, c_out, 16 * c_in, shift, v("x16only" in lean and "x16", "mask16" in lean and "m16", want16 and "out16", "no32" in lean and "no32"))
        if thin:
            by8 = thin_groups_ok(c_out) and al("w") and out_al and mask_al
            mfma = by8 and c_out % 32 == 0 and shift
            if is_lean and ("x16only" in lean or not mfma):
                return ERROR
            if mfma:
                return Form("fwd_thin_mfma", "shift", v("mask16" in lean and "m16", want16 and "out16", "no32" in lean and "no32"),
                            dict(rows=M, row_tiles=_cdiv(M, 32), rows_in_last_tile=M - (_cdiv(M, 32) - 1) * 32, col_tiles=c_out // 32))
            if by8:
                return Form("fwd_thin8", "div", v(want16 and "out16"), dict(rows=M, pixels_per_block=256 // (c_out // 8)))
            return Form("fwd_thin", "div", v(want16 and "out16cvt"), dict(rows=M, pixels_per_block=256 // c_out))
        if fast and x_al and al("w") and out_al and mask_al and al("bias") and fast_ok:
            return _lds_conv("fwd", M, c_out, 16 * c_in, shift, v(want16 and "out16"))
        vec = c_in % 4 == 0 and x_al
        return Form("fwd_reg_vec" if vec else "fwd_reg_scalar", "div", v(want16 and "out16cvt"), _gemm_facts(M, c_out, 16 * c_in, 128, 128, 32))
    if op == "tfwd":
        M, hw = B * H * W, H * W
        shift = _pow2(hw) and _pow2(W)
        is_lean = bool(lean & {"x16only", "mask16", "no32"})
        fast_ok = fwd_fast_ok(True, B, H, W, c_in, c_out)
        thin4s = c_out == 1 and c_in % 4 == 0 and c_in <= 256 and _pow2(c_in) and W % 4 == 0 and al("w") and out_al and mask_al
        if is_lean and thin4s and "no32" not in lean and "mask16" not in lean:
            return Form("tfwd_thin4s", "div", v("x16", want16 and "out16cvt"), dict(rows=M, strips=M // 4, lanes_per_strip=c_in // 4))
        if is_lean:
            if not (fast_ok and fast and x_al and al("w") and out_al and al("bias") and c_out != 1):
                return ERROR
            return _lds_conv("tfwd", M, c_out, 4 * c_in, shift, v("x16only" in lean and "x16", "mask16" in lean and "m16", want16 and "out16", "no32" in lean and "no32"))
        if c_out == 1 and c_in % 4 == 0 and c_in <= 256 and x_al and al("w"):
            if _pow2(c_in) and W % 4 == 0 and out_al and mask_al:
                return Form("tfwd_thin4s", "div", v(want16 and "out16cvt"), dict(rows=M, strips=M // 4, lanes_per_strip=c_in // 4))
            if _pow2(c_in) and out_al and mask_al:         # (8-byte alignment: a tensor one float off has neither)
                return Form("tfwd_thin4", "div", v(want16 and "out16cvt"), dict(rows=M, lanes_per_pixel=c_in // 4))
            return Form("tfwd_thin", "div", v(want16 and "out16cvt"), dict(rows=4 * M))
        if fast and x_al and al("w") and out_al and mask_al and al("bias") and fast_ok:
            return _lds_conv("tfwd", M, c_out, 4 * c_in, shift, v(want16 and "out16"))
        vec = c_in % 4 == 0 and x_al and al("w")
        return Form("tfwd_reg_vec" if vec else "tfwd_reg_scalar", "div", v(want16 and "out16cvt"), _gemm_facts(M, c_out, 4 * c_in, 128, 128, 32))
    assert op == "wgrad" and H % 2 == 0 and W % 2 == 0
    Ho, Wo = H // 2, W // 2
    hw, pixels = Ho * Wo, B * Ho * Wo
    shift = _pow2(hw) and _pow2(Wo)
    no_x, no_dy = "x16only" in lean, bool(lean & {"x16only", "dy16only"})
    thin = c_in == 1 and thin_channels_ok(c_out)
    thin_mfma = thin and c_out % 32 == 0 and shift
    ok, S, rps = wgrad_fast(B, H, W, c_in, c_out)
    if thin:
        if no_x or (no_dy and not thin_mfma):
            return ERROR
        blocks = min(2048, _cdiv(pixels, 256))
        if thin_mfma:
            return Form("wgrad_thin_mfma", "shift", v(no_dy and "dy16"), dict(rows=pixels, blocks=blocks, odd_pixels=pixels % 2 == 1, col_tiles=c_out // 32))
        if thin_groups_ok(c_out) and al("dy"):
            return Form("wgrad_thin8", "div", (), dict(rows=pixels, blocks=blocks))
        return Form("wgrad_thin", "div", (), dict(rows=pixels, blocks=blocks))
    if not (ok or not (no_x or no_dy)):
        return ERROR
    if ok:
        narrow = c_out <= 64
        return Form("wgrad_lds_narrow" if narrow else "wgrad_lds", "shift", v(no_x and "x16", no_dy and "dy16"),
                    dict(rows=pixels, row_tiles=16 * c_in // 128, col_tiles=_cdiv(c_out, 128), cols_in_last_tile=c_out - (_cdiv(c_out, 128) - 1) * 128,
                         splits=S, rows_per_split=rps, rows_in_last_split=pixels - (S - 1) * rps, k_tiles=_cdiv(rps if S > 1 else pixels, 64),
                         tail_rows=(pixels - (S - 1) * rps) % 64))
    M = 16 * c_in + 1
    S = wgrad_splits(pixels, M, c_out)
    kps = _up(_cdiv(pixels, S), 32)
    return Form("wgrad_reg", "shift" if shift else "div", (),
                dict(rows=pixels, row_tiles=_cdiv(M, 128), rows_in_last_tile=M - (_cdiv(M, 128) - 1) * 128, col_tiles=_cdiv(c_out, 128), splits=S,
                     rows_per_split=kps, rows_in_last_split=max(0, pixels - (S - 1) * kps), k_tiles=_cdiv(kps, 32)))


# ---- the case table -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    expect: str                  # Form.key the case is there for
    op: str
    B: int
    H: int
    W: int
    c_in: int
    c_out: int
    why: str
    bias: bool = True            # fwd / tfwd: a bias is given; wgrad: the bias gradient is wanted
    relu: bool = False
    mask: str = ""               # "" / "f32" / "bf16" (the lean form: the bf16 copy of the mask source)
    off: tuple = ()              # float32 tensors handed over one float off 16-byte alignment
    lean: tuple = ()             # x16only / dy16only / no32 (mask "bf16" adds mask16)
    want16: bool = False         # ask for the bf16 result too
    adjacent: bool = False       # wgrad: dw and db as adjacent views of one buffer (the single-sum path)

    @property
    def lean_flags(self):
        return tuple(self.lean) + (("mask16",) if self.mask == "bf16" else ())

    @property
    def id(self):
        extra = "".join("-" + s for s in (("relu",) if self.relu else ()) + ((("mask" + self.mask),) if self.mask else ()) + tuple("off_" + o for o in self.off)
                        + self.lean + (("want16",) if self.want16 else ()) + (("adjacent",) if self.adjacent else ()) + (() if self.bias else ("nobias",)))
        return f"{self.op}-{self.B}x{self.H}x{self.W}-{self.c_in}to{self.c_out}{extra}"

    def form(self, lean=None, off=None, fast=True):
        return form(self.op, self.B, self.H, self.W, self.c_in, self.c_out, off=self.off if off is None else off,
                    lean=self.lean_flags if lean is None else lean, fast=fast, masked=bool(self.mask), want16=self.want16)

    def in_shape(self):
        return (self.B, self.H, self.W, self.c_in)

    def out_shape(self):
        if self.op == "tfwd":
            return (self.B, 2 * self.H, 2 * self.W, self.c_out)
        return (self.B, self.H // 2, self.W // 2, self.c_out)       # (wgrad: the shape of dy)

    def w_shape(self):
        return (4, 4, self.c_out, self.c_in) if self.op == "tfwd" else (4, 4, self.c_in, self.c_out)


CASES = []


def _c(expect, op, B, H, W, c_in, c_out, why, **kw):
    CASES.append(Case(expect, op, B, H, W, c_in, c_out, why, **kw))


# forward, one input channel: the f32 matrix-core form (c_out a multiple of 32 dividing 256, power-of-two output sizes)
_c("fwd_thin_mfma/shift", "fwd", 3, 4, 16, 1, 32, "48 pixels: a partial 32-pixel tile; Ho = 2, Wo = 8; float32 mask, bf16 result beside", relu=True, mask="f32", want16=True)
_c("fwd_thin_mfma/shift", "fwd", 1, 2, 2, 1, 32, "a single output pixel: every lane but one of the tile is past the end")
_c("fwd_thin_mfma/shift", "fwd", 2, 16, 4, 1, 256, "eight channel blocks; H > W; mask from its bf16 copy (M16)", relu=True, mask="bf16", want16=True)
_c("fwd_thin_mfma/shift", "fwd", 3, 4, 16, 1, 32, "bf16 result alone: the float32 one is never written", relu=True, lean=("no32",), want16=True)
_c("fwd_thin_mfma/shift", "fwd", 2, 2, 8, 1, 64, "one output row (H = 2)", relu=True)
_c("fwd_thin_mfma/shift", "fwd", 2, 8, 2, 1, 32, "one output column (W = 2)", mask="f32")
# ... the eight-channel-group form
_c("fwd_thin8/div", "fwd", 2, 4, 16, 1, 8, "c_out = 8: one group per pixel; H < W", relu=True)
_c("fwd_thin8/div", "fwd", 2, 16, 4, 1, 16, "c_out = 16; H > W; float32 mask", mask="f32")
_c("fwd_thin8/div", "fwd", 2, 6, 10, 1, 64, "c_out = 64 at a size that is no power of two; bf16 result from the epilogue", relu=True, want16=True)
_c("fwd_thin8/div", "fwd", 1, 12, 6, 1, 8, "sizes 12 and 6, H > W")
_c("fwd_thin8/div", "fwd", 3, 2, 12, 1, 16, "one output row", relu=True)
_c("fwd_thin8/div", "fwd", 3, 12, 2, 1, 8, "one output column", mask="f32")
# ... the scalar streaming form
_c("fwd_thin/div", "fwd", 2, 4, 16, 1, 1, "c_out = 1: 256 pixels per block")
_c("fwd_thin/div", "fwd", 3, 6, 10, 1, 2, "c_out = 2; float32 mask", mask="f32")
_c("fwd_thin/div", "fwd", 2, 12, 6, 1, 4, "c_out = 4; H > W; bf16 result by a conversion pass", relu=True, want16=True)
_c("fwd_thin/div", "fwd", 2, 4, 16, 1, 32, "the matrix-core shape with y one float off alignment", relu=True, off=("out",))
_c("fwd_thin/div", "fwd", 2, 10, 6, 1, 32, "the eight-group shape with the mask one float off alignment", mask="f32", off=("mask",))
_c("fwd_thin/div", "fwd", 2, 4, 4, 1, 16, "the eight-group shape with the kernel one float off alignment", off=("w",))
_c("fwd_thin/div", "fwd", 1, 2, 6, 1, 4, "one output row")
_c("fwd_thin/div", "fwd", 1, 6, 2, 1, 2, "one output column")
# ... one input channel, but a c_out the streaming kernels do not take: the register-staged GEMM with K = 16 (half a k-tile)
_c("fwd_reg_scalar/div", "fwd", 2, 6, 10, 1, 5, "c_in = 1, c_out = 5: K = 16", relu=True)
_c("fwd_reg_scalar/div", "fwd", 2, 10, 6, 1, 48, "c_in = 1, c_out = 48: K = 16; H > W", mask="f32")
# forward, LDS-DMA implicit GEMM (c_in a power of two >= 8, c_out a multiple of 32)
_c("fwd_lds_bn32/shift", "fwd", 3, 4, 16, 8, 32, "fewer rows than one 256-row tile; Ho = 2, Wo = 8", relu=True, mask="f32")
_c("fwd_lds_bn32/div", "fwd", 2, 6, 10, 8, 32, "sizes 6 and 10: the division path", relu=True)
_c("fwd_lds_bn32/shift", "fwd", 9, 8, 16, 8, 32, "288 rows: two 256-row tiles, the last one partial", relu=True)
_c("fwd_lds_bn32/shift", "fwd", 1, 2, 2, 8, 32, "one output pixel: every tap but four off the image")
_c("fwd_lds_bn32/div", "fwd", 2, 12, 2, 8, 32, "Wo = 1, H > W")
_c("fwd_lds_bn32/shift", "fwd", 2, 16, 4, 8, 96, "c_out = 96: three 32-column tiles; H > W", mask="f32")
_c("fwd_lds_bn32/div", "fwd", 2, 6, 12, 16, 96, "c_in = 16, c_out = 96; sizes 6 and 12", relu=True)
_c("fwd_lds_bn64/shift", "fwd", 2, 2, 16, 8, 64, "one output row; 64-column tile", relu=True)
_c("fwd_lds_bn64/shift", "fwd", 2, 4, 16, 16, 64, "c_in = 16; bf16 result beside the float32 one", relu=True, want16=True)
_c("fwd_lds_bn64/div", "fwd", 2, 10, 6, 16, 64, "sizes 10 and 6, H > W", mask="f32")
_c("fwd_lds_bn128/shift", "fwd", 2, 4, 16, 8, 128, "128-column tile; Ho = 2, Wo = 8", relu=True)
_c("fwd_lds_bn128/div", "fwd", 3, 12, 10, 16, 128, "90 rows; sizes 12 and 10", relu=True, mask="f32")
_c("fwd_lds_bn32/shift", "fwd", 3, 4, 16, 8, 32, "every lean form at once: x and mask from bf16 copies, bf16 result alone", relu=True, mask="bf16", lean=("x16only", "no32"), want16=True)
_c("fwd_lds_bn64/div", "fwd", 2, 6, 10, 16, 64, "x from its bf16 copy, both results", relu=True, lean=("x16only",), want16=True)
_c("fwd_lds_bn128/shift", "fwd", 2, 8, 4, 8, 128, "bf16 mask beside a float32 x", mask="bf16")
# forward, register-staged implicit GEMM
_c("fwd_reg_scalar/div", "fwd", 2, 6, 10, 3, 7, "c_in = 3: the scalar gather; K = 48 is one and a half k-tiles", relu=True)
_c("fwd_reg_scalar/div", "fwd", 2, 10, 6, 5, 8, "c_in = 5; H > W", mask="f32")
_c("fwd_reg_vec/div", "fwd", 3, 16, 4, 4, 5, "c_in = 4: the 16-byte gather; H > W")
_c("fwd_reg_vec/div", "fwd", 2, 4, 16, 12, 16, "c_in = 12: a tap boundary inside a k-tile", relu=True)
_c("fwd_reg_vec/div", "fwd", 2, 6, 12, 8, 24, "c_in = 8 with c_out = 24: not an LDS-DMA column count", relu=True, mask="f32")
_c("fwd_reg_vec/div", "fwd", 1, 2, 4, 8, 130, "c_out = 130: a second column tile of two columns")
_c("fwd_reg_vec/div", "fwd", 5, 12, 10, 4, 8, "150 output pixels: a second, partial row tile", relu=True, want16=True)
_c("fwd_reg_scalar/div", "fwd", 2, 2, 10, 3, 7, "one output row")
_c("fwd_reg_vec/div", "fwd", 2, 10, 2, 4, 6, "one output column")
_c("fwd_reg_scalar/div", "fwd", 3, 4, 16, 8, 32, "the LDS-DMA shape with x one float off alignment: register-staged, scalar gather", relu=True, mask="f32", off=("x",))
_c("fwd_reg_vec/div", "fwd", 3, 4, 16, 8, 32, "the LDS-DMA shape with the kernel off alignment", relu=True, off=("w",))
_c("fwd_reg_vec/div", "fwd", 3, 4, 16, 8, 32, "the LDS-DMA shape with y off alignment", relu=True, off=("out",))
_c("fwd_reg_vec/div", "fwd", 3, 4, 16, 8, 32, "the LDS-DMA shape with the mask off alignment", mask="f32", off=("mask",))
_c("fwd_reg_vec/div", "fwd", 3, 4, 16, 8, 32, "the LDS-DMA shape with the bias off alignment", off=("bias",))

# transposed forward, one output channel: the strip form 4s (c_in a power of two in 4 .. 256, input width a multiple of 4)
_c("tfwd_thin4s/div", "tfwd", 2, 3, 4, 4, 1, "c_in = 4: one lane per strip; w = 4: one strip per row")
_c("tfwd_thin4s/div", "tfwd", 2, 2, 8, 32, 1, "c_in = 32; w = 8; relu and float32 mask", relu=True, mask="f32")
_c("tfwd_thin4s/div", "tfwd", 1, 5, 12, 256, 1, "c_in = 256: a whole wave per strip; w = 12: three strips per row")
_c("tfwd_thin4s/div", "tfwd", 2, 1, 4, 8, 1, "h = 1: both neighbour rows off the image")
_c("tfwd_thin4s/div", "tfwd", 2, 8, 4, 16, 1, "h > w; bf16 result by a conversion pass", want16=True)
_c("tfwd_thin4s/div", "tfwd", 2, 3, 8, 32, 1, "the input from its bf16 copy (X16)", relu=True, mask="f32", lean=("x16only",))
# ... the one-pixel form 4 (width not a multiple of 4)
_c("tfwd_thin4/div", "tfwd", 2, 3, 1, 8, 1, "w = 1: both neighbour columns off the image")
_c("tfwd_thin4/div", "tfwd", 2, 1, 2, 16, 1, "h = 1, w = 2")
_c("tfwd_thin4/div", "tfwd", 2, 4, 6, 4, 1, "w = 6; relu and float32 mask", relu=True, mask="f32")
_c("tfwd_thin4/div", "tfwd", 1, 6, 2, 64, 1, "c_in = 64; h > w")
# ... the scalar streaming form (c_in a multiple of 4 up to 256 that is no power of two, or a misaligned out / mask)
_c("tfwd_thin/div", "tfwd", 2, 3, 4, 12, 1, "c_in = 12")
_c("tfwd_thin/div", "tfwd", 2, 4, 3, 20, 1, "c_in = 20; h > w; relu and float32 mask", relu=True, mask="f32")
_c("tfwd_thin/div", "tfwd", 1, 2, 5, 136, 1, "c_in = 136")
_c("tfwd_thin/div", "tfwd", 2, 3, 4, 16, 1, "the 4s shape with out one float off alignment", off=("out",))
_c("tfwd_thin/div", "tfwd", 2, 3, 4, 16, 1, "the 4s shape with the mask one float off alignment", mask="f32", off=("mask",))
_c("tfwd_thin/div", "tfwd", 2, 1, 3, 12, 1, "h = 1")
_c("tfwd_thin/div", "tfwd", 2, 3, 1, 20, 1, "w = 1", want16=True)
# ... one output channel, but a c_in the streaming kernels do not take
_c("tfwd_reg_scalar/div", "tfwd", 2, 3, 5, 6, 1, "c_out = 1 with c_in = 6: the register-staged GEMM, scalar gather")
_c("tfwd_reg_vec/div", "tfwd", 1, 2, 3, 512, 1, "c_out = 1 with c_in = 512: above the streaming kernels' 256")
_c("tfwd_reg_scalar/div", "tfwd", 2, 3, 4, 16, 1, "the 4s shape with its input one float off alignment", off=("x",))
# transposed forward, LDS-DMA (c_in a power of two >= 16, c_out a multiple of 32): four parity classes
_c("tfwd_lds_bn32/div", "tfwd", 2, 3, 5, 16, 32, "sizes 3 and 5; bias, relu and float32 mask", relu=True, mask="f32")
_c("tfwd_lds_bn32/shift", "tfwd", 2, 2, 8, 16, 32, "h = 2, w = 8: the shift path with h != w")
_c("tfwd_lds_bn32/shift", "tfwd", 5, 8, 8, 16, 32, "320 rows per class: two 256-row tiles, the last one partial", relu=True)
_c("tfwd_lds_bn32/shift", "tfwd", 3, 4, 1, 16, 96, "w = 1; three 32-column tiles")
_c("tfwd_lds_bn32/div", "tfwd", 2, 3, 1, 16, 32, "w = 1 on the division path", bias=False)
_c("tfwd_lds_bn64/shift", "tfwd", 2, 8, 2, 32, 64, "h > w; 64-column tile", relu=True, mask="f32")
_c("tfwd_lds_bn64/div", "tfwd", 2, 5, 3, 32, 64, "sizes 5 and 3; bf16 result beside the float32 one", want16=True)
_c("tfwd_lds_bn128/shift", "tfwd", 1, 1, 1, 32, 128, "h = w = 1: every neighbour tap off the image", mask="f32")
_c("tfwd_lds_bn128/div", "tfwd", 2, 1, 6, 32, 128, "h = 1", relu=True)
_c("tfwd_lds_bn64/shift", "tfwd", 2, 2, 4, 64, 64, "c_in = 64: four k-tiles")
_c("tfwd_lds_bn32/shift", "tfwd", 2, 2, 8, 16, 32, "bf16 mask, bf16 result beside", mask="bf16", want16=True)
_c("tfwd_lds_bn64/div", "tfwd", 2, 5, 3, 32, 64, "every lean form at once: input and mask from bf16 copies, bf16 result alone", relu=True, mask="bf16", lean=("x16only", "no32"), want16=True)
# transposed forward, register-staged
_c("tfwd_reg_scalar/div", "tfwd", 2, 3, 5, 3, 7, "c_in = 3: scalar gathers; float32 mask", mask="f32")
_c("tfwd_reg_vec/div", "tfwd", 2, 5, 3, 4, 5, "c_in = 4: K = 16, half a k-tile; h > w", relu=True)
_c("tfwd_reg_vec/div", "tfwd", 2, 2, 3, 8, 32, "c_in = 8 is below the LDS-DMA form's 16; float32 mask", mask="f32")
_c("tfwd_reg_vec/div", "tfwd", 1, 1, 2, 8, 130, "c_out = 130: a second column tile; h = 1", bias=False)
_c("tfwd_reg_scalar/div", "tfwd", 2, 1, 1, 3, 5, "h = w = 1")
_c("tfwd_reg_vec/div", "tfwd", 1, 3, 1, 4, 7, "w = 1", relu=True)
_c("tfwd_reg_vec/div", "tfwd", 3, 7, 7, 4, 5, "147 rows per class: a second, partial row tile", mask="f32", want16=True)
_c("tfwd_reg_scalar/div", "tfwd", 2, 3, 5, 16, 32, "the LDS-DMA shape with its input one float off alignment", relu=True, mask="f32", off=("x",))
_c("tfwd_reg_scalar/div", "tfwd", 2, 3, 5, 16, 32, "the LDS-DMA shape with the kernel off alignment", off=("w",))
_c("tfwd_reg_vec/div", "tfwd", 2, 3, 5, 16, 32, "the LDS-DMA shape with out off alignment", relu=True, off=("out",))
_c("tfwd_reg_vec/div", "tfwd", 2, 3, 5, 16, 32, "the LDS-DMA shape with the mask off alignment", mask="f32", off=("mask",))
_c("tfwd_reg_vec/div", "tfwd", 2, 3, 5, 16, 32, "the LDS-DMA shape with the bias off alignment", off=("bias",))

# kernel gradient, one input channel: the f32 matrix-core form
_c("wgrad_thin_mfma/shift", "wgrad", 3, 2, 2, 1, 32, "3 pixels: an odd count, the last pair half empty")
_c("wgrad_thin_mfma/shift", "wgrad", 2, 4, 16, 1, 256, "eight channel blocks; Ho = 2, Wo = 8")
_c("wgrad_thin_mfma/shift", "wgrad", 2, 16, 4, 1, 64, "H > W")
_c("wgrad_thin_mfma/shift", "wgrad", 3, 4, 8, 1, 32, "dy from its bf16 copy (DY16)", lean=("dy16only",))
_c("wgrad_thin_mfma/shift", "wgrad", 2, 2, 8, 1, 32, "one output row")
_c("wgrad_thin_mfma/shift", "wgrad", 2, 8, 2, 1, 32, "one output column")
_c("wgrad_thin_mfma/shift", "wgrad", 2, 4, 16, 1, 32, "dy one float off alignment: still this form (dword loads)", off=("dy",))
# ... the eight-channel-group form
_c("wgrad_thin8/div", "wgrad", 2, 4, 16, 1, 8, "c_out = 8; H < W")
_c("wgrad_thin8/div", "wgrad", 2, 16, 4, 1, 16, "c_out = 16; H > W")
_c("wgrad_thin8/div", "wgrad", 2, 6, 10, 1, 64, "c_out = 64 at a size that is no power of two")
_c("wgrad_thin8/div", "wgrad", 1, 12, 6, 1, 8, "sizes 12 and 6")
_c("wgrad_thin8/div", "wgrad", 3, 2, 12, 1, 16, "one output row")
_c("wgrad_thin8/div", "wgrad", 3, 12, 2, 1, 8, "one output column", bias=False)
# ... the scalar form
_c("wgrad_thin/div", "wgrad", 2, 4, 16, 1, 1, "c_out = 1")
_c("wgrad_thin/div", "wgrad", 2, 6, 10, 1, 2, "c_out = 2")
_c("wgrad_thin/div", "wgrad", 3, 12, 6, 1, 4, "c_out = 4; H > W")
_c("wgrad_thin/div", "wgrad", 2, 4, 16, 1, 16, "the eight-group shape with dy one float off alignment", off=("dy",))
_c("wgrad_thin/div", "wgrad", 1, 2, 6, 1, 4, "one output row")
_c("wgrad_thin/div", "wgrad", 1, 6, 2, 1, 2, "one output column")
_c("wgrad_reg/div", "wgrad", 2, 6, 10, 1, 5, "c_in = 1, c_out = 5: M = 17")
_c("wgrad_reg/div", "wgrad", 2, 10, 6, 1, 48, "c_in = 1, c_out = 48: M = 17; H > W")
# kernel gradient, LDS-DMA batch-split GEMM (channel counts multiples of 8, power-of-two output sizes, at least 64 pixels)
_c("wgrad_lds_narrow/shift", "wgrad", 4, 8, 8, 8, 8, "exactly 64 pixels: one whole k-tile; c_out = 8")
_c("wgrad_lds/shift", "wgrad", 5, 8, 8, 24, 72, "80 pixels: the last k-tile's rows past the end are zeroed; c_in = 24; c_out = 72: a partial column tile")
_c("wgrad_lds/shift", "wgrad", 17, 4, 4, 8, 136, "68 pixels; c_out = 136: a second column tile of eight columns")
_c("wgrad_lds_narrow/shift", "wgrad", 2, 4, 32, 8, 16, "Ho = 2, Wo = 16")
_c("wgrad_lds_narrow/shift", "wgrad", 2, 32, 4, 16, 8, "Ho = 16, Wo = 2")
_c("wgrad_lds_narrow/shift", "wgrad", 17, 16, 16, 8, 16, "1088 pixels in two uneven splits, 576 and 512; separate dw and db")
_c("wgrad_lds_narrow/shift", "wgrad", 17, 16, 16, 8, 16, "the same with dw and db adjacent in one buffer: the single slab sum", adjacent=True)
_c("wgrad_lds/shift", "wgrad", 5, 8, 8, 24, 72, "dw and db adjacent at a partial column tile", adjacent=True)
_c("wgrad_lds/shift", "wgrad", 5, 8, 8, 24, 72, "both tensors from their bf16 copies", lean=("x16only",))
_c("wgrad_lds_narrow/shift", "wgrad", 4, 16, 16, 16, 32, "the transposed layer's use: x := d out, dy := the layer's input, no bias gradient", bias=False)
_c("wgrad_lds_narrow/shift", "wgrad", 2, 2, 128, 8, 64, "one output row of 64 pixels; c_out = 64: the widest narrow tile")
_c("wgrad_reg/shift", "wgrad", 63, 2, 2, 8, 8, "63 pixels, one below the LDS-DMA form's threshold")
# kernel gradient, register-staged batch-split GEMM
_c("wgrad_reg/div", "wgrad", 2, 6, 6, 8, 8, "M = 129: the ones row alone in a second row tile")
_c("wgrad_reg/div", "wgrad", 2, 6, 10, 3, 7, "c_in = 3, c_out = 7; sizes 6 and 10")
_c("wgrad_reg/div", "wgrad", 2, 12, 6, 5, 8, "H > W on the division path")
_c("wgrad_reg/shift", "wgrad", 1, 4, 4, 8, 130, "c_out = 130: a second column tile")
_c("wgrad_reg/shift", "wgrad", 2, 4, 16, 4, 5, "Ho = 2, Wo = 8 on the shift path")
_c("wgrad_reg/shift", "wgrad", 2, 16, 4, 12, 16, "Ho = 8, Wo = 2 on the shift path; M = 193")
_c("wgrad_reg/shift", "wgrad", 8, 16, 16, 4, 8, "512 pixels: two splits of 256")
_c("wgrad_reg/shift", "wgrad", 9, 16, 16, 4, 8, "576 pixels: two splits of 288, nine k-tiles each")
_c("wgrad_reg/shift", "wgrad", 130, 4, 4, 4, 8, "520 pixels: two uneven splits, 288 and 232 -- the last k-tile of the last split is partial")
_c("wgrad_reg/div", "wgrad", 2, 2, 10, 3, 7, "one output row")
_c("wgrad_reg/div", "wgrad", 2, 10, 2, 4, 6, "one output column")
_c("wgrad_reg/shift", "wgrad", 4, 16, 16, 12, 16, "the transposed layer's use with c_out_t = 12: no bias gradient", bias=False)

# the remaining forms in the direction they had not seen yet (H < W and H > W for every kernel)
_c("tfwd_lds_bn128/shift", "tfwd", 2, 4, 2, 32, 128, "h > w with 128-column tiles", relu=True)
_c("tfwd_reg_scalar/div", "tfwd", 2, 5, 2, 6, 3, "h > w with the scalar gathers", mask="f32")
_c("wgrad_lds/shift", "wgrad", 2, 4, 32, 8, 72, "Ho = 2, Wo = 16 on the 128-column kernel: exactly one k-tile")
_c("wgrad_lds/shift", "wgrad", 3, 32, 4, 16, 136, "Ho = 16, Wo = 2: 96 pixels, half a k-tile past the end; two column tiles")

# column sums (conv2d_bias_grad): (pixels, c, dtype, why)
COLSUM_CASES = [
    (38, 2, "f32", "conv_colsum4_kernel at c = 2: a thread's float4 holds two pixels"),
    (5, 2048, "f32", "conv_colsum_kernel with c > 256: the chunk loop runs eight times"),
    (7, 300, "f32", "conv_colsum_kernel with a c that does not divide 256: a second, partial chunk"),
    (37, 8, "bf16", "conv_colsum8_bf16_kernel: an odd pixel count, element count a multiple of 8"),
]


def colsum_bound(pixels, want):
    """The bound of test_conv2d_bias_grad_sums_the_pixels / _of_a_bf16_tensor (absolute)."""
    return 1e-5 * np.sqrt(pixels) * max(1.0, np.max(np.abs(want)) / np.sqrt(pixels))


# ---- draws --------------------------------------------------------------------------------------------------------------------
def draw(case, seed=None):
    """The float32 tensors of a case as CPU torch tensors: normal data, kernel scaled by fan-in, bias 0.1 N(0, 1), normal mask source.
    fwd / tfwd: dict(x, w, bias, mask); wgrad: dict(x, dy)."""
    rng = np.random.default_rng(CASES.index(case) + 1000 if seed is None else seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    d = {"x": t(rng.standard_normal(case.in_shape()))}
    if case.op == "wgrad":
        d["dy"] = t(rng.standard_normal(case.out_shape()))
        return d
    fan = (4 if case.op == "tfwd" else 16) * case.c_in
    d["w"] = t(rng.standard_normal(case.w_shape()) / np.sqrt(fan))
    d["bias"] = t(0.1 * rng.standard_normal(case.c_out)) if case.bias else None
    d["mask"] = t(rng.standard_normal(case.out_shape())) if case.mask else None
    return d


def reference(case, d, f=None, rounded=True):
    """The reference of a case on the draws d, rounded where the form f (default: the case's own) rounds.  fwd / tfwd: one tensor;
    wgrad: (dw, db)."""
    f = case.form() if f is None else f
    ra, rb_ = f.rounding if rounded else (False, False)
    if case.op == "wgrad":
        return ref_weight_grad(d["x"], d["dy"], ra, rb_)
    mask = d["mask"]
    if mask is not None and case.mask == "bf16":
        mask = mask.to(torch.bfloat16)
    fn = ref_forward if case.op == "fwd" else ref_transpose
    return fn(d["x"], d["w"], d["bias"], case.relu, mask, ra, rb_)
