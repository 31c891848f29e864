"""-m gpu: every form of the convolution kernels (csrc/conv_bf16.hip, the conv modes of csrc/gemm_bf16s.hip) against a reference with
the same operand rounding, case by case (tests/conv_cases.py; tests/test_conv_cases_host.py shows each case is strong enough).

Bounds, in units of the reference's max-abs: 2e-6 for the bf16 GEMM forms (same bf16 products, float32 accumulation in another
order -- the bound test_conv_vae_loss_and_every_gradient_leaf holds them to), bias row of the kernel gradient included; 1e-5 for
the streaming one-channel forms (the float32 contract), lean variants included.  Every result is written into a sentinel-filled
buffer with guard floats on both sides: the guards survive, every element is written.  Two runs are bitwise equal.  The last test
prints the worst error of each form in units of its bound (profiles/conv_forms.txt)."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from tests import conv_cases as K

pytestmark = pytest.mark.gpu

IDS = [f"{i:03d}-{c.id}" for i, c in enumerate(K.CASES)]
GUARD, SENTINEL = 64, 7.25e9          # guard floats on each side (256 bytes: the view keeps the buffer's alignment)
WORST = {}                            # form key (+ variants) -> worst error in units of the form's bound


def _note(f, what, err):
    k = (f.key + (" [" + ",".join(f.variants) + "]" if f.variants else ""), what)
    WORST[k] = max(WORST.get(k, 0.0), err / f.bound)


def _dev(t, off=False):
    """A CPU float32 tensor on the device; off: as a view one float into a buffer (4-byte, not 8- or 16-byte aligned)."""
    if t is None:
        return None
    if not off:
        v = t.cuda().contiguous()
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _bf16(t):
    return None if t is None else t.to(torch.bfloat16).cuda().contiguous()


class Guarded:
    """A result view inside a sentinel-filled buffer, guard floats before and after."""

    def __init__(self, shape, off=False):
        self.n = math.prod(shape)
        self.buf = torch.full((2 * GUARD + self.n + 4,), SENTINEL, dtype=torch.float32, device="cuda")
        self.s = GUARD + (1 if off else 0)
        self.view = self.buf[self.s:self.s + self.n].view(shape)
        assert self.view.data_ptr() % 16 == (4 if off else 0)

    def check(self, what):
        assert bool((self.buf[:self.s] == SENTINEL).all()) and bool((self.buf[self.s + self.n:] == SENTINEL).all()), f"{what}: written outside the result"
        assert bool((self.view != SENTINEL).all()), f"{what}: an element of the result was not written"


def call(c, d, lean=None, want16=None, fast=True, off=None, adjacent=None):
    """Run a case through the wrappers of vae_training_amd/conv.py.  fwd / tfwd: (out32 or None, out16 or None); wgrad: (dw, db or None).
    Every float32 result is a guarded view, checked here."""
    from vae_training_amd.conv import conv2d_forward, conv2d_transpose_forward, conv2d_weight_grad
    lean = set(c.lean_flags if lean is None else lean)
    off = set(c.off if off is None else off)
    want16 = c.want16 if want16 is None else want16
    x = None if "x16only" in lean else _dev(d["x"], "x" in off)
    if c.op == "wgrad":
        adjacent = c.adjacent if adjacent is None else adjacent
        dy = None if lean & {"x16only", "dy16only"} else _dev(d["dy"], "dy" in off)
        nk = 16 * c.c_in * c.c_out
        if adjacent:
            g = Guarded((nk + c.c_out,))
            dw, db, guards = g.view[:nk], g.view[nk:], [g]
        else:
            gw, gb = Guarded((4, 4, c.c_in, c.c_out)), Guarded((c.c_out,)) if c.bias else None
            dw, db, guards = gw.view, (gb.view if gb else None), [gw] + ([gb] if gb else [])
        rw, rb_ = conv2d_weight_grad(x, dy, c.bias, dw, db, x16=_bf16(d["x"]) if x is None else None, dy16=_bf16(d["dy"]) if dy is None else None)
        torch.cuda.synchronize()
        for g in guards:
            g.check(c.id)
        assert rw.data_ptr() == dw.data_ptr() and (db is None) == (rb_ is None)
        return rw.reshape(4, 4, c.c_in, c.c_out), rb_
    w, bias = _dev(d["w"], "w" in off), _dev(d["bias"], "bias" in off)
    mask16 = _bf16(d["mask"]) if "mask16" in lean else None
    mask = _dev(d["mask"], "mask" in off) if c.mask and mask16 is None else None
    want32 = "no32" not in lean
    g = Guarded(c.out_shape(), "out" in off) if want32 else None
    kw = dict(fast=fast, want16=want16 or not want32, mask16=mask16, want32=want32, out=g.view if g else None)
    if c.op == "fwd":
        res = conv2d_forward(x, w, bias, c.relu, mask, x16=_bf16(d["x"]) if x is None else None, **kw)
    else:
        res = conv2d_transpose_forward(x, w, bias, c.relu, mask, y16=_bf16(d["x"]) if x is None else None, **kw)
    torch.cuda.synchronize()
    out, out16 = res if isinstance(res, tuple) else (res, None)
    if g:
        g.check(c.id)
        assert out.data_ptr() == g.view.data_ptr()
    else:
        assert out is None
    assert out16 is None or (out16.dtype == torch.bfloat16 and tuple(out16.shape) == c.out_shape())
    return out, out16


def _twin(c):
    """The float32-twin call of a lean case: every tensor float32, both results."""
    return dataclasses.replace(c, lean=(), mask="f32" if c.mask else "", want16=True)


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_every_form_matches_its_bf16_operand_reference(c):
    f, d = c.form(), K.draw(c)
    ref = K.reference(c, d, f)
    if c.op == "wgrad":
        dw, db = call(c, d)
        assert tuple(dw.shape) == (4, 4, c.c_in, c.c_out) and (db is None or tuple(db.shape) == (c.c_out,))
        e = K.rel(dw, ref[0])
        print(f"{c.id}: {f.key} dw {e:.3g} (bound {f.bound:g})")
        _note(f, "dw", e)
        eb = None
        if db is not None:
            eb = K.rel(db, ref[1])
            print(f"{c.id}: {f.key} db {eb:.3g}")
            _note(f, "db", eb)
        assert e <= f.bound and (eb is None or eb <= f.bound), (e, eb)
        dw2, db2 = call(c, d)
        assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))          # slabs + fixed-order sums: bitwise repeatable
        return
    out, out16 = call(c, d)
    again, again16 = call(c, d)
    if out is not None:
        assert tuple(out.shape) == c.out_shape()
        e = K.rel(out, ref)
        print(f"{c.id}: {f.key} {e:.3g} (bound {f.bound:g})")
        _note(f, "out", e)
        assert e <= f.bound, e
        assert torch.equal(out, again)
        if c.want16:
            assert torch.equal(out16, out.to(torch.bfloat16))                          # beside the float32 result: bitwise its rounding
    else:                                                                              # alone: bitwise the bf16 result of the twin call
        t = _twin(c)
        tf = t.form()
        assert tf.key == f.key, (tf.key, f.key)
        t32, t16 = call(t, d)
        e = K.rel(t32, K.reference(t, d, tf))
        print(f"{c.id}: {f.key} twin {e:.3g} (bound {f.bound:g})")
        _note(tf, "out", e)
        assert e <= f.bound, e
        assert torch.equal(t16, t32.to(torch.bfloat16)) and torch.equal(out16, t16)
        assert torch.equal(out16, again16)


def _probes(c):
    """(lean flags) of the two lean calls tried on every case: the gathered float32 tensor NULL beside its bf16 copy; and the other
    lean operand (fwd / tfwd: no float32 result, the mask -- if any -- as its bf16 copy; wgrad: only dy NULL)."""
    m = ("mask16",) if c.mask else ()
    if c.op == "wgrad":
        return [("x16only",), ("dy16only",)]
    # (a float32 mask one float off alignment stays out of the lean calls: the lean dispatch does not look at its alignment)
    return [("x16only",) + (m if "mask" in c.off or c.mask == "bf16" else ()), ("no32",) + m]


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_lean_calls_succeed_exactly_where_form_says(c):
    """This pins form() to the dispatch that actually runs: NULL float32 tensors are refused with VAEK_ERR_INVALID (-1) wherever
    form() returns "error", and where it names a form the call succeeds and matches that form's reference."""
    from vae_training_amd._lib import VaekError
    d = K.draw(c)
    for lean in _probes(c):
        f = c.form(lean=lean)
        if f.name == "error":
            with pytest.raises(VaekError) as ei:
                call(c, d, lean=lean)
            assert ei.value.code == -1, (lean, ei.value)
            continue
        got = call(c, d, lean=lean)                       # (a VaekError here: form() promised a lean form the library refuses)
        if c.op == "wgrad":
            ref = K.ref_weight_grad(d["x"], d["dy"], *f.rounding)
            e = K.rel(got[0], ref[0])
            eb = K.rel(got[1], ref[1]) if got[1] is not None else 0.0
            _note(f, "dw", e); _note(f, "db", eb)
            assert e <= f.bound and eb <= f.bound, (lean, f.key, e, eb)
            continue
        ref = K.reference(dataclasses.replace(c, mask="bf16" if "mask16" in lean else c.mask), d, f)
        out, out16 = got
        if out is not None:
            e = K.rel(out, ref)
            _note(f, "out", e)
            assert e <= f.bound, (lean, f.key, e)
        else:       # only the bf16 result: the reference within the form's bound plus one bf16 rounding (8 significant bits: half an ulp is at most 2^-8 relative)
            diff = (out16.double().cpu() - ref).abs()
            assert bool((diff <= 2.0 ** -8 * ref.abs() + f.bound * ref.abs().max()).all()), (lean, f.key, float(diff.max()))


LDS_CASES = [(i, c) for i, c in zip(IDS, K.CASES) if c.op != "wgrad" and "_lds_" in c.form().name and not c.lean_flags]


@pytest.mark.parametrize("c", [c for _, c in LDS_CASES], ids=[i for i, _ in LDS_CASES])
def test_lds_dma_and_register_staged_forms_agree_on_every_lds_case(c):
    """fast=False (no workspace) runs the register-staged kernel on the same bf16 products: 1e-5 of the result's scale between the
    two, and the register-staged result within its own 2e-6 of the reference."""
    d = K.draw(c)
    slow_form = c.form(fast=False)
    assert "_reg_" in slow_form.name
    a, _ = call(c, d)
    b, _ = call(c, d, fast=False)
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    e = K.rel(b, K.reference(c, d, slow_form))
    _note(slow_form, "out", e)
    assert e <= slow_form.bound, e


@pytest.mark.parametrize("pixels,ch,dtype,why", K.COLSUM_CASES)
def test_column_sums_at_their_edges(pixels, ch, dtype, why):
    from vae_training_amd.conv import conv2d_bias_grad
    rng = np.random.default_rng(pixels + ch)
    dy = torch.from_numpy(np.asarray(rng.standard_normal((pixels, ch)), np.float32)).cuda()
    if dtype == "bf16":
        dy = dy.to(torch.bfloat16).contiguous()
    want = dy.double().cpu().numpy().sum(axis=0)
    g = Guarded((ch,))
    got = conv2d_bias_grad(dy, g.view)
    torch.cuda.synchronize()
    g.check(why)
    err, bound = float(np.max(np.abs(got.double().cpu().numpy() - want))), K.colsum_bound(pixels, want)
    print(f"column sum {pixels} x {ch} {dtype}: {err:.3g} (bound {bound:.3g})")
    WORST[(f"colsum {pixels}x{ch} {dtype}", "db")] = err / bound
    assert err <= bound, (err, bound)
    g2 = Guarded((ch,))
    assert torch.equal(conv2d_bias_grad(dy, g2.view), got)                             # fixed-order sums


def test_report_the_worst_error_of_each_form():
    """Not a check of its own: prints what the tests above measured, in units of each form's bound (all <= 1 or they failed)."""
    print("\nworst error of each form, in units of its bound (2e-6 bf16 GEMM forms, 1e-5 streaming forms, the column sums' own):")
    for (k, what), v in sorted(WORST.items()):
        print(f"  {k:55s} {what:4s} {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
