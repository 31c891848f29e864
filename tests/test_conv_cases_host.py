"""No GPU: the convolution case table of tests/conv_cases.py is held to what it claims before any kernel runs against it.

* every case takes the form it is there for, and the table reaches every form (and decode path, and lean variant) form() can return;
* form() agrees with the library's own workspace queries (which touch no GPU);
* the references with no rounding ARE the float64 oracle's layer functions, non-square images included (1e-12 of their scale);
* sensitivity: one wrongly gathered corner element moves a case's reference by at least 100 times the bound the GPU test applies;
* headroom: the same bf16 products accumulated in float32 stay within a quarter of that bound, so another summation order fits."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import conv_vae_oracle as CO
from tests import conv_cases as K

IDS = [f"{i:03d}-{c.id}" for i, c in enumerate(K.CASES)]
VARIANT_FAMILIES = ("fwd_thin_mfma", "fwd_thin8", "fwd_lds", "tfwd_thin4s", "tfwd_lds", "wgrad_thin_mfma", "wgrad_lds")
LEAN_VARIANTS = ("x16", "m16", "dy16", "out16", "no32")


def _family(name):
    name = name.split("_bn")[0]
    return name[:-len("_narrow")] if name.endswith("_narrow") else name


def _pairs(f):
    return {(_family(f.name), v) for v in f.variants if v in LEAN_VARIANTS and _family(f.name) in VARIANT_FAMILIES}


def test_every_case_takes_the_form_it_is_there_for():
    assert len({c.id + c.why for c in K.CASES}) == len(K.CASES)
    for c in K.CASES:
        f = c.form()
        assert f.key == c.expect, (c.id, f.key, c.expect)
        assert max(np.prod(c.in_shape()), np.prod(c.out_shape()), np.prod(c.w_shape())) * 4 <= 400 * 1024, c.id      # a few hundred KB at most


def test_the_table_reaches_every_form_decode_path_and_lean_variant():
    """Sweep form() over a grid of shapes, alignments and lean flags: whatever it can return, some case is there for."""
    keys, pairs = set(), set()
    sizes = {"fwd": (2, 4, 6), "tfwd": (1, 3, 4), "wgrad": (2, 4, 6)}
    offs = [()] + [(n,) for n in ("x", "w", "out", "mask", "bias", "dy")]
    leans = [(), ("x16only",), ("mask16",), ("no32",), ("dy16only",), ("x16only", "mask16", "no32")]
    for op in ("fwd", "tfwd", "wgrad"):
        for B, H, W, ci, co, off, lean, w16 in itertools.product((1, 4, 63), sizes[op], sizes[op], (1, 3, 4, 8, 12, 16, 24), (1, 2, 5, 8, 16, 32, 64, 72, 96, 128, 130, 256),
                                                                 offs, leans, (False, True)):
            if op == "wgrad" and (set(lean) & {"mask16", "no32"} or set(off) - {"x", "dy"} or w16):
                continue
            if op != "wgrad" and ("dy16only" in lean or "dy" in off):
                continue
            f = K.form(op, B, H, W, ci, co, off=off, lean=lean, masked=True, want16=w16 or "no32" in lean)
            if f.name != "error":
                keys.add(f.key)
                pairs |= _pairs(f)
    have = {c.form().key for c in K.CASES}
    have_pairs = set().union(*(_pairs(c.form()) for c in K.CASES))
    assert keys - have == set(), sorted(keys - have)
    assert pairs - have_pairs == set(), sorted(pairs - have_pairs)
    # and by name, what the issue lists: both kernel-gradient LDS-DMA variants, all three BN, both decode paths of each GEMM form
    for k in ["wgrad_lds/shift", "wgrad_lds_narrow/shift", "wgrad_reg/shift", "wgrad_reg/div"] + [f"{op}_lds_bn{bn}/{d}" for op in ("fwd", "tfwd") for bn in (32, 64, 128) for d in ("shift", "div")]:
        assert k in have, k
    for p in [("fwd_thin_mfma", "m16"), ("tfwd_thin4s", "x16"), ("wgrad_thin_mfma", "dy16"), ("fwd_lds", "out16"), ("fwd_lds", "no32"), ("tfwd_lds", "out16"), ("tfwd_lds", "no32"),
              ("fwd_thin_mfma", "no32"), ("fwd_thin8", "out16")]:
        assert p in have_pairs, p


def test_every_kernel_sees_images_wider_than_high_and_higher_than_wide():
    seen = {}
    for c in K.CASES:
        seen.setdefault(c.form().name, set()).add((c.H < c.W) - (c.H > c.W))
    assert all({1, -1} <= v for v in seen.values()), {k: v for k, v in seen.items() if not {1, -1} <= v}


def test_the_tiling_edges_the_cases_are_there_for():
    """The tiling facts form() reports, at the cases whose reason names them."""
    by = {}
    for c in K.CASES:
        by.setdefault((c.op, c.B, c.H, c.W, c.c_in, c.c_out, c.off), c.form())
    f = by[("fwd", 9, 8, 16, 8, 32, ())].facts
    assert (f["row_tiles"], f["rows_in_last_tile"], f["BM"]) == (2, 32, 256)
    f = by[("tfwd", 5, 8, 8, 16, 32, ())].facts
    assert (f["row_tiles"], f["rows_in_last_tile"]) == (2, 64)
    f = by[("wgrad", 4, 8, 8, 8, 8, ())].facts
    assert (f["rows"], f["splits"], f["tail_rows"], f["k_tiles"]) == (64, 1, 0, 1)
    f = by[("wgrad", 5, 8, 8, 24, 72, ())].facts
    assert (f["rows"], f["tail_rows"], f["k_tiles"], f["row_tiles"], f["cols_in_last_tile"]) == (80, 16, 2, 3, 72)
    f = by[("wgrad", 17, 4, 4, 8, 136, ())].facts
    assert (f["rows"], f["tail_rows"], f["col_tiles"], f["cols_in_last_tile"]) == (68, 4, 2, 8)
    f = by[("wgrad", 17, 16, 16, 8, 16, ())].facts
    assert (f["rows"], f["splits"], f["rows_per_split"], f["rows_in_last_split"]) == (1088, 2, 576, 512)
    f = by[("wgrad", 2, 6, 6, 8, 8, ())].facts
    assert (f["row_tiles"], f["rows_in_last_tile"]) == (2, 1)
    f = by[("wgrad", 8, 16, 16, 4, 8, ())].facts
    assert (f["splits"], f["rows_per_split"], f["rows_in_last_split"]) == (2, 256, 256)
    f = by[("wgrad", 130, 4, 4, 4, 8, ())].facts
    assert (f["splits"], f["rows_per_split"], f["rows_in_last_split"]) == (2, 288, 232)
    assert by[("wgrad", 63, 2, 2, 8, 8, ())].name == "wgrad_reg" and by[("wgrad", 3, 2, 2, 1, 32, ())].facts["odd_pixels"]
    f = by[("fwd", 3, 4, 16, 1, 32, ())].facts
    assert (f["rows"], f["row_tiles"], f["rows_in_last_tile"]) == (48, 2, 16)


def test_form_agrees_with_the_library_workspace_queries():
    """vaek_conv2d_forward_workspace is non-zero exactly where form() says the LDS-DMA shapes hold (all aligned, a workspace), and both
    queries return the sizes form()'s restatement predicts.  Neither call touches a GPU."""
    from vae_training_amd import _lib
    lib = _lib.load()
    for c in K.CASES:
        n = C.c_size_t()
        if c.op == "wgrad":
            _lib.check(lib.vaek_conv2d_weight_grad_workspace(c.B, c.H, c.W, c.c_in, c.c_out, C.byref(n)))
            assert n.value == K.weight_grad_workspace_bytes(c.B, c.H, c.W, c.c_in, c.c_out), c.id
            f = K.form("wgrad", c.B, c.H, c.W, c.c_in, c.c_out)
            if f.name.startswith("wgrad_lds"):
                assert n.value >= 256 + f.facts["splits"] * (16 * c.c_in + 1) * c.c_out * 4
            continue
        t = c.op == "tfwd"
        _lib.check(lib.vaek_conv2d_forward_workspace(c.B, c.H, c.W, c.c_in, c.c_out, int(t), C.byref(n)))
        f = K.form(c.op, c.B, c.H, c.W, c.c_in, c.c_out)                # all aligned, float32 tensors
        lds = "_lds_" in f.name
        lean = K.form(c.op, c.B, c.H, c.W, c.c_in, c.c_out, lean=("x16only", "no32"), want16=True)
        assert (n.value != 0) == lds == ("_lds_" in lean.name), (c.id, n.value, f.key, lean.key)
        assert n.value == K.forward_workspace_bytes(t, c.B, c.H, c.W, c.c_in, c.c_out), c.id
        assert K.form(c.op, c.B, c.H, c.W, c.c_in, c.c_out, fast=False).name.find("_lds_") < 0


def _np(t):
    return t.numpy().astype(np.float64)


def _oracle(c, d):
    x = _np(d["x"])
    if c.op == "wgrad":
        dy = _np(d["dy"])
        if c.bias:
            _, dw, db = CO.conv_bwd(x, np.zeros((4, 4, c.c_in, c.c_out)), dy)
        else:                                                # the transposed layer's use: x := d out, dy := the layer's input
            _, dw, db = CO.conv_t_bwd(dy, np.zeros((4, 4, c.c_in, c.c_out)), x)
            db = dy.sum(axis=(0, 1, 2))
        return dw, db
    b = np.zeros(c.c_out) if d["bias"] is None else _np(d["bias"])
    out = (CO.conv_fwd if c.op == "fwd" else CO.conv_t_fwd)(x, _np(d["w"]), b)
    out = np.maximum(out, 0.0) if c.relu else out
    return out * (_np(d["mask"]) > 0) if c.mask else out


def _scale(a):
    return float(np.max(np.abs(a))) + 1e-300


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_unrounded_reference_is_the_float64_oracle(c):
    d = K.draw(c)
    ref, want = K.reference(c, d, rounded=False), _oracle(c, d)
    if c.op == "wgrad":
        assert tuple(ref[0].shape) == want[0].shape == (4, 4, c.c_in, c.c_out)
        assert np.max(np.abs(ref[0].numpy() - want[0])) <= 1e-12 * _scale(want[0])
        assert np.max(np.abs(ref[1].numpy() - want[1])) <= 1e-12 * _scale(want[1])
    else:
        assert tuple(ref.shape) == want.shape == c.out_shape()
        assert np.max(np.abs(ref.numpy() - want)) <= 1e-12 * _scale(want)


def _first(ref):
    return ref[0] if isinstance(ref, tuple) else ref


def corner_sensitivity(c, d):
    """The smaller of the two moves of the reference (in units of its max-abs) when ONE input element at an image corner is zeroed:
    the top-left pixel of the first image, the bottom-right pixel of the last (the channel of largest magnitude there)."""
    ref = _first(K.reference(c, d))
    moves = []
    for n, i, j in ((0, 0, 0), (c.B - 1, c.H - 1, c.W - 1)):
        e = dict(d)
        e["x"] = d["x"].clone()
        ch = int(e["x"][n, i, j].abs().argmax())
        e["x"][n, i, j, ch] = 0.0
        moves.append(float((_first(K.reference(c, e)) - ref).abs().max() / ref.abs().max()))
    return min(moves)


@pytest.mark.parametrize("c", K.CASES, ids=IDS)
def test_one_wrong_corner_element_moves_the_reference_far_beyond_the_bound(c):
    move = corner_sensitivity(c, K.draw(c))
    assert move >= 100 * c.form().bound, move


def f32_accumulated(c, d):
    """The same bf16 products as the reference, accumulated in float32 by NumPy (its own blocking and order)."""
    r = lambda t: t.to(torch.bfloat16).float().numpy()
    x = r(d["x"])
    if c.op == "wgrad":
        dy = r(d["dy"])
        return (np.tensordot(CO._patches(x), dy, axes=([0, 1, 2], [0, 1, 2])), dy.sum(axis=(0, 1, 2), dtype=np.float32))
    b = np.zeros(c.c_out, np.float32) if d["bias"] is None else d["bias"].numpy()
    out = (CO.conv_fwd if c.op == "fwd" else CO.conv_t_fwd)(x, r(d["w"]), b)
    assert out.dtype == np.float32
    out = np.maximum(out, 0.0) if c.relu else out
    return out * (d["mask"].numpy() > 0) if c.mask else out


def headroom(c, d):
    got, ref = f32_accumulated(c, d), K.reference(c, d)
    if c.op == "wgrad":
        assert got[0].dtype == np.float32 and got[1].dtype == np.float32
        return max(np.max(np.abs(g - r.numpy())) / _scale(r.numpy()) for g, r in zip(got, ref))
    return np.max(np.abs(got - ref.numpy())) / _scale(ref.numpy())


@pytest.mark.parametrize("c", [c for c in K.CASES if not c.form().streaming], ids=[i for i, c in zip(IDS, K.CASES) if not c.form().streaming])
def test_float32_accumulation_leaves_three_quarters_of_the_bound(c):
    h = headroom(c, K.draw(c))
    assert h <= 0.25 * K.BOUND_BF16, h


def test_column_sum_cases_take_the_kernels_they_name():
    """The dispatch of vaek_conv2d_bias_grad, restated: the flat 16-byte stream for a power-of-two c <= 1024 with pixels * c a multiple
    of 4, the per-column kernel otherwise (its chunk loop for c > 256)."""
    flat = lambda p, c: (c & (c - 1)) == 0 and c <= 1024 and (p * c) % 4 == 0
    (p0, c0, _, _), (p1, c1, _, _), (p2, c2, _, _), (p3, c3, t3, _) = K.COLSUM_CASES
    assert flat(p0, c0) and c0 == 2
    assert not flat(p1, c1) and c1 > 256 and c1 % 256 == 0
    assert not flat(p2, c2) and c2 > 256 and 256 % (c2 - 256) != 0
    assert t3 == "bf16" and c3 == 8 and p3 % 2 == 1 and (p3 * c3) % 8 == 0
