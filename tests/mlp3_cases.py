"""Shared case list of the three-hidden-layer whole-network step (csrc/fused_mlp3.hip): what tests/test_gpu_mlp3.py runs on the
GPU, and what tests/test_mlp3_inputs.py first proves free of relu kinks on the CPU (a first-layer pre-activation that changes
sign between float32 and float64 moves a gradient by far more than rounding, whatever kernel computes it).

A case is (config, dataset kwargs, batch rows, seed for gpu_util.random_problem, Engine kwargs)."""
from oracle import elbo_oracle as O

MAX_BATCH = 128          # kMlp3MaxBatch of csrc/fused_mlp3.hip
H3 = (200, 200, 200)     # the sphere script's hidden widths


def sphere(dd, pad, L, hidden=H3, dec_hidden=None):
    cfg = O.Config(dd + pad, L, tuple(hidden), tuple(dec_hidden or hidden), -3.0, True, "sphere")
    return cfg, dict(name="sphere", seed=69, dd=dd, pad=pad)


def _case(cd, B, seed=11, **kw):
    return (cd[0], cd[1], B, seed, kw)


SCRIPT_ROWS = [(3, 3, 6), (3, 13, 8), (5, 16, 16), (5, 5, 10), (7, 7, 13)]       # (dd, pad, L) of sphere_vae_padding_expts.sh

# contexts that take the new path
CASES = [_case(sphere(*r), 100) for r in SCRIPT_ROWS] + [
    _case(sphere(3, 3, 6), 128), _case(sphere(3, 3, 6), 37), _case(sphere(3, 3, 6), 5),
    _case(sphere(3, 3, 6, (200, 128, 64)), 100), _case(sphere(3, 3, 6, (256, 256, 256)), 100),
    _case(sphere(3, 18, 6, (64, 200, 96)), 100),                                   # D = 21
    _case(sphere(3, 3, 6), MAX_BATCH),
    _case(sphere(3, 3, 6, (66, 201, 130)), 100),                                   # widths that are no multiples of 4: no 16-byte weight loads
]

# the fence: neighbours that stay on the layer-by-layer kernels
FENCE = [
    _case(sphere(3, 3, 6, (256, 256)), 256),
    _case(sphere(3, 3, 6, (200, 200, 63)), 100),
    _case(sphere(3, 3, 6, (200, 200, 257)), 100),
    _case(sphere(3, 30, 6), 100),                                                  # D = 33
    _case((O.Config(7, 6, H3, H3, -3.0, True, "sigmoid"), dict(name="sigmoid", seed=69, dd=3, pad=3)), 100),
    _case(sphere(3, 3, 6), MAX_BATCH + 1),
    _case(sphere(3, 3, 6), 100, force_generic=True),
]


def case_id(c):
    cfg, dk, B, seed, kw = c
    return f"{dk['name']}-D{cfg.D}-L{cfg.L}-{'x'.join(map(str, cfg.enc_sizes[:-1]))}-B{B}" + ("-generic" if kw.get("force_generic") else "")
