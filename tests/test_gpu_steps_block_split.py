"""-m gpu: the tile paths of the persistent vaek_train_steps streamers at three feature blocks (csrc/linear_moments.hip), on each
kernel instantiation.  Written for the products dealt by OUTPUT BLOCK -- a multiplying wave owning whole blocks of a tile's
image, two halves of a shared block meeting through LDS, every block stored straight from the accumulators -- which passed them
and was dropped for its speed (profiles/lin_blocks_roles.txt); they hold for any deal of a tile's products and they cover what
the streamers do now: a lane's operand addresses formed per tile from a feature map made once per launch (LinFeatMap: the slot
and the ragged tile's validity column enter by masked adds).  What can go wrong: a block of the image in another block's place,
a part of a block left out or added twice, the ragged last tile read with a full tile's validity column (or a full one with the
ragged column), a slot offset added to a feature that does not live in the slot, the ring of three slots, the early signal of
the first image and the flush of the last two.

Against the float64 oracle with the tolerances and helpers of tests/test_gpu_steps.py and tests/test_gpu_steps_pace_paths.py
(loss 1e-5 relative at every step, every gradient leaf of the first step within 1e-4 of its own scale, parameters within 2 %
of one Adam step per step, Adam moments 2e-5 / 5e-5 of their scale); the scheduling-only property bitwise."""
import numpy as np
import pytest

from oracle import elbo_oracle as O
from tests.cases import build
from tests.gpu_util import engine_for, host
from tests.test_gpu_steps import _leafwise_grads_of_the_first_step, _problem, _run_pipelined
from tests.test_gpu_steps_chained import _assert_same, _batches, _chunks, _engine, _run, _state
from tests.test_gpu_steps_pace_paths import B_METRIC_MIN, _steps_against_the_oracle

pytestmark = pytest.mark.gpu

# 256 CUs: 231 streamers.  Batches of more than 231 x 256 = 59 136 rows (B_METRIC_MIN is that + 1) and of at most 231 x 288 take
# tiles of 288 rows -- the metric's instantiation; the smallest multiple of 288 among them is 206 x 288: full tiles only
B_METRIC_FULL = 59328
# the planted scales of the 16-feature blocks of [z1 | x | z2 | 1] at D = 12, L = 20: block 0 is z1[:, :16], block 1 is
# z1[:, 16:] and x, block 2 is z2 (and the constant feature, which has no scale)
PLANTED = (1.0, 8.0, 0.25)


def _against_the_oracle(cfg, B, p, batches, lr):
    """tests/test_gpu_steps_pace_paths.py's _steps_against_the_oracle on batches given by the caller"""
    n = len(batches)
    eng = engine_for(cfg, B)
    assert eng.supports_train_steps()
    _leafwise_grads_of_the_first_step(cfg, eng, p, batches[0], lr)
    params, grads, m, v, step, losses = _run_pipelined(eng, cfg, p, batches, lr)
    st = O.adam_init(p)
    want = []
    for i, (x, z1, z2) in enumerate(batches):
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, lr)
        want.append(loss)
        assert abs(losses[i] - loss) <= 1e-5 * abs(loss), (i, losses[i], loss)
    assert step == n
    got = host(grads)
    assert abs(got[eng.P] - loss) <= 1e-5 * abs(loss)
    assert abs(got[eng.P + 1] + got[eng.P + 2] - got[eng.P]) <= 1e-5 * abs(loss)
    assert np.max(np.abs(host(params) - O.flatten(cfg, p))) <= 0.02 * lr * n
    wm, wv = O.flatten(cfg, st["m"]), O.flatten(cfg, st["v"])
    assert np.max(np.abs(host(m) - wm)) <= 2e-5 * np.max(np.abs(wm)) + 1e-9
    assert np.max(np.abs(host(v) - wv)) <= 5e-5 * np.max(np.abs(wv)) + 1e-12
    return want


def test_metric_instantiation_on_full_tiles():
    """206 full tiles of 288 rows, one per streamer and batch: nothing ragged, every tile on the full validity column."""
    cfg, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, B_METRIC_FULL, 3, lr)


def test_metric_instantiation_with_a_ragged_last_tile_round_the_ring():
    """B = 59 137: the last tile has 97 of 288 rows.  Five steps are five items per streamer: the ring of three slots wraps, the
    first image is signalled early, the last two by the flush."""
    cfg, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, B_METRIC_MIN, 5, lr)


@pytest.mark.parametrize("B", [70000,                 # 274 tiles of 256 rows on 137 streamers, two each (the last one ragged)
                               66716])                # 261 tiles on 131 streamers: 130 take two per batch, the last one takes one
def test_more_than_one_tile_per_streamer_and_batch(B):
    """Above 231 x 288 rows a streamer takes several tiles of a batch (run-time instantiation): the slot, the item index
    and the image's batch advance at different rates, and with 261 tiles not at the same rate in every workgroup."""
    cfg, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, B, 3, lr)


@pytest.mark.parametrize("name", ["c1_linear_L20", "c1_linear_L2"])
def test_run_time_instantiation_on_two_tiles(name):
    """B = 300: two tiles of 256 rows, the second of 44.  L = 2 puts z1, x and z2 into the first two blocks (29 features): the
    blocks mix the tensors differently and the third block is the zero word."""
    cfg, dk, _, lr = build(name)
    _steps_against_the_oracle(cfg, dk, 300, 3, lr)


def test_planted_block_magnitudes_at_the_metric_instantiation():
    """Every 16-feature block of [z1 | x | z2] scaled by its own power of two (exact in float32: the products round as they did):
    the blocks of M then differ by factors of 4 to 1024 -- (0,0) x 1, (0,1) x 8, (1,1) x 64, (0,2) x 1/4, (1,2) x 2, (2,2) x 1/16 --
    so a block stored in another's place, or a half that is missing, moves the loss by far more than its 1e-5.  The oracle's loss
    on these batches is 2.7e3 .. 2.9e3 (asserted finite and in 1 .. 1e6)."""
    cfg, dk, _, lr = build("c1_linear_L20")
    p, batches = _problem(cfg, dk, B_METRIC_FULL, 3)
    s0, s1, s2 = PLANTED
    planted = []
    for x, z1, z2 in batches:
        z1 = z1.copy()
        z1[:, :16] *= s0
        z1[:, 16:] *= s1
        planted.append((np.ascontiguousarray(x * s1), z1, np.ascontiguousarray(z2 * s2)))
    want = _against_the_oracle(cfg, B_METRIC_FULL, p, planted, lr)
    assert all(np.isfinite(w) and 1.0 <= w <= 1e6 for w in want), want


def test_one_chained_call_equals_the_same_batches_in_two_calls():
    """70 steps in one call (two launches) against 50 + 20, bitwise, on the run-time instantiation's two tiles."""
    D, L, B, n = 12, 20, 300, 70
    seq = _batches(D, L, B, n)
    eng = _engine(D, L, B)
    want = _run(_engine(D, L, B), _state(eng, n + 8), _chunks(seq))
    got = _run(eng, _state(eng, n + 8), [seq])
    _assert_same(got, want, n)
