"""-m gpu: the paths of the persistent vaek_train_steps launch that the updater's output map and the launch boundary touch
(csrc/linear_moments.hip), on each kernel instantiation:

  * the updater's output map (LinUpdM::out_index: the loss slots and epsilon alone on lanes of the last wave, the left-over plain
    outputs -- the log-variance lanes among them -- as second outputs of the wave in front of it; one exponential per thread when the
    parameters are published) on the metric's instantiation (D = 12, L = 20, 288-row tiles) at its SMALLEST batch, whose last
    tile is ragged (97 of 288 rows), on the run-time instantiation, and with and without the tunable decoder variance
    (off_eps < 0: four special outputs instead of five);
  * the batches carried from one launch of a call to the next (kLinCarry: the updater starts four batches behind its streamers);
  * the drawing form multiplies the same tiles as the loaded one: bitwise equal at the metric instantiation's ragged batch.

Against the float64 oracle with tests/test_gpu_steps.py's tolerances and helpers (loss 1e-5 relative, parameters within 2 % of one
Adam step per step, every gradient leaf within 1e-4 of its own scale); scheduling-only properties bitwise."""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests.cases import build
from tests.gpu_util import engine_for, host
from tests.test_gpu_steps import _leafwise_grads_of_the_first_step, _problem, _run_pipelined
from tests.test_gpu_steps_chained import _assert_same, _batches, _chunks, _engine, _run, _state

pytestmark = pytest.mark.gpu

B_METRIC_MIN = 59137            # 256 CUs: 231 streamers x 256 rows + 1 -> tiles of 288 rows, 206 of them, the last one of 97 rows


def _steps_against_the_oracle(cfg, dk, B, n, lr):
    p, batches = _problem(cfg, dk, B, n)
    eng = engine_for(cfg, B)
    assert eng.supports_train_steps()
    _leafwise_grads_of_the_first_step(cfg, eng, p, batches[0], lr)
    params, grads, m, v, step, losses = _run_pipelined(eng, cfg, p, batches, lr)
    st = O.adam_init(p)
    for i, (x, z1, z2) in enumerate(batches):
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, lr)
        assert abs(losses[i] - loss) <= 1e-5 * abs(loss), (i, losses[i], loss)
    assert step == n
    got = host(grads)
    assert abs(got[eng.P] - loss) <= 1e-5 * abs(loss)
    assert got[eng.P + 3] == 0.0 and np.isfinite(got[eng.P + 1]) and np.isfinite(got[eng.P + 2])
    assert abs(got[eng.P + 1] + got[eng.P + 2] - got[eng.P]) <= 1e-5 * abs(loss)          # loss = mean Dkl + mean mse
    assert np.max(np.abs(host(params) - O.flatten(cfg, p))) <= 0.02 * lr * n
    wm, wv = O.flatten(cfg, st["m"]), O.flatten(cfg, st["v"])
    assert np.max(np.abs(host(m) - wm)) <= 2e-5 * np.max(np.abs(wm)) + 1e-9
    assert np.max(np.abs(host(v) - wv)) <= 5e-5 * np.max(np.abs(wv)) + 1e-12
    return eng


def test_metric_instantiation_at_its_smallest_batch_with_a_ragged_last_tile():
    cfg, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, B_METRIC_MIN, 3, lr)


def test_the_same_model_on_the_run_time_instantiation():
    cfg, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, 300, 3, lr)           # two tiles of 256 rows, the second of 44


def test_the_fixed_decoder_variance_fixture():
    cfg, dk, B, lr = build("linear_notdv")
    assert B == 8 and not cfg.tdv
    _steps_against_the_oracle(cfg, dk, B, 3, lr)


@pytest.mark.parametrize("B", [8, 300])
def test_the_same_model_without_the_tunable_decoder_variance(B):
    """D = 12, L = 20 without epsilon among the parameters: off_eps < 0, four special outputs instead of five."""
    cfg = O.Config(12, 20, (), (), -1.0, False, "linear_gaussian")
    _, dk, _, lr = build("c1_linear_L20")
    _steps_against_the_oracle(cfg, dk, B, 3, lr)


def test_batches_carried_across_a_launch_boundary():
    """64 + carry + 3 steps in one call (two launches: the second one's updater starts on the four batches the first one left it)
    against the same batches 50 at a time; then the same call AGAIN on the same workspace against a fresh context's -- it can only
    be equal if every arrival counter was left zero."""
    D, L, B, n = 12, 20, 3000, 64 + 4 + 3
    seq = _batches(D, L, B, n)
    eng = _engine(D, L, B)
    want = _run(_engine(D, L, B), _state(eng, n + 8), _chunks(seq))
    got = _run(eng, _state(eng, n + 8), [seq])              # (_run asserts that no bounded wait expired)
    _assert_same(got, want, n)
    again = _run(eng, _state(eng, n + 8), [seq])
    _assert_same(again, want, n)


def test_drawing_form_equals_loaded_form_at_the_metric_instantiation():
    """One step at the metric instantiation's smallest batch: the streamers that DRAW their tiles multiply the same bits as the
    ones that load what vaek_make_batch wrote."""
    D, L, B = 12, 20, B_METRIC_MIN
    eng = _engine(D, L, B)
    kind, dd, did, var, seed, tag, row0 = 0, 3, 3, 0.25, 77, 5, 1000
    assert eng.supports_train_steps_gen(kind)
    A = torch.randn(dd, did, generator=torch.Generator().manual_seed(11)).cuda().contiguous()
    got = _state(eng, 9)
    eng.set_loss_history(got[5])
    eng.train_steps_gen(*got[:5], 1, 1e-3, kind, A, dd, did, D - dd, var, seed, tag=tag, row0=row0)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    batch = eng.make_batch(kind, A, dd, did, D - dd, var, B, seed, step=0, tag=tag, row0=row0)
    want = _run(eng, _state(eng, 9), [[batch]])
    _assert_same(got, want, 1)
