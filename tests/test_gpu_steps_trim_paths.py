"""-m gpu: the item loops of the persistent streamers of vaek_train_steps (csrc/linear_moments.hip) -- one for the multiplying
waves and one for the loading waves, with the same barriers in both -- at the shapes and item counts where they take different
paths:

  * the metric instantiation (D = 12, L = 20, 288-row tiles) at its smallest batch, whose last tile is ragged, with 1, 2, 3, 4 and
    7 steps: with fewer than three items per streamer every item is a first or a last one (the counted wait of the first item has
    no image store to wait for, the last one's no pieces) and the trailing signals are the edge cases;
  * the benchmark's exact shape;
  * the run-time instantiation with one tile per streamer (a ragged last tile) and with two tiles per streamer;
  * a model whose tile rows are a few bytes (D = 3, L = 2) and the four-block instantiations (the other translation unit).

Each shape against the float64 oracle with tests/test_gpu_steps.py's tolerances (loss 1e-5 relative, parameters within 2 % of one
Adam step per step, Adam moments 2e-5 / 5e-5 of their scale), and CHAINED: one call of K steps is bitwise the same as the same
batches given in two calls.  The drawing form against vaek_make_batch + vaek_train_steps, bitwise."""
import functools

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O

pytestmark = pytest.mark.gpu

B_METRIC_MIN = 59137            # 231 x 256 + 1 rows -> tiles of 288 rows, 206 of them, the last one of 97 rows

#        D   L   B             K (steps)           what it reaches (on the 256 compute units of the MI355X)
SHAPES = [(12, 20, B_METRIC_MIN, (1, 2, 3, 4, 7)),   # the metric instantiation: 206 tiles of 288 rows, the last one ragged, one per streamer
          (12, 20, 65536, (3,)),                    # the benchmark's shape: 228 tiles of 288 rows
          (12, 20, 1000, (5,)),                     # run-time instantiation: 4 tiles of 256 rows, the last one ragged
          (12, 20, 70000, (3,)),                    # 274 tiles of 256 rows: two per streamer
          (3, 2, 777, (4,)),                        # rows of 8 and 12 bytes
          (20, 20, 300, (3,))]                      # four blocks: 2 tiles of 192 rows, the other translation unit
CASES = [(D, L, B, K) for (D, L, B, Ks) in SHAPES for K in Ks]


def _cfg(D, L):
    return O.Config(D, L, (), (), -1.0, True, "linear_gaussian")


@functools.lru_cache(maxsize=None)
def _reference(D, L, B):
    """One problem per shape and the oracle's trajectory over its longest K: (cfg, p0, batches, [(params, adam state, loss)])"""
    from tests.test_gpu_steps import _problem
    cfg = _cfg(D, L)
    n = max(K for (d, l, b, K) in CASES if (d, l, b) == (D, L, B))
    p0, batches = _problem(cfg, dict(name="linear_gaussian", seed=2, dd=3, did=3, pad=D - 3), B, n)
    traj, p, st = [], p0, O.adam_init(p0)
    for (x, z1, z2) in batches:
        p, st, loss = O.train_step(cfg, p, st, x, z1, z2, 1e-3)
        traj.append((O.flatten(cfg, p), O.flatten(cfg, st["m"]), O.flatten(cfg, st["v"]), loss))
    return cfg, p0, batches, traj


@pytest.mark.parametrize("D,L,B,K", CASES)
def test_k_steps_against_the_oracle_and_in_two_calls(D, L, B, K):
    from tests.gpu_util import dev, engine_for, host
    lr = 1e-3
    cfg, p0, batches, traj = _reference(D, L, B)
    eng = engine_for(cfg, B)
    assert eng.supports_train_steps()
    dbat = [tuple(dev(a) for a in b) for b in batches[:K]]

    def run(calls):
        st = [dev(O.flatten(cfg, p0)), eng.new_flat(eng.grad_len), eng.new_flat(), eng.new_flat(),
              torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(K + 8, dtype=torch.float32, device="cuda")]
        eng.set_loss_history(st[5])
        for call in calls:
            eng.train_steps(*st[:5], call, lr)
        torch.cuda.synchronize()
        eng.set_loss_history(None)
        assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
        return st

    got = run([dbat])
    params, grads, m, v, step, ring = got
    assert int(step.item()) == K
    losses = host(ring)[:K]
    for i in range(K):
        assert abs(losses[i] - traj[i][3]) <= 1e-5 * abs(traj[i][3]), (i, losses[i], traj[i][3])
    wp, wm, wv, loss = traj[K - 1]
    g = host(grads)
    assert abs(g[eng.P] - loss) <= 1e-5 * abs(loss)
    assert abs(g[eng.P + 1] + g[eng.P + 2] - g[eng.P]) <= 1e-5 * abs(loss)          # loss = mean Dkl + mean mse
    assert np.max(np.abs(host(params) - wp)) <= 0.02 * lr * K
    assert np.max(np.abs(host(m) - wm)) <= 2e-5 * np.max(np.abs(wm)) + 1e-9
    assert np.max(np.abs(host(v) - wv)) <= 5e-5 * np.max(np.abs(wv)) + 1e-12
    if K >= 2:          # chained: the same batches in two calls (the second call's streamers start in the slot the first one's left)
        from tests.test_gpu_steps_chained import _assert_same
        _assert_same(run([dbat[:K // 2], dbat[K // 2:]]), got, K)


def test_drawing_form_equals_loaded_form_over_three_steps():
    """vaek_train_steps_gen, three steps at the metric instantiation's ragged batch: the streamers that DRAW their tiles multiply
    the bits of vaek_make_batch + vaek_train_steps."""
    from tests.test_gpu_steps_chained import _assert_same, _engine, _run, _state
    D, L, B, n = 12, 20, B_METRIC_MIN, 3
    eng = _engine(D, L, B)
    kind, dd, did, var, seed, tag, row0 = 0, 3, 3, 0.25, 77, 5, 1000
    assert eng.supports_train_steps_gen(kind)
    A = torch.randn(dd, did, generator=torch.Generator().manual_seed(11)).cuda().contiguous()
    got = _state(eng, n + 8)
    eng.set_loss_history(got[5])
    eng.train_steps_gen(*got[:5], n, 1e-3, kind, A, dd, did, D - dd, var, seed, tag=tag, row0=row0)
    torch.cuda.synchronize()
    eng.set_loss_history(None)
    assert not eng.train_steps_gave_up(), hex(eng.train_steps_status_word)
    seq = [eng.make_batch(kind, A, dd, did, D - dd, var, B, seed, step=t, tag=tag, row0=row0) for t in range(n)]
    want = _run(eng, _state(eng, n + 8), [seq])
    _assert_same(got, want, n)
