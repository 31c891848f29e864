"""What a Lanczos call on the Hessian of the sample-average ELBO of three-hidden-layer MLP VAEs costs, and where the time goes: the
script shape of sphere_vae_padding_expts.sh line 1 (200|200|200 both ways, D = L = 6, P = 166 019, -tdv), 1000 drawn sphere rows, 32
steps -- 6 + 6 * 32 = 198 launches per call, ceil(rows K / 8) chain tiles per model.  K in {1, 8} and N in {1, 3}, N = 3 at K = 1 only:
3 * 1000 * 8 columns is above the cap of 2^14.

    python tools/time_mlp3_hessian.py [--repeats 20] [--rows 1000] [--steps 32] > profiles/mlp3_hessian.txt

Per (K, N), after one warm-up, `repeats` calls; reported in us per CALL as min / median / max:
    wall        host wall time of an eager call, a synchronise on both sides (198 launches issued from the host)
    replay      the same call captured into a graph once and replayed
    device      the sum of the kernels' own begin / end times (the library's profile: one event pair per launch), split by label:
                chain = the chain launches (gradient + 32 tangent), contraction = the contraction launches, vector = the launches over
                chunks of P (init, four per step, Gram, final)
Beside it: the launches of vaek_train_step_grads_only at batch 100 on the same model (the float32 gradient of the same function at K = 1).
There is no earlier device path to compare with.  No time or ratio is a pass condition."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--steps", type=int, default=32)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import elbo_oracle as O  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

D, L, H, DD, PADDING = 6, 6, (200, 200, 200), 3, 3
GRID = ((1, 1), (1, 3), (8, 1))                  # (K, N)


def _stat(t):
    return f"{min(t):9.1f} {statistics.median(t):9.1f} {max(t):9.1f}"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_mlp3_hessian.py measures on the GPU: none found")
    eng = Engine(100, D, L, H, H, -3.0, True, False)
    cfg = O.Config(D, L, H, H, -3.0, True, "sphere")
    P, nmax = eng.P, max(n for _, n in GRID)
    params = torch.as_tensor(np.stack([O.flatten(cfg, O.init_params(cfg, seed=r), np.float32) for r in range(nmax)])).cuda()
    rng = np.random.default_rng(D)
    seeds = torch.arange(1, nmax + 1, dtype=torch.int64).cuda()
    steps = torch.ones(nmax, dtype=torch.int32).cuda()
    v0 = torch.as_tensor(rng.standard_normal((nmax, P))).cuda()
    for K, N in GRID:
        basis = torch.zeros(N, opt.steps, P, dtype=torch.float64, device="cuda")
        out = torch.zeros(N, eng.sampled_elbo_hessian_record_len, dtype=torch.float64, device="cuda")
        ws = torch.zeros(eng.mlp3_sampled_elbo_hessian_workspace(N, opt.rows, K), dtype=torch.uint8, device="cuda")
        draw = dict(samples=K, kind=2, A=None, dd=DD, did=DD, pad=PADDING, var_added=0.0, x_seeds=seeds[:N], x_steps=steps[:N],
                    z_seeds=seeds[:N], z_steps=steps[:N])
        call = lambda: eng.mlp3_sampled_elbo_hessian_lanczos_replicas(params[:N], opt.rows, opt.steps, v0[:N], basis, out, ws, **draw)
        call()                                                            # warm-up
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                call()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        wall, replay, chain, contract, vector = [], [], [], [], []
        for _ in range(opt.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            replay.append((time.perf_counter() - t0) * 1e6)
            eng.profile_begin(256)
            call()
            torch.cuda.synchronize()
            rep = eng.profile_report()
            us = lambda pick: sum(r["total_ms"] for name, r in rep.items() if pick(name)) * 1e3
            chain.append(us(lambda n: n.endswith("_chain")))
            contract.append(us(lambda n: n.endswith("_contract")))
            vector.append(us(lambda n: not n.endswith(("_chain", "_contract"))))
            assert sum(r["count"] for r in rep.values()) == 6 + 6 * opt.steps, rep
        rec = out.cpu().numpy()
        head = f"200|200|200 D/L {D}/{L} P {P} N={N} rows={opt.rows} K={K} steps={opt.steps}"
        print(f"{head} wall   us per call min/median/max {_stat(wall)}", flush=True)
        print(f"{head} replay us per call min/median/max {_stat(replay)}", flush=True)
        print(f"{head} device us per call min/median/max {_stat([a + b + c for a, b, c in zip(chain, contract, vector)])}; median split chain "
              f"{statistics.median(chain):9.1f}, contraction {statistics.median(contract):9.1f}, vector {statistics.median(vector):9.1f}; chain "
              f"tiles per model {(opt.rows * K + 7) // 8}; workspace {ws.numel() / 2 ** 20:.1f} MiB; k {rec[:, 2].min():.0f} .. {rec[:, 2].max():.0f}, "
              f"sampled sharpness of model 0 {rec[0, 9]:.6e}, omega max {rec[:, 11].max():.1e}", flush=True)
    # beside it: the training kernels' gradient of the same model at batch 100
    x = torch.as_tensor(rng.standard_normal((100, D)), dtype=torch.float32).cuda()
    z1 = torch.as_tensor(rng.standard_normal((100, L)), dtype=torch.float32).cuda()
    z2 = torch.zeros(100, D, device="cuda")
    grads, step = eng.new_flat(eng.grad_len), torch.zeros(1, dtype=torch.int32, device="cuda")
    flat = params[0].contiguous()
    eng.grads_only(flat, grads, step, x, z1, z2)
    torch.cuda.synchronize()
    tot, labels = [], {}
    for _ in range(opt.repeats):
        eng.profile_begin(16)
        eng.grads_only(flat, grads, step, x, z1, z2)
        torch.cuda.synchronize()
        rep = eng.profile_report()
        tot.append(sum(r["total_ms"] for r in rep.values()) * 1e3)
        labels = {name: r["count"] for name, r in rep.items()}
    print(f"vaek_train_step_grads_only, step path {eng.step_path}, batch 100, the same model: device us per call min/median/max {_stat(tot)}; "
          f"launches {labels}", flush=True)


if __name__ == "__main__":
    main()
