"""What a Lanczos call on the Hessian of the sample-average ELBO costs, and where the time goes: N = 1 and 8 two-decoder linear VAEs
of the script shape sigmoid_dd7_pd20_ld_24 (D / L = 28 / 24, P = 2121, -tdv), 1000 drawn sigmoid rows, K = 8 and K = 64 drawn samples
per row, 32 steps -- 3 + 2 * 32 = 67 launches per call, ceil(rows K / 256) column tiles per model.

    python tools/time_sampled_hessian.py [--replicas 1,8] [--samples 8,64] [--repeats 20] [--rows 1000] [--steps 32] > profiles/sampled_hessian.txt

Per K and N, after one warm-up, `repeats` calls; reported in us per CALL as min / median / max:
    wall        host wall time of an eager call, a synchronise on both sides (67 launches issued from the host)
    replay      the same call captured into a graph once and replayed
    device      the sum of the kernels' own begin / end times (the library's profile: one event pair per launch), split by label:
                tiles = the column-tile launches (gradient + 32 H v), steps = the per-replica Lanczos launches (init, 32 steps, final)
There is no earlier device path to compare with.  No time or ratio is a pass condition."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,8")
ap.add_argument("--samples", default="8,64")
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--steps", type=int, default=32)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

D, L, DD, PADDING = 28, 24, 7, 20


def _stat(t):
    return f"{min(t):9.1f} {statistics.median(t):9.1f} {max(t):9.1f}"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_sampled_hessian.py measures on the GPU: none found")
    reps, ks = [int(s) for s in opt.replicas.split(",")], [int(s) for s in opt.samples.split(",")]
    eng = Engine(100, D, L, (), (), -3.0, True, True)
    P, nmax = eng.P, max(reps)
    rng = np.random.default_rng(D)
    th = (0.3 * rng.standard_normal((nmax, P))).astype(np.float32)
    th[:, -1] = 1.0
    params = torch.as_tensor(th).cuda()
    A = torch.as_tensor(rng.standard_normal((nmax, DD)), dtype=torch.float32).cuda()
    seeds = torch.arange(1, nmax + 1, dtype=torch.int64).cuda()
    steps = torch.ones(nmax, dtype=torch.int32).cuda()
    v0 = torch.as_tensor(rng.standard_normal((nmax, P))).cuda()
    for K in ks:
        for N in reps:
            basis = torch.zeros(N, opt.steps, P, dtype=torch.float64, device="cuda")
            out = torch.zeros(N, eng.sampled_elbo_hessian_record_len, dtype=torch.float64, device="cuda")
            ws = torch.zeros(eng.sampled_elbo_hessian_workspace(N, opt.rows, K), dtype=torch.uint8, device="cuda")
            draw = dict(samples=K, kind=1, A=A[:N], dd=DD, did=1, pad=PADDING, var_added=0.0, x_seeds=seeds[:N], x_steps=steps[:N],
                        z_seeds=seeds[:N], z_steps=steps[:N], a_stride=DD)
            call = lambda: eng.sampled_elbo_hessian_lanczos_replicas(params[:N], opt.rows, opt.steps, v0[:N], basis, out, ws, **draw)
            call()                                                        # warm-up
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    call()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            wall, replay, tiles, vectors = [], [], [], []
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
                eng.profile_begin(128)
                call()
                torch.cuda.synchronize()
                rep = eng.profile_report()
                tiles.append(sum(r["total_ms"] for name, r in rep.items() if name.endswith("_tiles")) * 1e3)
                vectors.append(sum(r["total_ms"] for name, r in rep.items() if "lanczos" in name) * 1e3)
                assert sum(r["count"] for r in rep.values()) == 3 + 2 * opt.steps, rep
            rec = out.cpu().numpy()
            head = f"D/L {D}/{L} two decoders P {P} N={N:3d} rows={opt.rows} K={K:3d} steps={opt.steps}"
            print(f"{head} wall   us per call min/median/max {_stat(wall)}", flush=True)
            print(f"{head} replay us per call min/median/max {_stat(replay)}", flush=True)
            print(f"{head} device us per call min/median/max {_stat([a + b for a, b in zip(tiles, vectors)])}; median split tiles "
                  f"{statistics.median(tiles):9.1f}, steps {statistics.median(vectors):9.1f}; tiles per model {(opt.rows * K + 255) // 256}; "
                  f"k {rec[:, 2].min():.0f} .. {rec[:, 2].max():.0f}, sampled sharpness of model 0 {rec[0, 9]:.6e}, omega max {rec[:, 11].max():.1e}",
                  flush=True)


if __name__ == "__main__":
    main()
