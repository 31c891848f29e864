"""What a Lanczos call on the Hessian of the exact ELBO costs, and where the time goes: N = 1, 64, 256 one-decoder linear VAEs of
D / L = 12 / 20 (P = 533) and 32 / 32 (P = 2145), -tdv, 1000 drawn linear_gaussian rows, 32 steps -- one workgroup per model.

    python tools/time_elbo_hessian.py [--replicas 1,64,256] [--repeats 20] [--rows 1000] [--steps 32] > profiles/elbo_hessian.txt

Per shape and N, after one warm-up of every leg, `repeats` calls of each leg ALTERNATED call by call; the time of a call is the
kernel's own begin / end (the library's profile: one event pair per launch), reported as min / median / max in us, next to the host
wall time per call of the Lanczos leg (a synchronise on both sides).  The legs and what their differences say:

    setup1      vaek_elbo_hvp_replicas, nvec = 0, 1 row        parameter images, R, S R, gradient, record: everything but the rows
    setup       vaek_elbo_hvp_replicas, nvec = 0               ... plus the moments of `rows` rows:      moments = setup - setup1
    hvp32       vaek_elbo_hvp_replicas, nvec = 32              ... plus 32 products H v (global in/out): HVPs    = hvp32 - setup
    lanczos     vaek_elbo_hessian_lanczos_replicas, 32 steps   ... plus reorthogonalisation, the solve of T and omega:
                                                                                                         vectors = lanczos - hvp32
There is no earlier device path to compare with.  No time or ratio is a pass condition."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,64,256")
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--steps", type=int, default=32)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

SHAPES = ((12, 20, 3, 9), (32, 32, 16, 16))      # D, L, dd = did, pad
LABEL = {"setup1": "elbo_hvp_replicas", "setup": "elbo_hvp_replicas", "hvp32": "elbo_hvp_replicas", "lanczos": "elbo_hessian_replicas"}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_elbo_hessian.py measures on the GPU: none found")
    reps = [int(s) for s in opt.replicas.split(",")]
    for D, L, dd, pad in SHAPES:
        eng = Engine(100, D, L, (), (), -1.0, True, False)
        P, nmax = eng.P, max(reps)
        rng = np.random.default_rng(D)
        th = (0.3 * rng.standard_normal((nmax, P))).astype(np.float32)
        th[:, -1] = 1.0
        params = torch.as_tensor(th).cuda()
        A = torch.as_tensor(rng.standard_normal((nmax, dd * dd)), dtype=torch.float32).cuda()
        seeds = torch.arange(1, nmax + 1, dtype=torch.int64).cuda()
        steps = torch.ones(nmax, dtype=torch.int32).cuda()
        v0 = torch.as_tensor(rng.standard_normal((nmax, P))).cuda()
        v = torch.as_tensor(rng.standard_normal((32, P))).cuda()
        for N in reps:
            hv = torch.zeros(N, 32, P, dtype=torch.float64, device="cuda")
            rec = torch.zeros(N, 4, dtype=torch.float64, device="cuda")
            basis = torch.zeros(N, opt.steps, P, dtype=torch.float64, device="cuda")
            out = torch.zeros(N, eng.elbo_hessian_record_len, dtype=torch.float64, device="cuda")
            draw = dict(kind=0, A=A[:N], dd=dd, did=dd, pad=pad, var_added=0.01, x_seeds=seeds[:N], x_steps=steps[:N], a_stride=dd * dd)
            legs = {
                "setup1": lambda: eng.elbo_hvp_replicas(params[:N], 1, rec, **draw),
                "setup": lambda: eng.elbo_hvp_replicas(params[:N], opt.rows, rec, **draw),
                "hvp32": lambda: eng.elbo_hvp_replicas(params[:N], opt.rows, rec, v=v, hv=hv, **draw),
                "lanczos": lambda: eng.elbo_hessian_lanczos_replicas(params[:N], opt.rows, opt.steps, v0[:N], basis, out, **draw),
            }
            for fn in legs.values():                                      # warm-up of every leg
                fn()
            torch.cuda.synchronize()
            us, wall = {name: [] for name in legs}, []
            for _ in range(opt.repeats):
                for name, fn in legs.items():
                    eng.profile_begin(4)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if name == "lanczos":
                        wall.append((time.perf_counter() - t0) * 1e6)
                    r = eng.profile_report()[LABEL[name]]
                    us[name].append(r["total_ms"] / r["count"] * 1e3)
            med = {name: statistics.median(t) for name, t in us.items()}
            rec_h = out.cpu().numpy()
            for name, t in us.items():
                print(f"D/L {D}/{L} P {P} N={N:4d} rows={opt.rows} {name:8s} device us per call min/median/max {min(t):9.1f} {med[name]:9.1f} {max(t):9.1f}",
                      flush=True)
            tot = med["lanczos"]
            parts = dict(fixed=med["setup1"], moments=med["setup"] - med["setup1"], HVPs=med["hvp32"] - med["setup"], vectors=tot - med["hvp32"])
            print(f"D/L {D}/{L} P {P} N={N:4d} lanczos host wall us per call median {statistics.median(wall):9.1f}; split of the median "
                  + ", ".join(f"{k} {p:8.1f} us ({100.0 * p / tot:4.1f}%)" for k, p in parts.items())
                  + f"; k {rec_h[:, 2].min():.0f} .. {rec_h[:, 2].max():.0f}, sharpness of model 0 {rec_h[0, 9]:.6e}, omega max {rec_h[:, 11].max():.1e}",
                  flush=True)


if __name__ == "__main__":
    main()
