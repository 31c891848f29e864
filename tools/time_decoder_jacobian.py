"""What a decoder-Jacobian event costs: R three-hidden-layer MLP VAEs (200|200|200 both ways) of the five shapes of
sphere_vae_padding_expts.sh, 1000 latent rows, R = 1 and 3, evaluated two ways on the same device:

    torch   for each model: the decoder restated with torch ops, torch.autograd.functional.jacobian of its row sum over the 1000 rows
            (rows are independent, so that is every row's J at once), G = J^T J in float64 and a batched torch.linalg.eigvalsh --
            what a user of the package would write today --, then the means over the rows, read back per model
    fused   one vaek_mlp3_decoder_jacobian_replicas call (three launches) and one device -> host copy of the R model records

    python tools/time_decoder_jacobian.py [--replicas 1,3] [--repeats 9] [--rows 1000]

Per (shape, R): one warm-up event of each leg, then `repeats` timed events of each, the legs ALTERNATED repeat by repeat.  A timed event
starts after a device synchronise and ends in one with the results on the host.  Reported: min / median / max of the wall time per event
in ms, and the two legs' mean spectra of model 0 (the legs draw different latents: close, not equal).  Nothing is promised and no
bound is set: the figures go to profiles/decoder_jacobian.txt and DESIGN 3.20."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--rows", type=int, default=1000)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import elbo_oracle as O  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

H = (200, 200, 200)
SCRIPT_ROWS = [(3, 3, 6), (3, 13, 8), (5, 16, 16), (5, 5, 10), (7, 7, 13)]       # (dd, pad, L) of sphere_vae_padding_expts.sh
TOL = 1e-4


def torch_event(views, L, rows):
    out = []
    for p in views:
        layers = [(p["Decoder"][f"FC{i}"]["kernel"], p["Decoder"][f"FC{i}"]["bias"]) for i in range(4)]

        def dec_sum(z):
            h = z
            for i, (W, b) in enumerate(layers):
                h = h @ W + b
                if i < 3:
                    h = torch.relu(h)
            return h.sum(0)
        z = torch.randn(rows, L, device="cuda")
        J = torch.autograd.functional.jacobian(dec_sum, z, vectorize=True).permute(1, 0, 2).double()      # [rows, D, L]
        G = J.transpose(1, 2) @ J
        lam = torch.linalg.eigvalsh(G).flip(-1)
        rank = (lam > TOL * lam[:, :1]).sum(1).double()
        out.append((lam.mean(0).cpu(), torch.diagonal(G, dim1=1, dim2=2).mean(0).cpu(), float(rank.mean())))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for dd, pad, L in SCRIPT_ROWS:
    D = dd + pad
    cfg = O.Config(D, L, H, H, -3.0, True, None)
    eng = Engine(100, D, L, H, H, -3.0, True, False)
    assert eng.supports_mlp3_decoder_jacobian()
    for R in [int(s) for s in opt.replicas.split(",")]:
        params = torch.stack([torch.as_tensor(O.flatten(cfg, O.init_params(cfg, seed=r), np.float32)) for r in range(R)]).cuda().contiguous()
        views = [eng.views(params[r]) for r in range(R)]
        out = torch.zeros(R, eng.decoder_jacobian_record_len, dtype=torch.float64, device="cuda")
        ws = torch.empty(eng.mlp3_decoder_jacobian_workspace(R, opt.rows), dtype=torch.uint8, device="cuda")
        seeds = torch.arange(1, R + 1, dtype=torch.int64, device="cuda")
        steps = torch.ones(R, dtype=torch.int32, device="cuda")

        def fused_event():
            eng.mlp3_decoder_jacobian_replicas(params, opt.rows, out, ws, z_seeds=seeds, z_steps=steps, rank_tol=TOL, z_tag=8)
            return out.cpu().numpy()
        legs = [("torch", lambda: torch_event(views, L, opt.rows)), ("fused", fused_event)]
        secs = {name: [] for name, _ in legs}
        for _, fn in legs:
            timed(fn)
        last = {}
        for _ in range(max(opt.repeats, 3)):
            for name, fn in legs:
                s, last[name] = timed(fn)
                secs[name].append(s)
        for name, _ in legs:
            ms_ = [s * 1e3 for s in secs[name]]
            print(f"D={D:3d} L={L:3d} R={R:2d} rows={opt.rows} {name:5s} ms/event min/median/max {min(ms_):9.3f} {statistics.median(ms_):9.3f} "
                  f"{max(ms_):9.3f}", flush=True)
        print(f"D={D:3d} L={L:3d} R={R:2d} model 0 mean rank: torch {last['torch'][0][2]:.3f} fused {last['fused'][0][1]:.3f}; largest mean "
              f"eigenvalue: torch {float(last['torch'][0][0][0]):.4f} fused {last['fused'][0][8]:.4f}", flush=True)
