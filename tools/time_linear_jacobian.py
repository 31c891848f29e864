"""What a decoder-Jacobian call of linear VAEs costs: vaek_linear_decoder_jacobian_replicas (two launches) on two-decoder models of
(D, L) = (7, 6) -- line 1 of sigmoid_vae_padding_expts.sh -- and (28, 24) -- line 6, the D cap --, 1000 drawn latent rows, N = 1 and 3.

    python tools/time_linear_jacobian.py [--replicas 1,3] [--repeats 9] [--calls 200] [--rows 1000] [--out profiles/linear_jacobian.txt]

Per (shape, N): a warm-up window, then `repeats` timed windows of `calls` back-to-back calls each; a window starts after a device
synchronise and ends in one, so the figure is the device's time per call with the launches of a window queued behind each other (a
window of 200 calls lasts tens of milliseconds).  One more leg times a single call followed by the device -> host copy of the N model
records: what an n_print event waits for.  Reported: min / median / max over the windows in microseconds per call, and the profile
counters' view of the two launches (vaek_profile: device time per launch label).  Nothing existing does this job -- the models had no
decoder-Jacobian call -- so there is nothing to be faster than: figures to record, not a threshold.  They go to
profiles/linear_jacobian.txt and DESIGN 3.26."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--replicas", default="1,3")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rows", type=int, default=1000)
ap.add_argument("--out", default=None)
opt = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle import elbo_oracle as O  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

SHAPES = [(7, 6), (28, 24)]
TOL = 1e-4
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


say(f"vaek_linear_decoder_jacobian_replicas, two decoders, {opt.rows} drawn latent rows, rank_tol {TOL:g}; us per call, min / median / max over "
    f"{max(opt.repeats, 3)} windows of {opt.calls} calls ({torch.cuda.get_device_name(0)})")
for D, L in SHAPES:
    cfg = O.Config(D, L, (), (), -3.0, True, "sigmoid")
    eng = Engine(100, D, L, (), (), -3.0, True, True)
    assert eng.supports_linear_decoder_jacobian()
    for R in [int(s) for s in opt.replicas.split(",")]:
        rng = np.random.default_rng(R)
        flats = []
        for r in range(R):
            p = O.init_params(cfg, seed=r)
            p["SigDecoder/FC0/kernel"] = rng.standard_normal(p["SigDecoder/FC0/kernel"].shape)      # u reaches both parts of the sigmoid
            flats.append(torch.as_tensor(O.flatten(cfg, p, np.float32)))
        params = torch.stack(flats).cuda().contiguous()
        out = torch.zeros(R, eng.decoder_jacobian_record_len, dtype=torch.float64, device="cuda")
        ws = torch.empty(eng.linear_decoder_jacobian_workspace(R, opt.rows), dtype=torch.uint8, device="cuda")
        seeds = torch.arange(1, R + 1, dtype=torch.int64, device="cuda")
        steps = torch.ones(R, dtype=torch.int32, device="cuda")

        def call():
            eng.linear_decoder_jacobian_replicas(params, opt.rows, out, ws, z_seeds=seeds, z_steps=steps, rank_tol=TOL, z_tag=8)

        def event():
            call()
            return out.cpu()

        for name, fn, calls in (("queued calls", call, opt.calls), ("call + readback", event, max(opt.calls // 10, 1))):
            window(fn, calls)                            # warm-up
            us = [window(fn, calls) for _ in range(max(opt.repeats, 3))]
            say(f"D={D:3d} L={L:3d} N={R:2d} rows={opt.rows} {name:15s} us/call min/median/max {min(us):9.1f} {statistics.median(us):9.1f} {max(us):9.1f}")
        eng.profile_begin()
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        rep = eng.profile_report()
        say(f"D={D:3d} L={L:3d} N={R:2d} per launch over 20 profiled calls: " + "; ".join(
            f"{k} " + ", ".join(f"{kk}={vv:.4g}" if isinstance(vv, float) else f"{kk}={vv}" for kk, vv in v.items()) for k, v in sorted(rep.items())))
        rec = out.cpu().numpy()
        say(f"D={D:3d} L={L:3d} N={R:2d} model 0: mean / min / max rank {rec[0, 1]:.3f} {rec[0, 2]:.0f} {rec[0, 3]:.0f}, max sweeps {rec[0, 5]:.0f}, "
            f"largest mean eigenvalue {rec[0, 8]:.4f}")
if opt.out:
    with open(os.path.join(ROOT, opt.out) if not os.path.isabs(opt.out) else opt.out, "w") as f:
        f.write("\n".join(lines) + "\n")
