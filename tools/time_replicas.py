"""What R replicas in one launch cost: vaek_train_loop_gen_replicas on the six distinct shapes of sigmoid_vae_padding_expts.sh at the
reference's batch size, R = 1, 16, 64, 256, 512, against the way a sweep runs without it -- R vaek_train_loop_gen calls one
after another on the same stream, one workgroup each (that kernel is unchanged by the replica form, so the same build is its own
A/B):

    python tools/time_replicas.py [--shapes 0,1,2,3,4,5] [--batch 100] [--steps 1024] [--repeats 5] [--replicas 1,16,64,256,512]
                                  [--baseline_max 64]

Per shape and R: one warm-up call of each leg, then `repeats` timed calls of each, the legs ALTERNATED repeat by repeat; a timed
call trains `steps` steps of every replica and ends in a device synchronise.  Reported, min / median / max over the repeats:

    us/launch-step   wall time of the call / steps: what one step of the whole launch costs, however many replicas ride in it
    Msteps/s         aggregate model-steps per second, R * steps / wall time

The sequential leg runs R * steps steps, so it is timed only up to --baseline_max replicas (its per-replica cost does not depend
on R: every call is the same one-workgroup launch) and printed as `seq`.  The expectation this is here to confirm or refute: the
launch-step time at R <= 256 (one workgroup per CU) stays close to R = 1, and R = 512 costs about twice R = 256."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="0,1,2,3,4,5")
ap.add_argument("--batch", type=int, default=100)
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--replicas", default="1,16,64,256,512")
ap.add_argument("--baseline_max", type=int, default=64)
opt = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from vae_training_amd.engine import Engine  # noqa: E402

# (dd, pad, L) of the script's six distinct rows; D = dd + pad + 1, two decoders, epsilon -3, tunable decoder variance
SHAPES = [(3, 3, 6), (3, 13, 8), (5, 16, 16), (5, 5, 10), (7, 7, 13), (7, 20, 24)]
LR = 1e-4


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fmt(xs):
    return f"{min(xs):9.2f} {statistics.median(xs):9.2f} {max(xs):9.2f}"


for i in [int(s) for s in opt.shapes.split(",")]:
    dd, pad, L = SHAPES[i]
    D = dd + pad + 1
    eng = Engine(opt.batch, D, L, (), (), -3.0, True, True)
    assert eng.supports_train_loop_gen(1)
    for R in [int(s) for s in opt.replicas.split(",")]:
        g = torch.Generator().manual_seed(R)
        P, GL = eng.P, eng.grad_len
        p0 = (torch.randn(R, P, generator=g) * 0.3).cuda()
        A = torch.randn(R, dd, generator=g).cuda().contiguous()
        seeds = torch.arange(1, R + 1, dtype=torch.int64, device="cuda") * 7919
        new = lambda: [p0.clone(), torch.zeros(R, GL, device="cuda"), torch.zeros(R, P, device="cuda"), torch.zeros(R, P, device="cuda"),
                       torch.zeros(R, dtype=torch.int32, device="cuda")]
        rep, seq = new(), new()
        nb = eng.train_loop_replicas_workspace(R)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None

        def replicas():
            eng.train_loop_gen_replicas(*rep, opt.steps, LR, 1, A, dd, 1, pad, 0.0, seeds, a_stride=dd, workspace=ws)

        seeds_host = seeds.tolist()                        # host copies: no device read inside the timed window

        def sequential():
            for r in range(R):
                eng.train_loop_gen(seq[0][r], seq[1][r], seq[2][r], seq[3][r], seq[4][r:r + 1], opt.steps, LR, 1, A[r], dd, 1, pad, 0.0,
                                   seeds_host[r])

        legs = [("replicas", replicas)] + ([("seq", sequential)] if R <= opt.baseline_max else [])
        secs = {name: [] for name, _ in legs}
        for _, fn in legs:
            timed(fn)
        for _ in range(opt.repeats):
            for name, fn in legs:
                secs[name].append(timed(fn))
        for name, _ in legs:
            us = [s / opt.steps * 1e6 for s in secs[name]]
            rate = [R * opt.steps / s / 1e6 for s in secs[name]]
            print(f"D={D:2d} L={L:2d} B={opt.batch:3d} R={R:4d} {name:8s} us/launch-step min/median/max {fmt(us)}   "
                  f"Msteps/s min/median/max {fmt(rate)}", flush=True)
        finite = bool(torch.isfinite(rep[0]).all())
        same = R > opt.baseline_max or all(torch.equal(a, b) for a, b in zip(rep, seq))
        print(f"D={D:2d} L={L:2d} R={R:4d} finite {finite}; replicas bitwise equal to the sequential calls: "
              f"{same if R <= opt.baseline_max else 'not run'}", flush=True)
