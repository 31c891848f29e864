"""Graph-captured training loop: the reference's hot loop (model.py:221-222 -- get_batch, sample_latent,
train_step, append loss) with NOTHING on the host per step.

The launches of a step -- the Philox dataset + latent draw (K7) and the two kernels of vaek_train_step --
are captured G steps at a time into a hipGraph; the Adam step counter, the RNG step and the loss ring
buffer all live on the device, so replays need no arguments.  At the reference's own batch size (100)
the per-step Python of the drop-in path (~50 us) is 3-4x the GPU time; this loop removes it without
changing what a step computes.

`pipeline=True` (default) draws batch n+1 WHILE step n trains (vaek_train_step_gen): the draw does not
depend on the weights, so its work items ride in the finalize launch of step n -- which by itself keeps
9 of 256 CUs busy -- and write the other of two batch buffers; at <= 256 rows the whole step, draw included,
is ONE launch (10 us per step at the reference's batch size 100).  The draw takes its step from a counter pair the
generator advances itself, not from the Adam step counter that same launch is incrementing.  Same
counters, same Philox streams: losses and parameters are bit-identical to `pipeline=False`
(vaek_make_batch, then vaek_train_step).  (A second stream / parallel graph branch for the draw was
measured first: cross-branch edges of a hipGraph cost far more than the 7 us they were meant to hide.)

`moments` (default: whenever the model qualifies -- a linear VAE on the linear_gaussian or sphere dataset): the steps go through
vaek_train_steps_gen, the headline kernel of bench.py (csrc/linear_moments.hip): up to 64 steps per persistent launch, every
step's batch drawn INSIDE the launch by the workgroups that multiply it -- the same Philox counters as above, so the same
batches bit for bit, but no batch buffer, no hipGraph and nothing per step on the host: one library call per run of steps
between two events of the reference's schedule (stats every 5 000, plot + save every 50 000: model.py:213-220).  The losses land
in the same device ring.  Losses and parameters agree with the per-sample loop to summation order (tests/test_gpu_loop.py).

`resident` (default: RESIDENT_DEFAULT where the model has no moments path and the engine supports it -- small-batch linear VAEs the
moment form does not cover: the two-decoder models of the sigmoid dataset above all; `moments=False` on a model that HAS a moments
path still means the hipGraph loop, resident=True asks for this one there too): the steps go through vaek_train_loop_gen
(csrc/linear_resident.hip), a plain loop of steps inside ONE workgroup with parameters and Adam state on chip and the batches drawn
in the kernel -- the same Philox counters again.  Like the moments path it is one library call per run of steps, no batch buffer and
no hipGraph; there is one workgroup, so there is nothing to wait for and check() has nothing to poll.  `moments` keeps priority:
every model that takes it today still does.

ReplicaLoop (below GraphLoop) is the resident loop for a SWEEP: R models of one shape, one workgroup each, in one launch per run of
steps (vaek_train_loop_gen_replicas); `run.py --sweep_dataset_seeds` drives it.  ReplicaGraphLoop (below it) is the sweep of the
models the resident loop does not cover but the whole-network "mlp3" step does: the pipelined hipGraph loop with every step ONE
vaek_train_step_gen_replicas call for all R models.

`trajectory_every=K` (GraphLoop with the resident loop, ReplicaLoop; opt-in): the resident kernel records, at every Adam step t with
t % K == 0, the parameters that step's gradient was evaluated at and the step's gradient buffer, into a device ring the loop owns
(vaek_train_loop_gen_traj / vaek_train_loop_gen_replicas_traj) -- the reference's `params_and_gradients` list (vae.py:207), which
the reference never fills.  `trajectory()` / `trajectory(r)` returns them in step order; run() stays one library call."""
from __future__ import annotations

import numpy as np
import torch


def _trajectory_capacity(loop_name, models, every, capacity):
    """Records per ring: every recorded step of the longest schedule among the models, ceil(num_batches / K), unless given."""
    if int(every) < 1:
        raise RuntimeError(f"{loop_name}(trajectory_every={every}): need an integer >= 1")
    if capacity is not None:
        if int(capacity) < 1:
            raise RuntimeError(f"{loop_name}(trajectory_capacity={capacity}): need an integer >= 1")
        return int(capacity)
    nb = max(int(getattr(m, "num_batches", 0) or 0) for m in models)
    if nb < 1:
        raise RuntimeError(f"{loop_name}(trajectory_every={every}): the model has no num_batches to size the ring by; pass trajectory_capacity")
    return -(-nb // int(every))


def _trajectory_view(ring, every, first_step, last_step, P):
    """(steps, params [n, P], grads [n, P + 4]) of the records a ring [cap, >= 2 P + 4] (already on the host) holds for the Adam steps
    first_step < t <= last_step with t % every == 0, oldest first: the last `cap` of them, each from slot (t // every - 1) % cap."""
    cap = ring.shape[0]
    idx = list(range(first_step // every + 1, last_step // every + 1))[-cap:]
    slots = torch.tensor([(i - 1) % cap for i in idx], dtype=torch.int64)
    rec = ring[slots] if idx else ring[:0]
    return torch.tensor([i * every for i in idx], dtype=torch.int64), rec[:, :P], rec[:, P:2 * P + 4]


def _wrap_signed(value, bits):
    """`value` modulo 2^bits as the signed integer of that width: how a seed (64) or an RNG step (32) goes into an int64 / int32 tensor."""
    value &= (1 << bits) - 1
    return value - (1 << bits) if value >> (bits - 1) else value


def _replica_setup(self, vae_models, name, noun, draws, verb, cap, signature, covered):
    """What the constructors of the replica classes share.  Sets on `self`: ms, eng, specs (device_spec() of every model), kind, dd,
    did, pad, var, A ([R, a_stride] stack of the dataset matrices, or None), a_stride and R, after refusing -- in this order -- no
    models, a -dd / -did the device draw does not support, world > 1, what `covered()` refuses (called with eng and kind set), more
    than `cap` models (an attribute of the engine; "vaek_" + cap is its ABI name) and a model whose `signature(m, spec)` differs
    from model 0's.  `name` is the class in the messages, one `noun` ("launch", "call", "step") `verb`s ("trains", "evaluates") the
    replicas, and `draws` ("batches", "rows") is what the generator draws for it."""
    ms = list(vae_models)
    if not ms:
        raise RuntimeError(f"{name}: no models")
    from .datasets import DEVICE_DRAW_MAX_DIM
    self.ms = ms
    m0 = ms[0]
    self.eng = m0.model.module.engine(m0.batch_size, m0.optimizer.global_batch)
    self.specs = specs = [m.dataset.device_spec() for m in ms]
    self.kind, _, self.dd, self.did, self.pad, self.var = specs[0]
    if self.dd > DEVICE_DRAW_MAX_DIM or self.did > DEVICE_DRAW_MAX_DIM:
        raise RuntimeError(f"{name} draws its {draws} with libvaek's Philox generator, which supports -dd / -did <= "
                           f"{DEVICE_DRAW_MAX_DIM} (got {self.dd} / {self.did})")
    if self.eng.world > 1:
        raise RuntimeError(f"{name}: data parallelism (world > 1) is not supported: the replicas are independent models on one GPU")
    covered()
    R = len(ms)
    if R > getattr(self.eng, cap):
        raise RuntimeError(f"{name}: {R} models, at most {getattr(self.eng, cap)} fit one {noun} (vaek_{cap})")
    want = signature(m0, specs[0])
    for r, (m, sp) in enumerate(zip(ms, specs)):
        got = signature(m, sp)
        if got != want:
            raise RuntimeError(f"{name}: model {r} differs from model 0 in shape, architecture or dataset kind ({got} against "
                               f"{want}): one {noun} {verb} replicas of ONE shape")
    self.R = R
    if specs[0][1] is None:
        self.A, self.a_stride = None, 0
    else:
        self.A = torch.stack([sp[1].reshape(-1).to(device=self.eng.device, dtype=torch.float32) for sp in specs]).contiguous()
        self.a_stride = self.A.shape[1]


def _event_rows(name, m0, rows, lo, hi, cap_fn, note=""):
    """The rows per event of a replica evaluation: `rows`, else model 0's print_batch_size, refused outside lo .. hi (hi: the engine's
    cap, `cap_fn` the C function that reports it)."""
    rows = int(getattr(m0, "print_batch_size", 1000) if rows is None else rows)
    if not lo <= rows <= hi:
        raise RuntimeError(f"{name}: {rows} rows per event, need {lo} .. {hi} ({cap_fn}{note})")
    return rows


def _seed_step_tensors(seeds, steps, dev):
    """The uint64 seeds and uint32 RNG steps of a call as the int64 / int32 device tensors the library takes (their bits)."""
    return (torch.tensor([_wrap_signed(s, 64) for s in seeds], dtype=torch.int64).to(dev),
            torch.tensor([_wrap_signed(s, 32) for s in steps], dtype=torch.int32).to(dev))


def _check_solve(name, r, m, what, mat, sweeps, off, bound):
    """Refuse the record of model r whose Jacobi solve (`what`, of the matrix `mat`) hit the sweep cap with off_F above `bound` =
    2^-40 of the matrix's norm; `name` is the class in the message."""
    if not off <= bound:
        raise RuntimeError(f"{name}: model {r} ({getattr(m, 'dirname', '?')}): the {what} stopped at the cap of "
                           f"{int(sweeps)} sweeps with off_F = {off:.3e} > 2^-40 |{mat}|_F = {bound:.3e}")


# What GraphLoop(resident=None) resolves to where the engine supports the resident loop and the model has no moments path.  The gate
# is tools/time_resident.py: True only once the resident loop's slowest repeat has beaten the hipGraph loop's fastest on all seven
# shapes.  That table has NOT been measured yet, so the default is off: resident=True asks for the loop explicitly.
RESIDENT_DEFAULT = False


class GraphLoop:
    def __init__(self, vae_model, steps_per_graph=200, seed=None, loss_capacity=1 << 20, pipeline=True, moments=None, resident=None,
                 trajectory_every=None, trajectory_capacity=None):
        m = vae_model
        self.m = m
        ds = m.dataset
        self.kind, self.A, self.dd, self.did, self.pad, self.var = ds.device_spec()
        from .datasets import DEVICE_DRAW_MAX_DIM
        if self.dd > DEVICE_DRAW_MAX_DIM or self.did > DEVICE_DRAW_MAX_DIM:
            raise RuntimeError(f"--fast_loop draws its batches with libvaek's Philox kernel, which supports -dd / -did <= "
                               f"{DEVICE_DRAW_MAX_DIM} (got {self.dd} / {self.did}); run without --fast_loop")
        self.B = m.batch_size
        self.eng = m.model.module.engine(self.B, m.optimizer.global_batch)
        ex = m.optimizer.exchange
        if self.eng.world > 1 and not (ex is not None and ex.in_library) and not self.eng.supports_train_steps_gen(self.kind):
            raise RuntimeError("GraphLoop under data parallelism needs the in-library P2P exchange (GradExchange mode 'p2p'): "
                               "an RCCL all-reduce between the two halves of the step is not captured")
        can = self.eng.supports_train_steps_gen(self.kind)
        if moments and not can:
            raise RuntimeError("GraphLoop(moments=True): vaek_train_steps_gen does not cover this model / dataset")
        self.moments = can if moments is None else bool(moments)
        can_res = not self.moments and self.eng.supports_train_loop_gen(self.kind)
        if resident and not can_res:
            raise RuntimeError("GraphLoop(resident=True): " + ("the moments path has priority" if self.moments else
                                                               "vaek_train_loop_gen does not cover this model / dataset"))
        # by default only where there is no moments path to take: a caller who switches an available moments path off
        # (moments=False) has always been asking for the per-sample hipGraph loop, and still gets it
        self.resident = (can_res and not can and RESIDENT_DEFAULT) if resident is None else bool(resident)
        if trajectory_every is not None and not self.resident:
            raise RuntimeError(f"GraphLoop(trajectory_every={trajectory_every}): the trajectory ring is written by the resident loop "
                               "(vaek_train_loop_gen_traj); " + ("pass resident=True" if can_res else
                                                                  "vaek_train_loop_gen does not cover this model / dataset" if not self.moments
                                                                  else "the moments path has priority on this model"))
        self.row0 = self.eng.rank * self.B           # ranks draw disjoint rows of the global batch
        self.seed = (ds.key[0] ^ ds.key[1] ^ m.key[1]) if seed is None else seed
        self.pipeline = bool(pipeline) and not self.moments and not self.resident
        self.G = int(steps_per_graph)
        if self.pipeline and self.G % 2:
            self.G += 1                              # two batch buffers: a replay must start on the parity it was captured on
        dev = self.eng.device

        def bufs():
            return (torch.empty(self.B, self.eng.D, dtype=torch.float32, device=dev),
                    torch.empty(self.B, self.eng.L, dtype=torch.float32, device=dev),
                    torch.empty(self.B, self.eng.D, dtype=torch.float32, device=dev))
        self.bufs = [] if self.moments or self.resident else [bufs() for _ in range(2 if self.pipeline else 1)]
        self.loss_ring = torch.zeros(loss_capacity, dtype=torch.float32, device=dev)
        self.eng.set_loss_history(self.loss_ring)
        self.graph = None
        self.graph_parity = 0
        self.steps_done_at_attach = m.optimizer.state.step
        self.trajectory_every = None if trajectory_every is None else int(trajectory_every)
        self.traj_ring = None
        if trajectory_every is not None:         # every recorded step of the schedule, sized once
            cap = _trajectory_capacity("GraphLoop", [m], trajectory_every, trajectory_capacity)
            self.traj_ring = torch.zeros(cap, self.eng.trajectory_record_len, dtype=torch.float32, device=dev)
        if self.pipeline:
            n = m.optimizer.state.step
            # the generator's own step counter, a pair used alternately (vaek_make_batch_next): the draw of batch k
            # reads counter[k % 2] and stores k + 1 into the other slot.  Invariant between steps: the batch of the
            # next step n is in bufs[n % 2] and counter[(n + 1) % 2] == n + 1.
            self.counter = torch.tensor([n, n], dtype=torch.int32, device=dev)
            self._make(self.bufs[n % 2], counter=self.counter, which=n % 2)

    def _make(self, out, **kw):
        self.eng.make_batch(self.kind, self.A, self.dd, self.did, self.pad, self.var, self.B, self.seed,
                            tag=0, row0=self.row0, out=out, **kw)

    def _one(self):
        st = self.m.optimizer.state
        lr = self.m.optimizer.optimizer_def.learning_rate
        if self.pipeline:
            n = st.step
            self.eng.train_step_gen(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, self.bufs[n % 2], lr,
                                    self.kind, self.A, self.dd, self.did, self.pad, self.var, self.bufs[(n + 1) % 2],
                                    self.seed, self.counter, (n + 1) % 2, tag=0, row0=self.row0)
        else:
            x, z1, z2 = self.bufs[0]
            self._make(self.bufs[0], step_dev=st.step_dev)
            self.eng.train_step(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, x, z1, z2, lr)
        st.step += 1

    def _capture(self):
        for _ in range(2):                       # warm-up outside capture (lazy kernel attributes etc.)
            self._one()
        torch.cuda.synchronize()
        self.graph_parity = self.m.optimizer.state.step % 2
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(self.G):
                    self._one()
        torch.cuda.current_stream().wait_stream(side)
        # capture does not execute: take back the host-side step mirror it advanced
        self.m.optimizer.state.step -= self.G
        self.graph = g
        return 2

    def run(self, n_steps):
        """Exactly n_steps train steps."""
        if self.moments or self.resident:
            if n_steps > 0:
                st = self.m.optimizer.state
                call = self.eng.train_steps_gen if self.moments else self.eng.train_loop_gen
                kw = {} if self.traj_ring is None else dict(trajectory=dict(buf=self.traj_ring, every=self.trajectory_every))
                call(self.m.model.flat, st.grads, st.m, st.v, st.step_dev, n_steps,
                     self.m.optimizer.optimizer_def.learning_rate, self.kind, self.A, self.dd, self.did, self.pad,
                     self.var, self.seed, tag=0, row0=self.row0, **kw)
                st.step += n_steps
            return
        done = 0
        if self.graph is None and n_steps >= self.G + 2:
            done += self._capture()
        st = self.m.optimizer.state
        if self.graph is not None and self.pipeline and n_steps - done > self.G and st.step % 2 != self.graph_parity:
            self._one()                          # back onto the buffer parity the graph was captured on
            done += 1
        if self.graph is not None and (not self.pipeline or st.step % 2 == self.graph_parity):
            while n_steps - done >= self.G:
                self.graph.replay()
                st.step += self.G
                done += self.G
        for _ in range(n_steps - done):
            self._one()

    def describe(self):
        """One line for run.py: which of the three loops this is."""
        if self.moments:
            return "persistent moment launches (vaek_train_steps_gen)"
        if self.resident:
            return (f"resident linear kernel, {self.eng.train_loop_steps_per_launch} steps per launch" +
                    ("" if self.traj_ring is None else f", trajectory record every {self.trajectory_every} steps "
                                                       f"(ring of {self.traj_ring.shape[0]})"))
        return f"hipGraph of {self.G} steps" + (", next batch drawn inside the step's launch" if self.pipeline else "")

    def check(self):
        """Synchronous.  The persistent launches of the moments path wait for each other's hand-offs with bounded spins: one that
        expired has produced garbage -- stop loudly."""
        if self.moments:
            torch.cuda.synchronize()
            if self.eng.train_steps_gave_up():
                raise RuntimeError(f"a bounded in-launch wait of vaek_train_steps_gen expired (status {self.eng.train_steps_status_word:#x}): "
                                   "the steps since the last check are invalid")

    def losses(self):
        """Losses of all steps run so far in order (device -> host once)."""
        n = self.m.optimizer.state.step
        cap = self.loss_ring.numel()
        ring = self.loss_ring.cpu()
        if n <= cap:
            return ring[:n]
        k = n % cap
        return torch.cat([ring[k:], ring[:k]])

    @property
    def records_trajectory(self):
        return self.traj_ring is not None

    def trajectory(self):
        """(steps, params [n, P], grads [n, P + 4]) of the records this loop's steps have left, in step order (one device -> host
        copy): record i is Adam step steps[i] (1-based), the parameters its gradient was evaluated at (the state after
        steps[i] - 1 steps) and its gradient buffer (loss, mean Dkl, mean mse, 0 in the last four slots)."""
        if self.traj_ring is None:
            raise RuntimeError("GraphLoop.trajectory(): this loop records none (pass trajectory_every=K with resident=True)")
        return _trajectory_view(self.traj_ring.cpu(), self.trajectory_every, self.steps_done_at_attach, self.m.optimizer.state.step,
                                self.m.model.flat.numel())


class _ReplicaLosses:
    """What VAEModel.model_save_data asks of `model._graph_loop`: the train losses of one replica of a ReplicaLoop."""

    def __init__(self, loop, r):
        self.loop, self.r = loop, r

    def losses(self):
        return self.loop.losses(self.r)

    @property
    def records_trajectory(self):
        return self.loop.traj_ring is not None

    def trajectory(self):
        return self.loop.trajectory(self.r)


class ReplicaLoop:
    """A sweep as ONE launch per run of steps: R VAEModels of one shape -- the same batch size, data and latent dimension,
    architecture (a linear VAE the resident loop covers), epsilon, dataset kind, -dd, -did, padding and dataset noise -- each with
    its own dataset matrix, its own parameters and Adam state and its own learning rate, trained by vaek_train_loop_gen_replicas
    (csrc/linear_resident.hip): workgroup r of the launch is model r's resident loop.  Model r's RNG seed is the one GraphLoop
    derives for it (ds.key[0] ^ ds.key[1] ^ m.key[1]), so replica r trains on the batches GraphLoop(model r, resident=True) would
    draw and ends bitwise where that loop ends.

    The states live in [R, stride] stacks owned by the loop.  COPIES AT THE BOUNDARIES OF run(): every run(n) first copies each
    model's `model.flat` and `optimizer.state.{grads, m, v, step_dev}` into its row of the stacks, makes one library call, and
    copies the rows back (and advances `state.step`), so between two run() calls the models are ordinary models: compute_stats,
    plot_epoch, save, checkpoints and anything else that reads or writes their own tensors works unchanged, and a state loaded in
    between is picked up by the next run().  The copies are 5 R small device copies on each side of the call, per run of steps
    between two events of the schedule -- not per step.

    One workgroup per model and no cross-workgroup state: nothing to wait for, check() polls nothing."""

    def __init__(self, vae_models, loss_capacity=None, trajectory_every=None, trajectory_capacity=None):
        def covered():
            if not self.eng.supports_train_loop_gen(self.kind):
                raise RuntimeError("ReplicaLoop: vaek_train_loop_gen does not cover this model / dataset (it needs a float32 linear VAE with "
                                   "one or two decoders, D, L <= 32 and a batch of at most 256 rows)")
        _replica_setup(self, vae_models, "ReplicaLoop", "launch", "batches", "trains", "train_loop_max_replicas", self._signature, covered)
        ms, R, m0 = self.ms, self.R, self.ms[0]
        self.B = m0.batch_size
        dev = self.eng.device
        P, GL = m0.model.flat.numel(), m0.optimizer.state.grads.numel()
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.params, self.m, self.v, self.grads = f32(R, P), f32(R, P), f32(R, P), f32(R, GL)
        self.step_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        seeds = [(m.dataset.key[0] ^ m.dataset.key[1] ^ m.key[1]) & (2 ** 64 - 1) for m in ms]       # GraphLoop's, model by model
        self.seeds = torch.tensor([_wrap_signed(s, 64) for s in seeds], dtype=torch.int64, device=dev)
        self.lrs = torch.tensor([float(m.optimizer.optimizer_def.learning_rate) for m in ms], dtype=torch.float32, device=dev)
        if loss_capacity is None:             # every step of the longest schedule among the models
            loss_capacity = max(int(getattr(m, "num_batches", 0) or 0) for m in ms) or (1 << 16)
        self.rings = f32(R, int(loss_capacity))
        nb = self.eng.train_loop_replicas_workspace(R)
        self.workspace = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
        self.trajectory_every = None if trajectory_every is None else int(trajectory_every)
        self.traj_ring = None
        if trajectory_every is not None:         # one ring per model: every recorded step of the longest schedule, sized once
            cap = _trajectory_capacity("ReplicaLoop", ms, trajectory_every, trajectory_capacity)
            self.traj_ring = f32(R, cap, self.eng.trajectory_record_len)
            self.traj_from = [int(m.optimizer.state.step) for m in ms]

    @staticmethod
    def _signature(m, spec):
        eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
        cfg = getattr(eng, "cfg", None)
        arch = None if cfg is None else (cfg.n_enc_hidden, cfg.n_dec_hidden, cfg.sigmoid_decoder, cfg.tunable_eps, cfg.eps_cli, cfg.dtype,
                                         cfg.force_generic, cfg.global_batch)
        kind, A, dd, did, pad, var = spec
        return (m.batch_size, eng.D, eng.L, m.model.flat.numel(), arch, kind, None if A is None else A.numel(), dd, did, pad, float(var))

    def _rows(self, m, r):
        st = m.optimizer.state
        return ((self.params[r], m.model.flat), (self.grads[r], st.grads), (self.m[r], st.m), (self.v[r], st.v),
                (self.step_dev[r:r + 1], st.step_dev))

    def run(self, n_steps):
        """Exactly n_steps train steps of every model: one library call between the copies in and out."""
        if n_steps <= 0:
            return
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                row.copy_(own)
        kw = {} if self.traj_ring is None else dict(trajectory=dict(buf=self.traj_ring, every=self.trajectory_every))
        self.eng.train_loop_gen_replicas(self.params, self.grads, self.m, self.v, self.step_dev, n_steps, 0.0, self.kind, self.A,
                                         self.dd, self.did, self.pad, self.var, self.seeds, lrs=self.lrs, a_stride=self.a_stride,
                                         loss_hist=self.rings, workspace=self.workspace, tag=0, row0=0, **kw)
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                own.copy_(row)
            m.optimizer.state.step += n_steps

    def describe(self):
        """One line for run.py."""
        return (f"resident linear kernel, {self.R} replicas in one launch (vaek_train_loop_gen_replicas), "
                f"{self.eng.train_loop_steps_per_launch} steps per launch" +
                ("" if self.traj_ring is None else f", trajectory record every {self.trajectory_every} steps "
                                                   f"(rings of {self.traj_ring.shape[1]})"))

    def trajectory(self, r):
        """(steps, params [n, P], grads [n, P + 4]) of the records model r's steps in this loop have left, in step order (one device
        -> host copy of its ring); see GraphLoop.trajectory."""
        if self.traj_ring is None:
            raise RuntimeError("ReplicaLoop.trajectory(): this loop records none (pass trajectory_every=K)")
        m = self.ms[r]
        return _trajectory_view(self.traj_ring[r].cpu(), self.trajectory_every, self.traj_from[r], m.optimizer.state.step,
                                m.model.flat.numel())

    def stats_event(self, rows=None):
        """One stats event of every model in ONE launch (ReplicaStats, vaek_stats_event_replicas): [compute_stats' dict of model 0,
        ...], with the models' keys, draw counters and lists advanced exactly as compute_stats would advance them."""
        if getattr(self, "_stats", None) is None or (rows is not None and int(rows) != self._stats.rows):
            self._stats = ReplicaStats(self.ms, rows=rows)
        return self._stats.event()

    def check(self):
        """Nothing to poll: the launch has no waits."""

    def losses(self, r):
        """Losses of all steps model r has run so far, in order (device -> host once)."""
        n = self.ms[r].optimizer.state.step
        cap = self.rings.shape[1]
        ring = self.rings[r].cpu()
        if n <= cap:
            return ring[:n]
        k = n % cap
        return torch.cat([ring[k:], ring[:k]])

    def view(self, r):
        """Model r's `_graph_loop`: losses() without an argument, as VAEModel.model_save_data calls it."""
        return _ReplicaLosses(self, r)


class ReplicaStats:
    """The stats event of a sweep as ONE launch: what `compute_stats()` does for one model at every n_print step -- a batch of real
    rows, a batch of latents, VAE.loss on them, a fake batch sampled from the same latents, its score -- for R VAEModels of one
    shape (validated as in ReplicaLoop) through vaek_stats_event_replicas (csrc/linear_stats.hip): workgroup r evaluates model r.

    event() copies each model's `model.flat` into its row of an [R, P] stack owned by this object (the rule of ReplicaLoop.run:
    between two calls the models are ordinary models), makes ONE library call and ONE device -> host copy of the [R, 8 + L] records,
    and then does for every model exactly the host bookkeeping of compute_stats + compute_model_stats: the model's key is split,
    `_latent_draws` and the dataset's `_draws` advance, the seeds are the ones `_latent_pair` (tag 2) and `_device_batch` (tag 1)
    derive, `vae_losses`, `var_enc` and `var_dec` grow by one entry and `current_epsilon` becomes this event's eps.  After it every
    piece of host RNG state is what the host event would have left, so fused and host events can be mixed freely.  The fake batch
    is sampled with the model's `current_epsilon` as it was BEFORE the event, as sample_batch does.  Returns one stats dict per
    model, compute_stats' keys in its order; the values are host tensors (nothing to read back when they are printed)."""

    NAME = "ReplicaStats"              # ReplicaStatsMlp3 overrides the name and the three methods below __init__

    def __init__(self, vae_models, rows=None):
        from .datasets import SCORE_KEYS
        _replica_setup(self, vae_models, self.NAME, "launch", "batches", "evaluates", "train_loop_max_replicas", ReplicaLoop._signature,
                       self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.rows = _event_rows(self.NAME, m0, rows, 1, self.eng.stats_event_max_rows, "vaek_stats_event_max_rows")
        self.score_keys = SCORE_KEYS[self.kind]
        dev = self.eng.device
        self.L = self.eng.L
        self.record_len = self.eng.stats_record_len
        self.params = torch.zeros(R, m0.model.flat.numel(), dtype=torch.float32, device=dev)
        self.out = torch.zeros(R, self.record_len, dtype=torch.float32, device=dev)
        self._make_workspace()

    def _check_covered(self):
        if not self.eng.supports_stats_event(self.kind):
            raise RuntimeError("ReplicaStats: vaek_stats_event_replicas does not cover this model / dataset (it needs what the resident "
                               "loop needs: a float32 linear VAE with one or two decoders, D, L <= 32 and a train batch of at most 256 rows)")

    def _make_workspace(self):
        pass                           # the linear launch needs none

    def _call(self, *args, **kw):
        self.eng.stats_event_replicas(*args, **kw)

    def event(self):
        """One stats event of every model: [stats dict of model 0, ...]."""
        from . import random as vrandom
        dev = self.eng.device
        x_seeds, x_steps, z_seeds, z_steps, eps_in = [], [], [], [], []
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)
            key, m.key = vrandom.split(m.key)                                    # compute_stats
            ds = m.dataset
            ds._draws = getattr(ds, "_draws", 0) + 1                              # _device_batch: seed, step, tag 1
            x_seeds.append(ds.key[0] ^ ds.key[1])
            x_steps.append(ds._draws)
            m._latent_draws = getattr(m, "_latent_draws", 0) + 1                   # _latent_pair: seed, step, tag 2
            z_seeds.append(key[0] ^ key[1])
            z_steps.append(m._latent_draws)
            eps_in.append(m.current_epsilon)                                      # sample_batch: the PREVIOUS event's eps
        # an eps a host event left is a device tensor: it stays on the device (no read-back); every other one goes up in one copy
        on_dev = [torch.is_tensor(e) and e.device.type != "cpu" for e in eps_in]
        sample_eps = torch.tensor([0.0 if d else float(torch.as_tensor(e).reshape(-1)[0]) for e, d in zip(eps_in, on_dev)],
                                  dtype=torch.float32).to(dev)
        for r, (e, d) in enumerate(zip(eps_in, on_dev)):
            if d:
                sample_eps[r:r + 1].copy_(e.reshape(-1)[:1])
        self._call(self.params, self.rows, self.kind, self.A, self.dd, self.did, self.pad, self.var, *_seed_step_tensors(x_seeds, x_steps, dev),
                   *_seed_step_tensors(z_seeds, z_steps, dev), sample_eps, self.out, a_stride=self.a_stride, x_tag=1, z_tag=2)
        rec = self.out.cpu()                                                      # the event's ONE device -> host copy
        stats = []
        for r, m in enumerate(self.ms):
            row = rec[r]
            tdv = bool(getattr(m.model.module, "tunable_decoder_var", False))
            eps = row[3:4].clone() if tdv else m.epsilon                          # VAE.loss: a (1,) tensor under -tdv, else the CLI float
            m.vae_losses.append(row[0].clone())                                   # compute_model_stats
            m.var_enc.append(row[8:8 + self.L].clone())
            m.var_dec.append(eps.clone() if torch.is_tensor(eps) else eps)
            m.current_epsilon = eps.clone() if torch.is_tensor(eps) else eps
            st = {"VAE Loss": row[0].clone(), "KL divergence": row[1].clone(), "mse": row[2].clone()}
            for k, name in enumerate(self.score_keys):                            # score_batch's dict, in its order
                st[name] = row[4 + k].clone()
            stats.append(st)
        return stats


class ReplicaStatsMlp3(ReplicaStats):
    """ReplicaStats for three-hidden-layer MLP VAEs (vaek_mlp3_stats_event_replicas, csrc/mlp3_stats.hip): the same contract -- one
    parameter stack, ONE library call (two launches whatever R is) and ONE device -> host copy per event, the key split,
    `_latent_draws`, the dataset's `_draws`, tags 1 and 2, `vae_losses` / `var_enc` / `var_dec`, `current_epsilon`, compute_stats' keys
    in its order, fused and host events mixed freely -- on models Engine.supports_mlp3_stats_event covers, with the call's own
    workspace for the tile partials."""

    NAME = "ReplicaStatsMlp3"

    def _check_covered(self):
        if not self.eng.supports_mlp3_stats_event(self.kind):
            raise RuntimeError("ReplicaStatsMlp3: vaek_mlp3_stats_event_replicas does not cover this model / dataset (it needs a float32 VAE "
                               "with one decoder and exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, "
                               f"D, L <= 32; a linear VAE is ReplicaStats'; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def _make_workspace(self):
        nb = self.eng.mlp3_stats_event_workspace(self.R, self.rows)
        self.workspace = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.eng.device)

    def _call(self, *args, **kw):
        self.eng.mlp3_stats_event_replicas(*args, workspace=self.workspace, **kw)


class ReplicaLogLik:
    """The importance-weighted log-likelihood of R VAEModels of one shape in ONE library call (vaek_log_likelihood_replicas,
    csrc/linear_loglik.hip): per model, over `rows` data rows drawn from its dataset and `samples` = K posterior samples per row,
    the IWAE-K bound on log p(x) -- the `Average Log Likelihood` the reference reserves and never fills -- the K-sample ELBO estimate
    and the normalised effective sample size of the weights.

    The models are validated as in ReplicaLoop (one shape, architecture, epsilon, dataset kind, -dd, -did, padding, noise) but with
    NO condition on the batch size: the call reads parameters only, so models of any train batch -- and of different ones -- qualify.

    event() copies each model's `model.flat` into its row of an [R, P] stack owned by this object, makes ONE library call and ONE
    device -> host copy of the [R, 4] records.  It does NOT perturb the run: `m.key`, the dataset's `_draws` and `m._latent_draws` are
    neither split nor advanced.  Its draws have a counter of their own, `m._loglik_draws` (incremented before use: the first event
    draws under step 1), the seed dataset.key[0] ^ dataset.key[1] and the tags 3 (rows) and 4 (samples); tags 0, 1 and 2 belong to the
    train loop, the dataset's batches and the latents.  Returns per model {"Average Log Likelihood", "ELBO estimate", "Effective
    Sample Size"} (host tensors) and appends the first to `m.average_log_likelihoods`."""

    KEYS = ("Average Log Likelihood", "ELBO estimate", "Effective Sample Size")
    X_TAG, Z_TAG = 3, 4
    NAME = "ReplicaLogLik"             # ReplicaLogLikMlp3 overrides the name and the four methods below __init__

    def __init__(self, vae_models, samples, rows=None):
        _replica_setup(self, vae_models, self.NAME, "call", "rows", "evaluates", "train_loop_max_replicas", self._shape, self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.samples = int(samples)
        if not 1 <= self.samples <= self.eng.log_likelihood_max_samples:
            raise RuntimeError(f"{self.NAME}: {self.samples} samples per row, need 1 .. {self.eng.log_likelihood_max_samples} "
                               "(vaek_log_likelihood_max_samples)")
        self.rows = _event_rows(self.NAME, m0, rows, 1, self.eng.log_likelihood_max_rows, "vaek_log_likelihood_max_rows")
        self._check_size()
        dev = self.eng.device
        self.params = torch.zeros(R, m0.model.flat.numel(), dtype=torch.float32, device=dev)
        self.out = torch.zeros(R, self.eng.log_likelihood_record_len, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(max(self._workspace_bytes(), 8), dtype=torch.uint8, device=dev)

    def _check_covered(self):
        if not self.eng.supports_log_likelihood(self.kind):
            raise RuntimeError("ReplicaLogLik: vaek_log_likelihood_replicas does not cover this model / dataset (it needs a float32 linear "
                               "VAE -- no hidden layers -- with one or two decoders and D, L <= 32, D <= 28 with two decoders; this model's "
                               f"step path: {getattr(self.eng, 'step_path', '?')})")

    def _check_size(self):
        pass                           # rows and samples are the linear call's only caps

    def _workspace_bytes(self):
        return self.eng.log_likelihood_workspace(self.R, self.rows)

    def _call(self, *args, **kw):
        self.eng.log_likelihood_replicas(*args, **kw)

    @staticmethod
    def _shape(m, spec):
        """ReplicaLoop._signature without what depends on the batch size (the batch itself and the engine's global batch)."""
        sig = ReplicaLoop._signature(m, spec)
        arch = sig[4]
        return sig[1:4] + (None if arch is None else arch[:-1],) + sig[5:]

    def event(self):
        """One evaluation of every model: [{"Average Log Likelihood", "ELBO estimate", "Effective Sample Size"} of model 0, ...]."""
        dev = self.eng.device
        seeds, steps = [], []
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)
            m._loglik_draws = getattr(m, "_loglik_draws", 0) + 1
            ds = m.dataset
            seeds.append(ds.key[0] ^ ds.key[1])
            steps.append(m._loglik_draws)
        seeds, steps = _seed_step_tensors(seeds, steps, dev)
        self._call(self.params, self.rows, self.samples, seeds, steps, self.out, self.workspace, kind=self.kind,
                   A=self.A, dd=self.dd, did=self.did, pad=self.pad, var_added=self.var, x_seeds=seeds, x_steps=steps,
                   a_stride=self.a_stride, x_tag=self.X_TAG, z_tag=self.Z_TAG)
        rec = self.out.cpu()                                                      # the event's ONE device -> host copy
        stats = []
        for r, m in enumerate(self.ms):
            st = {name: rec[r, k].clone() for k, name in enumerate(self.KEYS)}
            m.average_log_likelihoods.append(st[self.KEYS[0]])
            stats.append(st)
        return stats


class ReplicaLogLikMlp3(ReplicaLogLik):
    """ReplicaLogLik for three-hidden-layer MLP VAEs (vaek_mlp3_log_likelihood_replicas, csrc/mlp3_loglik.hip): the same contract --
    one shape, any batch size, ONE library call and ONE device -> host copy per event, the same three keys, the counter
    `m._loglik_draws`, the seed dataset.key[0] ^ dataset.key[1], tags 3 and 4, nothing of the run touched, the first key appended to
    `m.average_log_likelihoods` -- on models Engine.supports_mlp3_log_likelihood covers, with one more cap: R * rows * samples at most
    Engine.mlp3_log_likelihood_max_columns."""

    NAME = "ReplicaLogLikMlp3"

    def _check_covered(self):
        if not self.eng.supports_mlp3_log_likelihood(self.kind):
            raise RuntimeError("ReplicaLogLikMlp3: vaek_mlp3_log_likelihood_replicas does not cover this model / dataset (it needs a float32 "
                               "VAE with one decoder and exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, "
                               f"D, L <= 32; a linear VAE is ReplicaLogLik's; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def _check_size(self):
        cols, cap = self.R * self.rows * self.samples, self.eng.mlp3_log_likelihood_max_columns
        if cols > cap:
            raise RuntimeError(f"ReplicaLogLikMlp3: {self.R} models x {self.rows} rows x {self.samples} samples = {cols} columns, at most "
                               f"{cap} fit one call (vaek_mlp3_log_likelihood_max_columns)")

    def _workspace_bytes(self):
        return self.eng.mlp3_log_likelihood_workspace(self.R, self.rows, self.samples)

    def _call(self, *args, **kw):
        self.eng.mlp3_log_likelihood_replicas(*args, **kw)


class ReplicaExactLogLik:
    """The EXACT log-likelihood, the exact ELBO and their difference KL(q(z|x) || p(z|x)) of R one-decoder linear VAEModels of one
    shape in ONE launch (vaek_exact_log_likelihood_replicas, csrc/exact_loglik.inc): such a model is a linear-Gaussian
    latent-variable model, p(x) = N(b_d, K^T K + e^eps I), so what ReplicaLogLik estimates has a closed form -- float64 on the device,
    through the eigenvectors of K^T K.

    The models are validated as in ReplicaLogLik (one shape, any batch size).  event() copies each model's `model.flat` into its row
    of an [R, P] stack owned by this object, makes ONE library call and ONE device -> host copy of the [R, 10 + D] float64 records.
    It does NOT perturb the run: `m.key`, the dataset's `_draws`, `m._latent_draws` and `m._loglik_draws` are left alone.  Its draws
    have a counter of their own, `m._exact_loglik_draws` (incremented before use), the seed dataset.key[0] ^ dataset.key[1] and row
    tag 3 -- ReplicaLogLik's row tag, so event(step=s) with the step a ReplicaLogLik event just used scores the rows that event
    scored, bit for bit (with `step` given the counter is neither read nor advanced).  Returns per model {"Exact Log Likelihood",
    "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning"} (Python floats; the last is the record's bound on the relative
    error of the smallest eigenvalue of the model covariance, (off_F + 64 D 2^-53 |K^T K|_F) e^-eps: large means ill-conditioned,
    reported, not hidden).  Raises RuntimeError naming the model where the solve ended with off_F > 2^-40 |K^T K|_F."""

    KEYS = ("Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning")
    SLOTS = (0, 1, 2, 8)
    X_TAG = ReplicaLogLik.X_TAG
    NAME = "ReplicaExactLogLik"
    OFF_BOUND = 2.0 ** -40

    def __init__(self, vae_models, rows=None):
        _replica_setup(self, vae_models, self.NAME, "launch", "rows", "evaluates", "train_loop_max_replicas", ReplicaLogLik._shape,
                       self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.rows = _event_rows(self.NAME, m0, rows, 1, self.eng.log_likelihood_max_rows, "vaek_log_likelihood_max_rows")
        dev = self.eng.device
        self.record_len = self.eng.exact_log_likelihood_record_len
        self.params = torch.zeros(R, m0.model.flat.numel(), dtype=torch.float32, device=dev)
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)

    def _check_covered(self):
        if not self.eng.supports_exact_log_likelihood(self.kind):
            raise RuntimeError("ReplicaExactLogLik: vaek_exact_log_likelihood_replicas does not cover this model / dataset (it needs a "
                               "float32 linear VAE -- no hidden layers -- with ONE decoder and D, L <= 32: the sigmoid second decoder has "
                               f"no closed form; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def event(self, step=None):
        """One evaluation of every model: [{"Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning"} of
        model 0, ...].  step: draw the rows under this RNG step (one int, or one per model) instead of the models' own counters."""
        dev = self.eng.device
        if step is not None:
            given = [int(s) for s in step] if isinstance(step, (list, tuple)) else [int(step)] * self.R
            if len(given) != self.R:
                raise RuntimeError(f"{self.NAME}.event(step=...): {len(given)} steps for {self.R} models")
        seeds, steps = [], []
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)
            if step is None:
                m._exact_loglik_draws = getattr(m, "_exact_loglik_draws", 0) + 1
                s = m._exact_loglik_draws
            else:
                s = given[r]
            ds = m.dataset
            seeds.append(ds.key[0] ^ ds.key[1])
            steps.append(s)
        seeds, steps = _seed_step_tensors(seeds, steps, dev)
        self.eng.exact_log_likelihood_replicas(self.params, self.rows, self.out, kind=self.kind, A=self.A, dd=self.dd, did=self.did,
                                               pad=self.pad, var_added=self.var, x_seeds=seeds, x_steps=steps, a_stride=self.a_stride,
                                               x_tag=self.X_TAG)
        rec = self.out.cpu().numpy()                                              # the event's ONE device -> host copy
        stats = []
        for r, m in enumerate(self.ms):
            row = rec[r]
            _check_solve(self.NAME, r, m, "solve of K^T K", "K^T K", row[5], row[6], self.OFF_BOUND * row[7])
            stats.append({name: float(row[k]) for name, k in zip(self.KEYS, self.SLOTS)})
        return stats

    IWAE_GAP = "IWAE Gap"

    def event_after(self, iwae_stats=None):
        """event() of an n_print event.  iwae_stats: what a ReplicaLogLik over the SAME models just returned, or None.  With it the rows
        are drawn under the step that event used (`m._loglik_draws`), so both score the same rows bitwise, and every dict gains
        "IWAE Gap" = Exact Log Likelihood - Average Log Likelihood: how far the IWAE-K bound is from the truth."""
        if iwae_stats is None:
            return self.event()
        stats = self.event(step=[m._loglik_draws for m in self.ms])
        for st, iw in zip(stats, iwae_stats):
            st[self.IWAE_GAP] = st[self.KEYS[0]] - float(iw[ReplicaLogLik.KEYS[0]])
        return stats


class ReplicaElboHessian:
    """The curvature of the loss surface R one-decoder linear VAEModels of one shape sit on, in ONE launch
    (vaek_elbo_hessian_lanczos_replicas, csrc/elbo_hessian.hip): `steps` <= 32 Lanczos steps with full reorthogonalisation on the
    Hessian of f = -mean exact ELBO over `rows` data rows -- the population training objective on those rows, float64, closed form
    -- give its extreme Ritz values (sharpness and the smallest curvature: minimum or saddle), a rigorous residual bound per value,
    and the exact gradient norm: how stationary the point Adam sits at really is.

    The models are validated as in ReplicaExactLogLik (one shape, any batch size).  event() copies each model's `model.flat` into its
    row of an [R, P] stack owned by this object, draws each model's start vector with vaek_rng_fill (float32 normals, widened), makes
    ONE Lanczos call and ONE device -> host copy of the [R, 140] float64 records.  It does NOT perturb the run: `m.key`, the
    dataset's `_draws`, `m._latent_draws` and the other events' counters are left alone.  Its draws have a counter of their own,
    `m._elbo_hessian_draws` (incremented before use), the seed dataset.key[0] ^ dataset.key[1] and the tags 9 (rows) and 10 (start
    vector); tags 0 .. 8 belong to the train loop, the dataset's batches, the latents, the log-likelihood, the spectra and the
    Jacobian.  event(step=s) draws the ROWS under step s and ReplicaExactLogLik's row tag instead, so the Hessian is that of the
    objective on the rows a ReplicaExactLogLik event just scored, bit for bit (the start vector stays under the own counter).
    Returns per model {"ELBO Hessian Ritz Values" (float64 [k], ascending), "ELBO Hessian Ritz Residuals" (float64 [k]: an eigenvalue
    of H lies within each of its Ritz value), "Sharpness" (the largest Ritz value), "ELBO Hessian Min Ritz", "ELBO Gradient Norm"}.
    Raises RuntimeError naming the model where the solve of T ended with off_F > 2^-40 |T|_F."""

    KEYS = ("ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm")
    X_TAG, V_TAG = 9, 10
    NAME = "ReplicaElboHessian"
    OFF_BOUND = 2.0 ** -40
    HEAD, BLOCK = 12, 32

    def __init__(self, vae_models, steps=32, rows=None):
        _replica_setup(self, vae_models, self.NAME, "launch", "rows", "evaluates", "train_loop_max_replicas", ReplicaLogLik._shape,
                       self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.steps = int(steps)
        if not 1 <= self.steps <= self.eng.elbo_hessian_max_steps:
            raise RuntimeError(f"{self.NAME}: {self.steps} Lanczos steps, need 1 .. {self.eng.elbo_hessian_max_steps} "
                               "(vaek_elbo_hessian_max_steps)")
        self.rows = _event_rows(self.NAME, m0, rows, 1, self.eng.log_likelihood_max_rows, "vaek_log_likelihood_max_rows")
        dev = self.eng.device
        self.P = P = m0.model.flat.numel()
        self.record_len = self.eng.elbo_hessian_record_len
        self.params = torch.zeros(R, P, dtype=torch.float32, device=dev)
        self.v0 = torch.zeros(R, P, dtype=torch.float64, device=dev)
        self.basis = torch.zeros(R, self.steps, P, dtype=torch.float64, device=dev)
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)

    def _check_covered(self):
        if not self.eng.supports_elbo_hessian(self.kind):
            raise RuntimeError("ReplicaElboHessian: vaek_elbo_hessian_lanczos_replicas does not cover this model / dataset (it needs a "
                               "float32 linear VAE -- no hidden layers -- with ONE decoder and D, L <= 32: the ELBO of other models has "
                               f"no closed form; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def event(self, step=None):
        """One evaluation of every model.  step: draw the ROWS under this RNG step (one int, or one per model) and ReplicaExactLogLik's
        row tag instead of the own counter and tag 9."""
        dev = self.eng.device
        if step is not None:
            given = [int(s) for s in step] if isinstance(step, (list, tuple)) else [int(step)] * self.R
            if len(given) != self.R:
                raise RuntimeError(f"{self.NAME}.event(step=...): {len(given)} steps for {self.R} models")
        seeds, steps = [], []
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)
            m._elbo_hessian_draws = getattr(m, "_elbo_hessian_draws", 0) + 1
            ds = m.dataset
            seed = ds.key[0] ^ ds.key[1]
            self.v0[r].copy_(self.eng.rng_fill(self.P, seed, step=m._elbo_hessian_draws, tag=self.V_TAG))      # widened on the copy
            seeds.append(seed)
            steps.append(m._elbo_hessian_draws if step is None else given[r])
        seeds, steps = _seed_step_tensors(seeds, steps, dev)
        self.eng.elbo_hessian_lanczos_replicas(self.params, self.rows, self.steps, self.v0, self.basis, self.out, kind=self.kind, A=self.A,
                                               dd=self.dd, did=self.did, pad=self.pad, var_added=self.var, x_seeds=seeds, x_steps=steps,
                                               a_stride=self.a_stride, x_tag=self.X_TAG if step is None else ReplicaExactLogLik.X_TAG)
        rec = self.out.cpu().numpy()                                              # the event's ONE device -> host copy
        stats = []
        for r, m in enumerate(self.ms):
            row = rec[r]
            _check_solve(self.NAME, r, m, "solve of the Lanczos matrix T", "T", row[4], row[5], self.OFF_BOUND * row[6])
            k, h, b = int(row[2]), self.HEAD, self.BLOCK
            stats.append({self.KEYS[0]: row[h:h + k].copy(), self.KEYS[1]: row[h + b:h + b + k].copy(), self.KEYS[2]: float(row[9]),
                          self.KEYS[3]: float(row[10]), self.KEYS[4]: float(row[1])})
        return stats

    def event_after(self, exact=False, iwae=False):
        """event() of an n_print event.  exact: a ReplicaExactLogLik over the SAME models has just had its event (iwae: after a
        ReplicaLogLik's, whose step it then used); the rows are drawn under the step that event used, so the Hessian is the one of the
        objective on the rows it scored."""
        if not exact:
            return self.event()
        return self.event(step=[m._loglik_draws if iwae else m._exact_loglik_draws for m in self.ms])


class ReplicaJacobianMlp3:
    """The decoder Jacobian spectra of R three-hidden-layer MLP VAEModels of one shape in ONE library call
    (vaek_mlp3_decoder_jacobian_replicas, csrc/mlp3_jacobian.hip): per model, over `rows` latent rows z, the eigenvalues of J^T J with
    J = d Decoder(z) / dz -- the squared singular values of the decoder's local linear map --, their numerical rank and the
    sensitivity |d Decoder / d z_l|^2 of every latent: how many directions of the latent space the decoder uses, and which are off.

    The models are validated as in ReplicaLogLik (one shape, any batch size).  `at` chooses the latents:
      "prior"      the call draws them: the z1 vaek_make_batch writes under the event's seed, step and latent tag -- the latents
                   sample_batch decodes at a stats event;
      "posterior"  per model the event's real rows are drawn with make_batch (row tag), mu comes from vaek_forward(sampling=0) and goes
                   to the call as explicit rows: the Jacobian on the encoded data manifold.
    event() copies each model's `model.flat` into its row of an [R, P] stack owned by this object, makes ONE
    vaek_mlp3_decoder_jacobian_replicas call for all models and ONE device -> host copy of the [R, 2 L + 8] float64 records.  It does NOT
    perturb the run: `m.key`, the dataset's `_draws`, `m._latent_draws` and the other events' counters are left alone.  Its draws have a
    counter of their own, `m._jacobian_draws` (incremented before use), the seed dataset.key[0] ^ dataset.key[1] and the tags 7 (rows)
    and 8 (latents); tags 0 .. 6 belong to the train loop, the dataset's batches, the latents, the log-likelihood and the spectra.
    Returns per model {"Decoder Jacobian Spectrum" (float64 [L], descending), "Decoder Jacobian Rank" (float64 [3]: mean, min, max),
    "Latent Sensitivity" (float64 [L])} and appends them to `m.jacobian_spectra`, `m.jacobian_ranks` and `m.latent_sensitivities`.
    Raises RuntimeError naming the model where a row's solve ended with off_F > 2^-40 |J^T J|_F."""

    KEYS = ("Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity")
    X_TAG, Z_TAG = 7, 8
    NAME = "ReplicaJacobianMlp3"
    OFF_BOUND = 2.0 ** -40
    MODES = ("prior", "posterior")

    def __init__(self, vae_models, rows=None, at="prior", rank_tol=1e-4):
        if at not in self.MODES:
            raise RuntimeError(f"{self.NAME}(at={at!r}): need one of {self.MODES}")
        self.at = at
        self.rank_tol = float(rank_tol)
        if not 0.0 <= self.rank_tol < 1.0:
            raise RuntimeError(f"{self.NAME}(rank_tol={rank_tol}): need 0 <= rank_tol < 1")
        _replica_setup(self, vae_models, self.NAME, "call", "rows", "evaluates", "train_loop_max_replicas", ReplicaLogLik._shape,
                       self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.rows = _event_rows(self.NAME, m0, rows, 1, self.eng.stats_event_max_rows, "vaek_stats_event_max_rows")
        self.L = self.eng.L
        cols, cap = R * self.rows * self.L, self.eng.mlp3_decoder_jacobian_max_columns
        if cols > cap:
            raise RuntimeError(f"{self.NAME}: {R} models x {self.rows} rows x {self.L} latents = {cols} columns, at most {cap} fit one call "
                               "(vaek_mlp3_decoder_jacobian_max_columns)")
        dev = self.eng.device
        self.record_len = self.eng.decoder_jacobian_record_len
        self.params = torch.zeros(R, m0.model.flat.numel(), dtype=torch.float32, device=dev)
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(max(self.eng.mlp3_decoder_jacobian_workspace(R, self.rows), 16), dtype=torch.uint8, device=dev)
        if at == "posterior":
            self.z = torch.zeros(R, self.rows, self.L, dtype=torch.float32, device=dev)

    def _check_covered(self):
        if not self.eng.supports_mlp3_decoder_jacobian():
            raise RuntimeError("ReplicaJacobianMlp3: vaek_mlp3_decoder_jacobian_replicas does not cover this model (it needs a float32 "
                               "VAE with one decoder and exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, "
                               "D, L <= 32; the Jacobian of a linear decoder is its kernel: ReplicaExactLogLik's record holds the "
                               f"eigenvalues of K^T K; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def event(self):
        """One evaluation of every model: [{"Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"} of model 0, ...]."""
        dev = self.eng.device
        L = self.L
        seeds, steps = [], []
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)
            m._jacobian_draws = getattr(m, "_jacobian_draws", 0) + 1
            ds = m.dataset
            seeds.append(ds.key[0] ^ ds.key[1])
            steps.append(m._jacobian_draws)
        if self.at == "posterior":
            for r, m in enumerate(self.ms):
                eng = m.model.module.engine(self.rows)                                 # forward takes at most its context's batch
                Ar = None if self.A is None else self.A[r]
                x, z1, z2 = eng.make_batch(self.kind, Ar, self.dd, self.did, self.pad, self.var, self.rows, seeds[r], step=steps[r],
                                           tag=self.X_TAG)
                _, mu = eng.forward(m.model.flat, x, z1, z2, sampling=False, want_mu=True)
                self.z[r].copy_(mu)
            self.eng.mlp3_decoder_jacobian_replicas(self.params, self.rows, self.out, self.workspace, z=self.z, rank_tol=self.rank_tol,
                                                    z_tag=self.Z_TAG)
        else:
            sd, st = _seed_step_tensors(seeds, steps, dev)
            self.eng.mlp3_decoder_jacobian_replicas(self.params, self.rows, self.out, self.workspace, z_seeds=sd, z_steps=st,
                                                    rank_tol=self.rank_tol, z_tag=self.Z_TAG)
        rec = self.out.cpu().numpy()                                                  # the event's ONE device -> host copy
        stats = []
        for r, m in enumerate(self.ms):
            row = rec[r]
            # slot [6] is the largest off_F / |G|_F over the rows: the bound is relative
            _check_solve(self.NAME, r, m, "solve of J^T J", "J^T J", row[5], row[6], self.OFF_BOUND)
            st = {self.KEYS[0]: row[8:8 + L].copy(), self.KEYS[1]: row[1:4].copy(), self.KEYS[2]: row[8 + L:8 + 2 * L].copy()}
            for name, attr in zip(self.KEYS, ("jacobian_spectra", "jacobian_ranks", "latent_sensitivities")):
                if not hasattr(m, attr):
                    setattr(m, attr, [])
                getattr(m, attr).append(st[name])
            stats.append(st)
        return stats


class ReplicaSpectrum:
    """The covariance spectra of a generated and of a real batch of R VAEModels of one shape: per model the eigenvalues of
    cov(fake batch) -- the reference's "learnt eigenvalue" -- and of cov(real batch) -- its "ground truth eigenvalue"
    (datasets.py:113-125), the `EigenValues` the reference saves and never fills (csrc/cov_spectrum.hip).

    The models are validated as in ReplicaLogLik (one shape, any batch size; data_dim <= 32).  Where the engine's
    supports_spectrum_event holds (linear VAEs) event() is one parameter stack, ONE fused call (vaek_spectrum_event_replicas: nothing
    of a row exists in HBM) and one device -> host copy.  Every other model -- the mlp3 sweep included -- takes the host route: per
    model make_batch and forward(sampling) under the same seeds, steps and tags into a [2R, rows, D] stack, then ONE
    vaek_cov_spectrum_rows call with n = 2R and one device -> host copy.

    event() does NOT perturb the run: `m.key`, the dataset's `_draws` and `m._latent_draws` are neither split nor advanced.  Its draws
    have a counter of their own, `m._spectrum_draws` (incremented before use), the seed dataset.key[0] ^ dataset.key[1] and the tags 5
    (rows) and 6 (latents); tags 0 .. 4 belong to the train loop, the dataset's batches, the latents and the log-likelihood.  The fake
    batch is sampled with the model's `current_epsilon`.  Returns per model {"learnt eigenvalue", "ground truth eigenvalue"} (float64
    arrays, ascending) and appends them to `m.ht_eigen` and `m.gt_eigen`.  Raises RuntimeError naming the model where a solve hit the
    sweep cap without converging (off_F > 2^-40 |C|_F)."""

    KEYS = ("learnt eigenvalue", "ground truth eigenvalue")
    X_TAG, Z_TAG = 5, 6
    NAME = "ReplicaSpectrum"
    OFF_BOUND = 2.0 ** -40
    VEC = False                        # ReplicaSubspace: the eigen records and entry points

    def __init__(self, vae_models, rows=None):
        _replica_setup(self, vae_models, self.NAME, "call", "rows", "evaluates", "train_loop_max_replicas", ReplicaLogLik._shape,
                       self._check_covered)
        R, m0 = self.R, self.ms[0]
        self.rows = _event_rows(self.NAME, m0, rows, 2, self.eng.stats_event_max_rows, "vaek_stats_event_max_rows", "; one row has no covariance")
        dev = self.eng.device
        self.D = self.eng.D
        self.record_len = self.eng.cov_eigen_record_len if self.VEC else self.eng.cov_spectrum_record_len
        self.fused = bool(self.eng.supports_spectrum_event(self.kind))
        self.buf = torch.zeros(2 * R * self.record_len + self._extra_doubles(), dtype=torch.float64, device=dev)
        self.out = self.buf[:2 * R * self.record_len].view(2 * R, self.record_len)          # [R, 2 records] on the fused route
        if self.fused:
            self.params = torch.zeros(R, m0.model.flat.numel(), dtype=torch.float32, device=dev)
        else:
            self.stack = torch.zeros(2 * R, self.rows, self.D, dtype=torch.float32, device=dev)

    def _extra_doubles(self):
        return 0                       # doubles behind the records in the one buffer event() copies to the host

    def _after_solve(self):
        pass                           # device work between the solve and the copy

    def _check_covered(self):
        if not self.eng.supports_cov_spectrum():
            raise RuntimeError(f"ReplicaSpectrum: vaek_cov_spectrum_rows does not cover this model (it needs data_dim <= 32; this model's "
                               f"data_dim: {getattr(self.eng, 'D', '?')})")

    def event(self):
        """One evaluation of every model: [{"learnt eigenvalue", "ground truth eigenvalue"} of model 0, ...]."""
        dev = self.eng.device
        R, D = self.R, self.D
        seeds, steps, eps_in = [], [], []
        for m in self.ms:
            m._spectrum_draws = getattr(m, "_spectrum_draws", 0) + 1
            ds = m.dataset
            seeds.append(ds.key[0] ^ ds.key[1])
            steps.append(m._spectrum_draws)
            eps_in.append(float(torch.as_tensor(m.current_epsilon).reshape(-1)[0]))       # sample_batch: the model's current eps
        if self.fused:
            for r, m in enumerate(self.ms):
                self.params[r].copy_(m.model.flat)
            sd, st = _seed_step_tensors(seeds, steps, dev)
            call = self.eng.eigen_event_replicas if self.VEC else self.eng.spectrum_event_replicas
            call(self.params, self.rows, self.kind, self.A, self.dd, self.did, self.pad, self.var, sd, st, sd, st,
                 torch.tensor(eps_in, dtype=torch.float32).to(dev), self.out.view(R, 2 * self.record_len), a_stride=self.a_stride,
                 x_tag=self.X_TAG, z_tag=self.Z_TAG)
        else:
            for r, m in enumerate(self.ms):
                eng = m.model.module.engine(self.rows)                                 # forward takes at most its context's batch
                Ar = None if self.A is None else self.A[r]
                eng.make_batch(self.kind, Ar, self.dd, self.did, self.pad, self.var, self.rows, seeds[r], step=steps[r], tag=self.X_TAG,
                               out=(self.stack[2 * r + 1], None, None))
                _, z1, z2 = eng.make_batch(self.kind, Ar, self.dd, self.did, self.pad, self.var, self.rows, seeds[r], step=steps[r],
                                           tag=self.Z_TAG, want_x=False)
                fake, _ = eng.forward(m.model.flat, None, z1, z2, sampling=True, eps=eps_in[r], want_mu=False)
                self.stack[2 * r].copy_(fake)
            (self.eng.cov_eigen_rows if self.VEC else self.eng.cov_spectrum_rows)(self.stack, self.rows, self.out)
        self._after_solve()
        host = self.buf.cpu().numpy()                                                 # the event's ONE device -> host copy
        rec = host[:2 * R * self.record_len].reshape(2 * R, self.record_len)
        stats = []
        for r, m in enumerate(self.ms):
            st = self._model_stats(r, m, rec, host)
            m.ht_eigen.append(st[self.KEYS[0]])
            m.gt_eigen.append(st[self.KEYS[1]])
            stats.append(st)
        return stats

    def _model_stats(self, r, m, rec, host):
        D = self.D
        st = {}
        for side, name in enumerate(self.KEYS):                                   # record 2 r: the fake side, 2 r + 1: the real side
            row = rec[2 * r + side]
            tail = row[2 * D + D * D:]                                             # sweeps, off_F, |C|_F, rows
            _check_solve(self.NAME, r, m, f"{name} solve", "C", tail[0], tail[1], self.OFF_BOUND * tail[2])
            st[name] = row[:D].copy()
        return st


class ReplicaSubspace(ReplicaSpectrum):
    """ReplicaSpectrum with eigenvectors: per model also the principal angles between the span of the k leading eigenvectors of
    cov(fake batch) and that of cov(real batch) -- whether the generator's mass lies in the subspace the data lives in -- and their
    distance |sin Theta|_F, the well-defined form of the reference's unused sin_theta_distance (utils.py:317-325).

    Validation, the counter `m._spectrum_draws`, the seed and the tags 5 / 6 are ReplicaSpectrum's, so event() perturbs nothing of the
    run and its eigenvalues are bitwise ReplicaSpectrum's under the same counter.  k defaults to the dimension of the dataset's linear
    span: linear_gaussian min(dd, did), sigmoid dd + 1, sphere dd.  Linear models: ONE vaek_eigen_event_replicas call, ONE
    vaek_subspace_angles call (a = fake, b = real, ka = kb = k) and one device -> host copy; every other model takes the host route
    (rows into one vaek_cov_eigen_rows call with n = 2R), then the same angles call.  Returns per model "learnt eigenvalue", "ground
    truth eigenvalue", "Principal Angles" (radians, ascending: arcsin sqrt clip(sin^2, 0, 1)) and "Subspace Distance" (the root of the
    record's direct sum of squares), and appends the last two to `m.principal_angles` and `m.subspace_distances`.  Raises RuntimeError
    naming the model where a solve -- of either covariance or of the angles -- ended above 2^-40 of its norm."""

    NAME = "ReplicaSubspace"
    VEC = True
    ANGLES, DISTANCE = "Principal Angles", "Subspace Distance"

    def __init__(self, vae_models, k=None, rows=None):
        self._k_arg = k
        super().__init__(vae_models, rows=rows)

    @staticmethod
    def default_k(kind, dd, did):
        """The dimension of the dataset's linear span: linear_gaussian min(dd, did), sigmoid dd + 1, sphere dd."""
        return {0: min(dd, did), 1: dd + 1, 2: dd}[int(kind)]

    def _extra_doubles(self):
        k = self.default_k(self.kind, self.dd, self.did) if self._k_arg is None else int(self._k_arg)
        if not 1 <= k <= self.D:
            raise RuntimeError(f"{self.NAME}: k = {k}, need 1 .. data_dim = {self.D}")
        self.k = k
        self.angle_len = self.eng.subspace_record_len(k)
        return self.R * self.angle_len

    def _after_solve(self):
        R, ln = self.R, self.record_len
        self.angles = self.buf[2 * R * ln:].view(R, self.angle_len)
        pairs = self.out.view(R, 2 * ln)                                               # pair r: a = the fake record, b = the real one
        self.eng.subspace_angles(pairs, pairs[:, ln:], self.k, self.k, self.angles, n=R, a_stride=2 * ln, b_stride=2 * ln)

    def _model_stats(self, r, m, rec, host):
        st = super()._model_stats(r, m, rec, host)
        k = self.k
        row = host[2 * self.R * self.record_len:].reshape(self.R, self.angle_len)[r]
        sin2, off = row[:k], row[k + 2]
        norm = float(np.sqrt(np.sum(sin2 * sin2) + off * off))
        _check_solve(self.NAME, r, m, "principal-angle solve", "G", row[k + 1], off, self.OFF_BOUND * norm)
        st[self.ANGLES] = np.arcsin(np.sqrt(np.clip(sin2, 0.0, 1.0)))
        st[self.DISTANCE] = float(np.sqrt(row[k]))
        for name, key in (("principal_angles", self.ANGLES), ("subspace_distances", self.DISTANCE)):
            if not hasattr(m, name):
                setattr(m, name, [])
            getattr(m, name).append(st[key])
        return st


class ReplicaGraphLoop:
    """A sweep of three-hidden-layer MLP VAEs (step path "mlp3") as GraphLoop's pipelined hipGraph loop with R models per step: R
    VAEModels of one shape -- validated as in ReplicaLoop: one batch size, data and latent dimension, architecture, epsilon,
    dataset kind, -dd, -did, padding and dataset noise -- each with its own dataset matrix, parameters, Adam state and learning
    rate.  Every step is ONE vaek_train_step_gen_replicas call (csrc/fused_mlp3.hip: two launches, blockIdx.y = model): it trains
    model r on its slice of one stacked batch buffer and draws model r's next batch into its slice of the other.  Model r's RNG
    seed is the one GraphLoop derives for it, so model r ends bitwise where GraphLoop(model r, moments=False, resident=False) ends.

    The states live in [R, stride] stacks owned by the loop, stride = P rounded up to a multiple of 4 (the library's stride rule);
    they are COPIED at the boundaries of run(), in before the steps and out after them, as in ReplicaLoop: between two run() calls
    every model is an ordinary model.  The stacked batch buffers hold each model's NEXT batch between runs; a model whose step
    counter was changed between two runs (a loaded checkpoint) has the buffers drawn afresh.

    As in GraphLoop there are two batch buffers and a generator counter pair per model ([R, 2]); a graph of steps_per_graph steps
    (made even) is captured once, after one eager warm-up step, and replayed on the buffer parity it was captured on.  Single GPU
    only.  Neither launch waits for anything: check() polls nothing."""

    def __init__(self, vae_models, steps_per_graph=200, loss_capacity=None):
        def covered():
            if not self.eng.supports_train_step_replicas():
                raise RuntimeError("ReplicaGraphLoop: vaek_train_step_gen_replicas does not cover this model (it needs the \"mlp3\" train step: "
                                   "float32, three hidden layers of 64 .. 256 units in encoder and decoder, D, L <= 32, a batch of at most 128 rows)")
        _replica_setup(self, vae_models, "ReplicaGraphLoop", "step", "batches", "trains", "train_step_max_replicas", ReplicaLoop._signature,
                       covered)
        ms, R, m0 = self.ms, self.R, self.ms[0]
        self.B = m0.batch_size
        self.G = int(steps_per_graph) + int(steps_per_graph) % 2      # two batch buffers: a replay starts on the parity it was captured on
        dev = self.eng.device
        D, L = self.eng.D, self.eng.L
        self.P, GL = m0.model.flat.numel(), m0.optimizer.state.grads.numel()
        self.stride = (self.P + 3) // 4 * 4
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.params, self.m, self.v, self.grads = f32(R, self.stride), f32(R, self.stride), f32(R, self.stride), f32(R, GL)
        self.step_dev = torch.zeros(R, dtype=torch.int32, device=dev)
        self.seed_list = [(m.dataset.key[0] ^ m.dataset.key[1] ^ m.key[1]) & (2 ** 64 - 1) for m in ms]      # GraphLoop's, model by model
        self.seeds = torch.tensor([_wrap_signed(s, 64) for s in self.seed_list], dtype=torch.int64, device=dev)
        self.lrs = torch.tensor([float(m.optimizer.optimizer_def.learning_rate) for m in ms], dtype=torch.float32, device=dev)
        if loss_capacity is None:             # every step of the longest schedule among the models
            loss_capacity = max(int(getattr(m, "num_batches", 0) or 0) for m in ms) or (1 << 16)
        self.rings = f32(R, int(loss_capacity))
        self.bufs = [(f32(R, self.B, D), f32(R, self.B, L), f32(R, self.B, D)) for _ in range(2)]
        self.counter = torch.zeros(R, 2, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(max(self.eng.train_step_replicas_workspace(R), 16), dtype=torch.uint8, device=dev)
        self.par = 0                          # the buffer that holds the next step's batches
        self.expect = None                    # the models' step counters at which self.bufs[self.par] is valid
        self.graph = None
        self.graph_parity = 0

    def _rows(self, m, r):
        st = m.optimizer.state
        P = self.P
        return ((self.params[r, :P], m.model.flat), (self.grads[r], st.grads), (self.m[r, :P], st.m), (self.v[r, :P], st.v),
                (self.step_dev[r:r + 1], st.step_dev))

    def _prime(self):
        """Model r's batch of its next step n_r into self.bufs[self.par][.][r] and its counter pair to (n_r, n_r + 1) in the order
        the steps alternate in -- GraphLoop's invariant, model by model (vaek_make_batch_next on each model's slices)."""
        p = self.par
        steps = [int(m.optimizer.state.step) for m in self.ms]
        self.counter.copy_(torch.tensor([[n, n] for n in steps], dtype=torch.int32))
        for r in range(self.R):
            self.eng.make_batch(self.kind, None if self.A is None else self.A[r], self.dd, self.did, self.pad, self.var, self.B,
                                self.seed_list[r], tag=0, row0=0, out=tuple(t[r] for t in self.bufs[p]), counter=self.counter[r], which=p)
        self.expect = steps

    def _one(self):
        p = self.par
        self.eng.train_step_gen_replicas(self.params, self.grads, self.m, self.v, self.step_dev, self.bufs[p], 0.0, self.kind, self.A,
                                         self.dd, self.did, self.pad, self.var, self.bufs[p ^ 1], self.seeds, self.counter, p ^ 1,
                                         lrs=self.lrs, a_stride=self.a_stride, loss_hist=self.rings, workspace=self.workspace, tag=0,
                                         row0=0)
        self.par = p ^ 1

    def _capture(self):
        self._one()                              # warm-up outside capture (lazy kernel attributes)
        torch.cuda.synchronize()
        self.graph_parity = self.par
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(self.G):          # an even number of steps: self.par ends where it began
                    self._one()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = g
        return 1

    def run(self, n_steps):
        """Exactly n_steps train steps of every model: one library call per step (or per replayed graph node) between the copies
        in and out."""
        if n_steps <= 0:
            return
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                row.copy_(own)
        if self.expect != [int(m.optimizer.state.step) for m in self.ms]:
            self._prime()
        done = 0
        if self.graph is None and n_steps >= self.G + 1:
            done += self._capture()
        if self.graph is not None and n_steps - done > self.G and self.par != self.graph_parity:
            self._one()                          # back onto the buffer parity the graph was captured on
            done += 1
        if self.graph is not None and self.par == self.graph_parity:
            while n_steps - done >= self.G:
                self.graph.replay()
                done += self.G
        for _ in range(n_steps - done):
            self._one()
        for r, m in enumerate(self.ms):
            for row, own in self._rows(m, r):
                own.copy_(row)
            m.optimizer.state.step += n_steps
        self.expect = [int(m.optimizer.state.step) for m in self.ms]

    def describe(self):
        """One line for run.py."""
        return (f"hipGraph of {self.G} steps, {self.R} replicas per step (vaek_train_step_gen_replicas), "
                "next batches drawn inside the step's second launch")

    def stats_event(self, rows=None):
        """One stats event of every model in ONE call (ReplicaStatsMlp3, vaek_mlp3_stats_event_replicas): [compute_stats' dict of model
        0, ...], with the models' keys, draw counters and lists advanced exactly as compute_stats would advance them."""
        if getattr(self, "_stats", None) is None or (rows is not None and int(rows) != self._stats.rows):
            self._stats = ReplicaStatsMlp3(self.ms, rows=rows)
        return self._stats.event()

    def check(self):
        """Nothing to poll: neither launch has a wait."""

    def losses(self, r):
        """Losses of all steps model r has run so far, in order (device -> host once)."""
        n = self.ms[r].optimizer.state.step
        cap = self.rings.shape[1]
        ring = self.rings[r].cpu()
        if n <= cap:
            return ring[:n]
        k = n % cap
        return torch.cat([ring[k:], ring[:k]])

    def view(self, r):
        """Model r's `_graph_loop`: losses() without an argument, as VAEModel.model_save_data calls it."""
        return _ReplicaLosses(self, r)
