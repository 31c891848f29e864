"""The evaluations of the n_print events, each ONE library call for R models of one shape: the fused stats events (ReplicaStats,
ReplicaStatsMlp3) and the observables that observables.py tables -- ReplicaLogLik / ReplicaLogLikMlp3, ReplicaExactLogLik,
ReplicaElboHessian, ReplicaSampledElboHessian / ReplicaSampledElboHessianMlp3, ReplicaSpectrum / ReplicaSubspace and ReplicaJacobianMlp3 / ReplicaJacobianLinear -- on one spine, ReplicaEvent.  trainer.py re-exports
every name of this module.

The RNG tags: 0 the train loop, 1 the dataset's batches, 2 the latents (ReplicaStats draws what compute_stats draws), 3 / 4 the
log-likelihood (rows / samples; the exact event and, after it, the Hessian can draw tag 3's rows again), 5 / 6 the spectra,
7 / 8 the Jacobian, 9 / 10 the Hessian, 11 / 12 / 13 the sampled Hessian (rows / samples / start vector),
14 / 15 / 16 the MLP sampled Hessian."""
from __future__ import annotations

import numpy as np
import torch


def _wrap_signed(value, bits):
    """`value` modulo 2^bits as the signed integer of that width: how a seed (64) or an RNG step (32) goes into an int64 / int32 tensor."""
    value &= (1 << bits) - 1
    return value - (1 << bits) if value >> (bits - 1) else value


def _signature(m, spec):
    """What the models of one ReplicaLoop share: batch size, dimensions, parameter count, architecture and dataset spec."""
    eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
    cfg = getattr(eng, "cfg", None)
    arch = None if cfg is None else (cfg.n_enc_hidden, cfg.n_dec_hidden, cfg.sigmoid_decoder, cfg.tunable_eps, cfg.eps_cli, cfg.dtype,
                                     cfg.force_generic, cfg.global_batch)
    kind, A, dd, did, pad, var = spec
    return (m.batch_size, eng.D, eng.L, m.model.flat.numel(), arch, kind, None if A is None else A.numel(), dd, did, pad, float(var))


def _shape(m, spec):
    """_signature without what depends on the batch size (the batch itself and the engine's global batch)."""
    sig = _signature(m, spec)
    arch = sig[4]
    return sig[1:4] + (None if arch is None else arch[:-1],) + sig[5:]


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


def _seed_step_tensors(seeds, steps, dev):
    """The uint64 seeds and uint32 RNG steps of a call as the int64 / int32 device tensors the library takes (their bits)."""
    return (torch.tensor([_wrap_signed(s, 64) for s in seeds], dtype=torch.int64).to(dev),
            torch.tensor([_wrap_signed(s, 32) for s in steps], dtype=torch.int32).to(dev))


class ReplicaEvent:
    """What the event classes share: the validation of the models (one shape, one GPU, at most train_loop_max_replicas) and of the
    rows per event, an [R, P] stack the parameters are copied into at every event (the rule of ReplicaLoop.run: between two calls
    the models are ordinary models), the event's own RNG counter on every model -- incremented before use, or replaced by a given
    `step=` --, the seed dataset.key[0] ^ dataset.key[1], ONE device -> host copy of the records, the refusal of a Jacobi solve that
    did not converge and per-model lists created on demand.  A subclass sets NAME, NOUN (what evaluates the replicas), SIGNATURE
    (what the models must share), ROWS = (fewest rows, the engine attribute that caps them, a note for the refusal) and COUNTER,
    and overrides _check_covered, _check_args (refusals between the models' and the rows') and _allocate (its buffers)."""

    NOUN, DRAWS = "launch", "rows"
    SIGNATURE = staticmethod(_shape)             # one shape, any batch size: the calls read parameters only
    ROWS = (1, "log_likelihood_max_rows", "")
    OFF_BOUND = 2.0 ** -40
    STACK = True                                 # the spine allocates the [R, P] stack; ReplicaSpectrum its own, on the fused route only

    def __init__(self, vae_models, rows=None):
        _replica_setup(self, vae_models, self.NAME, self.NOUN, self.DRAWS, "evaluates", "train_loop_max_replicas", self.SIGNATURE,
                       self._check_covered)
        self._check_args()
        lo, cap, note = self.ROWS
        rows = int(getattr(self.ms[0], "print_batch_size", 1000) if rows is None else rows)      # model 0's print batch unless given
        if not lo <= rows <= getattr(self.eng, cap):
            raise RuntimeError(f"{self.NAME}: {rows} rows per event, need {lo} .. {getattr(self.eng, cap)} (vaek_{cap}{note})")
        self.rows = rows
        if self.STACK:
            self.params = self._param_stack()
        self._allocate(self.R, self.eng.device)

    def _check_args(self):
        pass

    def _param_stack(self):
        return torch.zeros(self.R, self.ms[0].model.flat.numel(), dtype=torch.float32, device=self.eng.device)

    def _stack_params(self):
        for r, m in enumerate(self.ms):
            self.params[r].copy_(m.model.flat)

    def _seeds(self):
        return [m.dataset.key[0] ^ m.dataset.key[1] for m in self.ms]

    def _own_steps(self):
        """The RNG step of this event's draws, per model: its own counter on the model, incremented before use."""
        for m in self.ms:
            setattr(m, self.COUNTER, getattr(m, self.COUNTER, 0) + 1)
        return [getattr(m, self.COUNTER) for m in self.ms]

    def _given_steps(self, step):
        """event(step=...): one int for all models or one per model, as a list; None stays."""
        if step is None:
            return None
        given = [int(s) for s in step] if isinstance(step, (list, tuple)) else [int(step)] * self.R
        if len(given) != self.R:
            raise RuntimeError(f"{self.NAME}.event(step=...): {len(given)} steps for {self.R} models")
        return given

    def _drawn(self):
        """The keywords of a call that draws its rows: the dataset spec and the stack of dataset matrices."""
        return dict(kind=self.kind, A=self.A, dd=self.dd, did=self.did, pad=self.pad, var_added=self.var, a_stride=self.a_stride)

    def _records(self, buf=None):
        return (self.out if buf is None else buf).cpu()                           # the event's ONE device -> host copy

    def _check_solve(self, r, what, mat, sweeps, off, bound):
        """Refuse the record of model r whose Jacobi solve (`what`, of the matrix `mat`) hit the sweep cap with off_F above `bound` =
        2^-40 of the matrix's norm."""
        if not off <= bound:
            raise RuntimeError(f"{self.NAME}: model {r} ({getattr(self.ms[r], 'dirname', '?')}): the {what} stopped at the cap of "
                               f"{int(sweeps)} sweeps with off_F = {off:.3e} > 2^-40 |{mat}|_F = {bound:.3e}")

    @staticmethod
    def _append(m, **lists):
        """Append each value to the model's list of that name, created on demand."""
        for name, value in lists.items():
            if not hasattr(m, name):
                setattr(m, name, [])
            getattr(m, name).append(value)


class ReplicaStats(ReplicaEvent):
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

    NAME = "ReplicaStats"              # ReplicaStatsMlp3 overrides the name and three methods
    DRAWS = "batches"
    SIGNATURE = staticmethod(_signature)
    ROWS = (1, "stats_event_max_rows", "")

    def _allocate(self, R, dev):
        from .datasets import SCORE_KEYS
        self.score_keys = SCORE_KEYS[self.kind]
        self.L = self.eng.L
        self.record_len = self.eng.stats_record_len
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
        rec = self._records()
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


class ReplicaLogLik(ReplicaEvent):
    """The importance-weighted log-likelihood of R VAEModels of one shape in ONE library call (vaek_log_likelihood_replicas,
    csrc/linear_loglik.hip): per model, over `rows` data rows drawn from its dataset and `samples` = K posterior samples per row,
    the IWAE-K bound on log p(x) -- the `Average Log Likelihood` the reference reserves and never fills -- the K-sample ELBO estimate
    and the normalised effective sample size of the weights.

    The models are validated as in ReplicaLoop (one shape, architecture, epsilon, dataset kind, -dd, -did, padding, noise) but with
    NO condition on the batch size: the call reads parameters only, so models of any train batch -- and of different ones -- qualify.

    event() makes ONE library call and ONE device -> host copy of the [R, 4] records.  It does NOT perturb the run: `m.key`, the
    dataset's `_draws` and `m._latent_draws` are neither split nor advanced.  Its draws have a counter of their own,
    `m._loglik_draws` (the first event draws under step 1), and the tags 3 (rows) and 4 (samples).  Returns per model {"Average Log
    Likelihood", "ELBO estimate", "Effective Sample Size"} (host tensors) and appends the first to `m.average_log_likelihoods`."""

    KEYS = ("Average Log Likelihood", "ELBO estimate", "Effective Sample Size")
    X_TAG, Z_TAG = 3, 4
    NAME = "ReplicaLogLik"             # ReplicaLogLikMlp3 overrides the name and four methods
    NOUN = "call"
    COUNTER = "_loglik_draws"
    _shape = staticmethod(_shape)

    def __init__(self, vae_models, samples, rows=None):
        self.samples = int(samples)
        super().__init__(vae_models, rows)

    def _check_args(self):
        if not 1 <= self.samples <= self.eng.log_likelihood_max_samples:
            raise RuntimeError(f"{self.NAME}: {self.samples} samples per row, need 1 .. {self.eng.log_likelihood_max_samples} "
                               "(vaek_log_likelihood_max_samples)")

    def _allocate(self, R, dev):
        self._check_size()
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

    def event(self):
        """One evaluation of every model: [{"Average Log Likelihood", "ELBO estimate", "Effective Sample Size"} of model 0, ...]."""
        self._stack_params()
        seeds, steps = _seed_step_tensors(self._seeds(), self._own_steps(), self.eng.device)
        self._call(self.params, self.rows, self.samples, seeds, steps, self.out, self.workspace, x_seeds=seeds, x_steps=steps,
                   x_tag=self.X_TAG, z_tag=self.Z_TAG, **self._drawn())
        rec = self._records()
        stats = []
        for r, m in enumerate(self.ms):
            st = {name: rec[r, k].clone() for k, name in enumerate(self.KEYS)}
            m.average_log_likelihoods.append(st[self.KEYS[0]])
            stats.append(st)
        return stats


class ReplicaLogLikMlp3(ReplicaLogLik):
    """ReplicaLogLik for three-hidden-layer MLP VAEs (vaek_mlp3_log_likelihood_replicas, csrc/mlp3_loglik.hip): the same contract --
    one shape, any batch size, ONE library call and ONE device -> host copy per event, the same three keys, the counter
    `m._loglik_draws`, tags 3 and 4, nothing of the run touched, the first key appended to `m.average_log_likelihoods` -- on models
    Engine.supports_mlp3_log_likelihood covers, with one more cap: R * rows * samples at most
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


class ReplicaExactLogLik(ReplicaEvent):
    """The EXACT log-likelihood, the exact ELBO and their difference KL(q(z|x) || p(z|x)) of R one-decoder linear VAEModels of one
    shape in ONE launch (vaek_exact_log_likelihood_replicas, csrc/exact_loglik.inc): such a model is a linear-Gaussian
    latent-variable model, p(x) = N(b_d, K^T K + e^eps I), so what ReplicaLogLik estimates has a closed form -- float64 on the device,
    through the eigenvectors of K^T K.

    event() makes ONE library call and ONE device -> host copy of the [R, 10 + D] float64 records.  It does NOT perturb the run:
    `m.key`, the dataset's `_draws`, `m._latent_draws` and `m._loglik_draws` are left alone.  Its draws have a counter of their own,
    `m._exact_loglik_draws`, and row tag 3 -- ReplicaLogLik's row tag, so event(step=s) with the step a ReplicaLogLik event just used
    scores the rows that event scored, bit for bit (with `step` given the counter is neither read nor advanced).  Returns per model
    {"Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning"} (Python floats; the last is the record's
    bound on the relative error of the smallest eigenvalue of the model covariance, (off_F + 64 D 2^-53 |K^T K|_F) e^-eps: large
    means ill-conditioned, reported, not hidden).  Raises RuntimeError naming the model where the solve ended with off_F > 2^-40
    |K^T K|_F."""

    KEYS = ("Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning")
    SLOTS = (0, 1, 2, 8)
    X_TAG = ReplicaLogLik.X_TAG
    NAME = "ReplicaExactLogLik"
    COUNTER = "_exact_loglik_draws"
    IWAE_GAP = "IWAE Gap"

    def _allocate(self, R, dev):
        self.record_len = self.eng.exact_log_likelihood_record_len
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)

    def _check_covered(self):
        if not self.eng.supports_exact_log_likelihood(self.kind):
            raise RuntimeError("ReplicaExactLogLik: vaek_exact_log_likelihood_replicas does not cover this model / dataset (it needs a "
                               "float32 linear VAE -- no hidden layers -- with ONE decoder and D, L <= 32: the sigmoid second decoder has "
                               f"no closed form; this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def event(self, step=None):
        """One evaluation of every model: [{"Exact Log Likelihood", "Exact ELBO", "Posterior KL", "Exact Likelihood Conditioning"} of
        model 0, ...].  step: draw the rows under this RNG step (one int, or one per model) instead of the models' own counters."""
        given = self._given_steps(step)
        self._stack_params()
        seeds, steps = _seed_step_tensors(self._seeds(), self._own_steps() if given is None else given, self.eng.device)
        self.eng.exact_log_likelihood_replicas(self.params, self.rows, self.out, x_seeds=seeds, x_steps=steps, x_tag=self.X_TAG,
                                               **self._drawn())
        rec = self._records().numpy()
        stats = []
        for r in range(self.R):
            row = rec[r]
            self._check_solve(r, "solve of K^T K", "K^T K", row[5], row[6], self.OFF_BOUND * row[7])
            stats.append({name: float(row[k]) for name, k in zip(self.KEYS, self.SLOTS)})
        return stats

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


class ReplicaElboHessian(ReplicaEvent):
    """The curvature of the loss surface R one-decoder linear VAEModels of one shape sit on, in ONE launch
    (vaek_elbo_hessian_lanczos_replicas, csrc/elbo_hessian.hip): `steps` <= 32 Lanczos steps with full reorthogonalisation on the
    Hessian of f = -mean exact ELBO over `rows` data rows -- the population training objective on those rows, float64, closed form
    -- give its extreme Ritz values (sharpness and the smallest curvature: minimum or saddle), a rigorous residual bound per value,
    and the exact gradient norm: how stationary the point Adam sits at really is.

    event() draws each model's start vector with vaek_rng_fill (float32 normals, widened), makes ONE Lanczos call and ONE device ->
    host copy of the [R, 140] float64 records.  It does NOT perturb the run: `m.key`, the dataset's `_draws`, `m._latent_draws` and
    the other events' counters are left alone.  Its draws have a counter of their own, `m._elbo_hessian_draws`, and the tags 9 (rows)
    and 10 (start vector).  event(step=s) draws the ROWS under step s and ReplicaExactLogLik's row tag instead, so the Hessian is that
    of the objective on the rows a ReplicaExactLogLik event just scored, bit for bit (the start vector stays under the own counter).
    Returns per model {"ELBO Hessian Ritz Values" (float64 [k], ascending), "ELBO Hessian Ritz Residuals" (float64 [k]: an eigenvalue
    of H lies within each of its Ritz value), "Sharpness" (the largest Ritz value), "ELBO Hessian Min Ritz", "ELBO Gradient Norm"}.
    Raises RuntimeError naming the model where the solve of T ended with off_F > 2^-40 |T|_F."""

    KEYS = ("ELBO Hessian Ritz Values", "ELBO Hessian Ritz Residuals", "Sharpness", "ELBO Hessian Min Ritz", "ELBO Gradient Norm")
    X_TAG, V_TAG = 9, 10
    NAME = "ReplicaElboHessian"
    COUNTER = "_elbo_hessian_draws"
    HEAD, BLOCK = 12, 32

    def __init__(self, vae_models, steps=32, rows=None):
        self.steps = int(steps)
        super().__init__(vae_models, rows)

    def _check_args(self):
        if not 1 <= self.steps <= self.eng.elbo_hessian_max_steps:
            raise RuntimeError(f"{self.NAME}: {self.steps} Lanczos steps, need 1 .. {self.eng.elbo_hessian_max_steps} "
                               "(vaek_elbo_hessian_max_steps)")

    def _allocate(self, R, dev):
        self.P = P = self.params.shape[1]
        self.record_len = self.eng.elbo_hessian_record_len
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
        given = self._given_steps(step)
        self._stack_params()
        seeds, own = self._seeds(), self._own_steps()
        for r in range(self.R):
            self.v0[r].copy_(self.eng.rng_fill(self.P, seeds[r], step=own[r], tag=self.V_TAG))      # widened on the copy
        seeds, steps = _seed_step_tensors(seeds, own if given is None else given, self.eng.device)
        self.eng.elbo_hessian_lanczos_replicas(self.params, self.rows, self.steps, self.v0, self.basis, self.out, x_seeds=seeds,
                                               x_steps=steps, x_tag=self.X_TAG if given is None else ReplicaExactLogLik.X_TAG,
                                               **self._drawn())
        rec = self._records().numpy()
        stats = []
        for r in range(self.R):
            row = rec[r]
            self._check_solve(r, "solve of the Lanczos matrix T", "T", row[4], row[5], self.OFF_BOUND * row[6])
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


class ReplicaSampledElboHessian(ReplicaEvent):
    """The curvature of the SAMPLE-AVERAGE ELBO of R linear VAEModels of one shape with ONE OR TWO decoders
    (vaek_sampled_elbo_hessian_lanczos_replicas, csrc/sampled_hessian.hip): the rows and `samples` latent samples per row are fixed
    (common random numbers), so the Monte-Carlo ELBO f_K is a smooth function of the parameters; `steps` <= 32 Lanczos steps with full
    reorthogonalisation on its exact Hessian give what ReplicaElboHessian gives for the closed form -- which a model with the sigmoid
    second decoder does not have.

    event() draws each model's start vector with vaek_rng_fill, makes ONE Lanczos call (3 + 2 steps launches) and ONE device -> host
    copy of the [R, 142] float64 records.  It does NOT perturb the run: its draws have a counter of their own,
    `m._sampled_hessian_draws`, and the tags 11 (rows), 12 (samples) and 13 (start vector).  event(step=s) draws the ROWS under step s
    and ReplicaExactLogLik's row tag (or `x_tag`) instead; samples and start vector stay under the own counter.  Returns per model
    {"Sampled ELBO Hessian Ritz Values" (float64 [k], ascending), "Sampled ELBO Hessian Ritz Residuals" (float64 [k]), "Sampled
    Sharpness" (the largest Ritz value), "Sampled ELBO Hessian Min Ritz", "Sampled ELBO Gradient Norm"}.  Raises RuntimeError naming
    the model where the solve of T ended with off_F > 2^-40 |T|_F."""

    KEYS = ("Sampled ELBO Hessian Ritz Values", "Sampled ELBO Hessian Ritz Residuals", "Sampled Sharpness", "Sampled ELBO Hessian Min Ritz",
            "Sampled ELBO Gradient Norm")
    GAP = "Sharpness Sampling Gap"
    X_TAG, Z_TAG, V_TAG = 11, 12, 13
    NAME = "ReplicaSampledElboHessian"
    NOUN = "call"
    COUNTER = "_sampled_hessian_draws"
    HEAD, BLOCK = 12, 32
    MAX_REPLICA_COLUMNS = 1 << 16
    ENTRY = "sampled_elbo_hessian"               # the engine's supports_<ENTRY>, <ENTRY>_max_columns, _workspace and _lanczos_replicas
    COVERS = ("a float32 linear VAE -- no hidden layers -- with one or two decoders and D, L <= 32, D <= 28 with two")

    def __init__(self, vae_models, steps=32, samples=8, rows=None):
        self.steps, self.samples = int(steps), int(samples)
        super().__init__(vae_models, rows)

    def _check_args(self):
        if not 1 <= self.steps <= self.eng.elbo_hessian_max_steps:
            raise RuntimeError(f"{self.NAME}: {self.steps} Lanczos steps, need 1 .. {self.eng.elbo_hessian_max_steps} "
                               "(vaek_elbo_hessian_max_steps)")
        if not 1 <= self.samples <= self.eng.log_likelihood_max_samples:
            raise RuntimeError(f"{self.NAME}: {self.samples} samples per row, need 1 .. {self.eng.log_likelihood_max_samples} "
                               "(vaek_log_likelihood_max_samples)")

    def _allocate(self, R, dev):
        cols, cap = R * self.rows * self.samples, getattr(self.eng, self.ENTRY + "_max_columns")
        if self.rows * self.samples > self.MAX_REPLICA_COLUMNS or cols > cap:
            raise RuntimeError(f"{self.NAME}: {R} models x {self.rows} rows x {self.samples} samples = {cols} columns, at most {cap} fit one "
                               f"call and {self.MAX_REPLICA_COLUMNS} one model (vaek_{self.ENTRY}_max_columns)")
        self.P = P = self.params.shape[1]
        self.record_len = self.eng.sampled_elbo_hessian_record_len
        self.v0 = torch.zeros(R, P, dtype=torch.float64, device=dev)
        self.basis = torch.zeros(R, self.steps, P, dtype=torch.float64, device=dev)
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)
        self.workspace = torch.zeros(getattr(self.eng, self.ENTRY + "_workspace")(R, self.rows, self.samples), dtype=torch.uint8, device=dev)

    def _check_covered(self):
        if not getattr(self.eng, "supports_" + self.ENTRY)(self.kind):
            raise RuntimeError(f"{self.NAME}: vaek_{self.ENTRY}_lanczos_replicas does not cover this model / dataset (it "
                               f"needs {self.COVERS}; "
                               f"this model's step path: {getattr(self.eng, 'step_path', '?')})")

    def event(self, step=None, x_tag=None):
        """One evaluation of every model.  step: draw the ROWS under this RNG step (one int, or one per model) and ReplicaExactLogLik's
        row tag (x_tag: another event's) instead of the own counter and tag 11."""
        given = self._given_steps(step)
        self._stack_params()
        seeds, own = self._seeds(), self._own_steps()
        for r in range(self.R):
            self.v0[r].copy_(self.eng.rng_fill(self.P, seeds[r], step=own[r], tag=self.V_TAG))      # widened on the copy
        z_seeds, z_steps = _seed_step_tensors(seeds, own, self.eng.device)
        x_seeds, x_steps = _seed_step_tensors(seeds, own if given is None else given, self.eng.device)
        tag = self.X_TAG if given is None else (ReplicaExactLogLik.X_TAG if x_tag is None else int(x_tag))
        getattr(self.eng, self.ENTRY + "_lanczos_replicas")(self.params, self.rows, self.steps, self.v0, self.basis, self.out, self.workspace,
                                                            samples=self.samples, x_seeds=x_seeds, x_steps=x_steps, z_seeds=z_seeds,
                                                            z_steps=z_steps, x_tag=tag, z_tag=self.Z_TAG, **self._drawn())
        rec = self._records().numpy()
        stats = []
        for r in range(self.R):
            row = rec[r]
            self._check_solve(r, "solve of the Lanczos matrix T", "T", row[4], row[5], self.OFF_BOUND * row[6])
            k, h, b = int(row[2]), self.HEAD, self.BLOCK
            stats.append({self.KEYS[0]: row[h:h + k].copy(), self.KEYS[1]: row[h + b:h + b + k].copy(), self.KEYS[2]: float(row[9]),
                          self.KEYS[3]: float(row[10]), self.KEYS[4]: float(row[1])})
        return stats

    def event_after(self, ran):
        """event() of an n_print event.  ran: {observable name: what it returned} of the observables that already ran at this step.
        After a ReplicaElboHessian over the SAME models (one-decoder models only) the rows are the ones that event used -- its own, or
        the exact / IWAE event's where it followed one -- and every dict gains "Sharpness Sampling Gap" = Sampled Sharpness - Sharpness:
        how far K samples are from the closed form."""
        exact_stats = ran.get("elbo_hessian")
        if exact_stats is None:
            return self.event()
        if "exact_log_likelihood" in ran:
            attr, tag = "_loglik_draws" if "log_likelihood_samples" in ran else "_exact_loglik_draws", ReplicaExactLogLik.X_TAG
        else:
            attr, tag = ReplicaElboHessian.COUNTER, ReplicaElboHessian.X_TAG
        stats = self.event(step=[getattr(m, attr) for m in self.ms], x_tag=tag)
        for st, ex in zip(stats, exact_stats):
            st[self.GAP] = st[self.KEYS[2]] - float(ex[ReplicaElboHessian.KEYS[2]])
        return stats


class ReplicaSampledElboHessianMlp3(ReplicaSampledElboHessian):
    """ReplicaSampledElboHessian for R THREE-HIDDEN-LAYER MLP VAEModels of one shape (vaek_mlp3_sampled_elbo_hessian_lanczos_replicas,
    csrc/mlp3_hessian.hip): the same event, record and five keys -- the two classes cover disjoint models, as the two log-likelihood
    classes do -- with the R-op through both relu stacks.  ONE call per event for all models (6 + 6 steps launches) and ONE device -> host
    copy.  The default is K = 1 sample per row: the training loss's own estimator, and a column costs 39 KB of workspace at
    200|200|200.  It does NOT perturb the run: its draws have a counter of their own, `m._mlp_hessian_draws`, and the tags 14 (rows),
    15 (samples) and 16 (start vector).  At most 2^13 columns a model and 2^14 a call."""

    X_TAG, Z_TAG, V_TAG = 14, 15, 16
    NAME = "ReplicaSampledElboHessianMlp3"
    COUNTER = "_mlp_hessian_draws"
    MAX_REPLICA_COLUMNS = 1 << 13
    ENTRY = "mlp3_sampled_elbo_hessian"
    COVERS = "float32, one decoder, exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, D, L <= 32"

    def __init__(self, vae_models, steps=32, samples=1, rows=None):
        super().__init__(vae_models, steps, samples, rows)

    def event_after(self, ran):
        """event() of an n_print event: no other observable shares its rows."""
        return self.event()


class ReplicaJacobian(ReplicaEvent):
    """The decoder Jacobian spectra of R VAEModels of one shape in ONE library call: per model, over `rows` latent rows z, the
    eigenvalues of J^T J with J = d Decoder(z) / dz -- the squared singular values of the decoder's local linear map --, their
    numerical rank and the sensitivity |d Decoder / d z_l|^2 of every latent: how many directions of the latent space the decoder
    uses, and which are off.  The spine of ReplicaJacobianMlp3 and ReplicaJacobianLinear, which name the library call (ENTRY), its cap
    (_check_cap) and the models it covers (_check_covered); the two never meet on one model, so they share a counter and tags.

    `at` chooses the latents:
      "prior"      the call draws them: the z1 vaek_make_batch writes under the event's seed, step and latent tag -- the latents
                   sample_batch decodes at a stats event;
      "posterior"  per model the event's real rows are drawn with make_batch (row tag), mu comes from vaek_forward(sampling=0) and goes
                   to the call as explicit rows: the Jacobian on the encoded data manifold.
    event() makes ONE library call for all models and ONE device -> host copy of the [R, 2 L + 8] float64
    records.  It does NOT perturb the run: `m.key`, the dataset's `_draws`, `m._latent_draws` and the other events' counters are left
    alone.  Its draws have a counter of their own, `m._jacobian_draws`, and the tags 7 (rows) and 8 (latents).  Returns per model
    {"Decoder Jacobian Spectrum" (float64 [L], descending), "Decoder Jacobian Rank" (float64 [3]: mean, min, max), "Latent
    Sensitivity" (float64 [L])} and appends them to `m.jacobian_spectra`, `m.jacobian_ranks` and `m.latent_sensitivities`.  Raises
    RuntimeError naming the model where a row's solve ended with off_F > 2^-40 |J^T J|_F."""

    KEYS = ("Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity")
    X_TAG, Z_TAG = 7, 8
    NOUN = "call"
    ROWS = (1, "stats_event_max_rows", "")
    COUNTER = "_jacobian_draws"
    MODES = ("prior", "posterior")

    def __init__(self, vae_models, rows=None, at="prior", rank_tol=1e-4):
        if at not in self.MODES:
            raise RuntimeError(f"{self.NAME}(at={at!r}): need one of {self.MODES}")
        self.at = at
        self.rank_tol = float(rank_tol)
        if not 0.0 <= self.rank_tol < 1.0:
            raise RuntimeError(f"{self.NAME}(rank_tol={rank_tol}): need 0 <= rank_tol < 1")
        super().__init__(vae_models, rows)

    def _allocate(self, R, dev):
        self.L = self.eng.L
        self._check_cap(R)
        self.record_len = self.eng.decoder_jacobian_record_len
        self.out = torch.zeros(R, self.record_len, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(max(getattr(self.eng, self.ENTRY + "_workspace")(R, self.rows), 16), dtype=torch.uint8, device=dev)
        if self.at == "posterior":
            self.z = torch.zeros(R, self.rows, self.L, dtype=torch.float32, device=dev)

    def event(self):
        """One evaluation of every model: [{"Decoder Jacobian Spectrum", "Decoder Jacobian Rank", "Latent Sensitivity"} of model 0, ...]."""
        L = self.L
        self._stack_params()
        seeds, steps = self._seeds(), self._own_steps()
        if self.at == "posterior":
            for r, m in enumerate(self.ms):
                eng = m.model.module.engine(self.rows)                                 # forward takes at most its context's batch
                Ar = None if self.A is None else self.A[r]
                x, z1, z2 = eng.make_batch(self.kind, Ar, self.dd, self.did, self.pad, self.var, self.rows, seeds[r], step=steps[r],
                                           tag=self.X_TAG)
                _, mu = eng.forward(m.model.flat, x, z1, z2, sampling=False, want_mu=True)
                self.z[r].copy_(mu)
            src = dict(z=self.z)
        else:
            src = dict(zip(("z_seeds", "z_steps"), _seed_step_tensors(seeds, steps, self.eng.device)))
        getattr(self.eng, self.ENTRY + "_replicas")(self.params, self.rows, self.out, self.workspace, rank_tol=self.rank_tol,
                                                    z_tag=self.Z_TAG, **src)
        rec = self._records().numpy()
        stats = []
        for r, m in enumerate(self.ms):
            row = rec[r]
            # slot [6] is the largest off_F / |G|_F over the rows: the bound is relative
            self._check_solve(r, "solve of J^T J", "J^T J", row[5], row[6], self.OFF_BOUND)
            st = {self.KEYS[0]: row[8:8 + L].copy(), self.KEYS[1]: row[1:4].copy(), self.KEYS[2]: row[8 + L:8 + 2 * L].copy()}
            self._append(m, jacobian_spectra=st[self.KEYS[0]], jacobian_ranks=st[self.KEYS[1]], latent_sensitivities=st[self.KEYS[2]])
            stats.append(st)
        return stats


class ReplicaJacobianMlp3(ReplicaJacobian):
    """ReplicaJacobian for three-hidden-layer MLP VAEModels (vaek_mlp3_decoder_jacobian_replicas, csrc/mlp3_jacobian.hip):
    J(z) = K3^T M3 K2^T M2 K1^T M1 K0^T, the four decoder kernels with the relu masks of z between them, in float32."""

    NAME = "ReplicaJacobianMlp3"
    ENTRY = "mlp3_decoder_jacobian"

    def _check_cap(self, R):
        cols, cap = R * self.rows * self.L, self.eng.mlp3_decoder_jacobian_max_columns
        if cols > cap:
            raise RuntimeError(f"{self.NAME}: {R} models x {self.rows} rows x {self.L} latents = {cols} columns, at most {cap} fit one call "
                               "(vaek_mlp3_decoder_jacobian_max_columns)")

    def _check_covered(self):
        if not self.eng.supports_mlp3_decoder_jacobian():
            raise RuntimeError("ReplicaJacobianMlp3: vaek_mlp3_decoder_jacobian_replicas does not cover this model (it needs a float32 "
                               "VAE with one decoder and exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, "
                               "D, L <= 32; the Jacobian of a linear decoder is its kernel: ReplicaExactLogLik's record holds the "
                               "eigenvalues of K^T K; per-row records and two-decoder linear models are what ReplicaJacobianLinear "
                               f"(--linear_decoder_jacobian) is for; this model's step path: {getattr(self.eng, 'step_path', '?')})")


class ReplicaJacobianLinear(ReplicaJacobian):
    """ReplicaJacobian for linear VAEModels with one or two decoders (vaek_linear_decoder_jacobian_replicas, csrc/linear_jacobian.hip):
    J(z) = K_d^T + diag(sigmoid'(z K_s + b_s)) K_s^T in float64 -- with one decoder K_d^T at every z, with two a matrix that changes
    from row to row: the rank and the dead latents of the generators of the sigmoid experiment."""

    NAME = "ReplicaJacobianLinear"
    ENTRY = "linear_decoder_jacobian"

    def _check_cap(self, R):
        total, cap = R * self.rows, self.eng.linear_decoder_jacobian_max_rows
        if total > cap:
            raise RuntimeError(f"{self.NAME}: {R} models x {self.rows} rows = {total} rows, at most {cap} fit one call "
                               "(vaek_linear_decoder_jacobian_max_rows)")

    def _check_covered(self):
        if not self.eng.supports_linear_decoder_jacobian():
            raise RuntimeError("ReplicaJacobianLinear: vaek_linear_decoder_jacobian_replicas does not cover this model (it needs a float32 "
                               "linear VAE -- no hidden layers -- with one or two decoders, D, L <= 32, D <= 28 with two decoders; a "
                               "three-hidden-layer MLP model takes ReplicaJacobianMlp3 (--decoder_jacobian); this model's step path: "
                               f"{getattr(self.eng, 'step_path', '?')})")


class ReplicaSpectrum(ReplicaEvent):
    """The covariance spectra of a generated and of a real batch of R VAEModels of one shape: per model the eigenvalues of
    cov(fake batch) -- the reference's "learnt eigenvalue" -- and of cov(real batch) -- its "ground truth eigenvalue"
    (datasets.py:113-125), the `EigenValues` the reference saves and never fills (csrc/cov_spectrum.hip).

    Where the engine's supports_spectrum_event holds (linear VAEs) event() is one parameter stack, ONE fused call
    (vaek_spectrum_event_replicas: nothing of a row exists in HBM) and one device -> host copy.  Every other model -- the mlp3 sweep
    included -- takes the host route: per model make_batch and forward(sampling) under the same seeds, steps and tags into a
    [2R, rows, D] stack, then ONE vaek_cov_spectrum_rows call with n = 2R and one device -> host copy.

    event() does NOT perturb the run: `m.key`, the dataset's `_draws` and `m._latent_draws` are neither split nor advanced.  Its draws
    have a counter of their own, `m._spectrum_draws`, and the tags 5 (rows) and 6 (latents).  The fake batch is sampled with the
    model's `current_epsilon`.  Returns per model {"learnt eigenvalue", "ground truth eigenvalue"} (float64 arrays, ascending) and
    appends them to `m.ht_eigen` and `m.gt_eigen`.  Raises RuntimeError naming the model where a solve hit the sweep cap without
    converging (off_F > 2^-40 |C|_F)."""

    KEYS = ("learnt eigenvalue", "ground truth eigenvalue")
    X_TAG, Z_TAG = 5, 6
    NAME = "ReplicaSpectrum"
    NOUN = "call"
    ROWS = (2, "stats_event_max_rows", "; one row has no covariance")
    COUNTER = "_spectrum_draws"
    VEC = False                        # ReplicaSubspace: the eigen records and entry points
    STACK = False

    def _allocate(self, R, dev):
        self.D = self.eng.D
        self.fused = bool(self.eng.supports_spectrum_event(self.kind))          # else the host route, which reads each model's own parameters
        self.record_len = self.eng.cov_eigen_record_len if self.VEC else self.eng.cov_spectrum_record_len
        self.buf = torch.zeros(2 * R * self.record_len + self._extra_doubles(), dtype=torch.float64, device=dev)
        self.out = self.buf[:2 * R * self.record_len].view(2 * R, self.record_len)          # [R, 2 records] on the fused route
        if self.fused:
            self.params = self._param_stack()
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
        R = self.R
        seeds, steps = self._seeds(), self._own_steps()
        eps_in = [float(torch.as_tensor(m.current_epsilon).reshape(-1)[0]) for m in self.ms]       # sample_batch: the model's current eps
        if self.fused:
            self._stack_params()
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
        host = self._records(self.buf).numpy()
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
            self._check_solve(r, f"{name} solve", "C", tail[0], tail[1], self.OFF_BOUND * tail[2])
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
        self._check_solve(r, "principal-angle solve", "G", row[k + 1], off, self.OFF_BOUND * norm)
        st[self.ANGLES] = np.arcsin(np.sqrt(np.clip(sin2, 0.0, 1.0)))
        st[self.DISTANCE] = float(np.sqrt(row[k]))
        self._append(m, principal_angles=st[self.ANGLES], subspace_distances=st[self.DISTANCE])
        return st
