"""Command line of the reference (run.py:8-43, :350-369), flag for flag: `python run.py NAME
--dataset linear_gaussian ...` trains a VAE with the HIP kernels and leaves data/NAME/{args.json,
losses.npz, model.pkl, output_*.png}.  Flags the reference parses but never reads on the VAE path
(--num_epochs, --padding_type, -ii, -ufc, -wsl, -off, -ws) are accepted and inert, except -ws
which is rejected (out of scope).  Additions: --device, --force_generic, --sweep_dataset_seeds (main_sweep), --trajectory_every,
--fused_stats, --mlp_fused_stats, and the observables of the n_print events, which observables.py tables: --log_likelihood_samples,
--mlp_log_likelihood_samples, --exact_log_likelihood, --elbo_hessian, --sampled_elbo_hessian (with --sampled_elbo_hessian_samples), --mlp_sampled_elbo_hessian (with --mlp_sampled_elbo_hessian_samples),
--eigenvalues, --subspace, --decoder_jacobian (with --decoder_jacobian_tol), --linear_decoder_jacobian (with
--linear_decoder_jacobian_tol)."""
from __future__ import annotations

import argparse
import types

from . import observables
from .observables import FLAGS, JACOBIAN_DEFAULT_TOL, check_model, decoder_jacobian_tol      # noqa: F401 (names callers import here)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("name", help="The name of the experiment and output directory.")
    p.add_argument("--num_batches", dest="num_batches", type=int, default=15000, help="Number of batches to train on.")
    p.add_argument("--num_epochs", dest="num_epochs", type=int, default=10000)
    p.add_argument("--batch_size", dest="batch_size", type=int, default=100)
    p.add_argument("-lr", "--learning_rate", dest="learning_rate", type=float, default=0.0001)
    p.add_argument("--padding_dim", type=int, dest="padding_dim", default=0)
    p.add_argument("-ow", dest="overwrite", action="store_true")
    # the reference's default '4gaussian' is not one of its own choices (run.py:18-19): always pass --dataset
    p.add_argument("--dataset", dest="dataset", default="4gaussian", choices=["sphere", "linear_gaussian", "sigmoid"])
    p.add_argument("--layer_sizes", dest="layer_sizes", default="512|512",
                   help="Decoder MLP widths separated by pipes, e.g. 512|512|512; \"\" = linear")
    p.add_argument("--encoder_layer_sizes", dest="encoder_layer_sizes", default="512|512",
                   help="Encoder MLP widths separated by pipes; \"\" = linear")
    p.add_argument("--latent_dim", dest="latent_dimension", type=int, default=100)
    p.add_argument("-nojit", dest="nojit", action="store_true", help="accepted for compatibility (kernels are always eager launches)")
    p.add_argument("--padding_type", dest="padding_type", default="none", choices=["zero", "gaussian", "none"])
    p.add_argument("-ds", "--dataset_seed", dest="dataset_seed", type=int, default=69)
    p.add_argument("--state_dict", dest="state_dict", default=None)
    p.add_argument("--data_fn", dest="data_fn", default=None)
    p.add_argument("-ws", "--warm_start", action="store_true")
    p.add_argument("-ii", "--initialize_inverse", action="store_true")
    p.add_argument("-ufc", "--use_fred_covariance", action="store_true")
    p.add_argument("-e", "--epsilon", type=float, default=0.)
    p.add_argument("-tdv", dest="tunable_decoder_var", action="store_true")
    p.add_argument("-dn", "--dataset_noise", type=float, default=0.)
    p.add_argument("-dd", "--dataset_dimension", type=int, default=3)
    p.add_argument("-wsl", "--warm_start_linear", action="store_true")
    p.add_argument("-did", "--dataset_intrinsic_dimension", type=int, default=3)
    p.add_argument("-off", "--latent_off_dimension", type=int, default=1)
    p.add_argument("--device", type=int, default=None, help="HIP device ordinal (default: current)")
    p.add_argument("--force_generic", action="store_true", help="layer-by-layer kernels even where a fused path exists")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="Dense GEMM arithmetic (bf16: wide layers on bf16 MFMA)")
    p.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                   help="process-group backend when launched with torch.distributed.run (gloo: one-GPU rehearsal)")
    p.add_argument("--comm", default="auto", choices=["auto", "rccl", "p2p"],
                   help="data-parallel gradient exchange: in-kernel peer-to-peer granules (small models) or RCCL all-reduce "
                        "of per-layer buckets overlapped with the backward pass")
    p.add_argument("--fast_loop", action="store_true", default=None,
                   help="run the steps between stats/plots with nothing per step on the host (trainer.py): linear VAEs through "
                        "vaek_train_steps_gen (up to 64 steps per persistent launch, batches drawn inside it), other models from a "
                        "hipGraph with on-device Philox batches.  Default: on for the models vaek_train_steps_gen covers")
    p.add_argument("--no_fast_loop", dest="fast_loop", action="store_false",
                   help="the reference's loop shape: one get_batch + one train_step call per iteration (model.py:221-222)")
    p.add_argument("--sweep_dataset_seeds", dest="sweep_dataset_seeds", type=_int_list, default=None, metavar="S1,S2,...",
                   help="train one model per dataset seed together; output directories NAME_ds<seed>.  Linear VAEs the resident loop covers: "
                        "ONE launch per run of steps (trainer.ReplicaLoop: workgroup r of vaek_train_loop_gen_replicas trains the model of "
                        "seed r).  Three-hidden-layer MLP VAEs on the \"mlp3\" train step: a hipGraph loop whose every step trains all "
                        "models in two launches (trainer.ReplicaGraphLoop, vaek_train_step_gen_replicas).  Other models are refused; "
                        "single GPU only")
    p.add_argument("--trajectory_every", dest="trajectory_every", type=_positive_int, default=None, metavar="K",
                   help="record the model while it trains: every K-th Adam step the resident loop stores the parameters that step's "
                        "gradient was evaluated at and the gradient itself (trainer.GraphLoop(resident=True, trajectory_every=K); with "
                        "--sweep_dataset_seeds trainer.ReplicaLoop).  Each output directory gains trajectory.npz (steps, params, grads and "
                        "the leaf table) and losses.npz a Correlation Ratio per record (vae.py:143-179).  Linear VAEs the resident loop "
                        "covers only; other models are refused before any step; single GPU only")
    p.add_argument("--fused_stats", dest="fused_stats", action="store_true",
                   help="with --sweep_dataset_seeds on models the resident loop covers: the stats event at every n_print step is ONE launch "
                        "for all models (trainer.ReplicaStats, vaek_stats_event_replicas) instead of one compute_stats() per model.  The "
                        "same draws, the same host RNG bookkeeping, the same keys in losses.npz.  Refused before any step without "
                        "--sweep_dataset_seeds and on a sweep of three-hidden-layer MLP VAEs (their fused event is --mlp_fused_stats)")
    p.add_argument("--mlp_fused_stats", dest="mlp_fused_stats", action="store_true",
                   help="--fused_stats for a sweep of three-hidden-layer MLP VAEs (trainer.ReplicaStatsMlp3, "
                        "vaek_mlp3_stats_event_replicas): with --sweep_dataset_seeds on models the \"mlp3\" train step covers, the stats "
                        "event at every n_print step is ONE call (two launches) for all models instead of one compute_stats() per model.  "
                        "The same draws, the same host RNG bookkeeping, the same keys in losses.npz; combines with "
                        "--mlp_log_likelihood_samples.  Refused before any step, with the step path, without --sweep_dataset_seeds, "
                        "on a sweep the resident loop takes (use --fused_stats) and with --fused_stats")
    p.add_argument("--log_likelihood_samples", dest="log_likelihood_samples", type=_positive_int, default=None, metavar="K",
                   help="at every n_print step also evaluate the importance-weighted log-likelihood of the model(s) on K posterior samples "
                        "per row of a print batch (trainer.ReplicaLogLik, vaek_log_likelihood_replicas): losses.npz gains a non-empty "
                        "'Average Log Likelihood' (the IWAE-K bound), 'ELBO estimate' and 'Effective Sample Size'.  The evaluation has its "
                        "own RNG counter and tags, so the training run is bitwise the one without the flag.  Alone or with "
                        "--sweep_dataset_seeds (one call for all models); float32 linear VAEs with D, L <= 32 only; other models are refused "
                        "before any step; single GPU only")
    p.add_argument("--exact_log_likelihood", dest="exact_log_likelihood", action="store_true",
                   help="at every n_print step also evaluate, in closed form and float64, the exact log-likelihood of a print batch under "
                        "the model, the exact ELBO and their difference KL(q(z|x) || p(z|x)) (trainer.ReplicaExactLogLik, "
                        "vaek_exact_log_likelihood_replicas): losses.npz gains 'Exact Log Likelihood', 'Exact ELBO', 'Posterior KL' and "
                        "'Exact Likelihood Conditioning'.  With --log_likelihood_samples K both events score the same rows and 'IWAE "
                        "Gap' = Exact Log Likelihood - Average Log Likelihood is added.  The evaluation has its own RNG counter, so the "
                        "training run and every other stat are bitwise the ones without the flag.  Alone or with --sweep_dataset_seeds "
                        "(one launch for all models); float32 linear VAEs with ONE decoder and D, L <= 32 only (the sigmoid second "
                        "decoder has no closed form); other models are refused before any step; single GPU only")
    p.add_argument("--elbo_hessian", dest="elbo_hessian", nargs="?", type=_hessian_steps, const=ELBO_HESSIAN_MAX_STEPS, default=None,
                   metavar="STEPS",
                   help="at every n_print step also run STEPS (1 .. 32, default 32) Lanczos steps with full reorthogonalisation on the "
                        "Hessian of the exact ELBO of the model(s) on a print batch, in closed form and float64 "
                        "(trainer.ReplicaElboHessian, vaek_elbo_hessian_lanczos_replicas): losses.npz gains 'ELBO Hessian Ritz Values' and "
                        "'ELBO Hessian Ritz Residuals' (k each), 'Sharpness' (the largest Ritz value), 'ELBO Hessian Min Ritz' and 'ELBO "
                        "Gradient Norm'; the stats line shows the last three.  With --exact_log_likelihood both events score the same "
                        "rows.  The evaluation has its own RNG counter and tags, so the training run and every other stat are bitwise "
                        "the ones without the flag.  Alone or with --sweep_dataset_seeds (one launch for all models); refused where "
                        "--exact_log_likelihood is: MLP and two-decoder models and data parallelism, before any step")
    p.add_argument("--sampled_elbo_hessian", dest="sampled_elbo_hessian", nargs="?", type=_hessian_steps, const=ELBO_HESSIAN_MAX_STEPS,
                   default=None, metavar="STEPS",
                   help="--elbo_hessian for the models it refuses: at every n_print step run STEPS (1 .. 32, default 32) Lanczos steps on "
                        "the Hessian of the SAMPLE-AVERAGE ELBO of the model(s) -- a print batch of rows and K fixed latent samples per "
                        "row (--sampled_elbo_hessian_samples), float64, exact derivatives of that function "
                        "(trainer.ReplicaSampledElboHessian, vaek_sampled_elbo_hessian_lanczos_replicas): losses.npz gains 'Sampled ELBO "
                        "Hessian Ritz Values' and 'Sampled ELBO Hessian Ritz Residuals' (k each), 'Sampled Sharpness', 'Sampled ELBO "
                        "Hessian Min Ritz' and 'Sampled ELBO Gradient Norm'.  Linear VAEs with one OR two decoders (the sigmoid second "
                        "decoder included), D, L <= 32.  With --elbo_hessian on a one-decoder model both events use the same rows and "
                        "'Sharpness Sampling Gap' = Sampled Sharpness - Sharpness is added.  Its own RNG counter and tags: the training "
                        "run and every other stat are bitwise the ones without the flag.  Alone or with --sweep_dataset_seeds; MLP "
                        "models, data parallelism and models x rows x K above 2^22 (rows x K above 2^16) are refused before any step")
    p.add_argument("--sampled_elbo_hessian_samples", dest="sampled_elbo_hessian_samples", type=_positive_int, default=None, metavar="K",
                   help="with --sampled_elbo_hessian: K latent samples per row (default 8); refused without --sampled_elbo_hessian")
    p.add_argument("--mlp_sampled_elbo_hessian", dest="mlp_sampled_elbo_hessian", nargs="?", type=_hessian_steps,
                   const=ELBO_HESSIAN_MAX_STEPS, default=None, metavar="STEPS",
                   help="--sampled_elbo_hessian for three-hidden-layer MLP VAEs (trainer.ReplicaSampledElboHessianMlp3, "
                        "vaek_mlp3_sampled_elbo_hessian_lanczos_replicas): at every n_print step STEPS (1 .. 32, default 32) Lanczos steps "
                        "on the Hessian of the sample-average ELBO of the model(s) on a print batch of rows and K fixed latent samples per "
                        "row (--mlp_sampled_elbo_hessian_samples), float64 through both relu stacks; the same five keys in losses.npz.  Its "
                        "own RNG counter and tags: the training run and every other stat are bitwise the ones without the flag.  Alone or "
                        "with --sweep_dataset_seeds; combines with the other mlp3 flags.  Linear models (use --sampled_elbo_hessian), other "
                        "MLPs, data parallelism and models x rows x K above 2^14 (rows x K above 2^13) are refused before any step")
    p.add_argument("--mlp_sampled_elbo_hessian_samples", dest="mlp_sampled_elbo_hessian_samples", type=_positive_int, default=None,
                   metavar="K",
                   help="with --mlp_sampled_elbo_hessian: K latent samples per row (default 1, the training loss's own estimator); refused "
                        "without --mlp_sampled_elbo_hessian")
    p.add_argument("--mlp_log_likelihood_samples", dest="mlp_log_likelihood_samples", type=_positive_int, default=None, metavar="K",
                   help="--log_likelihood_samples for three-hidden-layer MLP VAEs (trainer.ReplicaLogLikMlp3, "
                        "vaek_mlp3_log_likelihood_replicas): the same three stats from the same draws, the training run bitwise the one "
                        "without the flag.  Alone or with --sweep_dataset_seeds (one call for all models); float32, one decoder, three "
                        "hidden layers of 64 .. 256 units both ways, D, L <= 32, models x 1000 rows x K at most 2^22; linear models (use "
                        "--log_likelihood_samples), other models and both flags together are refused before any step; single GPU only")
    p.add_argument("--subspace", dest="subspace", default=None, type=subspace_arg, metavar="auto|K",
                   help="at every n_print step also evaluate the principal angles between the span of the K leading eigenvectors of "
                        "cov(generated print batch) and that of cov(real print batch) (trainer.ReplicaSubspace, csrc/cov_spectrum.hip): "
                        "losses.npz gains 'Subspace Distance' (|sin Theta|_F) and 'Principal Angles' (radians, ascending) per event.  "
                        "auto: the dimension of the dataset's linear span (linear_gaussian min(dd, did), sigmoid dd + 1, sphere dd).  "
                        "With --eigenvalues one device call serves both and EigenValues is bitwise what --eigenvalues alone writes.  "
                        "Needs data_dim <= 32, K in 1 .. data_dim and one GPU; the training run is bitwise the run without the flag")
    p.add_argument("--eigenvalues", dest="eigenvalues", action="store_true",
                   help="at every n_print step also evaluate the covariance spectrum of a generated print batch and of a real one "
                        "(trainer.ReplicaSpectrum, csrc/cov_spectrum.hip): losses.npz gains 'learnt eigenvalue' and 'ground truth "
                        "eigenvalue' per event and 'EigenValues' = (learnt, ground truth), the key the reference saves empty.  Linear "
                        "VAEs: one fused launch (vaek_spectrum_event_replicas); other models: make_batch + forward per model and one "
                        "vaek_cov_spectrum_rows call.  The evaluation has its own RNG counter and tags, so the training run is bitwise "
                        "the one without the flag.  Alone or with --sweep_dataset_seeds; combines with the stats and log-likelihood "
                        "flags; data_dim <= 32; single GPU only")
    p.add_argument("--decoder_jacobian", dest="decoder_jacobian", default=None, choices=["prior", "posterior"],
                   help="at every n_print step also evaluate the spectrum of the decoder Jacobian J(z) = d Decoder(z) / dz of a "
                        "three-hidden-layer MLP VAE on a print batch of latent rows (trainer.ReplicaJacobianMlp3, "
                        "vaek_mlp3_decoder_jacobian_replicas): losses.npz gains 'Decoder Jacobian Spectrum' (mean eigenvalues of J^T J, "
                        "descending), 'Decoder Jacobian Rank' (mean, min, max numerical rank) and 'Latent Sensitivity' (mean "
                        "|d Decoder / d z_l|^2 per latent, next to 'Encoder Variance'); the stats line shows the mean rank.  prior: the "
                        "latents sample_batch decodes; posterior: the encoder means of a real print batch.  The evaluation has its own RNG "
                        "counter and tags, so the training run is bitwise the one without the flag.  Alone or with --sweep_dataset_seeds "
                        "(one call for all models); combines with --mlp_fused_stats and --mlp_log_likelihood_samples; float32, one decoder, "
                        "three hidden layers of 64 .. 256 units both ways, D, L <= 32; linear models (J is the decoder kernel: use "
                        "--exact_log_likelihood), other models and data parallelism are refused before any step")
    p.add_argument("--decoder_jacobian_tol", dest="decoder_jacobian_tol", type=_rank_tol, default=None, metavar="T",
                   help="with --decoder_jacobian: an eigenvalue of J^T J counts towards the rank where it exceeds T times the largest "
                        "(0 <= T < 1, default 1e-4); refused without --decoder_jacobian")
    p.add_argument("--linear_decoder_jacobian", dest="linear_decoder_jacobian", default=None, choices=["prior", "posterior"],
                   help="--decoder_jacobian for linear VAEs with one or two decoders (trainer.ReplicaJacobianLinear, "
                        "vaek_linear_decoder_jacobian_replicas): at every n_print step the spectrum of J(z) = K_d^T + "
                        "diag(sigmoid'(z K_s + b_s)) K_s^T on a print batch of latent rows, formed and solved in float64; the same three "
                        "keys in losses.npz, the mean rank on the stats line.  With two decoders (-sig) J changes from row to row: the rank "
                        "says how many latent directions the generator moves its output along, 'Latent Sensitivity' which latents are "
                        "off.  prior / posterior as for --decoder_jacobian.  Its own RNG counter and tags: the training run and every "
                        "other stat are bitwise the ones without the flag.  Alone or with --sweep_dataset_seeds; combines with the other "
                        "linear flags.  D, L <= 32 (D <= 28 with two decoders); MLP models (use --decoder_jacobian), --decoder_jacobian "
                        "itself, data parallelism, -dd / -did > 16 and models x rows above 2^20 are refused before any step")
    p.add_argument("--linear_decoder_jacobian_tol", dest="linear_decoder_jacobian_tol", type=_rank_tol, default=None, metavar="T",
                   help="with --linear_decoder_jacobian: an eigenvalue of J^T J counts towards the rank where it exceeds T times the "
                        "largest (0 <= T < 1, default 1e-4); refused without --linear_decoder_jacobian")
    return p


ELBO_HESSIAN_MAX_STEPS = 32      # vaek_elbo_hessian_max_steps(): the size of the device's Jacobi routine


def _hessian_steps(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer")
    if not 1 <= k <= ELBO_HESSIAN_MAX_STEPS:
        raise argparse.ArgumentTypeError(f"{k} Lanczos steps: need 1 .. {ELBO_HESSIAN_MAX_STEPS}")
    return k


def _rank_tol(text):
    try:
        t = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number")
    if not 0.0 <= t < 1.0:
        raise argparse.ArgumentTypeError(f"{text} is not in [0, 1)")
    return t


def _positive_int(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not an integer")
    if k < 1:
        raise argparse.ArgumentTypeError(f"{k} is not >= 1")
    return k


def _int_list(text):
    try:
        vals = [int(t) for t in text.split(",") if t.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of integers")
    if not vals:
        raise argparse.ArgumentTypeError("an empty list of seeds")
    return vals


def subspace_arg(v):
    """--subspace: "auto" or a positive integer K."""
    if v == "auto":
        return v
    try:
        k = int(v)
    except ValueError:
        k = 0
    if k < 1:
        import argparse
        raise argparse.ArgumentTypeError(f"--subspace takes auto or an integer K >= 1, got {v!r}")
    return k


def parse_arguments(argv=None):
    args = build_parser().parse_args(argv)
    args.model = "VAE"
    args.latent_distribution = "gaussian"
    args.tqdm = True
    return args


def get_dataset(name, seed, padding_dimension, batch_size, args, world=1, rank=0):
    from . import random as vrandom
    from .datasets import LinearGaussianDataset, SigmoidDataset, SphereDataset
    dev = None if getattr(args, "device", None) is None else f"cuda:{args.device}"
    ds = None
    if name == "sphere":
        ds = SphereDataset(seed, dimension=args.dataset_dimension, padding_dimension=args.padding_dim, device=dev)
    elif name == "linear_gaussian":
        ds = LinearGaussianDataset(seed, dimension=args.dataset_dimension,
                                   intrinsic_dimension=args.dataset_intrinsic_dimension,
                                   padding_dimension=args.padding_dim, var_added=args.dataset_noise, device=dev)
    elif name == "sigmoid":
        ds = SigmoidDataset(seed, dimension=args.dataset_dimension, padding_dimension=args.padding_dim, device=dev)
    if ds is not None and world > 1:
        # same manifold (A was drawn from the seed above) on every rank, a different sample stream per rank
        ds.key = vrandom.split(ds.key, world)[rank]
    return ds


def get_model(args, dataset, output_dir, dist=None):
    from . import random as vrandom
    from .vae import VAEModel
    if args.model != "VAE":
        raise NameError(f"model {args.model!r}: only the VAE branch exists (run.py:250-268)")
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0
    if world > 1:
        return _get_model_dp(args, dataset, output_dir, dist, world, rank)
    return VAEModel(dirname=output_dir, batch_size=args.batch_size, learning_rate=args.learning_rate, dataset=dataset,
                    num_batches=args.num_batches, num_epochs=args.num_epochs, layer_sizes=args.layer_sizes,
                    encoder_layer_sizes=args.encoder_layer_sizes, state_dict=args.state_dict, data_fn=args.data_fn,
                    epsilon=args.epsilon, tqdm=args.tqdm, latent_dimension=args.latent_dimension,
                    tunable_decoder_var=args.tunable_decoder_var, warm_start=args.warm_start,
                    dataset_name=args.dataset, latent_off_dimension=args.latent_off_dimension,
                    force_generic=getattr(args, "force_generic", False), fast_loop=getattr(args, "fast_loop", False),
                    dtype=getattr(args, "dtype", "f32"))


def _get_model_dp(args, dataset, output_dir, dist, world, rank):
    """Data parallel (this build's addition; the reference is single-device): --batch_size is the GLOBAL
    batch, every rank trains on batch_size / world rows of its own sample stream, gradients are summed
    over ranks (parallel.GradExchange: P2P inside the finalize kernel, or RCCL overlapped with the
    backward pass) and every replica applies the identical Adam update."""
    from . import random as vrandom
    from .parallel import GradExchange, shard_rows
    from .vae import VAEModel
    lo, hi = shard_rows(args.batch_size, world, rank)
    m = VAEModel(dirname=output_dir, batch_size=hi - lo, learning_rate=args.learning_rate, dataset=dataset,
                 num_batches=args.num_batches, num_epochs=args.num_epochs, layer_sizes=args.layer_sizes,
                 encoder_layer_sizes=args.encoder_layer_sizes, state_dict=args.state_dict, data_fn=args.data_fn,
                 epsilon=args.epsilon, tqdm=args.tqdm and rank == 0, latent_dimension=args.latent_dimension,
                 tunable_decoder_var=args.tunable_decoder_var, warm_start=args.warm_start, dataset_name=args.dataset,
                 latent_off_dimension=args.latent_off_dimension, force_generic=getattr(args, "force_generic", False),
                 dtype=getattr(args, "dtype", "f32"), world=world, rank=rank, global_batch=args.batch_size)
    eng = m.model.module.engine(hi - lo, args.batch_size)
    m.optimizer.exchange = GradExchange(eng, dist, mode=getattr(args, "comm", "auto"))
    if rank == 0:
        how = m.optimizer.exchange.mode + ("" if m.optimizer.exchange.in_library or eng.fused else ", per-layer buckets overlapped with the backward pass")
        print(f"Data parallel: world {world}, {hi - lo} rows per rank, gradient exchange {how}")
    m.key = vrandom.split(m.key, world)[rank]              # identical initial parameters, different latent draws
    m.rank = rank
    return m


TRAJECTORY_NEEDS = ("a model the resident loop covers (vaek_supports_train_loop_gen): a float32 linear VAE with one or two decoders, "
                    "D, L <= 32, a batch of at most 256 rows, -dd / -did <= 16, on one GPU")


def check_trajectory_model(m):
    """--trajectory_every: refuse, before any step, a model whose steps would not run in the resident loop."""
    from .datasets import DEVICE_DRAW_MAX_DIM
    eng = m.model.module.engine(m.batch_size, m.optimizer.global_batch)
    kind, _, dd, did, _, _ = m.dataset.device_spec()
    if eng.world > 1 or dd > DEVICE_DRAW_MAX_DIM or did > DEVICE_DRAW_MAX_DIM or not eng.supports_train_loop_gen(kind):
        raise RuntimeError(f"--trajectory_every needs {TRAJECTORY_NEEDS} (this model's step path: {getattr(eng, 'step_path', '?')}, "
                           f"batch {m.batch_size}, world {eng.world})")


def write_trajectory(m, loop):
    """trajectory.npz in the model's output directory: steps [n] (1-based Adam steps), params [n, P] (the parameters each step's
    gradient was evaluated at), grads [n, P + 4] (loss, mean Dkl, mean mse, 0 behind the P gradients) and the leaf table of
    vaek_leaf_info (leaf_names, leaf_offsets, leaf_shapes as rows x cols, a vector being 1 x n)."""
    import os

    import numpy as np
    steps, th, g = loop.trajectory()
    leaves = m.model.module.leaves
    shapes = [(1, sh[0]) if len(sh) == 1 else tuple(sh) for _, sh in leaves.values()]
    np.savez(os.path.join(m.dirname, "trajectory"), steps=steps.numpy(), params=th.numpy(), grads=g.numpy(),
             leaf_names=np.array(list(leaves), dtype=np.str_), leaf_offsets=np.array([off for off, _ in leaves.values()], dtype=np.int64),
             leaf_shapes=np.array(shapes, dtype=np.int64).reshape(-1, 2))


def sweep_loop(models, trajectory_every=None):
    """The loop of --sweep_dataset_seeds: ReplicaLoop where the resident loop covers the models (small-batch linear VAEs), else
    ReplicaGraphLoop where the engine's step has a replica form (the "mlp3" step), else a refusal that names both.  With
    --trajectory_every only ReplicaLoop will do."""
    from .trainer import ReplicaGraphLoop, ReplicaLoop
    m0 = models[0]
    eng = m0.model.module.engine(m0.batch_size, m0.optimizer.global_batch)
    if trajectory_every is not None:
        check_trajectory_model(m0)
        return ReplicaLoop(models, trajectory_every=trajectory_every)
    if eng.world > 1 or eng.supports_train_loop_gen(m0.dataset.device_spec()[0]):
        return ReplicaLoop(models)           # today's behaviour, its own refusals included
    if eng.supports_train_step_replicas():
        return ReplicaGraphLoop(models)
    raise RuntimeError("--sweep_dataset_seeds: neither replica loop covers this model: trainer.ReplicaLoop (vaek_train_loop_gen_replicas) "
                       "needs a float32 linear VAE with one or two decoders, D, L <= 32 and a batch of at most 256 rows; "
                       "trainer.ReplicaGraphLoop (vaek_train_step_gen_replicas) needs the \"mlp3\" train step: float32, three hidden "
                       f"layers of 64 .. 256 units both ways, D, L <= 32, a batch of at most 128 rows (this model's step path: {eng.step_path})")


FUSED_STATS_NEEDS = ("--sweep_dataset_seeds on models the resident loop covers (trainer.ReplicaLoop): the fused event evaluates the "
                     "models of a sweep in one launch, workgroup r model r")


def check_fused_stats_args(args):
    """--fused_stats without --sweep_dataset_seeds: refused before anything is created."""
    if getattr(args, "fused_stats", False) and not getattr(args, "sweep_dataset_seeds", None):
        raise RuntimeError(f"--fused_stats needs {FUSED_STATS_NEEDS}; a single model's stats event is compute_stats()")


MLP_FUSED_STATS_NEEDS = ("--sweep_dataset_seeds on three-hidden-layer MLP VAEs (trainer.ReplicaGraphLoop, the \"mlp3\" train step): the "
                         "fused event evaluates the models of a sweep in one call (vaek_mlp3_stats_event_replicas)")


def refuse_mlp_fused_stats_single(step_path):
    """--mlp_fused_stats without --sweep_dataset_seeds: refused before any step (main() calls it once the model's engine exists)."""
    raise RuntimeError(f"--mlp_fused_stats needs {MLP_FUSED_STATS_NEEDS}; a single model's stats event is compute_stats() (this model's "
                       f"step path: {step_path})")


def check_mlp_fused_stats_loop(loop, fused_stats=False):
    """--mlp_fused_stats on a sweep: refuse, before any step, both stats flags together, a sweep whose loop is ReplicaLoop (that is
    --fused_stats' sweep) and models the call does not cover."""
    from .trainer import ReplicaLoop
    eng = loop.eng
    path = getattr(eng, "step_path", "?")
    if fused_stats:
        raise RuntimeError("--fused_stats (sweeps the resident loop takes: linear VAEs) and --mlp_fused_stats (sweeps of three-hidden-layer "
                           f"MLP VAEs) cover disjoint sweeps: give the one that matches the sweep's step path ({path!r})")
    if isinstance(loop, ReplicaLoop):
        raise RuntimeError(f"--mlp_fused_stats needs {MLP_FUSED_STATS_NEEDS}; this sweep's step path is {path!r} "
                           "(trainer.ReplicaLoop): use --fused_stats")
    if not eng.supports_mlp3_stats_event(loop.kind):
        raise RuntimeError(f"--mlp_fused_stats needs {MLP_FUSED_STATS_NEEDS}; this sweep's step path is {path!r}, which "
                           "vaek_supports_mlp3_stats_event does not cover")


# ---- the observables of the n_print events: observables.EVERY_OBSERVABLE holds their NEEDS texts, refusals and banners; the names below
# are what callers and tests import
LOGLIK_NEEDS = FLAGS["log_likelihood_samples"][1].needs
MLP_LOGLIK_NEEDS = FLAGS["mlp_log_likelihood_samples"][1].needs
EXACT_LOGLIK_NEEDS = FLAGS["exact_log_likelihood"][1].needs
ELBO_HESSIAN_NEEDS = FLAGS["elbo_hessian"][1].needs
SAMPLED_ELBO_HESSIAN_NEEDS = FLAGS["sampled_elbo_hessian"][1].needs
MLP_SAMPLED_ELBO_HESSIAN_NEEDS = FLAGS["mlp_sampled_elbo_hessian"][1].needs
EIGEN_NEEDS = FLAGS["eigenvalues"][1].needs
SUBSPACE_NEEDS = FLAGS["subspace"][1].needs
JACOBIAN_NEEDS = FLAGS["decoder_jacobian"][1].needs
LINEAR_JACOBIAN_NEEDS = FLAGS["linear_decoder_jacobian"][1].needs


def check_log_likelihood_model(m, samples):
    """--log_likelihood_samples: refuse, before any step, a model the log-likelihood call does not cover or a K above its cap."""
    check_model("log_likelihood_samples", m, samples)


def check_mlp_log_likelihood_model(m, samples, n_models=1):
    """--mlp_log_likelihood_samples: refuse, before any step, a model the call does not cover, a K above its cap or more columns
    (models x print rows x K) than one call takes."""
    check_model("mlp_log_likelihood_samples", m, samples, n_models)


def check_exact_log_likelihood_model(m):
    """--exact_log_likelihood: refuse, before any step, a model the exact call does not cover."""
    check_model("exact_log_likelihood", m)


def check_elbo_hessian_model(m):
    """--elbo_hessian: refuse, before any step, a model the Lanczos call does not cover."""
    check_model("elbo_hessian", m)


def check_sampled_elbo_hessian_model(m, steps=ELBO_HESSIAN_MAX_STEPS, n_models=1):
    """--sampled_elbo_hessian: refuse, before any step, a model the sampled Lanczos call does not cover."""
    check_model("sampled_elbo_hessian", m, steps, n_models)


def check_mlp_sampled_elbo_hessian_model(m, steps=ELBO_HESSIAN_MAX_STEPS, n_models=1):
    """--mlp_sampled_elbo_hessian: refuse, before any step, a model the MLP sampled Lanczos call does not cover."""
    return check_model("mlp_sampled_elbo_hessian", m, steps, n_models)


def check_eigenvalues_model(m):
    """--eigenvalues: refuse, before any step, a model the spectrum calls do not cover."""
    check_model("eigenvalues", m)


def check_subspace_model(m, k):
    """--subspace: refuse, before any step, a model the eigen calls do not cover or a K outside 1 .. data_dim.  Returns K (None: auto)."""
    return check_model("subspace", m, k)


def check_decoder_jacobian_model(m, n_models=1):
    """--decoder_jacobian: refuse, before any step, a model the call does not cover or more columns (models x print rows x L) than one
    call takes."""
    check_model("decoder_jacobian", m, None, n_models)


def check_linear_decoder_jacobian_model(m, n_models=1):
    """--linear_decoder_jacobian: refuse, before any step, a model the call does not cover or more rows (models x print rows) than one
    call takes."""
    check_model("linear_decoder_jacobian", m, None, n_models)


def check_log_likelihood_flags(args):
    """--log_likelihood_samples and --mlp_log_likelihood_samples cover disjoint models: both together are refused before anything is
    created."""
    if getattr(args, "log_likelihood_samples", None) is not None and getattr(args, "mlp_log_likelihood_samples", None) is not None:
        raise RuntimeError("--log_likelihood_samples (linear VAEs) and --mlp_log_likelihood_samples (three-hidden-layer MLP VAEs) cover "
                           "disjoint models: give the one that matches the model's step path")


def check_decoder_jacobian_flags(args):
    """--decoder_jacobian_tol without --decoder_jacobian, --linear_decoder_jacobian_tol without --linear_decoder_jacobian, and the two
    Jacobian flags together (they cover disjoint models and write the same keys): refused before anything is created."""
    if getattr(args, "decoder_jacobian_tol", None) is not None and getattr(args, "decoder_jacobian", None) is None:
        raise RuntimeError("--decoder_jacobian_tol sets the rank threshold of --decoder_jacobian prior|posterior: give that flag too")
    if getattr(args, "linear_decoder_jacobian_tol", None) is not None and getattr(args, "linear_decoder_jacobian", None) is None:
        raise RuntimeError("--linear_decoder_jacobian_tol sets the rank threshold of --linear_decoder_jacobian prior|posterior: give that "
                           "flag too")
    if getattr(args, "decoder_jacobian", None) is not None and getattr(args, "linear_decoder_jacobian", None) is not None:
        raise RuntimeError("--decoder_jacobian (three-hidden-layer MLP VAEs) and --linear_decoder_jacobian (linear VAEs) cover disjoint "
                           "models: give the one that matches the model's step path")


def check_sampled_elbo_hessian_flags(args):
    """--sampled_elbo_hessian_samples without --sampled_elbo_hessian: refused before anything is created."""
    if getattr(args, "sampled_elbo_hessian_samples", None) is not None and getattr(args, "sampled_elbo_hessian", None) is None:
        raise RuntimeError("--sampled_elbo_hessian_samples sets the samples per row of --sampled_elbo_hessian [STEPS]: give that flag too")


def check_mlp_sampled_elbo_hessian_flags(args):
    """--mlp_sampled_elbo_hessian_samples without --mlp_sampled_elbo_hessian: refused before anything is created."""
    if getattr(args, "mlp_sampled_elbo_hessian_samples", None) is not None and getattr(args, "mlp_sampled_elbo_hessian", None) is None:
        raise RuntimeError("--mlp_sampled_elbo_hessian_samples sets the samples per row of --mlp_sampled_elbo_hessian [STEPS]: give that "
                           "flag too")


def main_sweep(args):
    """--sweep_dataset_seeds: one dataset and one VAEModel per seed, the reference's schedule (model.py:207-222: stats every n_print
    steps, plot + save every n_plot steps and at the last step) for each model at each event, and ONE loop.run between
    events for all of them: trainer.ReplicaLoop where the resident loop covers the models, else trainer.ReplicaGraphLoop where the
    "mlp3" step's replica form does (sweep_loop)."""
    import copy
    import os

    from .utils import make_output_dir
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("--sweep_dataset_seeds trains independent models on one GPU: it does not combine with data parallelism")
    seeds = list(args.sweep_dataset_seeds)
    if len(set(seeds)) != len(seeds):
        raise ValueError("--sweep_dataset_seeds: a seed is listed twice (the output directories would collide)")
    models = []
    for seed in seeds:
        a = copy.copy(args)
        a.dataset_seed = seed
        out = make_output_dir(f"{args.name}_ds{seed}", args.overwrite, a)
        ds = get_dataset(args.dataset, seed, args.padding_dim, args.batch_size, args)
        if ds is None:
            raise ValueError("--dataset must be one of sphere, linear_gaussian, sigmoid")
        models.append(get_model(a, ds, out))
    tevery = getattr(args, "trajectory_every", None)
    loop = sweep_loop(models, tevery) if tevery is not None else sweep_loop(models)      # refuses, before any step, what no replica loop covers
    eng = loop.eng
    fused_stats = bool(getattr(args, "fused_stats", False))
    mlp_fused_stats = bool(getattr(args, "mlp_fused_stats", False))
    if mlp_fused_stats:                      # before any step
        check_mlp_fused_stats_loop(loop, fused_stats)
    if fused_stats:                          # before any step
        from .trainer import ReplicaLoop
        if not isinstance(loop, ReplicaLoop):
            raise RuntimeError(f"--fused_stats needs {FUSED_STATS_NEEDS}; this sweep's step path is {eng.step_path!r} "
                               "(trainer.ReplicaGraphLoop), whose fused stats event is --mlp_fused_stats")
    sweep = types.SimpleNamespace()          # what the observable flags set; the event objects are kept on it too
    for fl in observables.attach(args, models, sweep, build=True):      # refused, and the events built, before any step
        if fl.save_flag:
            for m in models:
                setattr(m, fl.dest, True)    # model_save_data
    print(f"Train step: {eng.step_path} kernels (vaek_train_step_path), replica sweep over dataset seeds {seeds}")
    print(f"Train loop: {loop.describe()}")
    if fused_stats:
        print(f"Stats events: one launch for {len(models)} models (vaek_stats_event_replicas)")
    if mlp_fused_stats:
        print(f"Stats events: one call for {len(models)} models (vaek_mlp3_stats_event_replicas)")
    for ob, event in observables.active(models, sweep):
        for fl in ob.flags:
            if fl.value(args) is not None:
                print(fl.banner_sweep(event, len(models), sweep))
    for r, m in enumerate(models):
        m._graph_loop = loop.view(r)
        score = m.dataset.score_batch(m.dataset.get_batch(m.print_batch_size))
        print(f"Score for real data (dataset seed {seeds[r]}): { {k: float(v) for k, v in score.items()} if isinstance(score, dict) else score}")
    m0 = models[0]
    n, n_print, n_plot = m0.num_batches, m0.n_print, m0.n_plot
    events = sorted(set(list(range(0, n, n_print)) + list(range(0, n, n_plot)) + [n - 1]))
    pos = 0
    for ev in events:
        loop.run(ev - pos)
        pos = ev
        loop.check()
        fused = loop.stats_event() if (fused_stats or mlp_fused_stats) and ev % n_print == 0 else None      # every model's event in one call
        extra = observables.run_events(models, sweep) if ev % n_print == 0 else None      # every model's observables: one call each
        for r, m in enumerate(models):
            m.batchnum = ev
            if ev % n_print == 0:
                stats = m.compute_stats() if fused is None else fused[r]
                stats.update(extra[r])
                m.write_stats(stats)
            if ev % n_plot == 0 or ev == n - 1:
                m.plot_epoch()
                m.save()
    loop.run(n - pos)
    loop.check()
    for r, m in enumerate(models):
        m.plot()
        m.save(final=True)
        if tevery is not None:
            write_trajectory(m, loop.view(r))
    return 0


def main(args):
    import os

    check_fused_stats_args(args)
    check_log_likelihood_flags(args)
    check_decoder_jacobian_flags(args)
    check_sampled_elbo_hessian_flags(args)
    check_mlp_sampled_elbo_hessian_flags(args)
    if getattr(args, "sweep_dataset_seeds", None):
        return main_sweep(args)
    from .utils import get_output_dir, make_output_dir
    dist = None
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:                            # before a process group exists
        observables.refuse_data_parallel(args, world)
    if world > 1:
        import torch
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0")) if args.dist_backend == "nccl" else 0
        torch.cuda.set_device(local)
        args.device = local
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    if rank == 0:
        output_dir = make_output_dir(args.name, args.overwrite, args)
    if dist is not None:
        dist.barrier()
        output_dir = get_output_dir(args.name)
    dataset = get_dataset(args.dataset, args.dataset_seed, args.padding_dim, args.batch_size, args, world, rank)
    if dataset is None:
        raise ValueError("--dataset must be one of sphere, linear_gaussian, sigmoid")
    model = get_model(args, dataset, output_dir, dist)
    if getattr(args, "mlp_fused_stats", False):      # before any step
        refuse_mlp_fused_stats_single(getattr(model.model.module.engine(model.batch_size, model.optimizer.global_batch), "step_path", "?"))
    tevery = getattr(args, "trajectory_every", None)
    if tevery is not None:
        if world > 1:
            raise RuntimeError(f"--trajectory_every needs {TRAJECTORY_NEEDS}: it does not combine with data parallelism")
        check_trajectory_model(model)            # before any step
        model.trajectory_every = tevery          # train() takes GraphLoop(resident=True, trajectory_every=K) and prints the Train loop: line
    for fl in observables.attach(args, [model], model, build=False):      # refused before any step; the n_print events read the
        print(fl.banner_one(model))                                       # attributes (GenerativeModel._stats_event)
    if rank == 0:
        eng = model.model.module.engine(model.batch_size, model.optimizer.global_batch)
        loop = {True: "graph loop (--fast_loop)", None: "loop chosen by model"}.get(getattr(args, "fast_loop", False), "one library call per step")
        print(f"Train step: {eng.step_path} kernels (vaek_train_step_path), {loop}")
    model.train()
    model.plot()
    model.save(final=True)
    if tevery is not None:
        write_trajectory(model, model._graph_loop)
    if dist is not None:
        model.check_replicas()
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main(parse_arguments()))
