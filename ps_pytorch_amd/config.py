"""CLI flag surface, compatible with the reference's argparse contract.

Flag names/semantics mirror /root/reference/src/distributed_nn.py:24-68 and
single_machine.py (the declared compatibility surface); new MI355X-specific
knobs are added under their own names and default to sane values.
"""
from __future__ import annotations

import argparse
import dataclasses
from typing import Optional


def str2bool(v: str) -> bool:
    # The reference used `type=bool`, where any non-empty string is truthy
    # (SURVEY.md §5 "Config / flag system"); we accept the same spellings but
    # parse them properly.
    if isinstance(v, bool):
        return v
    return v.lower() not in ("", "0", "false", "no", "none")


def add_fit_args(parser: argparse.ArgumentParser) -> argparse.ArgumentParser:
    """Training flags (reference parity: distributed_nn.py:24-68)."""
    parser.add_argument('--batch-size', type=int, default=128, metavar='N',
                        help='per-worker input batch size for training')
    parser.add_argument('--test-batch-size', type=int, default=500, metavar='N',
                        help='input batch size for testing')
    parser.add_argument('--epochs', type=int, default=100, metavar='N',
                        help='number of epochs to train')
    parser.add_argument('--max-steps', type=int, default=10000, metavar='N',
                        help='the maximum number of iterations')
    parser.add_argument('--lr', type=float, default=0.01, metavar='LR',
                        help='learning rate')
    parser.add_argument('--momentum', type=float, default=0.5, metavar='M',
                        help='SGD momentum')
    parser.add_argument('--seed', type=int, default=1, metavar='S',
                        help='random seed')
    parser.add_argument('--log-interval', type=int, default=10, metavar='N',
                        help='batches between log lines')
    parser.add_argument('--network', type=str, default='LeNet', metavar='N',
                        help='LeNet | ResNet18/34/50/101/152 | '
                             'VGG11/13/16/19[_BN|_plain][_ref] (_ref = the '
                             'reference dropout classifier head)')
    parser.add_argument('--mode', type=str, default='normal', metavar='N',
                        help='normal | kill | timeout : straggler handling '
                             '(kill = PS signal on quota, ref backward_signal_kill; '
                             'timeout = local --kill-threshold abort)')
    parser.add_argument('--kill-threshold', type=float, default=7.0, metavar='KT',
                        help='timeout threshold (s) that triggers straggler kill')
    parser.add_argument('--dataset', type=str, default='MNIST', metavar='N',
                        help='MNIST | Cifar10 | Cifar100 | SVHN | ImageNet-syn')
    parser.add_argument('--comm-type', type=str, default='Bcast', metavar='N',
                        help='Bcast (collective weight distribution) | Async (P2P)')
    parser.add_argument('--num-aggregate', type=int, default=5, metavar='N',
                        help='how many worker gradients count per iteration')
    parser.add_argument('--eval-freq', type=int, default=50, metavar='N',
                        help='checkpoint every this many steps')
    parser.add_argument('--train-dir', type=str, default='output/models/', metavar='N',
                        help='shared directory for model_step_<k> checkpoints')
    parser.add_argument('--compress-grad', type=str, default='compress', metavar='N',
                        help='compress | None : wire compression for gradients')
    parser.add_argument('--data-dir', type=str, default=None, metavar='DIR',
                        help='directory holding real dataset files (MNIST idx / '
                             'CIFAR pickle batches / SVHN .mat); falls back to '
                             './<name>_data, then synthetic data')
    parser.add_argument('--enable-gpu', type=str2bool, nargs='?', const=True,
                        default=False, help='run compute on GPUs (one rank per GPU)')
    parser.add_argument('--no-cuda', action='store_true', default=False,
                        help='disables GPU training (overrides --enable-gpu; '
                             'reference flag parity, distributed_nn.py:42)')
    # --- MI355X-native knobs (new; not in the reference) ---
    parser.add_argument('--wire-dtype', type=str, default='fp32',
                        help='fp32 | bf16 : uncompressed wire dtype (one declared '
                             'dtype end-to-end; SURVEY.md §2.4 dtype-quirk note)')
    parser.add_argument('--compute-dtype', type=str, default='bf16',
                        help='bf16 | fp32 : worker compute dtype on GPU')
    parser.add_argument('--bucket-mb', type=float, default=4.0,
                        help='gradient bucket size (MB) for overlapped RCCL ops')
    parser.add_argument('--overlap', type=str2bool, nargs='?', const=True, default=True,
                        help='overlap gradient push with backward (side HIP stream)')
    parser.add_argument('--aggregation', type=str, default='collective',
                        help='collective (reduce-to-root) | gather (per-worker P2P, '
                             'enables arrival-order --num-aggregate selection)')
    parser.add_argument('--error-feedback', type=str2bool, nargs='?',
                        const=True, default=False,
                        help='error feedback for the lossy gradient wire '
                             'codecs (gather+compress int8, or an fp32 '
                             'gradient on a bf16 wire): each worker keeps '
                             'what the codec dropped and adds it to its next '
                             'gradient. The residual is worker-local and not '
                             'checkpointed: --resume-step restarts it from '
                             'zero, like the momentum buffer. With '
                             '--num-aggregate below the worker count a late '
                             'payload the PS discards is still charged to '
                             'its worker\'s residual')
    parser.add_argument('--compress-codec', type=str, default='q8',
                        help='q8 | topk : gather-mode gradient codec under '
                             '--compress-grad compress. q8 = block-scaled '
                             'int8 (4x under an fp32 wire); topk = the '
                             '--topk-k largest magnitudes of every 256 '
                             'elements as (u8 index, bf16 value), the rest '
                             'carried in the error-feedback residual '
                             '(switches --error-feedback on)')
    parser.add_argument('--topk-k', type=int, default=16, metavar='K',
                        help='4 | 8 | 16 | 32 : elements kept per 256-block '
                             'by --compress-codec topk (3*K bytes per block '
                             'on the wire)')
    parser.add_argument('--fan-in', type=str, default='arrival',
                        help='arrival | fused : PS-side gradient fan-in of '
                             '--aggregation gather. arrival = every payload '
                             'is accumulated as it arrives (the sum is taken '
                             'in arrival order), then one optimizer pass; '
                             'fused = once a bucket\'s first --num-aggregate '
                             'workers are known, one kernel decodes their '
                             'payloads, sums them in ascending worker rank, '
                             'applies the update to that slice and re-packs '
                             'its broadcast payload: the result depends on '
                             'which workers counted, not on their arrival '
                             'order (at most 16 workers)')
    parser.add_argument('--resume-step', type=int, default=0,
                        help='warm-start: load train-dir/model_step_<K> '
                             'into the global model before training '
                             '(parameters only — the reference checkpoints '
                             'no optimizer state; 0 = fresh start)')
    parser.add_argument('--optimizer', type=str, default='sgd',
                        help='PS-side optimizer: sgd | adam | lars (the '
                             'reference ships optim/adam.py but hardwires SGD '
                             'at sync_replicas_master_nn.py:126 — here the '
                             'fused flat optimizers are selectable; lars = '
                             'momentum SGD with a per-tensor trust ratio, '
                             'the large-batch recipe, and the one optimizer '
                             'whose --lr-schedule a captured step graph '
                             'follows)')
    parser.add_argument('--weight-decay', type=float, default=0.0,
                        metavar='WD',
                        help='L2 weight decay of the PS-side optimizer (lars '
                             'exempts 1-D tensors: biases, BN affine)')
    parser.add_argument('--lars-eta', type=float, default=1e-3, metavar='ETA',
                        help='LARS trust coefficient: per tensor the step is '
                             'lr * eta*|w| / (|g| + wd*|w|)')
    parser.add_argument('--lr-schedule', type=str, default='constant',
                        help='constant | step | poly | cosine over '
                             '--max-steps, after --warmup-steps of linear '
                             'warmup: step multiplies by --lr-decay-gamma '
                             'every --lr-decay-steps, poly decays with power '
                             '2 to zero, cosine is one half period. sgd and '
                             'adam follow it on the eager paths only (their '
                             'kernels take lr by value, so graph capture is '
                             'refused); lars reads it on the device')
    parser.add_argument('--warmup-steps', type=int, default=0, metavar='N',
                        help='linear LR warmup from lr/N over the first N '
                             'steps')
    parser.add_argument('--lr-decay-steps', type=int, default=0, metavar='N',
                        help='steps between decays of --lr-schedule step')
    parser.add_argument('--lr-decay-gamma', type=float, default=0.1,
                        metavar='G',
                        help='decay factor of --lr-schedule step')
    parser.add_argument('--engine', type=str, default='ps',
                        help='ps (1 PS + N-1 workers, the reference design) | '
                             'allreduce (collective DP on all N ranks — the '
                             'reference\'s vendored data_parallel_dist.py, built '
                             'properly)')
    parser.add_argument('--loader', type=str, default='torch',
                        help='torch | fused : real-data batch pipeline (torch '
                             '= tensor-op augmentation with a CPU generator; '
                             'fused = one in-tree kernel per batch with '
                             'counter-based Philox draws, capturable into the '
                             'step graph; synthetic data ignores it)')
    parser.add_argument('--train-metrics', type=str2bool, nargs='?',
                        const=True, default=False,
                        help='Prec@1 / Prec@5 of the training batches on the '
                             'log lines (the reference trainer\'s step line, '
                             'nn_ops.py:80-86): counted on the device by the '
                             'fused loss kernel, inside the captured step, '
                             'and read once per --log-interval; covers the '
                             'steps since the last log line')
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description='ps_pytorch_amd')
    add_fit_args(parser)
    return parser.parse_args(argv)


@dataclasses.dataclass
class JobConfig:
    """Normalized config shared by all roles."""
    network: str = 'LeNet'
    dataset: str = 'MNIST'
    batch_size: int = 128
    test_batch_size: int = 500
    epochs: int = 100
    max_steps: int = 10000
    lr: float = 0.01
    momentum: float = 0.5
    seed: int = 1
    log_interval: int = 10
    mode: str = 'normal'
    kill_threshold: float = 7.0
    comm_type: str = 'Bcast'
    num_aggregate: int = 5
    eval_freq: int = 50
    train_dir: str = 'output/models/'
    compress_grad: str = 'compress'
    data_dir: Optional[str] = None
    enable_gpu: bool = False
    wire_dtype: str = 'fp32'
    compute_dtype: str = 'bf16'
    bucket_mb: float = 4.0
    overlap: bool = True
    aggregation: str = 'collective'
    engine: str = 'ps'
    optimizer: str = 'sgd'
    resume_step: int = 0
    loader: str = 'torch'
    error_feedback: bool = False
    train_metrics: bool = False
    compress_codec: str = 'q8'
    topk_k: int = 16
    fan_in: str = 'arrival'
    weight_decay: float = 0.0
    lars_eta: float = 1e-3
    lr_schedule: str = 'constant'
    warmup_steps: int = 0
    lr_decay_steps: int = 0
    lr_decay_gamma: float = 0.1

    def __post_init__(self) -> None:
        if self.lr_schedule not in ('constant', 'step', 'poly', 'cosine'):
            raise ValueError(f"unknown --lr-schedule {self.lr_schedule!r}")
        if self.weight_decay < 0:
            raise ValueError(f"--weight-decay must be >= 0, got "
                             f"{self.weight_decay!r}")
        if self.warmup_steps < 0:
            raise ValueError(f"--warmup-steps must be >= 0, got "
                             f"{self.warmup_steps!r}")
        if self.lr_schedule == 'step' and self.lr_decay_steps < 1:
            raise ValueError("--lr-schedule step needs --lr-decay-steps >= 1")
        # a warmup as long as the run would leave the decay nothing to span
        if self.warmup_steps >= max(self.max_steps, 1) and self.warmup_steps:
            import warnings
            warnings.warn(f"--warmup-steps {self.warmup_steps} covers all "
                          f"--max-steps {self.max_steps}; clamping to "
                          f"{max(self.max_steps, 1) - 1}")
            self.warmup_steps = max(self.max_steps, 1) - 1
        if self.fan_in not in ('arrival', 'fused'):
            raise ValueError(f"unknown --fan-in {self.fan_in!r}")
        if self.compress_codec not in ('q8', 'topk'):
            raise ValueError(f"unknown --compress-codec {self.compress_codec!r}")
        if self.topk_k not in (4, 8, 16, 32):
            raise ValueError(f"--topk-k must be 4, 8, 16 or 32, got "
                             f"{self.topk_k!r}")
        if self.loader not in ('torch', 'fused'):
            raise ValueError(f"unknown --loader {self.loader!r}")
        if self.mode not in ('normal', 'kill', 'timeout'):
            raise ValueError(f"unknown --mode {self.mode!r}")
        if self.aggregation not in ('collective', 'gather'):
            raise ValueError(f"unknown --aggregation {self.aggregation!r}")
        if self.optimizer not in ('sgd', 'adam', 'lars'):
            raise ValueError(f"unknown --optimizer {self.optimizer!r}")
        # --mode kill needs arrival-order fan-in: the PS's kill verdict fires
        # from the gather drain's first-k quota (parallel/ps.py); a collective
        # reduce has no arrival order and would never send a verdict, hanging
        # every worker at its end-of-step verdict recv. Normalize rather than
        # reject: the reference's --mode kill ran on its (gather-like)
        # per-layer P2P protocol without a separate aggregation flag.
        if self.mode == 'kill' and self.aggregation != 'gather':
            import warnings
            warnings.warn("--mode kill requires --aggregation gather "
                          "(arrival-order first-k drives the kill verdict); "
                          "switching aggregation to 'gather'")
            self.aggregation = 'gather'
        # The fused fan-in replaces the PS's per-arrival accumulate of the
        # gather drain; a collective reduce sums in flight and the allreduce
        # engine has no PS, so there is nothing for it to fuse there.
        if self.fan_in == 'fused':
            import warnings
            if self.engine != 'ps':
                warnings.warn("--fan-in fused applies to the PS engine's "
                              f"gather fan-in only; --engine {self.engine} "
                              "runs without it")
                self.fan_in = 'arrival'
            elif self.aggregation != 'gather':
                warnings.warn("--fan-in fused needs --aggregation gather "
                              "(a collective reduce has no per-worker "
                              "payloads to fuse); running the arrival "
                              "fan-in")
                self.fan_in = 'arrival'
        # The top-k codec exists only as a gather-mode payload of the PS
        # engine (a sum of sparse payloads cannot ride a reduction) and only
        # on the error-feedback path: without feedback most coordinates
        # would never be sent. Anything else falls back to what the same
        # flags do without it.
        if self.compress_codec == 'topk':
            import warnings
            if self.engine != 'ps':
                warnings.warn("--compress-codec topk applies to the PS "
                              "engine's gather push only; --engine "
                              f"{self.engine} runs without it")
                self.compress_codec = 'q8'
            elif not self.compress or self.aggregation != 'gather':
                warnings.warn("--compress-codec topk needs --compress-grad "
                              "compress and --aggregation gather (collective "
                              "mode ignores gradient codecs); running "
                              "without the topk codec")
                self.compress_codec = 'q8'
            elif not self.error_feedback:
                warnings.warn("--compress-codec topk only converges with "
                              "error feedback (unsent coordinates live in "
                              "the residual); switching --error-feedback on")
                self.error_feedback = True
        # Error feedback only has something to feed back where the push
        # loses bits: the int8 codec (gather + compress) or a bf16 wire under
        # an fp32 gradient. A lossless wire gets the same normalize-and-warn
        # treatment; the transport re-checks per rank with the actual dtypes
        # (the bf16 wire only exists on GPUs).
        if self.error_feedback and not (self.compress
                                        or self.wire_dtype == 'bf16'):
            import warnings
            warnings.warn("--error-feedback has nothing to feed back on a "
                          "lossless fp32 gradient wire (--compress-grad None "
                          "--wire-dtype fp32); running without it")
            self.error_feedback = False
        if self.error_feedback and self.engine != 'ps':
            import warnings
            warnings.warn("--error-feedback applies to the PS engine's "
                          "gradient push only; running without it")
            self.error_feedback = False

    @property
    def compress(self) -> bool:
        return str(self.compress_grad).lower() in ('compress', 'true', '1')

    @classmethod
    def from_args(cls, args: argparse.Namespace) -> "JobConfig":
        known = {f.name for f in dataclasses.fields(cls)}
        kw = {k: v for k, v in vars(args).items() if k in known}
        if getattr(args, 'no_cuda', False):
            kw['enable_gpu'] = False
        return cls(**kw)


def num_classes_of(dataset: str) -> int:
    d = dataset.lower()
    if d in ('mnist', 'cifar10', 'svhn'):
        return 10
    if d == 'cifar100':
        return 100
    if d in ('imagenet-syn', 'imagenet'):
        return 1000
    raise ValueError(f"unknown dataset {dataset!r}")


def input_shape_of(dataset: str):
    d = dataset.lower()
    if d == 'mnist':
        return (1, 28, 28)
    if d in ('cifar10', 'cifar100', 'svhn'):
        return (3, 32, 32)
    if d in ('imagenet-syn', 'imagenet'):
        return (3, 224, 224)
    raise ValueError(f"unknown dataset {dataset!r}")
