"""Command line of the reference (argparser.py:46-203): same flag names, defaults and ``--method``
presets, declared from a table.  Differences, both documented in SURVEY.md section 0: ``UCD`` is an
accepted ``--method`` (the reference's parser rejects the preset its own code handles), and
``--opt_level`` selects the activation precision of this build (O0 = fp32 like apex O0, O1..O3 = bf16
autocast with fp32 master weights) instead of an apex mode."""
from __future__ import annotations

import argparse
import math

from . import tasks

# method -> option overrides (reference argparser.py:15-39)
METHOD_PRESETS = {
    "FT": {},
    "LWF": {"loss_kd": 100},
    "LWF-MC": {"icarl": True, "icarl_importance": 10},
    "ILT": {"loss_kd": 100, "loss_de": 100},
    "EWC": {"regularizer": "ewc", "reg_importance": 500},
    "RW": {"regularizer": "rw", "reg_importance": 100},
    "PI": {"regularizer": "pi", "reg_importance": 500},
    "MiB": {},
    "att": {},
    "UCD": {"loss_kd": 10, "unce": True, "unkd": True, "init_balanced": True},
    # PLOP (Douillard et al., CVPR 2021): entropy pseudo-labels with the adaptive factor, Local POD on the features, plain cross
    # entropy, no distillation of the logits, no contrastive term.  The preset leaves PLOP's POD on the logits off; --method PLOP
    # --pod_logits is the complete method
    "PLOP": {"pseudo": "entropy", "pseudo_adaptive": True, "pod_factor": 0.01, "pod_last_factor": 0.0005, "init_balanced": True,
             "pixcon_weight": 0.0},
    # SDR (Michieli and Zanuttigh, CVPR 2021) without its sparsity term: MiB's unbiased losses plus prototype matching, feature
    # clustering and prototype repulsion on the pre-logits.  The three weights are recalled from SDR's published command line and
    # not checked against its code
    "SDR": {"loss_kd": 10, "unce": True, "unkd": True, "init_balanced": True, "pixcon_weight": 0.0, "sdr_match": 0.01,
            "sdr_attract": 0.001, "sdr_repel": 0.001},
}
NUM_CLASSES = {"voc": 21, "ade": 150, "city": 20}


def modify_command_options(opts):
    if opts.dataset in NUM_CLASSES:
        opts.num_classes = NUM_CLASSES[opts.dataset]
    if not opts.visualize:
        opts.sample_num = 0
    for key, value in METHOD_PRESETS.get(opts.method, {}).items():
        setattr(opts, key, value)
    if getattr(opts, "pseudo", None) is not None and (opts.bce or opts.icarl):
        raise ValueError("--pseudo cannot be combined with --bce / --icarl / --method LWF-MC: the pseudo-labels carry a per-image "
                         "weight on the cross entropy, which the BCE kernel does not take and PLOP does not define for it")
    if getattr(opts, "focal_loss", False) and (opts.bce or opts.icarl):
        raise ValueError("--focal_loss cannot be combined with --bce / --icarl / --method LWF-MC: the reference defines the focal "
                         "modulation on the soft-max cross entropy only")
    opts.no_overlap = not opts.overlap
    opts.no_cross_val = not opts.cross_val
    return opts


def _flag(name, **kw):
    return (name, kw)


class _EvalScales(argparse.Action):
    """--eval_scales: the plain view is always evaluated (loss and teacher terms come from it), so the list must hold 1.0"""

    def __call__(self, parser, namespace, values, option_string=None):
        if 1.0 not in values:
            parser.error(f"{option_string} must contain 1.0 (the plain view), got {' '.join(str(v) for v in values)}")
        if any(v <= 0 for v in values):
            parser.error(f"{option_string} takes positive scales, got {' '.join(str(v) for v in values)}")
        setattr(namespace, self.dest, values)


def _pseudo_bins(text):
    """--pseudo_nb_bins: what the histogram kernel takes"""
    value = int(text)
    if not 2 <= value <= 1024:
        raise argparse.ArgumentTypeError(f"the number of bins must be in 2 .. 1024, got {value}")
    return value


def _unit_interval(text):
    """--pseudo_adaptive_min: a floor of the per-image weight on the cross entropy, which the loss kernels take in [0, 1]"""
    value = float(text)
    if not 0.0 <= value <= 1.0:
        raise argparse.ArgumentTypeError(f"the value must be in [0, 1], got {text}")
    return value


def _focal_gamma(text):
    """--focal_loss_gamma: the exponent of the focal modulation, finite and >= 0"""
    value = float(text)
    if not (math.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"gamma must be finite and >= 0, got {text}")
    return value


def _focal_alpha(text):
    """--focal_loss_alpha: the factor of the focal loss, finite and > 0"""
    value = float(text)
    if not (math.isfinite(value) and value > 0.0):
        raise argparse.ArgumentTypeError(f"alpha must be finite and > 0, got {text}")
    return value


def _weight(text):
    """--sdr_match / --sdr_attract / --sdr_repel: the weight of a loss term, finite and >= 0 (0: the term is off)"""
    value = float(text)
    if not (math.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"the weight must be finite and >= 0, got {text}")
    return value


class _PodScales(argparse.Action):
    """--pod_scales: 1 to 4 strictly increasing scales, each in 1 .. 8 (what the Local POD kernels take)"""

    def __call__(self, parser, namespace, values, option_string=None):
        if not 1 <= len(values) <= 4 or any(not 1 <= v <= 8 for v in values) or any(b <= a for a, b in zip(values, values[1:])):
            parser.error(f"{option_string} takes 1 to 4 strictly increasing scales in 1 .. 8, got {' '.join(str(v) for v in values)}")
        setattr(namespace, self.dest, values)


def eval_views(opts):
    """The test-time views of ``--eval_scales`` / ``--eval_flip`` as ``[(scale, flip), ...]``: the plain view ``(1.0, False)`` first,
    then the other scales in the order given, each followed by its mirror under ``--eval_flip``.  ``--fusion-mode`` says how their
    class distributions are fused (``Trainer.test``; csrc/seg_views.hip)."""
    scales = [float(s) for s in (getattr(opts, "eval_scales", None) or [1.0])]
    flip = bool(getattr(opts, "eval_flip", False))
    ordered = [1.0] + [s for s in scales if s != 1.0]
    return [(s, f) for s in ordered for f in ((False, True) if flip else (False,))]


_ON, _OFF = dict(action="store_true", default=False), dict(action="store_false", default=True)
_ARGS = [
    # performance
    _flag("--local_rank", type=int, default=0), _flag("--random_seed", type=int, default=42),
    _flag("--num_workers", type=int, default=0),
    # HBM budget per process, in GiB, for decoded samples kept on the device (ucd_amd/datacache.py); 0: decode every epoch
    _flag("--cache_gb", type=float, default=0.0),
    # dataset
    _flag("--data_root", type=str, default="data"),
    _flag("--dataset", type=str, default="voc", choices=["voc", "ade", "city"]),
    _flag("--num_classes", type=int, default=None),
    # method (overrides other parameters)
    _flag("--method", type=str, default=None, choices=list(METHOD_PRESETS)),
    # train
    _flag("--epochs", type=int, default=30), _flag("--fix_bn", **_ON),
    _flag("--batch_size", type=int, default=4), _flag("--crop_size", type=int, default=512),
    _flag("--lr", type=float, default=0.007), _flag("--momentum", type=float, default=0.9),
    _flag("--weight_decay", type=float, default=1e-4),
    _flag("--lr_policy", type=str, default="poly", choices=["poly", "step"]),
    _flag("--lr_decay_step", type=int, default=5000), _flag("--lr_decay_factor", type=float, default=0.1),
    _flag("--lr_power", type=float, default=0.9), _flag("--bce", **_ON),
    # validation
    _flag("--val_on_trainset", **_ON), _flag("--cross_val", **_ON), _flag("--crop_val", **_OFF),
    # logging
    _flag("--logdir", type=str, default="./logs"), _flag("--name", type=str, default="Experiment"),
    _flag("--sample_num", type=int, default=0), _flag("--debug", **_ON), _flag("--visualize", **_OFF),
    _flag("--print_interval", type=int, default=10), _flag("--val_interval", type=int, default=1),
    _flag("--ckpt_interval", type=int, default=1),
    # model
    _flag("--backbone", type=str, default="resnet101", choices=["resnet50", "resnet101"]),
    _flag("--output_stride", type=int, default=16, choices=[8, 16]), _flag("--no_pretrained", **_ON),
    _flag("--norm_act", type=str, default="iabn_sync", choices=["iabn_sync", "iabn", "abn", "std"]),
    _flag("--fusion-mode", metavar="NAME", type=str, choices=["mean", "voting", "max"], default="mean"),
    _flag("--pooling", type=int, default=32), _flag("--temperature", type=float, default=0.07),
    # test / checkpoints
    _flag("--test", **_ON), _flag("--ckpt", default=None, type=str),
    # test-time views (the final test pass and evaluate.py): scales of the image, each also mirrored; fused by --fusion-mode
    _flag("--eval_scales", type=float, nargs="+", default=[1.0], action=_EvalScales), _flag("--eval_flip", **_ON),
    # distillation (ILT)
    _flag("--freeze", **_ON), _flag("--loss_de", type=float, default=0.), _flag("--loss_kd", type=float, default=0.),
    # Local POD feature distillation (PLOP): factor of the four backbone stage maps (0: off; PLOP uses 0.01), of the head output,
    # and the pooling scales (ucd_amd.loss.fused_local_pod)
    _flag("--pod_factor", type=float, default=0.), _flag("--pod_last_factor", type=float, default=0.0005),
    _flag("--pod_scales", type=int, nargs="+", default=[1, 2, 4], action=_PodScales),
    # PLOP's POD on the logits, next to --pod_factor: the logits become a sixth level (factor --pod_last_factor, the student's
    # new-class channels summed into the background; ucd_amd.loss.fused_local_pod_logits) and the head output an ordinary one
    # (factor --pod_factor); --pod_logits_norm 0: that level's embeddings are not normalised
    _flag("--pod_logits", **_ON), _flag("--pod_logits_norm", type=int, default=1, choices=[0, 1]),
    # PLOP's pseudo-labelling (ucd_amd.loss.fused_pseudo_labels): background pixels take the teacher's class where the entropy of
    # its soft-max, as a fraction of log K, is below the class's median over the training set (floored at --pseudo_threshold;
    # histogram of --pseudo_nb_bins bins); --pseudo_adaptive weighs an image's cross entropy by its share of kept candidates
    _flag("--pseudo", type=str, default=None, choices=["entropy"]), _flag("--pseudo_threshold", type=float, default=0.001),
    _flag("--pseudo_nb_bins", type=_pseudo_bins, default=100), _flag("--pseudo_adaptive", **_ON),
    _flag("--pseudo_adaptive_min", type=_unit_interval, default=0.0),
    # focal cross entropy (the reference's FocalLoss): the criterion of the train step and of validation becomes
    # alpha (1 - p_t)^gamma CE, inside the fused logit-loss kernels (ucd_amd.loss.fused_seg_losses(focal=...)); with --unce the
    # unbiased cross entropy is modulated, under --pseudo_adaptive the image's weight multiplies it
    _flag("--focal_loss", **_ON), _flag("--focal_loss_gamma", type=_focal_gamma, default=2.0),
    _flag("--focal_loss_alpha", type=_focal_alpha, default=1.0),
    # SDR's class-prototype feature losses on the raw pre-logits (ucd_amd.loss.fused_proto_losses), each weight 0 = off: the batch
    # means against the previous step's prototypes (needs a teacher), the pixels against their class's running prototype, the
    # batch means against each other
    _flag("--sdr_match", type=_weight, default=0.), _flag("--sdr_attract", type=_weight, default=0.),
    _flag("--sdr_repel", type=_weight, default=0.),
    # regularisers (EWC / RW / PI; --method EWC|RW|PI): ucd_amd.regularizer, after the UCD step
    _flag("--regularizer", default=None, type=str, choices=["ewc", "rw", "pi"]),
    _flag("--reg_importance", type=float, default=1.), _flag("--reg_alpha", type=float, default=0.9),
    _flag("--reg_no_normalize", **_ON), _flag("--reg_iterations", type=int, default=10),
    # iCaRL
    _flag("--icarl", **_ON), _flag("--icarl_importance", type=float, default=1.),
    _flag("--icarl_disjoint", **_ON), _flag("--icarl_bkg", **_ON),
    # MiB / UCD switches
    _flag("--init_balanced", **_ON), _flag("--unkd", **_ON), _flag("--alpha", default=1., type=float),
    _flag("--unce", **_ON),
    # incremental protocol
    _flag("--task", type=str, default="19-1", choices=tasks.get_task_list()),
    _flag("--step", type=int, default=0), _flag("--no_mask", **_ON), _flag("--overlap", **_ON),
    _flag("--step_ckpt", default=None, type=str),
    _flag("--opt_level", type=str, choices=["O0", "O1", "O2", "O3"], default="O0"),
    _flag("--MASTER_PORT", type=str, default="29501"),
]


def get_argparser():
    parser = argparse.ArgumentParser(description="UCD incremental segmentation (MI355X-native hot path)")
    for name, kw in _ARGS:
        parser.add_argument(name, **kw)
    return parser
