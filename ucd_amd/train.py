"""``Trainer``: one UCD training iteration on an MI355X, reference interface (train.py:15-384).

``Trainer(model, model_old, device, opts, trainer_state, classes)`` and
``.train(cur_epoch, optim, train_loader, scheduler, print_int, logger) -> (epoch_loss, reg_loss)`` keep
the reference's call shapes.  The iteration is the reference's ``train.py:95-151`` with the UCD branch
repaired as intended (``pre_contractive_pixel`` returns five values and
``PixelConLossV2`` takes five):

    teacher forward (eval, no grad)          train.py:100-102
    student forward (train)                  :108
    loss = mean(CE(out, labels)) + PixCon(student/teacher pre-logits) / 100          :115-116
    lkd  = loss_kd * KD(out, out_old)        :131-133
    backward; gradient all-reduce; SGD; PolyLR step                                   :135-151

What changed for the hardware: activations are channels-last bf16 (``--opt_level`` O1..O3) or fp32 (O0);
the contrastive term is one fused HIP operation with no host round trip; the per-iteration ``.item()``
reads (train.py:153-157, >= 5 device syncs) are replaced by device-side accumulators read once per
``print_int`` iterations; gradient averaging overlaps the backward (ucd_amd.ddp).
The logit losses - (unbiased or plain) CE with no, the plain or the unbiased KD at any ``--alpha``: FT, LWF, ILT, MiB, UCD -
come from one fused HIP kernel on the low-resolution logits (``UCD_SEG_KD_EX=0``: only the pairs without ``--alpha`` / plain
KD); ILT's encoder term is one HIP operation on the raw maps (``UCD_FUSED_LDE=0``: torch), which puts ILT inside the graphs.
EWC / PI / RW (``--method EWC|PI|RW``) add the weight-space penalty of ucd_amd.regularizer between the gradient
all-reduce and the optimiser (train.py:139-145).  ``--bce``, ``--icarl`` and ``--method LWF-MC`` take the per-class binary cross
entropy and the combined iCaRL term (train.py:119-124) from their own fused HIP kernel (``fused_seg_bce``, csrc/seg_gather.hip),
inside the graphs like the others.  ``validate`` and ``test`` (train.py:185-375) share one loop: losses and confusion matrix on the
device, the teacher-side terms evaluated eagerly, ``test`` rendering its outputs through ``ucd_amd.visual``.  Out of scope (raise ``NotImplementedError``): ``--icarl_disjoint`` with a teacher, and any BCE
run on a CPU device.
"""
from __future__ import annotations

import math
from functools import reduce

import torch
import torch.distributed as dist
import torch.nn as nn

from . import switches as _switches
from .contrastive import ucd_contrastive_loss
from .loss import (KnowledgeDistillationLoss, UnbiasedCrossEntropy, UnbiasedKnowledgeDistillationLoss,
                   POD_SCALES, fused_attn_mse, fused_local_pod, fused_local_pod_logits, fused_pseudo_labels, fused_seg_bce,
                   fused_seg_losses, pseudo_hist, pseudo_median, _focal_check, focal_modulate, fused_proto_losses, proto_classes,
                   proto_update)


def _raw(features, name):
    return features.raw(name) if hasattr(features, "raw") else features[name]


class Trainer:
    def __init__(self, model, model_old, device, opts, trainer_state=None, classes=None):
        self.model_old, self.model, self.device = model_old, model, device
        if classes is not None:
            tot_classes = reduce(lambda a, b: a + b, classes)
            self.old_classes = tot_classes - classes[-1]
            self.tot_classes = tot_classes
        else:
            self.old_classes, self.tot_classes = 0, getattr(opts, "num_classes", None) or 21
        # BCE family (train.py:34-36, :55-66): the criterion is the binary cross entropy of every class, --icarl adds the combined
        # distillation term next to a teacher.  Both come from one fused HIP kernel on the low-resolution logits (fused_seg_bce)
        self.bce = bool(opts.bce or opts.icarl)
        self.icarl_combined = bool(opts.icarl and not getattr(opts, "icarl_disjoint", False) and model_old is not None)
        self.icarl = float(getattr(opts, "icarl_importance", 1.0))
        if self.bce and device.type != "cuda":
            raise NotImplementedError("BCE / iCaRL (--bce, --icarl, --method LWF-MC) exist on the GPU only: the losses are one fused "
                                      "HIP kernel (ucd_amd.loss.fused_seg_bce), there is no CPU path")
        if opts.icarl and getattr(opts, "icarl_disjoint", False) and model_old is not None:
            raise NotImplementedError("BCE / iCaRL: --icarl_disjoint with a teacher is not supported - the reference's loop never assigns "
                                      "its loss on that branch (train.py:110-116 has no else), so there is nothing to be at parity with")
        self.temperature = opts.temperature
        self.pixcon_weight = getattr(opts, "pixcon_weight", 0.01)      # the reference hard-codes /100 (train.py:116)
        # the reference clamps down-sampled labels at the VOC bound 20 (utils/utils.py:267-268); datasets
        # with more classes need the real bound
        self.max_label = max(20, self.tot_classes - 1)
        if opts.unce and self.old_classes != 0:
            self.criterion = UnbiasedCrossEntropy(old_cl=self.old_classes, ignore_index=255, reduction="none")
        else:
            self.criterion = nn.CrossEntropyLoss(ignore_index=255, reduction="none")
        self.lde = opts.loss_de
        self.lde_flag = self.lde > 0. and model_old is not None
        self.lde_loss = nn.MSELoss()
        # the encoder term from the raw maps in one HIP operation (UCD_FUSED_LDE=0: attention maps + MSELoss in torch)
        self.fused_lde = self.lde_flag and device.type == "cuda" and _switches.get("UCD_FUSED_LDE", "1") != "0"
        # Local POD feature distillation (PLOP, --pod_factor): the raw outputs of body.mod2 .. mod5 (factor pod_factor) and the raw
        # pre-logits (pod_last_factor), student against teacher, each level one fused HIP operation (ucd_amd.loss.fused_local_pod);
        # gamma = sqrt(all classes / new classes) is PLOP's adaptive factor
        self.pod = float(getattr(opts, "pod_factor", 0.) or 0.)
        self.pod_flag = self.pod > 0. and model_old is not None
        if self.pod_flag:
            self.pod_last = float(getattr(opts, "pod_last_factor", 0.0005))
            self.pod_scales = tuple(int(s) for s in (getattr(opts, "pod_scales", None) or POD_SCALES))
            self.pod_slope = getattr(model, "module", model).pod_slope()
            getattr(model_old, "module", model_old).pod_slope()              # the teacher's maps are undone the same way
            self.pod_gamma = math.sqrt(self.tot_classes / max(self.tot_classes - self.old_classes, 1))
        # PLOP's POD on the logits (--pod_logits, next to --pod_factor): a sixth level on features["sem"], the student's new-class
        # channels summed into the background (ucd_amd.loss.fused_local_pod_logits); alone it requests nothing
        self.pod_logits = self.pod_flag and bool(getattr(opts, "pod_logits", False))
        self.pod_logits_norm = int(getattr(opts, "pod_logits_norm", 1))
        # PLOP's pseudo-labelling (--pseudo entropy): the cross entropy sees the labels of ucd_amd.loss.fused_pseudo_labels - a
        # background pixel takes the teacher's class where the teacher is confident, 255 where not - and, under --pseudo_adaptive,
        # a per-image weight.  The per-class thresholds come from one pass of the teacher over the training set
        # (find_pseudo_thresholds) and travel in the trainer state.  KD, POD, the contrastive term and validation keep the labels
        self.pseudo_flag = getattr(opts, "pseudo", None) is not None and model_old is not None
        self.pseudo_thresholds = self.pseudo_hist = None
        if self.pseudo_flag:
            if self.bce:
                raise NotImplementedError("--pseudo with --bce / --icarl: the BCE kernel takes no per-image weight")
            self.pseudo_floor = float(getattr(opts, "pseudo_threshold", 0.001))
            self.pseudo_bins = int(getattr(opts, "pseudo_nb_bins", 100))
            self.pseudo_adaptive = bool(getattr(opts, "pseudo_adaptive", False))
            self.pseudo_f_min = float(getattr(opts, "pseudo_adaptive_min", 0.0))
            # (trainer_state is the PREVIOUS step's: its thresholds belong to another teacher.  load_state_dict, on a resume of
            # this step, brings this step's)
        # focal cross entropy (--focal_loss; the reference's FocalLoss): the criterion of the train step and of validation is
        # alpha (1 - exp(-ce))^gamma ce on the step's cross entropy - plain or unbiased, after the pseudo-labels, times the adaptive
        # factor - inside the fused logit-loss kernels (fused_seg_losses(focal=...)); UCD_FUSED_FOCAL=0, the CPU and runs without the
        # fused losses take focal_modulate on the cross-entropy map of the up-sampled logits
        self.focal = None
        if getattr(opts, "focal_loss", False):
            if self.bce:
                raise NotImplementedError("--focal_loss with --bce / --icarl: the focal modulation is defined on the soft-max cross "
                                          "entropy only")
            self.focal = _focal_check(getattr(opts, "focal_loss_gamma", 2.0), getattr(opts, "focal_loss_alpha", 1.0))
        # SDR's class-prototype feature losses (--sdr_match / --sdr_attract / --sdr_repel) on the raw pre-logits: the batch means
        # against the previous step's prototypes (needs a teacher; alone it requests nothing), the pixels against their class's
        # running prototype, the batch means against each other - one fused HIP operation (ucd_amd.loss.fused_proto_losses).  The
        # running prototypes (proto_sum fp64 [T, C], proto_n int64 [T]) are device tensors allocated once: a captured step graph
        # reads and updates them by address; they travel in the trainer state
        self.proto_w = (float(getattr(opts, "sdr_match", 0.) or 0.) if model_old is not None else 0.,
                        float(getattr(opts, "sdr_attract", 0.) or 0.), float(getattr(opts, "sdr_repel", 0.) or 0.))
        self.proto_flag = any(v > 0. for v in self.proto_w)
        self.proto_sum = self.proto_n = self.proto_old = None
        if self.proto_flag:
            channels = getattr(getattr(model, "module", model), "head_channels", None)
            if channels is not None:
                self._alloc_proto(int(channels))
            # the previous step's state holds exactly the old model's prototypes (unlike the pseudo thresholds, which belong to the
            # current teacher); without one, find_prototypes makes them from the teacher
            prev = trainer_state.get("proto") if trainer_state is not None else None
            if self.proto_w[0] > 0. and prev is not None:
                self._old_from_state(prev)
        self.lkd = opts.loss_kd
        self.lkd_flag = self.lkd > 0. and model_old is not None
        self.lkd_loss = (UnbiasedKnowledgeDistillationLoss if opts.unkd else KnowledgeDistillationLoss)(alpha=opts.alpha)
        # The frozen teacher (eval mode, no gradients, no collectives) is replayed from a hipGraph after two eager
        # warm-up steps: ~330 kernel launches of host work per step disappear, which matters once the per-GPU batch
        # is small (8-GPU regime: the step is launch-bound, not GPU-bound).
        self.graph_teacher = bool(getattr(opts, "graph_teacher", True)) and device.type == "cuda" and model_old is not None
        self._tg = None
        self._tg_seen = 0
        # the teacher has no dependence on the student before the losses: it runs on a side stream next to the student's
        # forward, filling the gaps that the small 33x33 layers of either network leave on the GPU
        self.overlap_teacher = (bool(getattr(opts, "overlap_teacher", True)) and device.type == "cuda" and model_old is not None
                                and _switches.get("UCD_TEACHER_OVERLAP", "1") != "0")
        self._side = torch.cuda.Stream(device) if self.overlap_teacher else None
        self.ret_intermediate = self.lde
        self.unce = bool(opts.unce and self.old_classes != 0)
        # fused up-sampling + CE + KD kernel: every pair of (unbiased or plain) CE with no, the plain or the
        # unbiased KD, at any finite non-zero --alpha (LWF, ILT, MiB, UCD).  UCD_SEG_KD_EX=0: only the pairs of the first
        # kernel - no KD, or unbiased CE + unbiased KD at alpha 1 - and the torch modules on up-sampled logits for the rest
        self.kd_mode = "unbiased" if opts.unkd else "plain"
        self.alpha = float(opts.alpha)
        first_pair = bool(opts.unkd) and self.unce and self.alpha == 1.0
        any_pair = _switches.get("UCD_SEG_KD_EX", "1") != "0" and math.isfinite(self.alpha) and self.alpha != 0.0
        self.fuse_logit_losses = (getattr(opts, "fused_logit_losses", True) and device.type == "cuda"
                                  and (not self.lkd_flag or first_pair or any_pair))
        if self.focal is not None and _switches.get("UCD_FUSED_FOCAL", "1") == "0":
            self.fuse_logit_losses = False           # the composition over up-sampled logits
        if self.bce:
            # the student never up-samples under BCE: a --loss_kd term next to it (--method LWF --bce) comes from the fused kernel
            # too (its CE value discarded, old_cl 1 next to a teacher), which only the any-pair form of that kernel serves
            if self.lkd_flag and not any_pair:
                raise NotImplementedError("BCE / iCaRL with --loss_kd needs the fused logit-loss kernel for the KD term (UCD_SEG_KD_EX=0 "
                                          "or an --alpha of 0 / inf would send it to the torch modules): BCE runs have no up-sampled "
                                          "logits")
            self.fuse_logit_losses = True
        # an ILT iteration reads the lazy attention maps of the Features dict unless both of its losses are fused: such a run stays
        # outside the teacher graph and the whole-step graph
        self.lde_lazy = self.lde_flag and not (self.fused_lde and self.fuse_logit_losses)
        self.amp = getattr(opts, "opt_level", "O0") != "O0"
        # test-time views of the final test pass (--eval_scales / --eval_flip) and the rule that fuses them (--fusion-mode)
        from .argparser import eval_views
        self.eval_views = eval_views(opts)
        self.fusion_mode = getattr(opts, "fusion_mode", "mean")
        # contrastive arithmetic: exact fp32 MFMA with fp32 activations (O0), fp16 operands otherwise
        self.pixcon_precision = getattr(opts, "pixcon_precision", None) or ("f16" if self.amp else "f32")
        # frozen teacher under autocast: static bf16 copies of its convolution weights (no per-call casts)
        self._teacher_w16 = None
        if self.amp and device.type == "cuda" and model_old is not None and getattr(opts, "bf16_weights", True):
            from .master import Bf16Weights
            self._teacher_w16 = Bf16Weights(model_old, trainable=False)
        # EWC / PI / RW (train.py:69-72): the whole UCD step, then the weight-space penalty (ucd_amd.regularizer).  Built after
        # the teacher's Bf16Weights, which moves its fp32 convolution weights into one flat buffer: theta_old then points at
        # the storage the teacher keeps, not at a copy it dropped
        self.regularizer, self.regularizer_flag = None, False
        if getattr(opts, "regularizer", None) is not None:
            from .regularizer import get_regularizer
            reg_state = trainer_state["regularizer"] if trainer_state is not None else None
            self.regularizer = get_regularizer(model, model_old, device, opts, reg_state)
            self.regularizer_flag = self.regularizer is not None
        self.last = {}
        # The WHOLE iteration (teacher + student forward, losses, backward, gradient buckets, optimiser) as one hipGraph,
        # captured after the eager warm-up iterations and replayed from then on: at the per-rank batch of the 8-GPU run
        # (3 images) the host needs ~14 ms to enqueue ~1200 launches of ~12 ms of kernels; a replay needs none of it.
        # UCD_STEP_GRAPH = auto (default): single-process runs only - a multi-rank capture would put the SyncBN and gradient
        # collectives into the graph, which no box available to this build can exercise; 1 = always try; 0 = never.
        sw = _switches.get("UCD_STEP_GRAPH", "auto")
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        self.step_graph = (device.type == "cuda" and bool(getattr(opts, "step_graph", True)) and sw != "0"
                           and (world == 1 or sw == "1") and not self.lde_lazy)
        self.step_graph_warmup = 3          # eager iterations before the capture (solver search, GEMM tuning, optimiser tables)
        self._sg = None
        self._sg_seen = 0
        self.graph_steps = 0                # iterations served by a graph replay (bench.py reports it)
        self.step_graph_error = None

    def enable_multi_rank_step_graph(self):
        """Turn the captured iteration on for a run with more than one rank (or a one-rank group with forced collectives), AFTER the
        eager iterations have been measured: both collective kinds must sit on library-owned RCCL communicators (the SyncBN exchanges:
        ucd_amd.comm.direct_comm of the default group; the gradient buckets: GradReducer.enable_direct) and every rank must agree -
        otherwise the run stays eager.  Collective: every rank calls it at the same point.  Returns True when the next iterations
        will be captured."""
        if self.device.type != "cuda" or _switches.get("UCD_STEP_GRAPH", "auto") == "0" or self.lde_lazy:
            return False
        ok = True
        if dist.is_available() and dist.is_initialized():
            from . import abn as _abn
            from .comm import _agree, direct_comm
            reducer = getattr(self.model, "reducer", None)
            ok = reducer is not None and reducer.enable_direct()
            ok = _agree(ok, None, self.device)
            if ok and (dist.get_world_size() > 1 or _abn._FORCE_SYNC):
                ok = direct_comm(None) is not None                          # same answer on every rank (its own agreement rounds)
        if ok:
            self.step_graph, self._sg, self._sg_seen, self.step_graph_error = True, None, 0, None
        return ok

    # ------------------------------------------------------------------------------------------
    def _autocast(self):
        return torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=self.amp and self.device.type == "cuda")

    def _teacher_eager(self, images, up):
        with torch.no_grad(), self._autocast():
            return self.model_old(images, x_b_old=None, x_pl_old=None, ret_intermediate=self.ret_intermediate, **up)

    def _teacher_forward(self, images, up):
        """(outputs_old, features_old); replayed from a captured graph when enabled and the input shape is stable."""
        if self._teacher_w16 is not None:
            self._teacher_w16.refresh_if_stale()
        if not self.graph_teacher or self.lde_lazy or torch.cuda.is_current_stream_capturing():
            return self._teacher_eager(images, up)          # (inside a whole-step capture the teacher is part of that graph)
        tg = self._tg
        if tg is not None and tg["shape"] == tuple(images.shape) and tg["up"] == bool(up):
            tg["images"].copy_(images)
            tg["graph"].replay()
            return tg["out"]
        self._tg_seen += 1
        if self._tg_seen <= 2:                      # eager warm-up: MIOpen solver search, workspaces, constants
            return self._teacher_eager(images, up)
        if self.step_graph and self._sg is None and self._sg_seen <= self.step_graph_warmup + 1:
            return self._teacher_eager(images, up)  # the whole-step capture is about to include the teacher: no graph of its own
        try:
            from .segmentation_module import Features
            static = images.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # thread_local: RCCL / watchdog threads of a multi-GPU run keep making HIP calls while this thread captures
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                outputs_old, f = self._teacher_eager(static, up)
                # materialise exactly what the step reads; the lazy attention maps are not part of the graph
                # (the stage taps of a Local POD run ride in the tuple: the capture pool must not hand their memory out again)
                out = (outputs_old, Features(f.raw("body"), f.raw("pre_logits"), f["sem"], f.stages))
            self._tg = {"graph": graph, "images": static, "out": out, "shape": tuple(images.shape), "up": bool(up)}
            graph.replay()
            return out
        except Exception as e:                      # capture is an optimisation: never lose the step over it
            self.graph_teacher = False
            self._tg = None
            self.teacher_graph_error = repr(e)[:200]            # bench.py prints it: a run without the graph is marked
            torch.cuda.synchronize()
            import warnings
            warnings.warn(f"teacher graph capture disabled: {e!r}")
            return self._teacher_eager(images, up)

    # -- the whole iteration as one graph --------------------------------------------------------------------------------
    def _graph_ready(self, optim):
        """Static preconditions of a capture: the gradient-bucket wrapper (gradients live at fixed addresses) and the
        one-launch optimiser with its tables in place (its hyper-parameters can then live on the device)."""
        from .optim import SGD
        return (hasattr(self.model, "finish_grad_sync") and hasattr(self.model, "zero_grad") and isinstance(optim, SGD)
                and optim.plan_is_current() and self._reg_plan_is_current())

    def _reg_plan_is_current(self):
        return not self.regularizer_flag or self.regularizer.plan_is_current()

    def _graph_step(self, images, labels, optim, scheduler):
        """Replay (or capture, then replay) the iteration; None when this call has to run eagerly."""
        key = (tuple(images.shape), tuple(labels.shape), images.dtype, labels.dtype, id(optim), self.model.training)
        sg = self._sg
        if sg is not None and sg["key"] == key and not (optim.plan_is_current() and self._reg_plan_is_current()):
            # parameters / gradients / momentum buffers moved (load_state_dict, add_param_group, a re-wrapped model): the captured
            # optimiser launch holds the old addresses - drop the graph, run eagerly, capture again after the warm-up count
            self._sg, self._sg_seen, sg = None, 0, None
            optim.device_hyper(False)
        if sg is not None and sg["key"] == key:
            sg["images"].copy_(images, non_blocking=True)
            sg["labels"].copy_(labels, non_blocking=True)
            optim.push_hyper()
            sg["graph"].replay()
            bw = getattr(self.model, "bf16_weights", None)
            if bw is not None:
                # the replayed optimiser step staled the flipped / transposed weights for any EAGER iteration that follows (another
                # batch shape, a dropped graph): the optimiser's post-hook, which sets this flag, does not run in a replay
                bw._flips_dirty = True
            if scheduler is not None:
                scheduler.step()
            self.graph_steps += 1
            self.last = sg["out"]
            return self.last
        if sg is not None:                          # another batch shape (last batch of an epoch, validation crop): eager
            return None
        self._sg_seen += 1
        if self._sg_seen <= self.step_graph_warmup or not self._graph_ready(optim):
            return None
        dev = self.device
        try:
            static_images = images.to(dev, dtype=torch.float32).contiguous(memory_format=torch.channels_last).clone(
                memory_format=torch.preserve_format)
            static_labels = labels.to(dev, dtype=torch.long).clone()
            optim.device_hyper(True)
            bw = getattr(self.model, "bf16_weights", None)
            if bw is not None:
                bw._flips_dirty = True              # the replayed iteration refreshes the flipped weights its optimiser step staled
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                out = self._eager_step(static_images, static_labels, optim, None)
            self._sg = {"graph": graph, "images": static_images, "labels": static_labels, "out": out, "key": key}
            self._tg = None                         # the separate teacher graph (and its memory pool) is not needed any more
        except Exception as e:                      # capture is an optimisation: never lose the step over it
            self.step_graph = False
            self._sg = None
            self.step_graph_error = repr(e)[:300]
            optim.device_hyper(False)
            torch.cuda.synchronize()
            import warnings
            warnings.warn(f"whole-step graph capture disabled: {e!r}")
            if hasattr(self.model, "zero_grad"):
                self.model.zero_grad()
            return None
        return self._graph_step(images, labels, optim, scheduler)        # nothing ran during the capture: replay it now

    def train_step(self, images, labels, optim, scheduler=None):
        """One iteration; returns device scalars (no host synchronisation)."""
        if self.step_graph and self.model_old is not None and self.model.training:
            out = self._graph_step(images, labels, optim, scheduler)
            if out is not None:
                return out
        return self._eager_step(images, labels, optim, scheduler)

    def _eager_step(self, images, labels, optim, scheduler=None):
        model, model_old = self.model, self.model_old
        images = images.to(self.device, dtype=torch.float32, non_blocking=True)
        labels = labels.to(self.device, dtype=torch.long, non_blocking=True)
        if self.device.type == "cuda":
            images = images.contiguous(memory_format=torch.channels_last)
        zero = torch.zeros((), device=self.device)
        lkd = lde = zero
        fuse = self.fuse_logit_losses
        up = {} if not fuse else {"upsample": False}
        if self.pod_flag:
            up["taps"] = True               # both networks hand out their stage maps (the teacher's on its side stream: joined below)
        if model_old is not None:
            if self._side is not None:
                main = torch.cuda.current_stream(self.device)
                self._side.wait_stream(main)                      # the batch is ready; last step's readers are done
                with torch.cuda.stream(self._side):
                    outputs_old, features_old = self._teacher_forward(images, up)
            else:
                outputs_old, features_old = self._teacher_forward(images, up)
        if hasattr(model, "zero_grad") and hasattr(model, "finish_grad_sync"):
            model.zero_grad()
        else:
            optim.zero_grad(set_to_none=True)
        with self._autocast():
            if model_old is None:
                outputs, features = model(images, ret_intermediate=self.ret_intermediate, **up)
            else:
                outputs, features = model(images, x_b_old=_raw(features_old, "body"),
                                          x_pl_old=_raw(features_old, "pre_logits"),
                                          ret_intermediate=self.ret_intermediate, **up)
        if model_old is not None and self._side is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._side)     # teacher outputs are needed from here on
        soft = None
        labels_ce, factor = labels, None
        if self.pseudo_flag:
            if self.pseudo_thresholds is None:
                raise RuntimeError("--pseudo: no thresholds yet - call Trainer.find_pseudo_thresholds(train_loader) before the first "
                                   "step (run.py does, unless the loaded trainer state carries them)")
            labels_ce, factor, pseudo_counts = fused_pseudo_labels(features_old["sem"], labels, self.pseudo_thresholds,
                                                                   self.pseudo_f_min)
            if not self.pseudo_adaptive:
                factor = None
        if self.bce:
            # train.py:112/116 with the BCE criterion, and :119-124: up-sampling + per-class BCE (+ the combined iCaRL term against
            # sigmoid(up(teacher))) + the gradient w.r.t. the low-res logits in one kernel; --unce is ignored (train.py:35-38)
            total, ce, soft = fused_seg_bce(features["sem"], features_old["sem"] if self.icarl_combined else None, labels, 1.0,
                                            self.icarl if self.icarl_combined else 0.0)
            if self.lkd_flag:
                # --loss_kd next to BCE: the KD term of the softmax kernel, its CE discarded; the two gradients add in autograd
                kd_total, _, kd = fused_seg_losses(features["sem"], features_old["sem"], labels, 1, 0.0, self.lkd,
                                                   kd=self.kd_mode, alpha=self.alpha)
                total = total + kd_total
        elif fuse:
            # one pass over the label map: bilinear up-sampling + CE (+ KD) + gradient w.r.t. the low-res logits
            total, ce, kd = fused_seg_losses(features["sem"], features_old["sem"] if self.lkd_flag else None, labels_ce,
                                             self.old_classes if self.unce else 1, 1.0,
                                             self.lkd if self.lkd_flag else 0.0,
                                             kd=self.kd_mode if self.lkd_flag else "unbiased",
                                             alpha=self.alpha if self.lkd_flag else 1.0, sample_weight=factor, focal=self.focal)
        else:
            ce = self.criterion(outputs.float() if outputs.dtype != torch.float32 else outputs, labels_ce)
            if self.focal is not None:
                ce = focal_modulate(ce, *self.focal)
            if factor is not None:
                ce = ce * factor.view(-1, 1, 1)
            ce = ce.mean()
        con = zero
        if model_old is not None and self.pixcon_weight != 0:
            con = ucd_contrastive_loss(_raw(features, "pre_logits"), labels, features_old["sem"],
                                       _raw(features_old, "pre_logits"), self.temperature, self.max_label,
                                       self.pixcon_precision)
        loss = ce + con * self.pixcon_weight                                      # train.py:116 (/100)
        if self.lde_flag:
            if self.fused_lde:
                lde = (fused_attn_mse(_raw(features, "body"), _raw(features_old, "body"), self.lde)
                       + fused_attn_mse(_raw(features, "pre_logits"), _raw(features_old, "pre_logits"), self.lde))
            else:
                lde = self.lde * (self.lde_loss(features["body"].float(), features_old["body"].float())
                                  + self.lde_loss(features["pre_logits"].float(), features_old["pre_logits"].float()))
        if self.lkd_flag:
            lkd = self.lkd * (kd if fuse else self.lkd_loss(outputs, outputs_old))   # train.py:131-133
        loss_tot = (total + con * self.pixcon_weight + lde) if fuse else (loss + lkd + lde)
        if self.pod_flag:
            lpod = self._local_pod(features, features_old)
            loss_tot = loss_tot + lpod
        if self.proto_flag:
            # the class of every low-resolution pixel (a background pixel takes the teacher's arg-max), then the three terms
            x_pl = _raw(features, "pre_logits")
            if self.proto_sum is None:
                self._alloc_proto(x_pl.shape[1])
            sem_t = features_old["sem"] if model_old is not None else None
            proto_cls = proto_classes(labels, sem_t, self.tot_classes, sem_t.shape[1] if sem_t is not None else 0, x_pl.shape[-2:])
            lproto, proto_parts = fused_proto_losses(x_pl, proto_cls, (self.proto_sum, self.proto_n), self.proto_old, self.proto_w)
            loss_tot = loss_tot + lproto
        loss_tot.backward()
        if self.proto_flag:
            proto_update((self.proto_sum, self.proto_n), proto_parts)        # the step used the state as it stood before this batch
        if hasattr(model, "finish_grad_sync"):
            model.finish_grad_sync()
        if self.regularizer_flag:
            # train.py:139-145: update the importance from the reduced data gradient, add reg_importance * penalty's gradient
            l_reg = self.regularizer.step()
        optim.step()
        if scheduler is not None:
            scheduler.step()
        self.last = {"loss": loss.detach(), "lkd": lkd.detach(), "lde": lde.detach(), "ce": ce.detach(),
                     "con": con.detach()}
        if self.regularizer_flag:
            self.last["reg"] = l_reg.detach()
        if self.pod_flag:
            self.last["LPOD"] = lpod.detach()
        if self.proto_flag:
            self.last["PROTO"] = lproto.detach()
        if self.pseudo_flag:
            kept = pseudo_counts.sum(dim=0).float()
            self.last["pseudo_kept"] = kept[0] / kept[1].clamp_min(1.0)      # share of the candidates that took a pseudo-label
        if self.icarl_combined:
            self.last["icarl"] = (self.icarl * soft).detach()       # l_icarl of train.py:123; its gradient is part of `total`
        return self.last

    def _local_pod(self, features, features_old):
        """L_pod = gamma / L * sum_l f_l * level_l over the L = 5 levels: the four stage maps (factor pod_factor, the slope of the
        block activation) and the raw pre-logits (pod_last_factor, slope 1).  The weight of a level goes into its call, so the sum
        needs no further launches of that size; a level with factor 0 is skipped.  Under --pod_logits L = 6: the pre-logits become
        an ordinary level (pod_factor) and the logits, the student's new-class channels summed into the background, are the last
        one (pod_last_factor, normalised unless --pod_logits_norm 0); its gradient adds into features["sem"] next to the loss
        kernel's, in autograd."""
        levels = [(s, t, self.pod_slope, self.pod) for s, t in zip(features.stages, features_old.stages)]
        levels.append((_raw(features, "pre_logits"), _raw(features_old, "pre_logits"), 1.0, self.pod if self.pod_logits else self.pod_last))
        L = len(levels) + int(self.pod_logits)
        lpod = None
        for x_s, x_t, slope, factor in levels:
            if factor == 0.:
                continue
            term = fused_local_pod(x_s, x_t, slope, self.pod_scales, self.pod_gamma * factor / L)
            lpod = term if lpod is None else lpod + term
        if self.pod_logits and self.pod_last != 0.:
            term = fused_local_pod_logits(features["sem"], features_old["sem"], self.pod_scales, self.pod_gamma * self.pod_last / L,
                                          self.pod_logits_norm)
            lpod = term if lpod is None else lpod + term
        return lpod

    def train(self, cur_epoch, optim, train_loader, scheduler=None, print_int=10, logger=None):
        """Train one epoch and return (epoch_loss, reg_loss) like the reference (train.py:76-183)."""
        if logger is not None:
            logger.info("Epoch %d, lr = %f" % (cur_epoch, optim.param_groups[0]["lr"]))
        dev = self.device
        epoch_loss = torch.zeros((), device=dev)
        reg_loss = torch.zeros((), device=dev)
        interval = torch.zeros((), device=dev)
        if hasattr(train_loader, "sampler") and hasattr(train_loader.sampler, "set_epoch"):
            train_loader.sampler.set_epoch(cur_epoch)
        self.model.train()
        n = 0
        multi_rank = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        proto_start = ((self.proto_sum.clone(), self.proto_n.clone()) if self.proto_flag and multi_rank and self.proto_sum is not None
                       else None)
        for cur_step, (images, labels) in enumerate(train_loader):
            r = self.train_step(images, labels, optim, scheduler)
            epoch_loss += r["loss"]
            reg_loss += r["lkd"] + r["lde"]
            interval += r["loss"] + r["lkd"] + r["lde"]
            if "reg" in r:                                      # train.py:154-157: l_reg counts as regularisation loss
                reg_loss += r["reg"]
                interval += r["reg"]
            if "icarl" in r:                                    # train.py:155-156: l_icarl counts as regularisation loss
                reg_loss += r["icarl"]
                interval += r["icarl"]
            if "LPOD" in r:                                     # the Local POD term counts as regularisation loss, next to lkd / lde
                reg_loss += r["LPOD"]
                interval += r["LPOD"]
            if "PROTO" in r:                                    # the class-prototype terms count as regularisation loss too
                reg_loss += r["PROTO"]
                interval += r["PROTO"]
            n += 1
            if (cur_step + 1) % print_int == 0:
                value = (interval / print_int).item()           # the only host sync of the interval
                self._check_mailbox()                           # a timed-out SyncBN mailbox exchange (its results are NaN) raises here
                if logger is not None:
                    logger.info(f"Epoch {cur_epoch}, Batch {cur_step + 1}/{len(train_loader)}, Loss={value}")
                    if "pseudo_kept" in r and getattr(logger, "debug_flag", False):
                        logger.debug(f"PSEUDO {r['pseudo_kept'].item()}")      # --debug only: the read synchronises
                    if "LPOD" in r and getattr(logger, "debug_flag", False):
                        # train.py:163, for runs with the Local POD term under --debug only (the reads synchronise); every other
                        # run logs what it always did
                        logger.debug(f"Loss made of: CE {r['loss'].item()}, LKD {r['lkd'].item()}, LDE {r['lde'].item()}, "
                                     f"LPOD {r['LPOD'].item()}")
                    if "PROTO" in r and getattr(logger, "debug_flag", False):
                        logger.debug(f"PROTO {r['PROTO'].item()}")             # --debug only: the read synchronises
                    logger.add_scalar("Loss", value, cur_epoch * len(train_loader) + cur_step + 1)
                interval.zero_()
        if proto_start is not None:
            self._merge_proto(*proto_start)
        if dist.is_available() and dist.is_initialized():
            if n:
                torch.cuda.synchronize() if dev.type == "cuda" else None
                self._check_mailbox()                           # before the epoch's reductions: a poisoned run must not report a loss
            dist.reduce(epoch_loss, dst=0)
            dist.reduce(reg_loss, dst=0)
            world = dist.get_world_size()
            rank = dist.get_rank()
        else:
            world, rank = 1, 0
        if rank == 0 and n:
            epoch_loss = epoch_loss / world / n
            reg_loss = reg_loss / world / n
        if logger is not None:
            logger.info(f"Epoch {cur_epoch}, Class Loss={epoch_loss}, Reg Loss={reg_loss}")
        return (epoch_loss, reg_loss)

    def _check_mailbox(self):
        """The one-shot SyncBN mailbox (csrc/comm.hip) latches a timed-out exchange in pinned host memory; a replayed step graph issues
        no host-side collective call that would report it, so the training loop polls the word at its host synchronisations and
        raises.  Costs one read of host memory; a no-op without a mailbox."""
        if self.device.type == "cuda" and dist.is_available() and dist.is_initialized():
            from .comm import check_mailbox
            check_mailbox(None)

    def _eval_terms(self, images, labels, sem, outputs, feats, up):
        """The reference's unscaled regularisation terms of one evaluation batch (train.py:207-240) as a device scalar: the KD value
        (``lkd_flag``), the encoder term on the body maps (``lde_flag``), the combined iCaRL term (``icarl_combined``) - the teacher
        runs eagerly, once, when any of the three is on - and the regulariser's penalty, which needs no teacher."""
        reg = torch.zeros((), device=self.device)
        if self.model_old is not None and (self.lde_flag or self.lkd_flag or self.icarl_combined):
            if self._teacher_w16 is not None:
                self._teacher_w16.refresh_if_stale()
            outputs_old, feats_old = self._teacher_eager(images, up)        # no graph replay: validation shapes differ
            if self.lkd_flag:
                if outputs is None:
                    reg = reg + fused_seg_losses(sem, feats_old["sem"], labels, 1 if self.bce else (self.old_classes if self.unce else 1),
                                                 0.0, 1.0, kd=self.kd_mode, alpha=self.alpha)[2]
                else:
                    reg = reg + self.lkd_loss(outputs.float(), outputs_old.float())
            if self.lde_flag:
                if self.fused_lde:
                    reg = reg + fused_attn_mse(_raw(feats, "body"), _raw(feats_old, "body"), 1.0)
                else:
                    reg = reg + self.lde_loss(feats["body"].float(), feats_old["body"].float())
            if self.icarl_combined:
                reg = reg + self.icarl * fused_seg_bce(sem, feats_old["sem"], labels)[2]
        if self.regularizer_flag:
            reg = reg + self.regularizer.penalty()
        return reg

    def _view_logits(self, images, views):
        """The low-resolution logits of the views after the plain one: the model once per ``(scale, flip)`` on the image resized
        bilinearly to ``int(size * scale + 0.5)`` and, for a mirror, flipped horizontally."""
        import torch.nn.functional as F
        H, W = images.shape[-2:]
        sems = []
        for scale, flip in views:
            x = images if scale == 1.0 else F.interpolate(images, size=(int(H * scale + 0.5), int(W * scale + 0.5)), mode="bilinear",
                                                          align_corners=False)
            if flip:
                x = x.flip(-1)
            with self._autocast():
                _, f = self.model(x, ret_intermediate=False, upsample=False)
            sems.append(f["sem"])
        return sems

    def _evaluate(self, loader, metrics, logger, on_batch, want_pred, views=None):
        """The loop ``validate`` and ``test`` share (train.py:185-270 and :271-375): class loss, regularisation terms and confusion
        matrix accumulated on the device, reduced to rank 0 and divided by ranks and batches.  ``want_pred(i)`` says whether batch
        ``i`` needs its int64 arg-max map; ``on_batch(i, images, labels, feats, prediction or None)`` sees every batch.

        ``views``: test-time views ``[(scale, flip), ...]`` with the plain view ``(1.0, False)`` first (``argparser.eval_views``).
        With more than the plain view the model also runs once per further view; the class loss and the teacher-side terms still
        come from the plain view, the confusion matrix and the prediction from the views fused by ``--fusion-mode`` in one kernel
        (``metrics.update_from_views``).  ``None`` or the plain view alone: the single-view path, unchanged."""
        views = [(float(s), bool(f)) for s, f in views] if views else [(1.0, False)]
        if views[0] != (1.0, False):
            raise ValueError(f"the first evaluation view must be the plain one (1.0, False), got {views[0]}")
        multi = len(views) > 1
        if multi and not (self.fuse_logit_losses and hasattr(metrics, "update_from_views")):
            raise RuntimeError("evaluation with scaled or mirrored views (--eval_scales / --eval_flip) needs the fused logit path: a "
                               "GPU device and a metrics object with update_from_views; there is no torch fall-back")
        metrics.reset()
        model = self.model
        dev = self.device
        class_loss = torch.zeros((), device=dev)
        reg_loss = torch.zeros((), device=dev)
        model.eval()
        n = 0
        with torch.no_grad():
            for i, (images, labels) in enumerate(loader):
                images = images.to(dev, dtype=torch.float32)
                labels = labels.to(dev, dtype=torch.long)
                pred = None
                if self.fuse_logit_losses and hasattr(metrics, "update_from_logits"):
                    # low-resolution logits only: loss and confusion matrix come from the fused kernels (the reference
                    # up-samples, copies predictions to the host and histograms there, train.py:236-246)
                    up, outputs = {"upsample": False}, None
                    with self._autocast():
                        _, feats = model(images, ret_intermediate=False, upsample=False)
                    sem = feats["sem"]
                    if self.bce:
                        class_loss += fused_seg_bce(sem, None, labels)[1]
                    else:
                        class_loss += fused_seg_losses(sem, None, labels, self.old_classes if self.unce else 1, 1.0, 0.0,
                                                       focal=self.focal)[1]
                    if multi:
                        # the fused prediction is what is scored, and what on_batch sees (the rendered files show it)
                        pred = torch.empty(labels.shape, dtype=torch.int64, device=dev) if want_pred(i) else None
                        metrics.update_from_views(labels, [sem] + self._view_logits(images, views[1:]), [f for _, f in views],
                                                  fusion=self.fusion_mode, pred=pred)
                    elif want_pred(i):
                        # the arg-max map the histogram is built from: no second pass over the logits
                        pred = torch.empty(labels.shape, dtype=torch.int64, device=dev)
                        metrics.update_from_logits(labels, sem, pred=pred)
                    else:
                        metrics.update_from_logits(labels, sem)
                else:
                    up = {}
                    with self._autocast():
                        outputs, feats = model(images, ret_intermediate=False)
                    sem = feats["sem"]
                    if self.bce:
                        # metrics without update_from_logits: the up-sampled logits only feed the arg-max, the loss stays on the kernel
                        class_loss += fused_seg_bce(sem, None, labels)[1]
                    else:
                        ce_map = self.criterion(outputs.float(), labels.clone())
                        class_loss += (ce_map if self.focal is None else focal_modulate(ce_map, *self.focal)).mean()
                    pred = outputs.argmax(dim=1)
                    metrics.update(labels, pred)
                    if self.bce:
                        outputs = None                      # the teacher-side terms of a BCE run come from the fused kernels
                if self.model_old is not None or self.regularizer_flag:
                    reg_loss += self._eval_terms(images, labels, sem, outputs, feats, up)
                if on_batch is not None:
                    on_batch(i, images, labels, feats, pred)
                n += 1
            metrics.synch(dev)
            score = metrics.get_results()
        if dist.is_available() and dist.is_initialized():
            dist.reduce(class_loss, dst=0)
            dist.reduce(reg_loss, dst=0)
            world = dist.get_world_size()
        else:
            world = 1
        class_loss = class_loss / world / max(n, 1)
        reg_loss = reg_loss / world / max(n, 1)
        if logger is not None:
            logger.info(f"Validation, Class Loss={class_loss}, Reg Loss={reg_loss} (without scaling)")
        return (class_loss, reg_loss), score

    def validate(self, loader, metrics, ret_samples_ids=None, logger=None, views=None):
        """Evaluation loop (train.py:185-270): ``((class_loss, reg_loss), score, samples)``, the losses as device scalars.

        The class loss and the confusion matrix come from the fused kernels on the low-resolution logits (under BCE: the fused BCE).
        With a teacher and any of ``--loss_kd``, ``--loss_de`` or the combined iCaRL term, the teacher runs eagerly per batch and
        "Reg Loss" is the mean over batches of the reference's unscaled terms (train.py:228-240): the KD value, the encoder term on
        the body maps, ``icarl_importance`` times the combined iCaRL term; with a regulariser (EWC / PI / RW) its penalty is added,
        which needs no teacher.  Without a teacher and a regulariser it is exactly 0.

        ``ret_samples_ids``: batch indices for which ``(images[0] as float32 numpy [3, H, W], labels[0], prediction[0])`` (numpy
        int64 [H, W] each) is appended to ``samples``; the prediction is the arg-max map the confusion matrix was built from.
        With ``None`` nothing extra is computed or copied.  ``views``: test-time views as in ``_evaluate``; only when passed - the
        validations between epochs stay single-view."""
        ids = None if ret_samples_ids is None else {int(v) for v in ret_samples_ids}
        samples = []

        def on_batch(i, images, labels, feats, pred):
            if i in ids:
                samples.append((images[0].detach().float().cpu().numpy(), labels[0].cpu().numpy(), pred[0].cpu().numpy()))

        losses, score = self._evaluate(loader, metrics, logger, on_batch if ids else None,
                                       (lambda i: i in ids) if ids else (lambda i: False), views=views)
        return losses, score, samples

    def test(self, loader, metrics, logger=None, sink=None):
        """The reference's ``Trainer.test`` (train.py:271-375): losses and metrics as in ``validate``, over every image.

        Without ``sink`` the samples are the reference's 4-tuples ``(image float32 [3, H, W], label, prediction, att)`` as numpy
        arrays, one per image; ``att`` is the attention map of train.py:339-343 (``ucd_amd.visual.attn_energy`` of the raw body map,
        up-sampled bilinearly to the image) - the whole test set then sits on the host, as in the reference.  With ``sink`` each
        batch is rendered on the device (``ucd_amd.visual.render``: prediction, colour-coded prediction and labels, de-normalised
        image, attention map) and ``sink(batch_index, rendered)`` receives the dict of device tensors, ``uint8`` but for ``att``; the
        sample list stays empty.  The rendered ``pred_u8`` has the bits of the map the confusion matrix is built from.

        The views are those of ``--eval_scales`` / ``--eval_flip`` (``argparser.eval_views``), fused by ``--fusion-mode``; with more
        than the plain view the prediction - in the samples and in the rendered ``pred_u8`` / ``pred_rgb`` - is the fused one."""
        from . import visual
        samples = []
        views = self.eval_views
        multi = len(views) > 1

        def on_batch(i, images, labels, feats, pred):
            body = _raw(feats, "body")
            if sink is not None:
                sink(i, visual.render(feats["sem"], labels, images, body, pred=pred if multi else None))
                return
            import torch.nn.functional as F
            att = F.interpolate(visual.attn_energy(body).unsqueeze(1), size=images.shape[-2:], mode="bilinear",
                                align_corners=False).squeeze(1)
            img, lab, prd, att = images.detach().float().cpu().numpy(), labels.cpu().numpy(), pred.cpu().numpy(), att.cpu().numpy()
            samples.extend((img[j], lab[j], prd[j], att[j]) for j in range(img.shape[0]))

        losses, score = self._evaluate(loader, metrics, logger, on_batch, lambda i: multi or sink is None, views=views)
        return losses, score, samples

    @torch.no_grad()
    def find_pseudo_thresholds(self, loader, logger=None):
        """One pass of the frozen teacher (eval mode) over ``loader``: the per-class histogram of the normalised entropy at the
        candidate pixels (ucd_amd.loss.pseudo_hist; summed over the ranks with one int64 all-reduce), then the interpolated median
        of every class, floored at ``--pseudo_threshold`` (ucd_amd.loss.pseudo_median: K x bins numbers on the host, in float64).
        Stores ``pseudo_hist`` and ``pseudo_thresholds`` (device tensors; both travel in ``state_dict``) and returns the
        thresholds as a numpy array."""
        if not self.pseudo_flag:
            raise RuntimeError("find_pseudo_thresholds needs --pseudo entropy and a teacher")
        hist = None
        self.model_old.eval()
        if self._teacher_w16 is not None:
            self._teacher_w16.refresh_if_stale()
        for images, labels in loader:
            images = images.to(self.device, dtype=torch.float32)
            labels = labels.to(self.device, dtype=torch.long)
            if self.device.type == "cuda":
                images = images.contiguous(memory_format=torch.channels_last)
            _, feats = self._teacher_eager(images, {"upsample": False} if self.fuse_logit_losses else {})
            sem = feats["sem"]
            if hist is None:
                hist = torch.zeros(sem.shape[1], self.pseudo_bins, dtype=torch.int64, device=self.device)
            pseudo_hist(sem, labels, hist)
        if hist is None:
            raise RuntimeError("find_pseudo_thresholds: the loader is empty")
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(hist)
        thresholds = pseudo_median(hist, self.pseudo_floor)
        self._set_pseudo(torch.from_numpy(thresholds), hist)
        if logger is not None:
            logger.info(f"Pseudo-label thresholds of the {len(thresholds)} old classes: " + " ".join(f"{t:.4f}" for t in thresholds))
        return thresholds

    def _load_pseudo(self, state):
        # (a state of another class split - the previous step's - is not this teacher's)
        if state is not None and self.pseudo_flag and (not self.old_classes or state["thresholds"].numel() == self.old_classes):
            self._set_pseudo(state["thresholds"], state["hist"])

    def _set_pseudo(self, thresholds, hist):
        """New values go INTO the thresholds tensor where one exists: a captured whole-step graph reads it by address."""
        thresholds = thresholds.to(self.device, dtype=torch.float32)
        if self.pseudo_thresholds is not None and self.pseudo_thresholds.shape == thresholds.shape:
            self.pseudo_thresholds.copy_(thresholds)
        else:
            if self._sg is not None:
                raise RuntimeError("the pseudo-label thresholds changed their class count under a captured step graph")
            self.pseudo_thresholds = thresholds.clone()
        self.pseudo_hist = hist.to(self.device)

    # -- SDR's class prototypes -------------------------------------------------------------------------------------------
    def _alloc_proto(self, channels):
        self.proto_sum = torch.zeros(self.tot_classes, channels, dtype=torch.float64, device=self.device)
        self.proto_n = torch.zeros(self.tot_classes, dtype=torch.int64, device=self.device)

    def _set_proto_old(self, O, valid):
        """New values go INTO the tensors where they exist (``_set_pseudo``'s rule): a captured step graph reads them by address."""
        O = O.to(self.device, dtype=torch.float32)
        valid = valid.to(self.device, dtype=torch.bool)
        if self.proto_old is not None and self.proto_old[0].shape == O.shape:
            self.proto_old[0].copy_(O)
            self.proto_old[1].copy_(valid)
        else:
            if getattr(self, "_sg", None) is not None:
                raise RuntimeError("the old prototypes changed their shape under a captured step graph")
            self.proto_old = (O.clone(), valid.clone())

    def _old_from_state(self, prev):
        """O and valid from rows 0 .. K-1 of a previous step's running prototypes (``state_dict()["proto"]``); a state of another
        feature width, or of fewer classes than the teacher has, is not used."""
        K = self.old_classes
        s, n = prev["sum"], prev["n"]
        if K < 1 or s.dim() != 2 or s.shape[0] < K or (self.proto_sum is not None and s.shape[1] != self.proto_sum.shape[1]):
            return False
        s, n = s[:K].double(), n[:K].long()
        valid = n > 0
        O = torch.where(valid.unsqueeze(1), s / n.clamp_min(1).unsqueeze(1).double(), torch.zeros_like(s))
        self._set_proto_old(O, valid)
        return True

    def _merge_proto(self, start_sum, start_n):
        """Every rank accumulated its own increments since ``start``: one all-reduce of the increments (sum and N), outside the step
        graph, leaves the same state on every rank."""
        inc_sum, inc_n = self.proto_sum - start_sum, self.proto_n - start_n
        dist.all_reduce(inc_sum)
        dist.all_reduce(inc_n)
        self.proto_sum.copy_(start_sum + inc_sum)
        self.proto_n.copy_(start_n + inc_n)

    @torch.no_grad()
    def find_prototypes(self, loader, logger=None):
        """One pass of the frozen teacher (eval mode) over ``loader``: the per-class sums of ITS raw pre-logits over the classes of
        its low-resolution pixels (a background pixel takes the teacher's arg-max, a new-class pixel none) - classify, the forward call
        with zero weights and the update, as in a step - summed over the ranks; leaves ``proto_old = (O, valid)`` and returns the
        number of valid classes.  Follows ``find_pseudo_thresholds``."""
        if not (self.proto_flag and self.proto_w[0] > 0. and self.model_old is not None):
            raise RuntimeError("find_prototypes needs --sdr_match and a teacher")
        K = self.old_classes
        state = None
        self.model_old.eval()
        if self._teacher_w16 is not None:
            self._teacher_w16.refresh_if_stale()
        for images, labels in loader:
            images = images.to(self.device, dtype=torch.float32)
            labels = labels.to(self.device, dtype=torch.long)
            if self.device.type == "cuda":
                images = images.contiguous(memory_format=torch.channels_last)
            _, feats = self._teacher_eager(images, {"upsample": False} if self.fuse_logit_losses else {})
            x_pl = _raw(feats, "pre_logits")
            if state is None:
                state = (torch.zeros(K, x_pl.shape[1], dtype=torch.float64, device=self.device),
                         torch.zeros(K, dtype=torch.int64, device=self.device))
            cls = proto_classes(labels, feats["sem"], K, K, x_pl.shape[-2:])
            _, parts = fused_proto_losses(x_pl, cls, state, None, (0., 0., 0.))
            proto_update(state, parts)
        if state is None:
            raise RuntimeError("find_prototypes: the loader is empty")
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(state[0])
            dist.all_reduce(state[1])
        self._old_from_state({"sum": state[0], "n": state[1]})
        count = int(self.proto_old[1].sum().item())
        if logger is not None:
            logger.info(f"Class prototypes of the old model: {count} of {K} classes are valid")
        return count

    def _load_proto(self, state):
        if state is None or not self.proto_flag:
            return
        if self.proto_sum is None:
            self._alloc_proto(state["sum"].shape[1])
        if state["sum"].shape == self.proto_sum.shape:          # (a state of another class split is not this step's)
            self.proto_sum.copy_(state["sum"])
            self.proto_n.copy_(state["n"])
            if state.get("old") is not None and self.proto_w[0] > 0.:
                self._set_proto_old(state["old"], state["old_valid"])

    def state_dict(self):
        state = {"regularizer": self.regularizer.state_dict() if self.regularizer_flag else None}
        if self.proto_flag and self.proto_sum is not None:
            state["proto"] = {"sum": self.proto_sum.cpu(), "n": self.proto_n.cpu(),
                              "old": None if self.proto_old is None else self.proto_old[0].cpu(),
                              "old_valid": None if self.proto_old is None else self.proto_old[1].cpu()}
        if self.pseudo_thresholds is not None:              # a resumed run does not repeat the pass over the training set
            state["pseudo"] = {"thresholds": self.pseudo_thresholds.cpu(), "hist": self.pseudo_hist.cpu()}
        return state

    def load_state_dict(self, state):
        if state["regularizer"] is not None and self.regularizer is not None:
            self.regularizer.load_state_dict(state["regularizer"])
        self._load_pseudo(state.get("pseudo"))
        self._load_proto(state.get("proto"))
