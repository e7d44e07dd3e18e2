"""The ``UCD_*`` A/B switches of the product path, resolved ONCE per process.

Every switch is an environment variable read at its first use and cached in a plain dict (the layer code asks ~600 times per
step; ``os.environ.get`` encodes the key on every call).  Tests and probes that flip a switch inside one process go through
``set`` / ``unset`` (which also keep ``os.environ`` in step for child processes) or call ``reload`` after changing the
environment themselves.  ``snapshot`` is what bench.py prints as ``own_kernels``: a run that lost a kernel family to a switch
(or to a fallback) is visible in its JSON line.
"""
from __future__ import annotations

import os

# name -> default; "1" = the own kernel / fusion is on
DEFAULTS = {
    "UCD_FUSED_CONV1X1": "1",      # conv + training-ABN nodes on csrc/conv1x1.hip (0: module path, library kernels)
    "UCD_BWD_LINK": "1",           # backward links inside a bottleneck (out_mode 3)
    "UCD_BLOCK_LINK": "1",         # block links across a block boundary (out_mode 4)
    "UCD_PROJ_ALIAS": "1",         # projection blocks: proj_conv reads the alias returned by conv1's node
    "UCD_DGRAD_VIA_FWD": "1",      # stride-1 input gradients on forward solvers / the own kernel
    "UCD_OWN_STRIDED": "1",        # strided conv2 / proj_conv on the own kernels
    "UCD_OWN_WGRAD": "1",          # weight gradients on csrc/wgrad.hip
    "UCD_F32_OWN_CONV": "0",       # fp32 (O0) stride-1 1x1 / 3x3 layers on csrc/conv_f32.hip: split-bf16 MFMA, ~1e-5 per product (0: MIOpen)
    "UCD_OWN_HEADS": "1",          # classifier heads (Ct <= 64) on the own GEMM kernels through a zero-padded 64-row weight (0: library)
    "UCD_OWN_STEM": "1",           # 7x7/2 stem forward on csrc/stem.hip
    "UCD_WGRAD3": "1",             # 3x3 weight gradients: one kernel row per workgroup (0: the 9-tap form; read by the library)
    "UCD_CONV_PIPE": "auto",       # pipeline of the GEMM kernel: auto | 2x64 | lw64 | lw256, anything else is refused (read by the library)
    "UCD_CONV_BN64_TILES": "128",  # launches of at most this many 128 x 128 tiles run on 128 x 64 tiles (0: never; read by the library)
    "UCD_CONV_LW64_TILES": "128",  # round 6: launches of at most this many 128 x 64 tiles run on 64-row loader-wave tiles - twice the CUs at 3 images per GPU (0: never; read by the library)
    "UCD_WGRAD_DEFER": "1",        # round 6: the slab sum of a weight gradient rides in the NEXT weight-gradient launch (0: a launch of its own behind every product)
    "UCD_WGRAD_STREAM": "1",       # round 6: the nodes' weight gradients run on a side stream of the library between the wrapper's flushes - off the chain of input-gradient products (0: on the compute stream); each one is launched one call behind its fork point, on a lowest-priority stream
    "UCD_CONV3_TAP_CLASSES": "1",  # stand-alone dilated 3x3 products (ASPP, forward and input gradient): rows ordered by tap class, every row tile walks only its live taps - same outputs bit for bit (0: raster order; 2: also the single-wave 64-row launches whose heaviest tile keeps its taps, which 1 leaves in raster order; read by the library, hip.conv3_tap_classes sets it inside a process)
    "UCD_STAT_ATOMIC": "1",        # conv + ABN nodes: statistics / link sums by fp32 atomics into arena slots, finalised by the apply passes (0: per-tile rows + reduction launches, bit-reproducible)
    "UCD_SEG_PK": "1",             # fused logit losses: packed math, fp64 LDS accumulators (0: the round-3 register form; read by the library)
    "UCD_SEG_KD_EX": "1",          # fused logit losses for every pair of {plain, unbiased} CE x {none, plain, unbiased} KD and any --alpha (ucd_seg_losses_ex); 0: only (any CE) or (unbiased CE + unbiased KD at alpha 1) fused, the rest on the torch modules
    "UCD_FUSED_LDE": "1",          # ILT's encoder term (--loss_de) as one HIP operation on the raw maps (ucd_attn_mse), ILT inside the teacher / whole-step graphs; 0: attention maps + MSELoss in torch, ILT eager
    "UCD_FUSED_POD": "1",          # Local POD feature distillation (--pod_factor) on csrc/pod.hip: one trip over each tapped map forward, one read + one write backward; with --pod_logits also the level on the logits (0: the torch compositions local_pod_torch / local_pod_logits_torch)
    "UCD_FUSED_PSEUDO": "1",       # PLOP's pseudo-labelling (--pseudo entropy) on csrc/pseudo_label.hip: labels, per-image factor and the threshold histogram from the low-resolution teacher rows, one launch each (0: the torch composition pseudo_labels_torch / pseudo_hist_torch on the up-sampled [B, K, H, W] logits)
    "UCD_FUSED_FOCAL": "1",        # focal cross entropy (--focal_loss) inside the fused logit-loss kernels (ucd_seg_losses_focal / ucd_seg_losses_gather_focal): the modulation is a few scalar operations on the pixel's log-probability (0: the torch composition focal_modulate on the cross-entropy map of the up-sampled [B, Ctot, H, W] logits)
    "UCD_FUSED_PROTO": "1",        # SDR's class-prototype feature losses (--sdr_match / --sdr_attract / --sdr_repel) on csrc/proto.hip: one launch for the classes of the low-resolution pixels, three forward (one pass over the pre-logits), one backward, one for the running prototypes (0: the torch compositions proto_classes_torch / proto_losses_torch)
    "UCD_VAL_DEVICE": "1",        # validation transforms (Resize + CenterCrop, full size) as ucd_val_image_path / ucd_val_label_path on raw samples (0: Pillow on the host per sample + the train path with the identity box; torch launches for the full image)
    "UCD_STEM_EVAL_FUSED": "1",    # frozen-statistics stem (the teacher): conv1 + norm + activation + max pool as one kernel (0: two kernels)
    "UCD_STEM_FOLD": "1",          # stem norm + max-pool as one pass
    "UCD_ABN_NODE": "1",           # C++ autograd nodes
    "UCD_SGD": "hip",              # one-launch optimiser step (torch: torch's fused SGD)
    "UCD_STEP_GRAPH": "auto",      # whole-step hipGraph: auto = world 1 only, 1 = always try, 0 = never
    "UCD_TEACHER_OVERLAP": "1",    # frozen teacher on a side stream beside the student's forward (0: in front of it, same stream)
    "UCD_DIRECT_RCCL": "1",        # library-owned RCCL communicator for SyncBN
    "UCD_IPC_SYNC": "auto",        # SyncBN exchanges (<= 128 KB) as a one-shot IPC mailbox kernel: auto = only on an explicit attach_mailbox() (bench.py's third phase; every rank owns its GPU, self-test passed on all of them) - a plain run.py job stays on RCCL; 1 = always (also ranks sharing a GPU: tests); 0 = RCCL
    "UCD_IPC_TIMEOUT_MS": "60000", # give-up time of a mailbox exchange (a dead peer: the next collective raises instead of hanging; rank skew of a first iteration must fit)
    "UCD_DDP_LATE_COPY": "1",      # world 1: the bf16 -> fp32 gradient copies of all buckets as ONE launch at the end of the backward
    "UCD_DDP_DIRECT": "auto",      # gradient buckets over a library-owned RCCL communicator: auto = one-rank groups and captured multi-rank steps, 1 / 0 force
    "UCD_FORCE_COLLECTIVES": "0",  # 1 | abn | ddp: a one-rank process group still issues every SyncBN / gradient collective (bench.py --force_dist)
}

_cache: dict = {}


def get(name: str, default: str | None = None) -> str:
    v = _cache.get(name)
    if v is None:
        if default is None:
            default = DEFAULTS.get(name, "")
        v = _cache[name] = os.environ.get(name, default)
    return v


def set(name: str, value) -> None:       # noqa: A001 - mirrors os.environ's vocabulary
    os.environ[name] = str(value)
    _cache[name] = str(value)


def unset(name: str) -> None:
    os.environ.pop(name, None)
    _cache.pop(name, None)


def reload() -> None:
    """Forget the cached values (after ``os.environ`` / ``monkeypatch.setenv`` changed a switch)."""
    _cache.clear()


def snapshot() -> dict:
    return {k: get(k) for k in DEFAULTS}
