"""Evaluate a trained step: ``python evaluate.py --task 15-5 --step 1 --step_ckpt checkpoints/step/15-5-voc_Experiment_1.pth ...``
(the reference's ``test.py``; same options as ``run.py``).

Builds the student of ``--step``, restores ``--step_ckpt`` (``strict=False``, like the reference), scores it on the test split of
every class seen so far and writes one set of files per image under ``<logdir>/<task>-<dataset>/<name>/predictions/``: the prediction
map, the colour-coded prediction, the colour-coded ground truth and the de-normalised image (``ucd_amd.visual``: rendered on the
device, only ``uint8`` copied).  No teacher, no optimiser.  ``--data_root synthetic`` evaluates on the closed-form synthetic
batches, as in ``run.py``.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch
import torch.distributed as dist

from . import argparser, tasks, visual
from .ddp import DistributedDataParallel
from .logger import Logger
from .metrics import StreamSegMetrics
from .run import DATASETS, SyntheticSegmentation, get_dataset
from .segmentation_module import make_model
from .train import Trainer


def main(opts):
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", opts.MASTER_PORT)
    use_cuda = torch.cuda.is_available()
    local_rank = int(os.environ.get("LOCAL_RANK", opts.local_rank))
    own_group = not dist.is_initialized()
    if own_group:
        if "RANK" in os.environ or "WORLD_SIZE" in os.environ:
            dist.init_process_group(backend="nccl" if use_cuda else "gloo")
        else:
            os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
            dist.init_process_group(backend="nccl" if use_cuda else "gloo", rank=0, world_size=1)
    device = torch.device("cuda", local_rank) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    rank, world_size = dist.get_rank(), dist.get_world_size()
    task_name = f"{opts.task}-{opts.dataset}"
    logdir = f"{opts.logdir}/{task_name}/{opts.name}/"
    logger = Logger(logdir, rank=rank, debug=opts.debug, step=opts.step)
    torch.manual_seed(opts.random_seed); np.random.seed(opts.random_seed); random.seed(opts.random_seed)

    classes = tasks.get_per_task_classes(opts.dataset, opts.task, opts.step)
    labels, labels_old, path_base = tasks.get_task_labels(opts.dataset, opts.task, opts.step)
    seen = list(labels_old) + list(labels)
    _, _, val_loader_of, real = get_dataset(opts, device, world_size, rank, labels, labels_old,
                                             use_cache=False)     # one pass: nothing is read twice
    if real:
        # test.py:87-90: the test split with every class seen so far
        image_set = "train" if opts.val_on_trainset else "val"
        path_base += "-ov" if opts.overlap else ""
        test_dst = DATASETS[opts.dataset](opts.data_root, train=opts.val_on_trainset, labels=seen,
                                          idxs_path=path_base + f"/test_on_{image_set}-{opts.step}.npy")
    else:
        test_dst = SyntheticSegmentation(max(2 * opts.batch_size, 2), opts.crop_size, [l for l in seen if l != 0] or [1],
                                         seed=1000 + opts.step)
    test_loader = val_loader_of(test_dst)

    logger.info("*** Test the model on all seen classes...")
    model = make_model(opts, classes=classes).to(device)
    if use_cuda:
        model = model.to(memory_format=torch.channels_last)
    if opts.step_ckpt is None:
        raise ValueError("evaluate needs --step_ckpt: the checkpoint of the step to score")
    state = torch.load(opts.step_ckpt, map_location="cpu")["model_state"]
    model.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}, strict=False)
    logger.info(f"*** Model restored from {opts.step_ckpt}")
    # wrapped after the weights are in place: the wrapper's bf16 working copies (O1..O3) are made from them
    model = DistributedDataParallel(model, delay_allreduce=True,
                                    bf16_weights=getattr(opts, "opt_level", "O0") != "O0" and getattr(opts, "bf16_weights", True))
    trainer = Trainer(model, None, device=device, opts=opts, classes=classes)
    model.eval()
    metrics = StreamSegMetrics(sum(classes))
    out_dir = os.path.join(logdir, "predictions") if world_size == 1 else os.path.join(logdir, "predictions", f"rank{rank}")
    sink = visual.SampleWriter(out_dir)
    logger.info(f"*** Views (scale, mirrored): {argparser.eval_views(opts)}, fused by {opts.fusion_mode}")
    val_loss, val_score, _ = trainer.test(loader=test_loader, metrics=metrics, logger=logger, sink=sink)
    logger.info(f"*** End of Test, Total Loss={float(val_loss[0]) + float(val_loss[1])}, Class Loss={float(val_loss[0])},"
                f" Reg Loss={float(val_loss[1])}")
    if rank == 0:
        logger.info(metrics.to_str(val_score))
        logger.info(f"Validation, T_MeanIoU={val_score['Mean IoU']}, T_MeanAcc={val_score['Mean Acc']} (without scaling)")
        logger.info(f"{sink.count} images written to {out_dir}")
    if own_group:
        dist.destroy_process_group()
    return val_loss, val_score


def cli():
    main(argparser.modify_command_options(argparser.get_argparser().parse_args()))


if __name__ == "__main__":
    cli()
