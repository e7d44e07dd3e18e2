"""GPU: ucd_batch_path (csrc/batch_path.hip) - the train transform of a batch of HBM-resident samples in one launch - against
oracle/datapipe.py (the numpy restatement pinned to Pillow by tests/golden/datapipe.npz), bit for bit on both outputs; the
wrapper's refusals; and the cached DeviceLoader end to end against the plain one."""
import random
import zlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import datapipe as OD
from ucd_amd import hip
from ucd_amd.datacache import DeviceSampleCache, sample_bytes
from ucd_amd.datapipe import DeviceImagePath, DeviceLabelPath, target_lut
from ucd_amd.dataset import DeviceBatcher, DeviceLoader
from ucd_amd import tasks

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (H0, W0), (i, j, h, w), flip
SHAPES = [((97, 131), (3, 5, 20, 17), False),          # up-scaling
          ((240, 250), (0, 0, 240, 250), True),        # all four borders; ~7x down at S = 33: the row window spans several LDS chunks
          ((120, 90), (10, 7, 100, 1), False),         # one column
          ((64, 300), (60, 0, 1, 300), True),          # one row
          ((33, 33), (0, 0, 33, 33), False),           # identity at S = 33
          ((101, 203), (50, 100, 51, 103), True),      # box ending at the last row and column
          ((500, 375), (17, 29, 333, 290), False)]     # VOC-sized
SIZES = (33, 65)


def _image(rng, H0, W0):                               # the recipe of tests/test_datapipe.py::_image
    return (rng.randint(0, 256, size=(H0 // 4 + 1, W0 // 4 + 1, 3)).repeat(4, 0).repeat(4, 1)[:H0, :W0]
            + rng.randint(-9, 10, size=(H0, W0, 3))).clip(0, 255).astype(np.uint8)


def _label_map(rng, H0, W0):
    return rng.choice([0, 1, 15, 16, 20, 255], size=(H0 // 8 + 1, W0 // 8 + 1)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:H0, :W0]


def _voc_lut():
    labels, labels_old, _ = tasks.get_task_labels("voc", "15-5", 1)
    return target_lut(labels, labels_old)


@pytest.fixture(scope="module")
def batch():
    """The seven samples and, computed once, what the oracle makes of each at each size."""
    rng = np.random.RandomState(77)
    lut = _voc_lut()
    samples = [(_image(rng, H0, W0), _label_map(rng, H0, W0), box, flip) for (H0, W0), box, flip in SHAPES]
    want = {S: [(OD.image_path(img, box, S, flip), OD.label_path(lab, box, S, flip, lut.numpy())) for img, lab, box, flip in samples]
            for S in SIZES}
    return samples, lut, want


def _run(samples, S, lut, dev):
    images, labels = hip.batch_path([torch.from_numpy(s[0]).to(dev) for s in samples], [torch.from_numpy(s[1]).to(dev) for s in samples],
                                    [s[2] for s in samples], [s[3] for s in samples], S, lut, MEAN, STD)
    B = len(samples)
    assert images.shape == (B, 3, S, S) and images.dtype == torch.float32 and images.is_contiguous(memory_format=torch.channels_last)
    assert labels.shape == (B, S, S) and labels.dtype == torch.int64 and labels.is_contiguous()
    return images.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.parametrize("S", SIZES)
def test_batch_path_matches_the_oracle_bit_for_bit(batch, S):
    samples, lut, want = batch
    dev = torch.device("cuda:0")
    images, labels = _run(samples, S, lut, dev)
    for n, (wi, wl) in enumerate(want[S]):
        assert np.array_equal(images[n], wi), (S, n, SHAPES[n])
        assert np.array_equal(labels[n], wl), (S, n, SHAPES[n])
    for n in range(len(samples)):                              # B = 1: every sample alone
        images, labels = _run(samples[n:n + 1], S, lut, dev)
        assert np.array_equal(images[0], want[S][n][0]) and np.array_equal(labels[0], want[S][n][1]), (S, n, SHAPES[n])
    # the pair of calls it replaces, on the same tensors (not the reference: the oracle above is)
    imgs = [torch.from_numpy(s[0]).to(dev) for s in samples]
    labs = [torch.from_numpy(s[1]).to(dev) for s in samples]
    boxes, flips = [s[2] for s in samples], [s[3] for s in samples]
    got_i, got_l = hip.batch_path(imgs, labs, boxes, flips, S, lut, MEAN, STD)
    assert torch.equal(got_i, DeviceImagePath(S, MEAN, STD)(imgs, boxes, flips)) and torch.equal(got_l, DeviceLabelPath(S, lut)(labs, boxes, flips))


def test_batch_path_matches_the_pillow_goldens():
    """The ten image cases and the label cases of tests/golden/datapipe.npz (inputs replayed as tests/test_datapipe.py does) through
    the new call, against the CRCs Pillow + torch produced."""
    g = load_golden("datapipe.npz")
    dev = torch.device("cuda:0")
    lut = torch.from_numpy(g["lut::voc_15-5_s1"])
    by_size = {}
    rng = np.random.RandomState(4048)
    for k, (H0, W0, i, j, h, w, flip, S) in enumerate(g["icases"].tolist()):
        assert (int(rng.randint(100, 501)), int(rng.randint(100, 501))) == (H0, W0)
        img = _image(rng, H0, W0)
        rng.randint(30, H0 + 1); rng.randint(30, W0 + 1); rng.randint(0, H0 - h + 1); rng.randint(0, W0 - w + 1)
        by_size.setdefault(S, []).append((img, np.zeros((H0, W0), np.uint8), (i, j, h, w), bool(flip), "image", int(g[f"img{k}::crc"][0])))
    rng = np.random.RandomState(2024)
    for k, (H0, W0, i, j, h, w, flip, S) in enumerate(g["cases"].tolist()):
        assert (int(rng.randint(120, 501)), int(rng.randint(120, 501))) == (H0, W0)
        lbl = rng.choice([0, 3, 7, 15, 16, 18, 20, 255], size=(H0 // 8 + 1, W0 // 8 + 1)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:H0, :W0]
        rng.randint(40, H0 + 1); rng.randint(40, W0 + 1); rng.randint(0, H0 - h + 1); rng.randint(0, W0 - w + 1)
        by_size.setdefault(S, []).append((np.zeros((H0, W0, 3), np.uint8), lbl, (i, j, h, w), bool(flip), "label", int(g[f"case{k}::crc"][0])))
    assert sum(len(v) for v in by_size.values()) == len(g["icases"]) + len(g["cases"]) and len(g["icases"]) == 10
    for S, items in by_size.items():
        images, labels = _run(items, S, lut, dev)
        for n, item in enumerate(items):
            res = np.ascontiguousarray(images[n]) if item[4] == "image" else labels[n]
            assert zlib.crc32(res.tobytes()) == item[5], (S, n, item[4], item[2])


def test_wrapper_refuses_before_any_launch(monkeypatch):
    dev = torch.device("cuda:0")
    lut = torch.arange(256, dtype=torch.uint8)
    img, lab = torch.zeros(40, 50, 3, dtype=torch.uint8), torch.zeros(40, 50, dtype=torch.uint8)

    def no_launch():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(hip, "load", no_launch)
    for box in [(0, 0, 41, 50), (0, 1, 40, 50), (-1, 0, 10, 10), (0, 0, 0, 10), (39, 49, 2, 1)]:
        with pytest.raises(ValueError, match="crop box"):
            hip.batch_path([img.to(dev)], [lab.to(dev)], [box], [False], 33, lut, MEAN, STD)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.batch_path([img], [lab], [(0, 0, 40, 50)], [False], 33, lut, MEAN, STD)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.batch_path([img.to(dev)], [lab], [(0, 0, 40, 50)], [False], 33, lut, MEAN, STD)


def test_library_skips_a_bad_descriptor_and_refuses_bad_arguments(batch):
    """The C call itself: a sample whose descriptor fails the bounds check is skipped - its outputs keep what they held - while the
    others are computed; B <= 0, S <= 0 or a null pointer is UCD_EINVAL.  The bad boxes lie inside the allocations they name (the
    declared H0 / W0 are smaller than the tensors), so that only the check keeps the kernel from using them."""
    samples, lut, want = batch
    dev, S = torch.device("cuda:0"), 33
    img, lab, box, flip = samples[0]
    H0, W0 = lab.shape
    imgs = [torch.from_numpy(img).to(dev) for _ in range(4)]
    labs = [torch.from_numpy(lab).to(dev) for _ in range(4)]
    rows = [[H0, W0, *box, int(flip), 0],
            [H0 - 80, W0, 3, 5, 20, 17, 0, 0],                 # i + h > H0
            [H0, W0 - 120, 3, 5, 20, 17, 0, 0],                # j + w > W0
            [H0, W0, 3, 5, 0, 17, 0, 0]]                       # h = 0
    desc = torch.tensor(rows, dtype=torch.int32, device=dev)
    iptr = torch.tensor([t.data_ptr() for t in imgs], dtype=torch.int64, device=dev)
    lptr = torch.tensor([t.data_ptr() for t in labs], dtype=torch.int64, device=dev)
    out_i = torch.full((4, S, S, 3), -7.0, device=dev)
    out_l = torch.full((4, S, S), -7, dtype=torch.int64, device=dev)
    lut_d = lut.to(dev)
    lib = hip.load()

    def call(images=iptr, labels=lptr, d=desc, B=4, size=S, table=lut_d, oi=out_i, ol=out_l):
        return lib.ucd_batch_path(hip.ptr(images), hip.ptr(labels), hip.ptr(d), B, size, hip.ptr(table), *MEAN, *STD, hip.ptr(oi), hip.ptr(ol),
                                  hip.stream())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out_i[0].permute(2, 0, 1).cpu().numpy(), want[S][0][0]) and np.array_equal(out_l[0].cpu().numpy(), want[S][0][1])
    assert bool((out_i[1:] == -7.0).all()) and bool((out_l[1:] == -7).all())
    for kw in (dict(B=0), dict(B=-3), dict(size=0), dict(images=None), dict(labels=None), dict(d=None), dict(table=None), dict(oi=None),
               dict(ol=None)):
        rc = call(**kw)
        assert rc == -1, kw                                    # UCD_EINVAL, before any launch
        assert b"ucd_batch_path" in lib.ucd_last_error()
    torch.cuda.synchronize()


# ---- the loader end to end -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ade(tmp_path_factory):
    from dataset_trees import make_ade_tree
    from test_datacache_cpu import ade12
    root = str(tmp_path_factory.mktemp("ade12gpu"))
    make_ade_tree(root, n=12)
    return ade12(root)


def _epochs(loader, epochs=3):
    random.seed(1234)
    out, counters = [], []
    for e in range(epochs):
        loader.sampler.set_epoch(e)
        if loader.cache is not None:
            loader.cache.reset_counters()
        out.append([(i.clone(), l.clone()) for i, l in loader])
        if loader.cache is not None:
            counters.append((loader.cache.hits, loader.cache.misses))
    torch.cuda.synchronize()
    return out, counters


def _same(a, b):
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        assert len(ea) == len(eb) > 0
        for (ia, la), (ib, lb) in zip(ea, eb):
            assert ia.shape == ib.shape and ia.stride() == ib.stride() and torch.equal(ia, ib) and torch.equal(la, lb)


def _five_sample_budget(ds, sampler):
    sampler.set_epoch(0)
    return sum(sample_bytes(*ds[i][1].shape) for i in list(sampler)[:5])


def test_cached_train_loader_yields_the_plain_loaders_batches(ade):
    dev = torch.device("cuda:0")
    batcher = DeviceBatcher(dev, 64, ade.lut, train=True)

    def loader(cache):
        sampler = torch.utils.data.distributed.DistributedSampler(ade, num_replicas=1, rank=0, shuffle=True)
        return DeviceLoader(ade, 4, sampler, batcher, num_workers=0, drop_last=True, cache=cache)
    plain, _ = _epochs(loader(None))
    assert len(plain[0]) == 3 and plain[0][0][0].shape == (4, 3, 64, 64) and plain[0][0][1].shape == (4, 64, 64)
    full, counters = _epochs(loader(DeviceSampleCache(dev, 1 << 30)))
    _same(full, plain)
    assert counters == [(0, 12), (12, 0), (12, 0)]
    tight, counters = _epochs(loader(DeviceSampleCache(dev, _five_sample_budget(ade, loader(None).sampler))))
    _same(tight, plain)
    assert counters == [(0, 12), (5, 7), (5, 7)]


@pytest.mark.parametrize("crop", [True, False])
def test_cached_validation_loader_yields_the_plain_loaders_batches(ade, crop):
    dev = torch.device("cuda:0")
    batcher = DeviceBatcher(dev, 64, ade.lut, train=False, crop=crop)

    def loader(cache):
        sampler = torch.utils.data.distributed.DistributedSampler(ade, num_replicas=1, rank=0, shuffle=False)
        return DeviceLoader(ade, 4 if crop else 1, sampler, batcher, num_workers=0, cache=cache)
    plain, _ = _epochs(loader(None), epochs=2)
    full, counters = _epochs(loader(DeviceSampleCache(dev, 1 << 30)), epochs=2)
    _same(full, plain)
    assert counters == [(0, 12), (12, 0)]
    tight, counters = _epochs(loader(DeviceSampleCache(dev, _five_sample_budget(ade, loader(None).sampler))), epochs=2)
    _same(tight, plain)
    assert counters == [(0, 12), (5, 7)]
