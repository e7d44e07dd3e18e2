"""CPU: the host logic of the HBM sample cache (ucd_amd/datacache.py, dataset.DeviceLoader(cache=...)) with a ``"cpu"`` cache and a
stand-in batcher, as tests/test_dataset.py::test_device_loader_decodes_in_worker_processes does for the plain loader: slab
bookkeeping, the epoch schedule (same sequence as the plain loader, every index decoded once, only the refused ones again), the
flag and the export."""
import os
import zlib

import pytest
import torch

from ucd_amd import argparser, tasks
from ucd_amd.datacache import DeviceSampleCache, sample_bytes
from ucd_amd.dataset import AdeSegmentationIncremental, DeviceLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCHS = 3


def _pair(g, H, W):
    return (torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g), torch.randint(0, 256, (H, W), dtype=torch.uint8, generator=g))


def test_cache_bookkeeping_slabs_alignment_and_budget():
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (33, 31), (16, 16), (9, 101), (50, 3)]
    pairs = [_pair(g, H, W) for H, W in shapes]
    need = [sample_bytes(H, W) for H, W in shapes]
    assert all(n % 16 == 0 for n in need) and need[0] == 112 + 48
    slab = need[0] + need[1] + need[2] + 8                      # three samples fill the first slab: the fourth does not fit into 8 bytes
    budget = slab + need[3]                                     # ... and the second slab has room for exactly the fourth
    cache = DeviceSampleCache("cpu", budget, slab_bytes=slab)
    assert len(cache) == 0 and cache.bytes_used == 0 and cache.slabs == [] and cache.get(0) is None
    for k in range(3):
        assert cache.put(k, *pairs[k]) and len(cache.slabs) == 1 and cache.bytes_used == sum(need[:k + 1])
    assert cache.put(3, *pairs[3]) and len(cache.slabs) == 2    # lazily: only now, and no larger than the budget leaves
    assert cache.bytes_reserved == budget and cache.bytes_used == sum(need[:4]) <= budget
    assert cache.put(4, *pairs[4]) is False and len(cache) == 4 and 4 not in cache and cache.get(4) is None
    assert cache.bytes_used == sum(need[:4]) and len(cache.slabs) == 2
    for k in range(4):
        image, label = cache.get(k)
        assert torch.equal(image, pairs[k][0]) and torch.equal(label, pairs[k][1]) and cache.shape(k) == shapes[k] and k in cache
        assert image.data_ptr() % 16 == 0 and label.data_ptr() % 16 == 0
        assert image.is_contiguous() and label.is_contiguous()
    assert (cache.hits, cache.misses) == (4, 2)
    cache.reset_counters()
    assert (cache.hits, cache.misses) == (0, 0)
    # a refusal does not close the cache: a sample that fits what the budget still allows is stored
    roomy = DeviceSampleCache("cpu", need[1] + need[0], slab_bytes=need[1])
    assert roomy.put(1, *pairs[1]) and roomy.put(3, *pairs[3]) is False and roomy.put(0, *pairs[0]) and len(roomy) == 2
    assert roomy.bytes_reserved <= roomy.budget_bytes
    # two caches on one budget: the second takes what the first has left
    shared = []
    a = DeviceSampleCache("cpu", need[1] + need[2], slab_bytes=need[1], siblings=shared)
    b = DeviceSampleCache("cpu", need[1] + need[2], slab_bytes=need[1], siblings=shared)
    shared += [a, b]
    assert a.put(1, *pairs[1]) and b.put(1, *pairs[1]) is False and b.put(2, *pairs[2]) and a.put(2, *pairs[2]) is False


class _Counting(torch.utils.data.Dataset):
    """Dataset proxy that records which indices are decoded."""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __getitem__(self, index):
        self.seen.append(index)
        return self.inner[index]

    def __len__(self):
        return len(self.inner)


def _batcher(samples):
    return [(tuple(i.shape), zlib.crc32(i.numpy().tobytes()), tuple(l.shape), zlib.crc32(l.numpy().tobytes())) for i, l in samples]


@pytest.fixture(scope="module")
def ade(tmp_path_factory):
    from dataset_trees import make_ade_tree
    root = str(tmp_path_factory.mktemp("ade12"))
    make_ade_tree(root, n=12)
    return ade12(root)


def ade12(root):
    """All 12 samples of the tree under the label table of ADE 100-50, step 0.  The step's own filter would drop the three images
    whose label sets ([0, 101], [0, 107]) hold none of the classes 1 .. 100, and 9 samples do not fill batches of 4: the listing
    is the unfiltered one, the table the step's."""
    from ucd_amd import datapipe
    labels, labels_old, _ = tasks.get_task_labels("ade", "100-50", 0)
    ds = AdeSegmentationIncremental(root, train=True)
    ds.lut = datapipe.ade_target_lut(list(labels), list(labels_old))
    assert len(ds) == 12
    return ds


def _sampler(ds):
    return torch.utils.data.distributed.DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True)


def _epochs(loader):
    out = []
    for e in range(EPOCHS):
        loader.sampler.set_epoch(e)
        if loader.cache is not None:
            loader.cache.reset_counters()
        out.append(list(loader))
        assert len(out[-1]) == len(loader) == 3
    return out


@pytest.fixture(scope="module")
def plain(ade):
    return _epochs(DeviceLoader(ade, 4, _sampler(ade), _batcher, num_workers=0, drop_last=True))


@pytest.mark.parametrize("workers", [0, 2])
def test_cached_loader_yields_the_plain_loaders_sequence(ade, plain, workers):
    loader = DeviceLoader(ade, 4, _sampler(ade), _batcher, num_workers=workers, drop_last=True, cache=DeviceSampleCache("cpu", 1 << 30))
    assert _epochs(loader) == plain
    assert len(loader.cache) == 12 and loader.batch_size == 4 and isinstance(loader.sampler, torch.utils.data.Sampler)


def test_every_index_is_decoded_once(ade, plain):
    ds = _Counting(ade)
    loader = DeviceLoader(ds, 4, _sampler(ade), _batcher, num_workers=0, drop_last=True, cache=DeviceSampleCache("cpu", 1 << 30))
    counters = []
    for e in range(EPOCHS):
        loader.sampler.set_epoch(e)
        loader.cache.reset_counters()
        assert list(loader) == plain[e]
        counters.append((loader.cache.hits, loader.cache.misses))
        assert sorted(ds.seen) == list(range(12))               # each once in epoch 0, none after it
    loader.sampler.set_epoch(0)
    assert ds.seen == list(loader.sampler)                      # ... in the order the batches needed them
    assert counters == [(0, 12), (12, 0), (12, 0)]


def test_tight_budget_decodes_only_the_refused_again(ade, plain):
    sampler = _sampler(ade)
    sampler.set_epoch(0)
    first = list(sampler)
    shapes = {i: tuple(ade[i][1].shape) for i in range(12)}
    budget = sum(sample_bytes(*shapes[i]) for i in first[:5])   # room for exactly the first five samples of epoch 0
    ds = _Counting(ade)
    loader = DeviceLoader(ds, 4, sampler, _batcher, num_workers=0, drop_last=True, cache=DeviceSampleCache("cpu", budget))
    for e in range(EPOCHS):
        sampler.set_epoch(e)
        loader.cache.reset_counters()
        ds.seen.clear()
        assert list(loader) == plain[e]
        order = list(sampler)
        if e == 0:
            assert ds.seen == order and sorted(loader.cache._views) == sorted(first[:5])
        else:
            assert ds.seen == [i for i in order if i not in first[:5]]
        assert loader.cache.bytes_used == budget == loader.cache.bytes_reserved and len(loader.cache) == 5
        assert (loader.cache.hits, loader.cache.misses) == ((0, 12) if e == 0 else (5, 7))


def test_validation_on_the_host_takes_no_cache(ade, monkeypatch):
    from ucd_amd import switches
    from ucd_amd.dataset import DeviceBatcher
    batcher = DeviceBatcher("cpu", 64, ade.lut, train=False, crop=True)
    sampler = torch.utils.data.SequentialSampler(ade)
    monkeypatch.delenv("UCD_VAL_DEVICE", raising=False)
    switches.reload()
    assert DeviceLoader(ade, 4, sampler, batcher, cache=DeviceSampleCache("cpu", 1 << 30)).cache is not None
    monkeypatch.setenv("UCD_VAL_DEVICE", "0")
    switches.reload()
    try:
        assert DeviceLoader(ade, 4, sampler, batcher, cache=DeviceSampleCache("cpu", 1 << 30)).cache is None
        train = DeviceBatcher("cpu", 64, ade.lut, train=True)
        assert DeviceLoader(ade, 4, sampler, train, cache=DeviceSampleCache("cpu", 1 << 30)).cache is not None
    finally:
        monkeypatch.undo()
        switches.reload()


def test_flag_and_export():
    parser = argparser.get_argparser()
    assert parser.parse_args([]).cache_gb == 0.0
    assert parser.parse_args(["--cache_gb", "1.5"]).cache_gb == 1.5
    header = open(os.path.join(ROOT, "include", "ucd_hip.h")).read()
    assert "int ucd_batch_path(" in header                      # test_host_cpu.py then checks the symbol and its binding
    from ucd_amd import hip
    assert "ucd_batch_path" in hip.SIGNATURES and callable(hip.batch_path)
    with pytest.raises(RuntimeError, match="GPU only"):
        hip.batch_path([torch.zeros(4, 4, 3, dtype=torch.uint8)], [torch.zeros(4, 4, dtype=torch.uint8)], [(0, 0, 4, 4)], [False], 8,
                       torch.arange(256, dtype=torch.uint8), (0.5, 0.5, 0.5), (0.2, 0.2, 0.2))
