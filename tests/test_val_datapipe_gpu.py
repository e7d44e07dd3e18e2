"""GPU: the validation transforms on the device (ucd_val_image_path / ucd_val_label_path, csrc/datapipe.hip) against Pillow itself -
``resize`` of the whole image, then ``crop`` - and against what the batcher computed before them: the train path fed Pillow's
resized-and-cropped bytes with the identity box, and the torch composition of the full-size branch.  Labels and the bytes behind
the images are exact; the float composition on the host is held to the 2e-6 tests/test_dataset.py uses."""
import functools
import os

import numpy as np
import pytest
import torch

from ucd_amd import datapipe, switches, tasks
from ucd_amd.dataset import DeviceBatcher, VOCSegmentationIncremental

PIL = pytest.importorskip("PIL.Image")

DEV = "cuda:0"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# source (H0, W0), S -> resized (oh, ow), window (i, j), kmax
CASES = [((37, 50), 33, (33, 44), (0, 6), 5),       # landscape; 5.5 rounds to 6
         ((37, 48), 33, (33, 42), (0, 4), 5),       # 4.5 rounds to 4; accumulated NEAREST index != floor rule inside the window
         ((50, 37), 33, (44, 33), (6, 0), 5),       # portrait
         ((20, 31), 33, (33, 51), (0, 9), 3),       # up-scaling
         ((131, 200), 33, (33, 50), (0, 8), 9),     # x4 down-scaling
         ((33, 33), 33, (33, 33), (0, 0), 3),       # identity
         ((33, 70), 33, (33, 70), (0, 18), 3),      # crop only
         ((16, 160), 33, (33, 330), (0, 148), 3),   # window far from index 0; NEAREST differs
         ((375, 500), 64, (64, 85), (0, 10), 13)]   # VOC aspect; NEAREST differs
IDS = [f"{c[0][0]}x{c[0][1]}-{c[1]}" for c in CASES]


def _lut():
    labels, labels_old, _ = tasks.get_task_labels("voc", "15-5", 1)
    return datapipe.target_lut(labels, labels_old)


@functools.lru_cache(maxsize=None)
def _source(H0, W0):
    """one raw sample of this size: random bytes; the label values span 0 .. 255"""
    rng = np.random.RandomState(1000 * H0 + W0)
    img = rng.randint(0, 256, size=(H0, W0, 3)).astype(np.uint8)
    lab = rng.randint(0, 256, size=(H0, W0)).astype(np.uint8)
    lab.reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)
    img.setflags(write=False); lab.setflags(write=False)
    return img, lab


@functools.lru_cache(maxsize=None)
def _pillow(H0, W0, S):
    """Pillow's Resize(S) + CenterCrop(S) of the sample: (image bytes [S, S, 3], label bytes [S, S], (oh, ow, i, j))"""
    img, lab = _source(H0, W0)
    oh, ow, i, j = datapipe.resize_center_crop_params(H0, W0, S)
    pi = PIL.fromarray(img).resize((ow, oh), PIL.BILINEAR).crop((j, i, j + S, i + S))
    pl = PIL.fromarray(lab).resize((ow, oh), PIL.NEAREST).crop((j, i, j + S, i + S))
    ri, rl = np.asarray(pi, dtype=np.uint8).copy(), np.asarray(pl, dtype=np.uint8).copy()
    ri.setflags(write=False); rl.setflags(write=False)
    return ri, rl, (oh, ow, i, j)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _normalised(u8):
    """ToTensor + Normalize of [H, W, 3] bytes in fp32 on the host, as tests/test_dataset.py composes it"""
    x = torch.from_numpy(np.array(u8)).permute(2, 0, 1).float().div(255)
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def _pillow_nearest_index(in_size, out_full, n):
    """the source indices Pillow's NEAREST resize takes for outputs 0 .. n - 1: a running double sum (Geometry.c, affine_transform
    with the scale-only matrix resize hands it)"""
    a, xo, idx = in_size / out_full, in_size / out_full * 0.5, []
    for _ in range(n):
        idx.append(int(xo))
        xo += a
    return idx


def test_cases_are_what_the_table_says_and_exercise_the_accumulated_nearest_rule():
    differs = []
    for (H0, W0), S, resized, window, kmax in CASES:
        oh, ow, i, j = datapipe.resize_center_crop_params(H0, W0, S)
        assert (oh, ow) == resized and (i, j) == window
        assert int(np.ceil(max(1.0, H0 / oh, W0 / ow))) * 2 + 1 == kmax
        for in_size, out_full, off in ((H0, oh, i), (W0, ow, j)):
            acc = _pillow_nearest_index(in_size, out_full, off + S)[off:]
            floor = [int(np.floor((x + 0.5) * (in_size / out_full))) for x in range(off, off + S)]
            if acc != floor:
                differs.append((H0, W0, S))
    # with the floor rule (or a sum restarted at the window) the label tests below cannot pass
    assert {(37, 48, 33), (16, 160, 33), (375, 500, 64)} <= set(differs)
    assert set(np.unique(_source(37, 50)[1])) == set(range(256))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_equal_pillow_nearest_resize_and_crop(case):
    (H0, W0), S = case[0], case[1]
    lut = _lut()
    _, rl, params = _pillow(H0, W0, S)
    y = datapipe.DeviceValLabelPath(lut)([_dev(_source(H0, W0)[1])], [params], (S, S))
    assert y.shape == (1, S, S) and y.dtype == torch.int64
    assert torch.equal(y[0].cpu(), torch.from_numpy(lut.numpy()[rl].astype(np.int64)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_images_equal_the_train_path_on_pillows_bytes(case):
    (H0, W0), S = case[0], case[1]
    ri, _, params = _pillow(H0, W0, S)
    x = datapipe.DeviceValImagePath(MEAN, STD)([_dev(_source(H0, W0)[0])], [params], (S, S))
    assert x.shape == (1, 3, S, S) and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
    before = datapipe.DeviceImagePath(S, MEAN, STD)([_dev(ri)], [(0, 0, S, S)], [False])
    diff = (x - before).abs().max().item()
    print(f"{H0}x{W0} -> {S}: max |device - train path on Pillow's bytes| = {diff:.3e}")
    assert torch.equal(x, before)                                              # what the batcher produced before, bit for bit
    torch.testing.assert_close(x[0].cpu(), _normalised(ri), rtol=0, atol=2e-6)


@pytest.mark.gpu
def test_one_launch_carries_three_sizes():
    """rows 1, 3 and 5 as one batch: per-image descriptors, the intermediate sized by the largest source"""
    S, picks = 33, [CASES[0], CASES[2], CASES[4]]
    lut = _lut()
    refs = [_pillow(c[0][0], c[0][1], S) for c in picks]
    params = [r[2] for r in refs]
    x = datapipe.DeviceValImagePath(MEAN, STD)([_dev(_source(*c[0])[0]) for c in picks], params, (S, S))
    y = datapipe.DeviceValLabelPath(lut)([_dev(_source(*c[0])[1]) for c in picks], params, (S, S))
    before = datapipe.DeviceImagePath(S, MEAN, STD)([_dev(r[0]) for r in refs], [(0, 0, S, S)] * 3, [False] * 3)
    assert x.shape == (3, 3, S, S) and y.shape == (3, S, S)
    assert torch.equal(x, before)
    for b, (ri, rl, _) in enumerate(refs):
        assert torch.equal(y[b].cpu(), torch.from_numpy(lut.numpy()[rl].astype(np.int64))), b
        torch.testing.assert_close(x[b].cpu(), _normalised(ri), rtol=0, atol=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("scale_mode", [0, 1])
@pytest.mark.parametrize("size", [(37, 50), (50, 37)])
def test_full_size_is_the_identity(size, scale_mode):
    H0, W0 = size
    img, lab = _source(H0, W0)
    lut = _lut()
    params = [(H0, W0, 0, 0)]
    y = datapipe.DeviceValLabelPath(lut)([_dev(lab)], params, (H0, W0))
    assert torch.equal(y[0].cpu(), torch.from_numpy(lut.numpy()[lab].astype(np.int64)))
    x = datapipe.DeviceValImagePath(MEAN, STD, scale_mode=scale_mode)([_dev(img)], params, (H0, W0))
    assert x.shape == (1, 3, H0, W0) and x.is_contiguous(memory_format=torch.channels_last)
    # the torch composition of the batcher's full-size branch, on the device
    m, s = torch.tensor(MEAN, device=DEV).view(3, 1, 1), torch.tensor(STD, device=DEV).view(3, 1, 1)
    before = ((_dev(img).permute(2, 0, 1).float().div_(255.0) - m) / s).unsqueeze(0)
    diff = (x - before).abs().max().item()
    print(f"full size {H0}x{W0}, scale_mode {scale_mode}: max |device - torch composition| = {diff:.3e}")
    torch.testing.assert_close(x, before, rtol=0, atol=2e-6)
    torch.testing.assert_close(x[0].cpu(), _normalised(img), rtol=0, atol=2e-6)
    back = ((x[0] * s + m) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    assert torch.equal(back.cpu(), torch.from_numpy(np.array(img)))            # the identity coefficients gave the byte back


CLASS_SETS = [[0, 1, 5], [0, 16], [0, 3, 17, 255], [0, 20, 255], [0, 2], [0, 15, 19], [0, 18, 16, 4], [0, 6, 255], [0, 17], [0, 20, 1]]


def _make_tree(root, n=10, seed=7):
    """a synthetic VOC tree, built like the one of tests/test_dataset.py"""
    rng = np.random.RandomState(seed)
    os.makedirs(root / "splits"); os.makedirs(root / "JPEGImages"); os.makedirs(root / "SegmentationClassAug")
    lines = []
    for k in range(n):
        H, W = int(rng.randint(90, 180)), int(rng.randint(90, 180))
        img = rng.randint(0, 256, size=(H // 6 + 1, W // 6 + 1, 3)).astype(np.uint8).repeat(6, 0).repeat(6, 1)[:H, :W]
        lab = rng.choice(CLASS_SETS[k % len(CLASS_SETS)], size=(H // 10 + 1, W // 10 + 1)).astype(np.uint8).repeat(10, 0).repeat(10, 1)[:H, :W]
        PIL.fromarray(img).save(root / "JPEGImages" / f"im{k}.png")
        PIL.fromarray(lab).save(root / "SegmentationClassAug" / f"im{k}.png")
        lines.append(f"/JPEGImages/im{k}.png /SegmentationClassAug/im{k}.png\n")
    (root / "splits" / "train_aug.txt").write_text("".join(lines))
    (root / "splits" / "val.txt").write_text("".join(lines[: n // 2]))


@pytest.mark.gpu
@pytest.mark.parametrize("crop", [True, False])
def test_device_batcher_validation_equals_the_host_form(tmp_path, crop):
    """DeviceBatcher(train=False): UCD_VAL_DEVICE=1 (one call per batch on raw samples) against UCD_VAL_DEVICE=0 (Pillow on the host /
    torch launches), exactly - every sample of the split; batches of 3 + 2 when cropped, of 1 at full size"""
    _make_tree(tmp_path)
    d = VOCSegmentationIncremental(str(tmp_path), train=False, labels=list(range(1, 21)))
    S = 65
    bt = DeviceBatcher(DEV, S, d.lut, train=False, crop=crop)
    step = 3 if crop else 1
    batches = [[d[k] for k in range(lo, min(lo + step, len(d)))] for lo in range(0, len(d), step)]
    got = {}
    try:
        for mode in ("0", "1"):
            switches.set("UCD_VAL_DEVICE", mode)
            got[mode] = [bt(samples) for samples in batches]
    finally:
        switches.unset("UCD_VAL_DEVICE")
    for samples, (x0, y0), (x1, y1) in zip(batches, got["0"], got["1"]):
        hw = (S, S) if crop else tuple(samples[0][0].shape[:2])
        assert x1.shape == x0.shape == (len(samples), 3) + hw and y1.shape == y0.shape == (len(samples),) + hw
        assert x1.dtype == x0.dtype and y1.dtype == y0.dtype == torch.int64
        assert x1.is_contiguous(memory_format=torch.channels_last)              # the layout the batcher's docstring promises
        assert torch.equal(y1, y0)
        print(f"crop={crop}: max |device - host form| = {(x1 - x0).abs().max().item():.3e}")
        assert torch.equal(x1, x0)
