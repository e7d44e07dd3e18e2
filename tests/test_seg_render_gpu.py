"""GPU: the evaluation output kernels (ucd_seg_render, ucd_attn_energy; csrc/seg_render.hip) through the C ABI and ucd_amd.visual.

Geometries: the smallest that still have partial tiles in both directions (65 x 97 pixels under 64 x 64 tiles: 2 x 2 blocks, the
second row of one pixel row, the second column of 33 pixels; 97 pixels = 291 bytes per RGB row, so consecutive rows start on every
dword phase), at two up-sampling factors, with 21 classes (the LDS-histogram regime of ucd_seg_confusion) and 151 (its global one).
Every output is written into one arena with guard bytes around it, at offsets that are not dword multiples for the byte maps."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ucd_amd import synth

pytestmark = pytest.mark.gpu

GEOMETRIES = {"s16-21": (2, 65, 97, 5, 7, 21), "s8-21": (2, 65, 97, 9, 13, 21), "s16-151": (1, 65, 97, 5, 7, 151)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUTPUTS = ("pred_u8", "pred_rgb", "label_rgb", "image_u8", "att")
SENTINEL = 0xA5
GUARD = 61                                  # bytes between two outputs: odd, so the byte maps start off the dword grid


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(geo):
    """(sem [B, Ctot, h, w], labels with 255 and ids past the classes, normalised images NCHW, the uniform images, body) on the device."""
    B, H, W, h, w, Ctot = GEOMETRIES[geo]
    seed = 700 + sorted(GEOMETRIES).index(geo)
    sem = synth.t_normal(seed, (B, Ctot, h, w), stream=1, scale=3.0)
    labels = torch.from_numpy(synth.randint(seed, (B, H, W), 0, Ctot + 4, stream=2))
    labels[labels >= Ctot] = 255
    labels[0, 0, :5] = torch.tensor([0, 1, 15, 255, Ctot - 1])
    u = torch.from_numpy(synth.randint(seed, (B, 3, H, W), 0, 1 << 24, stream=3).astype(np.float32) / np.float32(1 << 24))
    u[0, 0, 0, 0], u[0, 1, 0, 0] = 1.3, -0.2                              # outside the range on either side
    x = (u - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    body = synth.t_normal(seed, (B, 64, 5, 7), stream=4, scale=0.7)
    dev = _dev()
    return sem.to(dev), labels.to(dev), x.to(dev), u, body.to(dev)


def rows(sem):
    B, Ctot, h, w = sem.shape
    return sem.permute(0, 2, 3, 1).reshape(B * h * w, Ctot).float().contiguous()


def cmap_dev():
    from ucd_amd import visual
    return torch.from_numpy(visual.color_map("voc")).to(_dev())


def call_render(geo, sem, labels, images, att_low, want=OUTPUTS):
    """ucd_seg_render through the C ABI into one sentinel-filled arena: the outputs in ``want`` at guarded offsets; returns
    (dict of output tensors, the bytes outside every requested output are still the sentinel)."""
    from ucd_amd import hip
    B, H, W, h, w, Ctot = GEOMETRIES[geo]
    dev = _dev()
    sizes = {"pred_u8": B * H * W, "pred_rgb": 3 * B * H * W, "label_rgb": 3 * B * H * W, "image_u8": 3 * B * H * W, "att": 4 * B * H * W}
    offs, o = {}, GUARD
    for name in OUTPUTS:
        if name == "att":
            o = (o + 3) // 4 * 4                         # the only output with an alignment: fp32
        offs[name] = o
        o += sizes[name] + GUARD
    arena = torch.full((o,), SENTINEL, dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 4 == 0
    ptr = {name: (arena.data_ptr() + offs[name] if name in want else None) for name in OUTPUTS}
    s = rows(sem)
    cm = cmap_dev()
    strides = images.stride() if images is not None else (0, 0, 0, 0)
    ha, wa = att_low.shape[-2:] if att_low is not None else (1, 1)
    hip._check(hip.load().ucd_seg_render(hip.ptr(s), Ctot, hip.ptr(labels), hip.ptr(images), *strides, *MEAN, *STD, hip.ptr(cm),
                                         hip.ptr(att_low), ha, wa, B, H, W, h, w, Ctot, ptr["pred_u8"], ptr["pred_rgb"],
                                         ptr["label_rgb"], ptr["image_u8"], ptr["att"], hip.stream()), "ucd_seg_render")
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    untouched = np.ones(o, dtype=bool)
    out = {}
    for name in want:
        a, n = offs[name], sizes[name]
        untouched[a:a + n] = False
        raw = host[a:a + n].copy()
        out[name] = raw.view(np.float32).reshape(B, H, W) if name == "att" else raw.reshape((B, H, W) if name == "pred_u8" else (B, H, W, 3))
    return out, bool((host[untouched] == SENTINEL).all())


def confusion_pred(geo, sem, labels):
    from ucd_amd import hip
    B, H, W, h, w, Ctot = GEOMETRIES[geo]
    s = rows(sem)
    hist = torch.zeros(Ctot, Ctot, dtype=torch.int64, device=_dev())
    pred = torch.full((B, H, W), -1, dtype=torch.int64, device=_dev())
    hip._check(hip.load().ucd_seg_confusion(hip.ptr(s), Ctot, hip.ptr(labels), B, H, W, h, w, Ctot, Ctot, hip.ptr(hist), hip.ptr(pred),
                                            hip.stream()), "ucd_seg_confusion")
    return pred.cpu().numpy()


def energy(body):
    from ucd_amd import visual
    return visual.attn_energy(body)


@functools.lru_cache(maxsize=None)
def full_render(geo):
    """Every output of one call on the shared inputs (the reference of the per-output and repeat checks): computed once."""
    sem, labels, x, _, body = inputs(geo)
    att_low = energy(body.contiguous(memory_format=torch.channels_last))
    out, clean = call_render(geo, sem, labels, x, att_low)
    return out, clean, att_low


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_pred_has_the_bits_of_the_confusion_kernel(geo):
    """pred_u8 == the pred of ucd_seg_confusion, exactly: on N(0, 3^2) logits; on all-equal logits (all 0: the first maximum);
    with the row-wise maximum duplicated in two classes (the lower index wins)."""
    B, H, W, h, w, Ctot = GEOMETRIES[geo]
    sem, labels, _, _, _ = inputs(geo)
    out, clean, _ = full_render(geo)
    ref = confusion_pred(geo, sem, labels)
    assert clean
    assert len(np.unique(ref)) > min(Ctot, 15) // 2                  # a real map, not a constant
    np.testing.assert_array_equal(out["pred_u8"].astype(np.int64), ref)
    flat = torch.full_like(sem, 0.37)
    got, _ = call_render(geo, flat, labels, None, None, want=("pred_u8",))
    assert not got["pred_u8"].any()
    np.testing.assert_array_equal(got["pred_u8"].astype(np.int64), confusion_pred(geo, flat, labels))
    lo, hi = 3, Ctot - 2
    dup = sem.clone()
    top = sem.max(dim=1)[0] + 1.0
    dup[:, lo], dup[:, hi] = top, top                                # equal inputs, equal arithmetic: the two classes tie at every pixel
    got, _ = call_render(geo, dup, labels, None, None, want=("pred_u8",))
    assert (got["pred_u8"] == lo).all()
    np.testing.assert_array_equal(got["pred_u8"].astype(np.int64), confusion_pred(geo, dup, labels))


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_colour_coded_maps_are_palette_lookups(geo):
    """pred_rgb == cmap[pred] and label_rgb == cmap[label & 255], indexed in numpy; the labels include 255."""
    from ucd_amd import visual
    _, labels, _, _, _ = inputs(geo)
    out, _, _ = full_render(geo)
    cmap = visual.color_map("voc")
    lab = labels.cpu().numpy()
    assert (lab == 255).any()
    np.testing.assert_array_equal(out["pred_rgb"], cmap[out["pred_u8"]])
    np.testing.assert_array_equal(out["label_rgb"], cmap[lab & 255])


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_denormalised_image(layout):
    """image_u8 against the reference's formula ((x - (-mean / std)) / (1 / std)) * 255 (utils.Denormalize, run.py:344) in float64,
    truncated, on images uniform in [0, 1) and then normalised in fp32: |diff| <= 1 everywhere, at most 0.1 % of the elements
    differ.  The cap is reasoning, not a measurement: an fp32 evaluation has an absolute error of a few 1e-5 at 255, so it lands
    on the other side of an integer with a probability of that order per element, ten times below the cap (numpy float32 against
    float64 on these very inputs: no element of 37 830 differs).  A value outside the range is clamped (1.3 -> 255, -0.2 -> 0), not
    wrapped (the reference's astype(uint8) would give 75 and 205)."""
    geo = "s16-21"
    sem, labels, x, u, _ = inputs(geo)
    img = x if layout == "nchw" else x.contiguous(memory_format=torch.channels_last)
    assert (img.stride(1) == 1) == (layout == "channels_last")
    out, clean = call_render(geo, sem, labels, img, None, want=("image_u8",))
    assert clean
    got = out["image_u8"].astype(np.int64)                                     # [B, H, W, 3]
    x64 = x.cpu().numpy().astype(np.float64)
    m = np.asarray(MEAN, np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(STD, np.float64).reshape(1, 3, 1, 1)
    v = ((x64 - (-m / s)) / (1.0 / s)) * 255.0
    ref = np.clip(np.trunc(v), 0, 255).astype(np.int64).transpose(0, 2, 3, 1)
    diff = np.abs(got - ref)
    share = float((diff != 0).mean())
    print(f"image_u8 {layout}: max |diff| {diff.max()}, share differing {share:.2e}")
    assert diff.max() <= 1
    assert share <= 1e-3
    assert got[0, 0, 0, 0] == 255 and got[0, 0, 0, 1] == 0                     # 1.3 and -0.2: clamped
    if layout == "nchw":
        np.testing.assert_array_equal(full_render(geo)[0]["image_u8"], out["image_u8"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attn_energy_vs_float64(dtype):
    """ucd_attn_energy on a [2, 64, 5, 7] map against the float64 evaluation of the reference's train.py:339-342 from the same
    (already rounded) inputs.  Tolerance: relative 1e-4, the bound tests/test_kd_losses_gpu.py::test_attn_mse_vs_float64 holds
    ucd_attn_mse to for fp32 AND bf16 inputs (its loss is accumulated in fp32 from the rounded inputs, as this map is; the output
    here is fp32, so there is no bf16 output rounding to allow for).  Channels-last and NCHW inputs, and a row pitch off the 16-byte
    grid (the element-load path), give the same map; two calls give equal bits."""
    from ucd_amd import hip
    body = inputs("s16-21")[4].to(dtype)
    a64 = (body.double() ** 2).sum(dim=1)
    for l in range(a64.shape[0]):
        a64[l] = a64[l] / torch.norm(a64[l])
    got = energy(body.contiguous(memory_format=torch.channels_last))
    assert got.dtype == torch.float32 and got.shape == (2, 5, 7)
    np.testing.assert_allclose(got.cpu().numpy(), a64.cpu().numpy(), rtol=1e-4, atol=0)
    assert torch.equal(energy(body.contiguous(memory_format=torch.channels_last)), got)
    np.testing.assert_allclose(energy(body.contiguous()).cpu().numpy(), a64.cpu().numpy(), rtol=1e-4, atol=0)
    # rows of pitch 67 elements: neither base + pitch on the 16-byte grid -> element loads; the padding is NaN and must not be read
    B, Cc, h, w = body.shape
    padded = torch.full((B * h * w, 67), float("nan"), dtype=dtype, device=body.device)
    padded[:, :Cc] = body.permute(0, 2, 3, 1).reshape(B * h * w, Cc)
    a = torch.full((B * h * w + 8,), 777.0, device=body.device)
    hip._check(hip.load().ucd_attn_energy(hip.ptr(padded), 67, hip.dtype_code(padded), B, h * w, Cc, hip.ptr(a), hip.stream()),
               "ucd_attn_energy")
    np.testing.assert_allclose(a[:B * h * w].view(B, h, w).cpu().numpy(), a64.cpu().numpy(), rtol=1e-4, atol=0)
    assert bool((a[B * h * w:] == 777.0).all())


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_upsampled_attention_map(geo):
    """att against F.interpolate(att_low, align_corners=False) of the kernel's own att_low, on a 5 x 7 source grid whatever the
    logits' grid is.  Tolerance: 1e-5 absolute, the margin below which tests/test_metrics.py and tests/test_seglosses_gpu.py let an
    interpolated logit differ between the kernels' and torch's arithmetic (values of scale 2 there; the map here is below 1)."""
    B, H, W = GEOMETRIES[geo][:3]
    out, _, att_low = full_render(geo)
    assert att_low.shape == (B, 5, 7)
    ref = F.interpolate(att_low.unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False).squeeze(1)
    np.testing.assert_allclose(out["att"], ref.cpu().numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_repeatable_and_confined(geo):
    """Two runs give equal bits for every output; with a single output requested that output has the bits of the all-outputs call
    and every other byte of the arena - the other outputs' buffers and the guards around the requested one - keeps its fill."""
    sem, labels, x, _, _ = inputs(geo)
    first, clean, att_low = full_render(geo)
    assert clean
    again, clean = call_render(geo, sem, labels, x, att_low)
    assert clean
    for name in OUTPUTS:
        assert np.array_equal(first[name].view(np.uint8), again[name].view(np.uint8)), name
    for name in OUTPUTS:
        one, clean = call_render(geo, sem, labels, x, att_low, want=(name,))
        assert clean, name
        assert np.array_equal(one[name].view(np.uint8), first[name].view(np.uint8)), name


def test_visual_render_wraps_both_entries():
    """ucd_amd.visual.render: the dict of device tensors, equal to the C-ABI call; channels-last images; a custom palette."""
    from ucd_amd import visual
    geo = "s8-21"
    sem, labels, x, _, body = inputs(geo)
    first, _, _ = full_render(geo)
    r = visual.render(sem, labels, x.contiguous(memory_format=torch.channels_last), body)
    assert set(r) == {"pred_u8", "pred_rgb", "label_rgb", "image_u8", "att", "att_low", "label_u8"}
    for name in OUTPUTS:
        assert r[name].is_cuda and r[name].dtype == (torch.float32 if name == "att" else torch.uint8)
        assert np.array_equal(r[name].cpu().numpy(), first[name]), name
    assert torch.equal(r["label_u8"], labels.to(torch.uint8))
    pal = (np.arange(768).reshape(256, 3) * 7 % 256).astype(np.uint8)
    r2 = visual.render(sem, labels, cmap=pal, want=("pred_rgb",))
    assert set(r2) == {"pred_rgb", "label_u8"}
    np.testing.assert_array_equal(r2["pred_rgb"].cpu().numpy(), pal[first["pred_u8"]])
