"""CPU: the host half of the evaluation output path (ucd_seg_render / ucd_attn_energy, csrc/seg_render.hip; ucd_amd.visual) - the
exported symbols, every host-side refusal (decided before any device call: no GPU is needed to hear them), the palette against its
closed-form definition, and the GPU-only refusal of visual.render."""
import ctypes as C

import numpy as np
import pytest
import torch

EINVAL, EUNSUPPORTED = -1, -4


def test_symbols_are_exported():
    from ucd_amd import hip
    assert "ucd_seg_render" in hip.SIGNATURES and "ucd_attn_energy" in hip.SIGNATURES
    lib = hip.load()
    assert lib.ucd_seg_render is not None and lib.ucd_attn_energy is not None


def _render(lib, **over):
    """ucd_seg_render on a host buffer that no accepted call would take: every case here is refused before a device call."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = dict(sem=p, ld_s=21, labels=p, image=p, sb=3 * 65 * 97, sc=65 * 97, sh=97, sw=1, cmap=p, att_low=p, ha=5, wa=7, B=2, H=65, W=97,
             h=5, w=7, Ctot=21, pred_u8=p, pred_rgb=p, label_rgb=p, image_u8=p, att=p)
    a.update(over)
    rc = lib.ucd_seg_render(a["sem"], a["ld_s"], a["labels"], a["image"], a["sb"], a["sc"], a["sh"], a["sw"], 0.485, 0.456, 0.406, 0.229,
                            0.224, 0.225, a["cmap"], a["att_low"], a["ha"], a["wa"], a["B"], a["H"], a["W"], a["h"], a["w"], a["Ctot"],
                            a["pred_u8"], a["pred_rgb"], a["label_rgb"], a["image_u8"], a["att"], None)
    return rc, lib.ucd_last_error().decode()


NO_OUTPUT = dict(pred_u8=None, pred_rgb=None, label_rgb=None, image_u8=None, att=None)
RENDER_REFUSALS = [
    ("sem NULL", dict(sem=None), EINVAL, "sem"), ("cmap NULL", dict(cmap=None), EINVAL, "cmap"),
    ("B 0", dict(B=0), EINVAL, "B"), ("H 0", dict(H=0), EINVAL, "H"), ("W 0", dict(W=0), EINVAL, "W"),
    ("h 0", dict(h=0), EINVAL, "h"), ("w 0", dict(w=0), EINVAL, "w"), ("Ctot 0", dict(Ctot=0, ld_s=0), EINVAL, "Ctot"),
    ("ld_s below Ctot", dict(ld_s=20), EINVAL, "ld_s"), ("Ctot 256", dict(Ctot=256, ld_s=256), EINVAL, "Ctot"),
    ("label_rgb without labels", dict(labels=None), EINVAL, "labels"),
    ("image_u8 without image", dict(image=None), EINVAL, "image"),
    ("att without att_low", dict(att_low=None), EINVAL, "att_low"),
    ("att on an empty grid", dict(ha=0), EINVAL, "ha"),
    ("every output NULL", NO_OUTPUT, EINVAL, "output"),
    ("factor below 4 (rows)", dict(h=17), EUNSUPPORTED, "up-sampling factors >= 4"),
    ("factor below 4 (columns)", dict(w=25), EUNSUPPORTED, "up-sampling factors >= 4"),
    # 255 classes on 129 x 129 cells under 516 x 516 pixels (factor 4): (64 * 129 / 516 + 3)^2 = 19^2 cells x 255 floats > 150 KB
    ("LDS footprint", dict(H=516, W=516, h=129, w=129, Ctot=255, ld_s=255), EUNSUPPORTED, "exceed the LDS budget"),
]


@pytest.mark.parametrize("name,over,code,word", RENDER_REFUSALS, ids=[r[0] for r in RENDER_REFUSALS])
def test_seg_render_refusals(name, over, code, word):
    """Each refusal returns its code before anything is launched (the pointers are host memory: a launch could only fault), and
    the message names the entry and the argument."""
    from ucd_amd import hip
    rc, msg = _render(hip.load(), **over)
    assert rc == code, (name, rc, msg)
    assert msg.startswith("ucd_seg_render:") and word in msg, msg


def test_seg_render_refusals_are_worded_like_seg_confusion():
    """The geometry limits are ucd_seg_confusion's, in its words."""
    from ucd_amd import hip
    lib = hip.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    _, mine = _render(lib, h=17)
    assert lib.ucd_seg_confusion(p, 21, p, 2, 65, 97, 17, 7, 21, 21, p, None, None) == EUNSUPPORTED
    assert lib.ucd_last_error().decode().replace("ucd_seg_confusion", "ucd_seg_render") == mine
    _, mine = _render(lib, H=516, W=516, h=129, w=129, Ctot=255, ld_s=255)
    assert lib.ucd_seg_confusion(p, 255, p, 2, 516, 516, 129, 129, 255, 255, p, None, None) == EUNSUPPORTED
    assert lib.ucd_last_error().decode().replace("ucd_seg_confusion", "ucd_seg_render") == mine


ENERGY_REFUSALS = [
    ("x NULL", dict(x=None), "x"), ("a NULL", dict(a=None), "a"), ("dtype", dict(dtype=2), "dtype"), ("B 0", dict(B=0), "B"),
    ("HW 0", dict(HW=0), "HW"), ("C 0", dict(C=0, ld=0), "C"), ("ld below C", dict(ld=63), "ld"),
]


@pytest.mark.parametrize("name,over,word", ENERGY_REFUSALS, ids=[r[0] for r in ENERGY_REFUSALS])
def test_attn_energy_refusals(name, over, word):
    from ucd_amd import hip
    lib = hip.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    a = dict(x=p, ld=64, dtype=hip.F32, B=2, HW=35, C=64, a=p)
    a.update(over)
    rc = lib.ucd_attn_energy(a["x"], a["ld"], a["dtype"], a["B"], a["HW"], a["C"], a["a"], None)
    msg = lib.ucd_last_error().decode()
    assert rc == EINVAL, (name, rc, msg)
    assert msg.startswith("ucd_attn_energy:") and word in msg, msg


def voc_palette_closed_form():
    """The PASCAL VOC devkit's palette from its definition: walk the id three bits at a time, the j-th triple (r, g, b) = (bit 0,
    bit 1, bit 2) goes to bit 7 - j of the three channels."""
    cmap = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap


def test_color_map_is_the_voc_palette():
    from ucd_amd import visual
    cmap = visual.color_map("voc")
    assert cmap.dtype == np.uint8 and cmap.shape == (256, 3)
    np.testing.assert_array_equal(cmap, voc_palette_closed_form())
    for i, rgb in {0: (0, 0, 0), 1: (128, 0, 0), 15: (192, 128, 128), 255: (224, 224, 192)}.items():
        assert tuple(cmap[i]) == rgb, i
    for dataset in ("ade", "city", None):                      # one palette for every dataset (the docstring says why)
        np.testing.assert_array_equal(visual.color_map(dataset), cmap)
    own = np.arange(768).reshape(256, 3) % 256
    got = visual.color_map("voc", palette=own)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, own)
    with pytest.raises(ValueError):
        visual.color_map("voc", palette=np.zeros((21, 3)))


def test_render_refuses_cpu_tensors():
    from ucd_amd import visual
    with pytest.raises(RuntimeError, match="GPU only"):
        visual.render(torch.zeros(1, 21, 5, 7), labels=torch.zeros(1, 65, 97, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU only"):
        visual.attn_energy(torch.zeros(1, 64, 5, 7))
