"""CPU: the host half of the focal cross entropy (``--focal_loss``; ucd_seg_losses_focal / ucd_seg_losses_gather_focal,
ucd_amd.loss.focal_modulate / FocalLoss) - the command line, the symbols and their argument counts, the library's refusals (host
checks, before any device call), the torch composition against the reference's numbers (tests/golden/focal_losses.npz) and the
float64 definition (tests/focal_ref.py), and a Trainer on a small CPU network."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import focal_ref as R
import test_pod_cpu as P
from conftest import assert_matches_compact, load_golden
from ucd_amd import argparser, hip, switches
from ucd_amd.loss import FocalLoss, UnbiasedCrossEntropy, focal_modulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
ENTRIES = ("ucd_seg_losses_focal", "ucd_seg_losses_gather_focal")


def _parse(args):
    return argparser.modify_command_options(argparser.get_argparser().parse_args(["--task", "15-5", "--step", "1"] + list(args)))


def test_parser():
    o = _parse(["--method", "UCD"])
    assert (o.focal_loss, o.focal_loss_gamma, o.focal_loss_alpha) == (False, 2.0, 1.0)
    o = _parse(["--method", "PLOP", "--pod_logits", "--focal_loss", "--focal_loss_gamma", "0.5", "--focal_loss_alpha", "0.25"])
    assert (o.focal_loss, o.focal_loss_gamma, o.focal_loss_alpha, o.pseudo, o.pod_logits) == (True, 0.5, 0.25, "entropy", True)
    assert _parse(["--focal_loss", "--focal_loss_gamma", "0"]).focal_loss_gamma == 0.0
    for bad in ("-0.5", "nan", "inf"):
        with pytest.raises(SystemExit):
            _parse(["--focal_loss_gamma", bad])
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            _parse(["--focal_loss_alpha", bad])
    for combo in (["--bce"], ["--icarl"], ["--method", "LWF-MC"]):
        with pytest.raises(ValueError, match="--focal_loss"):
            _parse(combo + ["--focal_loss"])
    assert _parse(["--bce", "--focal_loss_gamma", "3"]).focal_loss is False         # the values alone request nothing


def test_symbols_header_and_argument_counts():
    """Both entries are declared in the header with the argument count hip.py gives them, and the shared library exports them."""
    with open(os.path.join(ROOT, "include", "ucd_hip.h")) as f:
        header = f.read()
    lib = hip.load()
    for name, base in zip(ENTRIES, ("ucd_seg_losses_ex_w", "ucd_seg_losses_gather_w")):
        decl = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
        assert decl, name
        args = [a for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if a.strip()]
        assert len(args) == len(hip.SIGNATURES[name][1]) == len(hip.SIGNATURES[base][1]) + 2, name
        assert "focal_gamma" in decl.group(1) and "focal_alpha" in decl.group(1)
        assert getattr(lib, name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ucd_amd", "libucd_hip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(nm.stdout.split())
        assert set(ENTRIES) <= exported
    assert switches.DEFAULTS["UCD_FUSED_FOCAL"] == "1" and "UCD_FUSED_FOCAL" in switches.snapshot()


_BUF = np.zeros(4096, dtype=np.float32)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("gamma,alpha,word", [(float("nan"), 1.0, "focal_gamma"), (-0.5, 1.0, "focal_gamma"),
                                              (float("inf"), 1.0, "focal_gamma"), (2.0, 0.0, "focal_alpha"),
                                              (2.0, -1.0, "focal_alpha"), (2.0, float("nan"), "focal_alpha")])
def test_entries_refuse_on_the_host(entry, gamma, alpha, word):
    """Host buffers: a call that got past its checks would fault, a refusal never touches them."""
    lib, b = hip.load(), _BUF.ctypes.data
    rc = getattr(lib, entry)(b, 4, None, 0, b, 1, 8, 8, 2, 2, 4, 2, 2, hip.KD_UNBIASED, 1.0, 255, 1.0, 0.0, None, gamma, alpha, b, b, 4,
                             b, 4096, None)
    msg = lib.ucd_last_error().decode()
    assert rc == hip.EINVAL and word in msg and entry in msg, (rc, msg)


def test_entries_keep_the_rules_of_the_calls_they_extend():
    lib, b = hip.load(), _BUF.ctypes.data
    for entry in ENTRIES:
        rc = getattr(lib, entry)(b, 4, None, 0, b, 1, 8, 8, 2, 2, 4, 2, 7, hip.KD_UNBIASED, 1.0, 255, 1.0, 0.0, None, 2.0, 1.0, b, b, 4, b,
                                 4096, None)
        assert rc == hip.EINVAL and "ce_old_cl" in lib.ucd_last_error().decode()
        rc = getattr(lib, entry)(None, 4, None, 0, b, 1, 8, 8, 2, 2, 4, 2, 2, hip.KD_UNBIASED, 1.0, 255, 1.0, 0.0, None, 0.0, 1.0, b, b, 4,
                                 b, 4096, None)
        assert rc == hip.EINVAL and "NULL" in lib.ucd_last_error().decode()


def test_composition_meets_the_reference_golden():
    """FocalLoss on the float64 up-sampled logits of make_kd_golden.unit_inputs against what the reference's class gave on them:
    loss rel 1e-6, gradient w.r.t. the low-resolution logits rel 1e-5 of its largest element (the file holds float32)."""
    import make_focal_golden as MF
    import make_kd_golden as MK
    gold = load_golden("focal_losses.npz")
    for shape in MK.UNIT_SHAPES:
        B, Ctot, K, h, H = shape
        sem, _, labels = MK.unit_inputs(shape)
        for gamma, alpha in MF.FOCAL:
            key = MF.focal_key(shape, gamma, alpha)
            s = sem.double().requires_grad_(True)
            up = F.interpolate(s, size=(H, H), mode="bilinear", align_corners=False)
            loss = FocalLoss(alpha=alpha, gamma=gamma)(up, labels)
            loss.backward()
            assert loss.item() == pytest.approx(float(gold[key + "|loss"][0]), rel=1e-6), key
            g = s.grad.numpy()
            if key + "|grad" in gold:
                g_r = gold[key + "|grad"].astype(np.float64)
                assert np.abs(g - g_r).max() <= 1e-5 * np.abs(g_r).max(), key
            else:
                gmax = float(np.abs(gold[key + "|grad::samples"]).max())
                assert_matches_compact(gold, key + "|grad", g, rtol=1e-5, atol=1e-5 * gmax)
            # sum reduction, and the definition written out
            total = FocalLoss(alpha=alpha, gamma=gamma, size_average=False)(up.detach(), labels)
            assert total.item() == pytest.approx(loss.item() * labels.numel(), rel=1e-12)
            assert R.focal_loss(sem.double(), labels, gamma, alpha)[0].item() == pytest.approx(loss.item(), rel=1e-12)


@pytest.mark.parametrize("gamma,alpha", [(2.0, 1.0), (0.5, 0.25), (3.5, 1.0), (0.0, 0.5)])
def test_composition_meets_the_definition_for_unbiased_ce_with_a_weight(gamma, alpha):
    import make_kd_golden as MK
    B, Ctot, K, h, H = shape = MK.UNIT_SHAPES[1]
    sem, _, labels = MK.unit_inputs(shape)
    weight = [0.25, 1.0]
    s = sem.double().requires_grad_(True)
    up = F.interpolate(s, size=(H, H), mode="bilinear", align_corners=False)
    ce = UnbiasedCrossEntropy(old_cl=K, ignore_index=255, reduction="none")(up, labels)
    loss = (focal_modulate(ce, gamma, alpha) * torch.tensor(weight, dtype=torch.float64).view(-1, 1, 1)).mean()
    loss.backward()
    r = sem.double().requires_grad_(True)
    ref, ce_r = R.focal_loss(r, labels, gamma, alpha, old_cl=K, weight=weight)
    ref.backward()
    assert torch.allclose(ce, ce_r, rtol=1e-12, atol=1e-14)
    assert loss.item() == pytest.approx(ref.item(), rel=1e-12)
    assert (s.grad - r.grad).abs().max().item() <= 1e-12 * r.grad.abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_zeros_give_finite_values_and_gradients(dtype):
    """gamma 0.5 on a map that holds exact zeros (ignored pixels, saturated pixels): 0^(gamma-1) * ce is never formed."""
    ce = torch.tensor([0.0, 0.0, 1e-30, 3e-9, 0.3, 2.0, 40.0, 0.0], dtype=dtype, requires_grad=True)
    for gamma in (0.5, 1.0, 2.0, 3.5):
        ce.grad = None
        f = focal_modulate(ce, gamma, 1.0)
        f.sum().backward()
        assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(ce.grad).all()), gamma
        assert f[0].item() == 0.0 and ce.grad[0].item() == 0.0 and f[7].item() == 0.0 and ce.grad[7].item() == 0.0
        big = ce.detach()[4:7].double()
        u = 1.0 - torch.exp(-big)
        assert torch.allclose(f.detach()[4:7].double(), u ** gamma * big, rtol=1e-5)
        assert torch.allclose(ce.grad[4:7].double(), u ** gamma + gamma * u ** (gamma - 1) * torch.exp(-big) * big, rtol=1e-5)
    ce.grad = None
    f = focal_modulate(ce, 0.0, 0.5)                              # gamma 0: alpha * ce, gradient alpha, zeros included
    f.sum().backward()
    assert torch.equal(f.detach(), 0.5 * ce.detach()) and bool((ce.grad == 0.5).all())


def test_argument_rules():
    ce = torch.zeros(3)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            focal_modulate(ce, bad, 1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            focal_modulate(ce, 2.0, bad)
        with pytest.raises(ValueError, match="alpha"):
            FocalLoss(alpha=bad)
    crit = FocalLoss()
    assert (crit.alpha, crit.gamma, crit.size_average, crit.ignore_index) == (1.0, 2.0, True, 255)


def test_cpu_trainer_uses_the_focal_criterion():
    """A step and a validation pass on the CPU: ce and the class loss are the focal criterion's mean of the run's own cross-entropy
    map (unbiased under --method UCD); the other terms are those of the run without the flag; --bce is refused."""
    plain, student0, _ = P._toy_trainer([])
    trainer, student, _ = P._toy_trainer(["--focal_loss", "--focal_loss_gamma", "0.5", "--focal_loss_alpha", "0.25"])
    assert trainer.focal == (0.5, 0.25) and plain.focal is None
    images, labels = P._toy_batch()
    r0 = plain.train_step(images, labels, torch.optim.SGD(student0.parameters(), lr=0.0))
    r = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    with torch.no_grad():
        ce_map = plain.criterion(student0(images)[0], labels)
    assert ce_map.mean().item() == pytest.approx(r0["ce"].item(), rel=1e-6)
    assert r["ce"].item() == pytest.approx(focal_modulate(ce_map, 0.5, 0.25).mean().item(), rel=1e-6)
    assert r["ce"].item() != r0["ce"].item() and r["lkd"].item() == r0["lkd"].item()
    assert any(not torch.equal(a.grad, b.grad) for a, b in zip(student.parameters(), student0.parameters()))

    class _Metrics:
        def reset(self): pass
        def update(self, labels, pred): pass
        def synch(self, dev): pass
        def get_results(self): return {}

    (class_loss, _), _, _ = trainer.validate([(images, labels)], _Metrics())
    (class_loss0, _), _, _ = plain.validate([(images, labels)], _Metrics())
    student0.eval()
    with torch.no_grad():
        ce_eval = plain.criterion(student0(images)[0], labels)
    assert class_loss0.item() == pytest.approx(ce_eval.mean().item(), rel=1e-6)
    assert class_loss.item() == pytest.approx(focal_modulate(ce_eval, 0.5, 0.25).mean().item(), rel=1e-6)
    from ucd_amd.train import Trainer
    opts = P._opts(["--focal_loss"])
    opts.bce = True
    with pytest.raises(NotImplementedError, match="--focal_loss"):
        Trainer(student, None, torch.device("cuda:0"), opts, classes=[16, 5])
