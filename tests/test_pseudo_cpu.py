"""CPU: the host half of PLOP's pseudo-labelling (``--pseudo entropy``; csrc/pseudo_label.hip, ucd_amd.loss.fused_pseudo_labels) -
the symbols, the library's refusals on host buffers, the plan, the interpolated median, the torch composition against the float64
reference (tests/pseudo_ref.py), the command line and a Trainer on a small CPU network."""
import numpy as np
import pytest
import torch

import pseudo_ref as R
import test_pod_cpu as P
from ucd_amd import argparser, hip, switches
from ucd_amd.loss import fused_pseudo_labels, pseudo_hist, pseudo_labels_torch, pseudo_median


def test_names_are_registered():
    assert {"ucd_pseudo_plan", "ucd_pseudo_hist", "ucd_pseudo_label", "ucd_seg_losses_ex_w", "ucd_seg_losses_gather_w"} <= set(hip.SIGNATURES)
    lib = hip.load()
    for name in ("ucd_pseudo_plan", "ucd_pseudo_hist", "ucd_pseudo_label", "ucd_seg_losses_ex_w", "ucd_seg_losses_gather_w"):
        assert getattr(lib, name) is not None
    assert switches.DEFAULTS["UCD_FUSED_PSEUDO"] == "1" and "UCD_FUSED_PSEUDO" in switches.snapshot()


# ---- refusals: host buffers - a call that got past its checks would fault, a refusal never touches them -----------------------------
_BUF = np.zeros(4096, dtype=np.float32)


def _p(v):
    return _BUF.ctypes.data if v == "ok" else v


def _label_rc(sem_t="ok", ld_t=4, labels="ok", B=1, H=8, W=8, h=2, w=2, K=4, thr="ok", f_min=0.0, out="other", counts="ok", factor="ok"):
    out = _BUF.ctypes.data + 2048 if out == "other" else _p(out)
    return hip.load().ucd_pseudo_label(_p(sem_t), ld_t, _p(labels), B, H, W, h, w, K, 255, _p(thr), f_min, out, _p(counts), _p(factor),
                                       None, None)


def _hist_rc(sem_t="ok", ld_t=4, labels="ok", B=1, H=8, W=8, h=2, w=2, K=4, bins=100, hist="ok"):
    return hip.load().ucd_pseudo_hist(_p(sem_t), ld_t, _p(labels), B, H, W, h, w, K, 255, bins, _p(hist), None)


@pytest.mark.parametrize("kwargs,code,word", [
    (dict(sem_t=None), hip.EINVAL, "sem_t"), (dict(labels=None), hip.EINVAL, "labels"), (dict(thr=None), hip.EINVAL, "thresholds"),
    (dict(out=None), hip.EINVAL, "labels_out"), (dict(counts=None), hip.EINVAL, "counts"), (dict(factor=None), hip.EINVAL, "factor"),
    (dict(out="ok"), hip.EINVAL, "alias"), (dict(B=0), hip.EINVAL, "B"), (dict(H=0), hip.EINVAL, "H"), (dict(h=0), hip.EINVAL, "h"),
    (dict(K=0), hip.EINVAL, "K"), (dict(h=9), hip.EINVAL, "smaller"), (dict(w=9), hip.EINVAL, "smaller"), (dict(ld_t=3), hip.EINVAL, "ld_t"),
    (dict(f_min=-0.1), hip.EINVAL, "f_min"), (dict(f_min=1.5), hip.EINVAL, "f_min"), (dict(f_min=float("nan")), hip.EINVAL, "f_min"),
    (dict(h=8, w=8, K=338, ld_t=338), hip.EUNSUPPORTED, "164076"),
])
def test_label_call_refuses_on_the_host(kwargs, code, word):
    assert _label_rc(**kwargs) == code
    assert word in hip.load().ucd_last_error().decode()


@pytest.mark.parametrize("kwargs,code,word", [
    (dict(hist=None), hip.EINVAL, "hist"), (dict(sem_t=None), hip.EINVAL, "sem_t"), (dict(bins=1), hip.EINVAL, "bins"),
    (dict(bins=0), hip.EINVAL, "bins"), (dict(bins=1025), hip.EINVAL, "bins"), (dict(W=0), hip.EINVAL, "W"),
    (dict(ld_t=3), hip.EINVAL, "ld_t"), (dict(B=70000), hip.EINVAL, "B"),
])
def test_hist_call_refuses_on_the_host(kwargs, code, word):
    assert _hist_rc(**kwargs) == code
    assert word in hip.load().ucd_last_error().decode()


def test_weighted_loss_entries_refuse_like_the_entries_they_extend():
    lib, b = hip.load(), _BUF.ctypes.data
    tail = (1, 8, 8, 2, 2, 4, 2, 2, hip.KD_UNBIASED, 1.0, 255, 1.0, 1.0, b)
    assert lib.ucd_seg_losses_ex_w(None, 4, b, 2, b, *tail, b, b, 4, b, 1 << 20, None) == hip.EINVAL
    assert "ucd_seg_losses_ex_w" in lib.ucd_last_error().decode()
    assert lib.ucd_seg_losses_gather_w(b, 3, b, 2, b, *tail, b, b, 4, b, 1 << 20, None) == hip.EINVAL
    assert "ucd_seg_losses_gather_w" in lib.ucd_last_error().decode() and "ld_s" in lib.ucd_last_error().decode()


def test_plan():
    """VOC at 513 / 33, ADE at --output_stride 8 with the 141 classes of its last 100-10 step, and factor 1 with the most classes."""
    voc = hip.pseudo_plan(513, 513, 33, 33, 16, 100)
    assert voc == {"tile": (64, 64), "grid": (9, 9), "threads": 256, "lds_bytes": 7 * 7 * 17 * 4 + 16 * 100 * 4, "lds_hist": True}
    assert hip.pseudo_plan(513, 513, 33, 33, 16)["lds_bytes"] == 7 * 7 * 17 * 4 + 8
    ade = hip.pseudo_plan(512, 512, 64, 64, 141, 100)
    assert ade["tile"] == (64, 64) and ade["lds_bytes"] == 11 * 11 * 141 * 4 + 141 * 100 * 4 and ade["lds_hist"]
    one = hip.pseudo_plan(32, 32, 32, 32, 255, 100)
    assert one["tile"] == (8, 8) and one["threads"] == 64 and one["grid"] == (4, 4) and not one["lds_hist"]
    assert one["lds_bytes"] == 11 * 11 * 255 * 4 <= 160 * 1024
    # the tile shrinks one halving at a time, y first
    assert hip.pseudo_plan(64, 64, 64, 64, 4)["tile"] == (64, 64) and hip.pseudo_plan(64, 64, 64, 64, 16)["tile"] == (32, 64)
    assert hip.pseudo_plan(64, 64, 64, 64, 30)["tile"] == (32, 32) and hip.pseudo_plan(64, 64, 64, 64, 40)["tile"] == (16, 32)
    with pytest.raises(RuntimeError, match="164076 bytes"):
        hip.pseudo_plan(32, 32, 32, 32, 338)


# ---- the median ---------------------------------------------------------------------------------------------------------------------
def test_median_on_crafted_histograms():
    hist = np.zeros((5, 10), dtype=np.int64)
    hist[1, 3] = 8                              # a single bin: its middle
    hist[2, 2], hist[2, 7] = 5, 5               # mass split exactly in half between two bins: the upper edge of the first
    hist[3] = np.arange(10)                     # a ramp
    hist[4, 0] = 1                              # one pixel in the first bin
    got = pseudo_median(hist, 0.001)
    assert got.dtype == np.float64 and got.shape == (5,)
    assert got[0] == 0.001                      # an empty class gets the floor
    assert got[1] == 0.35 and got[2] == 0.3 and got[4] == 0.05
    assert np.array_equal(got, R.median(hist, 0.001))
    # against the definition on expanded samples: half of the mass lies below the median
    cum = np.cumsum(hist[3])
    j = int(got[3] * 10)
    assert cum[j - 1] + (got[3] * 10 - j) * hist[3, j] == pytest.approx(hist[3].sum() / 2)
    # the floor is honoured, for a class with mass too
    assert np.array_equal(pseudo_median(hist, 0.32), np.array([0.32, 0.35, 0.32, max(got[3], 0.32), 0.32]))
    assert np.array_equal(pseudo_median(torch.from_numpy(hist), 0.001), got)
    g = np.random.default_rng(3).integers(0, 50, size=(7, 100))
    assert np.array_equal(pseudo_median(g, 0.001), R.median(g, 0.001))


# ---- the torch composition (CPU tensors; the A/B arm of UCD_FUSED_PSEUDO) against the reference ------------------------------------
@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("geo", [(5, 5, 65, 65), (9, 12, 33, 47), (32, 32, 32, 32)])
def test_torch_composition_matches_the_reference(K, geo):
    c = R.case(K, *geo)
    z32 = c.z.float()
    out, factor, counts = fused_pseudo_labels(z32, c.labels, torch.from_numpy(c.thresholds).float(), 0.0)       # CPU: the composition
    assert int(((out != c.labels_out) & ~c.loose).sum()) == 0
    assert torch.equal(counts[:, 1].long(), c.den) and bool(((counts[:, 0].long() - c.num).abs() <= c.loose.flatten(1).sum(1)).all())
    want = counts[:, 0].double() / (counts[:, 1].double() + 1e-6)
    assert torch.equal(factor, want.float())
    hist = pseudo_hist(z32, c.labels, torch.zeros(K, 100, dtype=torch.int64))
    assert hist.sum().item() == c.cand.sum().item() and int((hist - c.hist).abs().sum()) <= 2 * int((c.bin_loose | c.tie).sum())
    # float64 logits: the reference itself
    out64, _, counts64 = pseudo_labels_torch(c.z, c.labels, torch.from_numpy(c.thresholds))
    assert torch.equal(out64, c.labels_out) and torch.equal(counts64[:, 0].long(), c.num)


def test_argument_rules():
    z, lab = torch.zeros(2, 4, 3, 3), torch.zeros(2, 9, 9, dtype=torch.int64)
    with pytest.raises(ValueError, match="thresholds"):
        fused_pseudo_labels(z, lab, torch.zeros(3))
    with pytest.raises(ValueError, match="int64"):
        fused_pseudo_labels(z, lab.int(), torch.zeros(4))
    with pytest.raises(ValueError, match="smaller"):
        fused_pseudo_labels(z, lab[:, :2], torch.zeros(4))
    with pytest.raises(ValueError, match="f_min"):
        fused_pseudo_labels(z, lab, torch.zeros(4), 1.5)
    with pytest.raises(ValueError, match="bins"):
        pseudo_hist(z, lab, torch.zeros(4, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="hist"):
        pseudo_hist(z, lab, torch.zeros(3, 10, dtype=torch.int64))


# ---- command line and trainer ------------------------------------------------------------------------------------------------------
def _parse(args):
    return argparser.modify_command_options(argparser.get_argparser().parse_args(["--task", "15-5", "--step", "1"] + list(args)))


def test_parser():
    o = _parse(["--method", "UCD"])
    assert (o.pseudo, o.pseudo_threshold, o.pseudo_nb_bins, o.pseudo_adaptive, o.pseudo_adaptive_min) == (None, 0.001, 100, False, 0.0)
    o = _parse(["--method", "PLOP"])
    assert (o.pseudo, o.pseudo_adaptive, o.pod_factor, o.pod_last_factor, o.init_balanced) == ("entropy", True, 0.01, 0.0005, True)
    assert (o.loss_kd, o.unce, o.unkd, o.pixcon_weight) == (0.0, False, False, 0.0)        # plain CE, no KD, no contrastive term
    o = _parse(["--method", "UCD", "--pseudo", "entropy", "--pseudo_nb_bins", "1024", "--pseudo_threshold", "0.01"])
    assert (o.pseudo, o.pseudo_nb_bins, o.pseudo_threshold, o.loss_kd) == ("entropy", 1024, 0.01, 10)
    for bad in ("1", "1025", "0"):
        with pytest.raises(SystemExit):
            _parse(["--pseudo_nb_bins", bad])
    with pytest.raises(SystemExit):
        _parse(["--pseudo", "softmax"])
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit):
            _parse(["--pseudo_adaptive_min", bad])
    assert _parse(["--pseudo_adaptive_min", "1"]).pseudo_adaptive_min == 1.0
    for combo in (["--bce"], ["--icarl"], ["--method", "LWF-MC"]):
        with pytest.raises(ValueError, match="--pseudo"):
            _parse(combo + ["--pseudo", "entropy"])


def _loader():
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(2, 3, 36, 44, generator=g), torch.randint(0, 21, (2, 36, 44), generator=g)) for _ in range(2)]


def test_trainer_thresholds_state_and_the_flag_off():
    trainer, student, teacher = P._toy_trainer(["--pseudo", "entropy", "--pseudo_adaptive", "--pseudo_nb_bins", "50"])
    assert trainer.pseudo_flag and trainer.pseudo_thresholds is None
    images, labels = P._toy_batch()
    with pytest.raises(RuntimeError, match="find_pseudo_thresholds"):
        trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    loader = _loader()
    got = trainer.find_pseudo_thresholds(loader)
    # the reference: float64 histogram of the same teacher logits
    hist = torch.zeros(16, 50, dtype=torch.int64)
    loose = 0
    with torch.no_grad():
        for x, y in loader:
            sem = teacher(x)[1]["sem"]
            cand, arg, u, gap = R.view(sem.double(), y)
            hist += R.histogram(cand, arg, u, 16, 50)
            ub = u * 50
            loose += int((cand & (((ub - ub.round()).abs() < R.MARGIN * 50) | (gap < R.MARGIN))).sum())
    assert trainer.pseudo_hist.sum().item() == hist.sum().item()
    assert int((trainer.pseudo_hist - hist).abs().sum()) <= 2 * loose
    if loose == 0:
        assert np.array_equal(got, R.median(hist.numpy(), 0.001))
    assert np.allclose(got, R.median(hist.numpy(), 0.001), atol=2 * loose / max(hist.sum(1).min().item(), 1) / 50 + 1e-12)
    assert torch.equal(trainer.pseudo_thresholds, torch.from_numpy(got).float())
    # a step: the cross entropy moved, the share of kept candidates is a proper fraction
    r = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    assert 0.0 < r["pseudo_kept"].item() < 1.0
    plain, student0, _ = P._toy_trainer([])
    r0 = plain.train_step(images, labels, torch.optim.SGD(student0.parameters(), lr=0.0))
    assert r["ce"].item() != r0["ce"].item() and r["lkd"].item() == r0["lkd"].item()
    # by hand: the composition's labels and factor on the reduction='none' map
    with torch.no_grad():
        sem_t = teacher(images)[1]["sem"]
        lab2, f, _ = pseudo_labels_torch(sem_t, labels, trainer.pseudo_thresholds, 0.0)
        ce_map = plain.criterion(student0(images)[0], lab2)
    assert r["ce"].item() == pytest.approx((ce_map * f.view(-1, 1, 1)).mean().item(), rel=1e-6)
    # the state round-trips; the flag off (or no teacher) is the plain trainer, bit for bit
    state = trainer.state_dict()
    other, _, _ = P._toy_trainer(["--pseudo", "entropy"])
    other.load_state_dict(state)
    assert torch.equal(other.pseudo_thresholds, trainer.pseudo_thresholds) and torch.equal(other.pseudo_hist, trainer.pseudo_hist)
    # new thresholds go into the tensor a captured step would read by address
    held = trainer.pseudo_thresholds
    trainer.load_state_dict({"regularizer": None, "pseudo": {"thresholds": state["pseudo"]["thresholds"] * 0.5, "hist": state["pseudo"]["hist"]}})
    assert trainer.pseudo_thresholds is held and torch.equal(held, other.pseudo_thresholds * 0.5)
    trainer.find_pseudo_thresholds(loader)
    assert trainer.pseudo_thresholds is held and torch.equal(held, other.pseudo_thresholds)
    assert "pseudo" not in plain.state_dict() and plain.pseudo_flag is False and "pseudo_kept" not in r0
    plain.load_state_dict(state)                                        # a state with thresholds does not disturb a run without the flag
    assert plain.pseudo_thresholds is None
    off, student1, _ = P._toy_trainer(["--pseudo_threshold", "0.5"])
    r1 = off.train_step(images, labels, torch.optim.SGD(student1.parameters(), lr=0.0))
    assert all(torch.equal(r1[k], r0[k]) for k in r0) and set(r1) == set(r0)
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(student1.parameters(), student0.parameters()))
    from ucd_amd.train import Trainer
    assert Trainer(student, None, torch.device("cpu"), P._opts(["--pseudo", "entropy"]), classes=[16, 5]).pseudo_flag is False


def test_the_lds_bound_holds_the_exact_footprint():
    """The plan sizes the staged cells with (tile h / H + 3) per axis; the kernels index them with the exact span of
    upsample_index.h (restated here in float32): the span never exceeds the bound, over every tile of these geometries."""
    f = np.float32

    def src(dst, n, scale):
        s = max(f(f(scale) * f(f(dst) + f(0.5))) - f(0.5), f(0))
        i0 = min(int(s), n - 1)
        return i0, i0 + (1 if i0 < n - 1 else 0)

    def span(t0, tile, out, n, scale):
        return src(min(t0 + tile, out) - 1, n, scale)[1] - src(t0, n, scale)[0] + 1

    for H, W, h, w in [(65, 65, 5, 5), (33, 47, 9, 12), (32, 32, 32, 32), (513, 513, 33, 33), (512, 512, 64, 64), (129, 129, 17, 17),
                       (100, 37, 99, 36), (1000, 1000, 999, 7)]:
        for K in (1, 16, 101, 255, 337):
            plan = hip.pseudo_plan(H, W, h, w, K)
            ty, tx = plan["tile"]
            by, bx = int(f(ty * f(h)) / f(H)) + 3, int(f(tx * f(w)) / f(W)) + 3
            assert plan["lds_bytes"] == by * bx * (K | 1) * 4 + 8
            assert max(span(t, ty, H, h, f(h) / f(H)) for t in range(0, H, ty)) <= by
            assert max(span(t, tx, W, w, f(w) / f(W)) for t in range(0, W, tx)) <= bx
