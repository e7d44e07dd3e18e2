"""GPU: ucd_seg_views (csrc/seg_views.hip) - bilinear up-sampling of every view, per-view soft-max, fusion by mean / max / voting,
arg-max and the confusion matrix in one kernel - against a float64 yardstick that is torch on the CPU:

    u_v = F.interpolate(sem_v.double(), size=(H, W), mode="bilinear", align_corners=False), .flip(-1) for a mirrored view
    P_v = u_v.softmax(1);  score = sum_v P_v | max_v P_v | number of views whose arg-max is the class;  argmax: first maximum

A pixel is left out of the comparison where the yardstick itself is undecided: for mean and max where the float64 gap between the
two best scores is below 1e-5, for voting where any view's two best up-sampled logits are closer than 1e-4.  Everything else must
match exactly, pred and histogram alike (the histogram against the yardstick's over the kept pixels plus the kernel's own pairs on
the left-out ones); at most 0.5 % of the pixels may be left out.  Logits are N(0, 3^2), torch.manual_seed(0)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from ucd_amd import hip
from ucd_amd.metrics import StreamSegMetrics

pytestmark = pytest.mark.gpu

RULES = ("mean", "max", "voting")
CAP = 0.005
# name -> B, H, W, Ctot, n_classes, [(h, w, mirrored)]
CASES = {
    # edge tiles, non-integer factors, the LDS histogram
    "voc21": (2, 70, 93, 21, 21, [(h, w, f) for h, w in ((3, 4), (5, 6), (8, 11)) for f in (False, True)]),
    # the global histogram, more classes than a wave has lanes
    "ade151": (1, 64, 96, 151, 151, [(h, w, f) for h, w in ((4, 6), (7, 9)) for f in (False, True)]),
    # 151 classes at factors 2 and 4: the plan walks down to a 16 x 16 pixel tile or below
    "ade151_small_tile": (1, 64, 96, 151, 151, [(32, 48, False), (16, 24, True), (32, 48, True)]),
    # a 21-class map scored against 16 classes: predictions >= n are not counted
    "voc21_vs16": (2, 70, 93, 21, 16, [(5, 6, False), (8, 11, True)]),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and what the float64 yardstick needs of them, computed once: the per-view probabilities' sum and maximum,
    the votes, and the smallest gap between the two best logits over the views."""
    B, H, W, Ctot, n, views = CASES[name]
    torch.manual_seed(0)
    sems = [torch.randn(B, Ctot, h, w) * 3 for h, w, _ in views]
    labels = torch.randint(0, n, (B, H, W))
    labels[torch.rand(B, H, W) < 0.1] = 255                       # ignored
    labels[torch.rand(B, H, W) < 0.05] = n + 2                    # above the classes: not counted
    labels[torch.rand(B, H, W) < 0.02] = -1
    mean = torch.zeros(B, Ctot, H, W, dtype=torch.float64)
    mx = torch.zeros_like(mean)
    votes = torch.zeros_like(mean)
    logit_gap = torch.full((B, H, W), float("inf"), dtype=torch.float64)
    for sem, (_, _, flip) in zip(sems, views):
        u = F.interpolate(sem.double(), size=(H, W), mode="bilinear", align_corners=False)
        if flip:
            u = u.flip(-1)
        p = u.softmax(1)
        mean += p
        mx = torch.maximum(mx, p)
        votes.scatter_add_(1, u.argmax(1, keepdim=True), torch.ones(B, 1, H, W, dtype=torch.float64))
        top = u.topk(2, dim=1).values
        logit_gap = torch.minimum(logit_gap, top[:, 0] - top[:, 1])
    ref = {}
    for rule, score in (("mean", mean), ("max", mx), ("voting", votes)):
        top = score.topk(2, dim=1).values
        undecided = (logit_gap < 1e-4) if rule == "voting" else (top[:, 0] - top[:, 1] < 1e-5)
        ref[rule] = (score.argmax(1), undecided)
    return sems, [f for _, _, f in views], labels, ref


def _hist(labels, pred, n, mask):
    ok = mask & (labels >= 0) & (labels < n) & (pred < n)
    return torch.bincount(n * labels[ok] + pred[ok], minlength=n * n).reshape(n, n)


def _check(name, rule, got_pred, got_hist):
    B, H, W, Ctot, n, views = CASES[name]
    _, _, labels, ref = _case(name)
    ref_pred, undecided = ref[rule]
    share = undecided.double().mean().item()
    print(f"{name} / {rule}: {100 * share:.4f} % of {undecided.numel()} pixels left out")
    assert share <= CAP
    kept = ~undecided
    got_pred = got_pred.cpu()
    assert torch.equal(got_pred[kept], ref_pred[kept]), f"{(got_pred[kept] != ref_pred[kept]).sum().item()} kept pixels differ"
    want = _hist(labels, ref_pred, n, kept) + _hist(labels, got_pred, n, undecided)
    assert torch.equal(got_hist.cpu().long(), want)
    assert int(want.sum()) > 0


def _run(name, rule, with_pred=True):
    B, H, W, Ctot, n, views = CASES[name]
    sems, flips, labels, _ = _case(name)
    dev = torch.device("cuda:0")
    m = StreamSegMetrics(n)
    pred = torch.full((B, H, W), -7, dtype=torch.int64, device=dev) if with_pred else None
    m.update_from_views(labels.to(dev), [s.to(dev) for s in sems], flips, fusion=rule, pred=pred)
    assert m.total_samples == B and m.confusion_matrix.is_cuda and m.confusion_matrix.dtype == torch.float64
    return pred, m.confusion_matrix


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", ["voc21", "ade151", "ade151_small_tile", "voc21_vs16"])
def test_fused_views_match_the_float64_yardstick(name, rule):
    B, H, W, Ctot, n, views = CASES[name]
    plan = hip.seg_views_plan(H, W, views, Ctot, n)
    print(name, plan)
    if name == "ade151_small_tile":
        assert plan["tile_y"] * plan["tile_x"] <= 256
    pred, hist = _run(name, rule)
    assert int(pred.min()) >= 0 and int(pred.max()) < Ctot
    _check(name, rule, pred, hist)


@pytest.mark.parametrize("rule", RULES)
def test_a_padded_leading_dimension_changes_nothing(rule):
    """ld > Ctot through the C ABI: rows of 24 floats with 21 classes, the padding filled with a value that would win every arg-max."""
    name = "voc21_vs16"
    B, H, W, Ctot, n, views = CASES[name]
    sems, flips, labels, _ = _case(name)
    dev = torch.device("cuda:0")
    rows = []
    for s in sems:
        buf = torch.full((s.shape[0] * s.shape[2] * s.shape[3], 24), 1e6, dtype=torch.float32, device=dev)
        buf[:, :Ctot] = s.to(dev).permute(0, 2, 3, 1).reshape(-1, Ctot)
        rows.append(buf[:, :Ctot])
        assert rows[-1].stride(0) == 24
    hist = torch.zeros(n, n, dtype=torch.int64, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    hip.seg_views(rows, [(h, w) for h, w, _ in views], flips, labels.to(dev), Ctot, n, rule, hist, pred)
    dense_pred, dense_hist = _run(name, rule)
    assert torch.equal(pred, dense_pred) and torch.equal(hist.double(), dense_hist)
    _check(name, rule, pred, hist)
    assert int((pred >= n).sum()) > 0                    # the case does hold predictions outside the scored classes


def test_voting_over_the_plain_view_is_the_confusion_kernel():
    """One plain view: every rule's arg-max is the view's; voting takes it from the logits alone, with seg_confusion_kernel's
    expression - pred and matrix of update_from_logits, bit for bit."""
    B, H, W, Ctot = 2, 129, 129, 21
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sem = (torch.randn(B, Ctot, 9, 9) * 3).to(dev)
    sem[0, :, 2, 3] = 0.0                                # all-equal logits: the first maximum
    sem[1, 7, 4:6, 4:6] = sem[1, 3, 4:6, 4:6]            # two classes with the same bits
    labels = torch.randint(0, Ctot, (B, H, W), device=dev)
    labels[:, ::7, ::5] = 255
    a, b = StreamSegMetrics(Ctot), StreamSegMetrics(Ctot)
    pa = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    pb = torch.empty_like(pa)
    a.update_from_logits(labels, sem, pred=pa)
    b.update_from_views(labels, [sem], [False], fusion="voting", pred=pb)
    assert torch.equal(pa, pb) and torch.equal(a.confusion_matrix, b.confusion_matrix)
    assert a.total_samples == b.total_samples == B


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", ["voc21", "ade151"])
def test_two_calls_give_the_same_bits(name, rule):
    p1, h1 = _run(name, rule)
    p2, h2 = _run(name, rule)
    _, h3 = _run(name, rule, with_pred=False)
    assert torch.equal(p1, p2) and torch.equal(h1, h2) and torch.equal(h1, h3)


def test_histogram_accumulates_and_bad_arguments_are_refused():
    name = "voc21"
    B, H, W, Ctot, n, views = CASES[name]
    sems, flips, labels, _ = _case(name)
    dev = torch.device("cuda:0")
    m = StreamSegMetrics(n)
    dsems = [s.to(dev) for s in sems]
    m.update_from_views(labels.to(dev), dsems, flips)
    once = m.confusion_matrix.clone()
    m.update_from_views(labels.to(dev), dsems, flips)
    assert torch.equal(m.confusion_matrix, 2 * once) and m.total_samples == 2 * B
    with pytest.raises(ValueError, match="pred must be"):
        m.update_from_views(labels.to(dev), dsems, flips, pred=torch.empty(B, H, W, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="one flip per view"):
        m.update_from_views(labels.to(dev), dsems, flips[:-1])
    with pytest.raises(RuntimeError, match="UCD_EINVAL|code -1"):
        m.update_from_views(labels.to(dev), dsems * 3, flips * 3)               # 18 views
