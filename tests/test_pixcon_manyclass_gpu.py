"""GPU: the contrastive loss with more teacher classes than the anchor block's probability rows fit the LDS for (fp32: K > 110,
the "wide" positives kernel that reads those rows from global memory) and past the fp16 path's former bound (K > 112), up to
the 254 classes a byte label allows - ADE 100-10 steps 2 .. 5 have K = 111 .. 141.  Reference: the float64 / float32 CPU
oracle, which has no class bound.  Bars: the ones tests/test_pixcon_gpu.py holds the two precisions to.

K = 111 and K = 113 are the first class counts on the new side of either threshold (K = 110 / 112 and below keep the launch they
had: tests/test_pixcon_plan_cpu.py); no path chunks the classes (the plan reports class_chunk = 0), so there is no chunk
boundary to place cases at."""
import pytest
import torch

from oracle import contrastive as OC
from ucd_amd import synth

pytestmark = pytest.mark.gpu

#        B  N   h   K    H    new ids                 max_label
CASES = [(2, 32, 9, 111, 144, list(range(111, 121)), 120),
         (2, 64, 12, 113, 192, list(range(113, 123)), 122),
         (2, 64, 12, 141, 192, list(range(141, 151)), 150),      # ADE 100-10 step 5
         (1, 32, 8, 254, 128, [254], 254)]                        # the last label below the padding value
IDS = ["K%d" % c[3] for c in CASES]
T = 0.07
_REF = {}


def _reference(case):
    """Inputs and the oracle's results of a case, computed once and shared (nothing below writes to them)."""
    if case[3] not in _REF:
        B, N, h, K, H, new_ids, max_label = case
        f_n, f_o, l_po, labels = synth.contrastive_case(3000 + N + h, B, N, h, h, K, H, H, new_ids)
        ref_in = f_n.clone().requires_grad_(True)
        prep = OC.pre_contrastive_pixel(ref_in, labels, l_po, f_o, max_label=max_label)
        ref = OC.pixcon_loss(prep["a"], prep["c"], prep["la"], prep["lc"], prep["P"], T)
        ref.backward()
        _, da, neg, G, num = OC.pixcon_loss_backward(prep["a"], prep["c"], prep["la"], prep["lc"], prep["P"], T)
        _REF[case[3]] = dict(inputs=(f_n, f_o, l_po, labels), prep=prep, loss=ref.item(), grad_in=ref_in.grad, da=da, neg=neg, num=num)
    return _REF[case[3]]


def _to_dev(r):
    dev = torch.device("cuda:0")
    f_n, f_o, l_po, labels = [t.to(dev) for t in r["inputs"]]
    return f_n.contiguous(memory_format=torch.channels_last), f_o, l_po, labels


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_are_not_degenerate(case):
    """Anchors, old contrast rows and several labels on both sides: teacher classes above the old bounds carry weight in P."""
    r = _reference(case)
    prep = r["prep"]
    A, C = prep["a"].shape[0], prep["c"].shape[0]
    assert A >= 64 and C - A >= 50 and len(torch.unique(prep["lc"])) >= 40, (A, C)
    assert (r["num"] > 0).sum().item() >= A - 1
    assert prep["P"].min().item() < 0.01 and prep["P"].max().item() > 0.99
    # P without the classes past the old bound (110 fp32, 112 fp16) is off by far more than any bar below
    bound = 112 if case[3] > 112 else 110
    P_cut = prep["pa"][:, :bound] @ prep["pc"][:, :bound].T
    free = ~((prep["la"] >= prep["min_new"])[:, None] & (prep["lc"] >= prep["min_new"])[None, :])
    assert ((P_cut - prep["P"]).abs() * free).max().item() > 1e-2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_prep_and_loss_vs_oracle(case):
    from ucd_amd import hip
    from ucd_amd.contrastive import pixcon_loss_raw, pixcon_prepare, ucd_contrastive_loss
    B, N, h, K, H, new_ids, max_label = case
    r = _reference(case)
    prep = r["prep"]
    assert hip.pixcon_loss_plan(B * h * h, K, "f32")["path"] == "f32/wide"
    fn_d, fo_d, lpo_d, lab_d = _to_dev(r)
    # integer side, unsorted order == oracle order
    pb = pixcon_prepare(fn_d, lab_d, lpo_d, fo_d, max_label=max_label, sort_by_label=False)
    m = pb.meta_host()
    assert (m.A, m.Co, m.min_new) == (int(prep["keep"].sum()), int(prep["keep_o"].sum()), prep["min_new"])
    keep_idx = torch.nonzero(prep["keep"])[:, 0].int()
    old_idx = torch.nonzero(prep["keep_o"])[:, 0].int()
    assert torch.equal(pb.anchor_pix[:m.A].cpu(), keep_idx)
    assert torch.equal(pb.old_pix[:m.Co].cpu(), old_idx)
    assert torch.equal(pb.row_label[:m.A].cpu().long(), prep["la"])
    assert torch.equal(pb.row_label[m.Apad:m.Apad + m.Co].cpu().long(), prep["lc"][m.A:])
    assert m.n_valid == int(((prep["la"].view(-1, 1) == prep["lc"].view(1, -1)).sum(1) - 1 > 0).sum())
    torch.testing.assert_close(pb.pcat[:m.A, :K].cpu(), prep["pa"], rtol=1e-5, atol=1e-7)
    # sorted order: same sets, grouped by label, stable
    pbs = pixcon_prepare(fn_d, lab_d, lpo_d, fo_d, max_label=max_label, sort_by_label=True)
    ms = pbs.meta_host()
    order = torch.argsort(prep["la"], stable=True)
    assert (ms.A, ms.Co, ms.min_new, ms.n_valid) == (m.A, m.Co, m.min_new, m.n_valid)
    assert torch.equal(pbs.anchor_pix[:ms.A].cpu(), keep_idx[order])
    assert torch.equal(pbs.row_label[:ms.A].cpu().long(), prep["la"][order])
    order_o = torch.argsort(prep["lc"][m.A:], stable=True)
    assert torch.equal(pbs.old_pix[:ms.Co].cpu(), old_idx[order_o])
    assert torch.equal(pbs.row_label[ms.Apad:ms.Apad + ms.Co].cpu().long(), prep["lc"][m.A:][order_o])
    # loss in both row orders
    for batch in (pb, pbs):
        loss_out, grad_a, stats = pixcon_loss_raw(batch, T, True, True, need_grad=True, row_stats=True)
        err = abs(loss_out[0].item() - r["loss"]) / abs(r["loss"])
        print("K", K, "sorted", batch.sorted, "loss rel err", err)
        assert err < 1e-4
        assert int(loss_out[1].item()) == m.n_valid
    # row sums and the anchor gradient, oracle order
    loss_out, grad_a, stats = pixcon_loss_raw(pb, T, True, True, need_grad=True, row_stats=True)
    torch.testing.assert_close(stats[0, :m.A].cpu().double(), r["neg"], rtol=1e-4, atol=0)
    torch.testing.assert_close(stats[1, :m.A].cpu().double(), r["num"], rtol=0, atol=0)
    da = r["da"]
    print("K", K, "grad_a max err / max", (grad_a[:m.A, :N].cpu().double() - da).abs().max().item() / da.abs().max().item())
    torch.testing.assert_close(grad_a[:m.A, :N].cpu().double(), da, rtol=1e-3, atol=1e-4 * da.abs().max().item())
    # the sorted batch's gradient is the same one, row for row
    _, grad_s, _ = pixcon_loss_raw(pbs, T, True, True, need_grad=True)
    torch.testing.assert_close(grad_s[:m.A, :N].cpu().double(), da[order], rtol=1e-3, atol=1e-4 * da.abs().max().item())
    # end to end through autograd
    x = fn_d.clone().requires_grad_(True)
    loss = ucd_contrastive_loss(x, lab_d, lpo_d, fo_d, T, max_label)
    loss.backward()
    assert abs(loss.item() - r["loss"]) / abs(r["loss"]) < 1e-4
    scale = r["grad_in"].abs().max().item()
    assert (x.grad.cpu() - r["grad_in"]).abs().max().item() / scale < 1e-3


@pytest.mark.parametrize("prec", ["f16", "f16_split"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp16_performance_mode_vs_oracle(case, prec):
    from ucd_amd import hip
    from ucd_amd.contrastive import pixcon_loss_raw, pixcon_prepare, ucd_contrastive_loss
    B, N, h, K, H, new_ids, max_label = case
    r = _reference(case)
    assert hip.pixcon_loss_plan(B * h * h, K, prec)["path"] == "f16/split"
    fn_d, fo_d, lpo_d, lab_d = _to_dev(r)
    da, neg = r["da"], r["neg"]
    for sort in (False, True):
        pb = pixcon_prepare(fn_d, lab_d, lpo_d, fo_d, max_label=max_label, sort_by_label=sort, fp16=True)
        loss_out, grad_a, stats = pixcon_loss_raw(pb, T, True, True, need_grad=True, row_stats=True, precision=prec)
        err = abs(loss_out[0].item() - r["loss"]) / abs(r["loss"])
        print("K", K, prec, "sorted", sort, "loss rel err", err)
        assert err < 1e-3
        m = pb.meta_host()
        order = torch.argsort(pb.anchor_pix[:m.A].cpu())                      # rows back to the oracle's pixel order
        torch.testing.assert_close(stats[0, :m.A].cpu().double()[order], neg, rtol=2e-3, atol=0)
        gerr = (grad_a[:m.A, :N].cpu().double()[order] - da).abs().max().item() / da.abs().max().item()
        print("K", K, prec, "sorted", sort, "grad err / max", gerr)
        assert gerr < 2e-3, gerr
    x = fn_d.clone().requires_grad_(True)
    loss = ucd_contrastive_loss(x, lab_d, lpo_d, fo_d, T, max_label, prec)
    loss.backward()
    assert abs(loss.item() - r["loss"]) / abs(r["loss"]) < 1e-3
    scale = r["grad_in"].abs().max().item()
    assert (x.grad.cpu() - r["grad_in"]).abs().max().item() / scale < 2e-3


def test_reference_shaped_entry_points_at_141_classes():
    """pre_contractive_pixel(materialize_P=True) -> (a, c, la, lc, P) and PixelConLossV2 on it, K = 141: the returned P against the
    oracle's, and the loss / input gradient of the fused kernel behind the tuple (pixel-order rows, P formed in-tile)."""
    from ucd_amd.contrastive import PixelConLossV2, pre_contractive_pixel
    case = CASES[2]
    B, N, h, K, H, new_ids, max_label = case
    r = _reference(case)
    prep = r["prep"]
    fn_d, fo_d, lpo_d, lab_d = _to_dev(r)
    x = fn_d.clone().requires_grad_(True)
    tup = pre_contractive_pixel(x, lab_d, l_po=lpo_d, f_o=fo_d, max_label=max_label, materialize_P=True)
    a, c, la, lc, P = tup
    assert torch.equal(la.cpu().long() & 0xFF, prep["la"]) and torch.equal(lc.cpu().long() & 0xFF, prep["lc"])
    torch.testing.assert_close(a.detach().cpu(), prep["a"].detach().float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c.cpu(), prep["c"].detach().float(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(P.cpu(), prep["P"].float(), rtol=1e-4, atol=1e-6)
    crit = PixelConLossV2(temperature=T)
    loss = crit(tup)
    assert abs(loss.item() - r["loss"]) / abs(r["loss"]) < 1e-4
    loss.backward()
    scale = r["grad_in"].abs().max().item()
    assert (x.grad.cpu() - r["grad_in"]).abs().max().item() / scale < 1e-3
    # the five tensors unpacked, as the reference's trainer passes them: same kernel, found through the anchors tensor
    assert abs(crit(a, c, la, lc, P).item() - r["loss"]) / abs(r["loss"]) < 1e-4
    # foreign tensors with the same values: ucd_pixcon_loss_given_p reads the materialised P
    lf = crit(a.detach().clone(), c.clone(), la.clone(), lc.clone(), P.clone())
    assert abs(lf.item() - r["loss"]) / abs(r["loss"]) < 1e-4
