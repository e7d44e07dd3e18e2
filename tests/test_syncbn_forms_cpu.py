"""CPU: the float64 reference of the multi-rank norm forms (oracle/syncbn_forms.py) against the existing restatement of the
combination (oracle/syncbn.py), against float64 autograd through batch norm over the concatenated batch, and - the reason a pass
of tests/test_syncbn_forms_gpu.py means something - against itself with each of the four mistakes a multi-rank kernel sequence
can make: every quantity the mistake should move differs by at least ten times the bar the GPU tests hold it to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import syncbn_forms as R
from oracle.syncbn import combine_rank_moments

STEM_SHAPES = [(2, 64, 9, 11), (1, 64, 8, 8)]
SLOPES = {"leaky_relu": R.SLOPE, "identity": 1.0}


def _d(ts):
    return [t.double() for t in ts]


@pytest.fixture(scope="module")
def conv():
    case = R.conv_case()
    case.update(R.link_case(case))
    return case


@pytest.fixture(scope="module", params=[(s, a) for s in STEM_SHAPES for a in SLOPES])
def stem(request):
    shape, act = request.param
    return R.stem_case(shape, SLOPES[act]), SLOPES[act]


def test_combination_agrees_with_the_oracle_and_the_concatenated_batch(conv):
    rows = _d(conv["ys"])
    M = conv["M"]
    packs = [R.rank_pack(x) for x in rows]
    mean, m2 = R.combine(packs, M)
    gathered = np.stack([np.stack([p[0].numpy(), p[1].numpy()]) for p in packs])
    om, ov, om2 = combine_rank_moments(gathered, M)
    np.testing.assert_allclose(mean.numpy(), om, rtol=1e-12, atol=0)
    np.testing.assert_allclose(m2.numpy(), om2, rtol=1e-12, atol=0)
    np.testing.assert_allclose((m2 / (R.WORLD * M)).numpy(), ov, rtol=1e-12, atol=0)
    full = torch.cat(rows)
    torch.testing.assert_close(mean, full.mean(0), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(m2 / (R.WORLD * M), full.var(0, unbiased=False), rtol=1e-12, atol=0)
    # the inputs are what the issue asks for: the between-rank term is most of the variance, no ill-conditioned channel
    within = torch.stack([p[1] for p in packs]).sum(0)
    assert ((m2 - within) / m2).min() > 0.5
    assert (full.mean(0).abs() / full.std(0)).max() < 5


@pytest.mark.parametrize("act", list(SLOPES))
def test_reference_equals_autograd_through_batch_norm_of_the_concatenated_batch(conv, act):
    slope = SLOPES[act]
    rows, dys = _d(conv["ys"]), _d(conv["dys"])
    w, b, rm, rv = (conv[n].double() for n in ("weight", "bias", "running_mean", "running_var"))
    k = R.forward_constants(rows, w, rm, rv)
    full = torch.cat(rows).requires_grad_(True)
    gamma = (w.abs() + R.EPS).requires_grad_(True)
    beta = b.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    out = F.leaky_relu(F.batch_norm(full, rm_t, rv_t, gamma, beta, True, R.MOMENTUM, R.EPS), slope)
    out.backward(torch.cat(dys))
    torch.testing.assert_close(k["running_mean"], rm_t, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(k["running_var"], rv_t, rtol=1e-12, atol=1e-13)
    pres = [R.apply_rows(x, k, b, slope) for x in rows]
    torch.testing.assert_close(torch.cat([p[1] for p in pres]), out.detach(), rtol=1e-11, atol=1e-12)
    dzs = [dy * R.act_grad(p[0], slope) for dy, p in zip(dys, pres)]
    bw = R.backward_rows(rows, dzs, k, w)
    torch.testing.assert_close(torch.cat(bw["dx"]), full.grad, rtol=1e-9, atol=1e-11)
    sign = torch.where(w < 0, -1.0, 1.0).double()
    torch.testing.assert_close(torch.stack([l[0] for l in bw["local"]]).sum(0), beta.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(torch.stack([l[1] for l in bw["local"]]).sum(0), gamma.grad * sign, rtol=1e-10, atol=1e-9)
    assert sign[R.NEG_CHANNEL] == -1 and sign.sum() == len(sign) - 2


def test_stem_inputs_have_no_tie_and_no_ill_conditioned_channel(stem):
    case, slope = stem
    zs = _d(case["zs"])
    k = R.stem_forward(zs, *(case[n].double() for n in ("weight", "bias", "running_mean", "running_var")), slope)
    for pre in k["pre"]:
        margin, _ = R.window_margin(R.act_fn(pre, slope))
        assert margin.min() >= 2                     # no tie in the bf16 activation, and none a last fp32 bit away
        assert pre.abs().min() >= 1e-3
    full = torch.cat([R.rows_of(z) for z in zs])
    assert (full.mean(0).abs() / full.std(0)).max() < 5
    # the pool's decision on the rounded map is max_pool2d's
    for pre, idx in zip(k["pre"], k["idx"]):
        _, ti = F.max_pool2d(R.bf16_round(R.act_fn(pre, slope)), 3, 2, 1, return_indices=True)
        assert torch.equal(ti.flatten(2), idx)


def _moved(true, wrong, bar_, what, channels=slice(None)):
    """|wrong - true| >= 10 x the GPU tests' bar, in every (selected) channel."""
    t, w = true[..., channels], wrong[..., channels]
    short = (w - t).abs() < 10 * R.bar(t, **bar_)
    assert not short.any(), (what, int(short.sum()), float(((w - t).abs() / R.bar(t, **bar_)).min()))


def _moved_l2(true, wrong, what, channels=slice(None)):
    t = torch.cat([x[..., channels].reshape(-1) for x in true])
    w = torch.cat([x[..., channels].reshape(-1) for x in wrong])
    rel = ((w - t).norm() / t.norm()).item()
    assert rel >= 10 * R.BF16_L2, (what, rel)


def _check_mistakes(ref):
    """ref(mistake) -> (constants dict, list of forward outputs, backward dict): the cases are not degenerate."""
    k, ys, bw = ref(None)
    for m in ("no_between", "count_m"):
        km, ym, bm = ref(m)
        for name, b in (("var", R.BAR_VAR), ("invstd", R.BAR_INVSTD), ("scale", R.BAR_SCALE), ("running_var", R.BAR_RVAR)):
            _moved(k[name], km[name], b, (m, name))
        _moved_l2(ys, ym, (m, "forward output"))
        _moved_l2(bw["dx"], bm["dx"], (m, "dx"))
    _, _, bm = ref("global_grads")
    for r, (lt, lw) in enumerate(zip(bw["local"], bm["local"])):
        _moved(lt[0], lw[0], R.BAR_GRAD_SUMS, ("global_grads", "d bias", r))
        _moved(lt[1], lw[1], R.BAR_GRAD_SUMS, ("global_grads", "d weight", r))
    _, _, bm = ref("no_sign")
    neg = slice(R.NEG_CHANNEL, R.NEG_CHANNEL + 1)
    for r, (lt, lw) in enumerate(zip(bw["local"], bm["local"])):
        _moved(lt[1], lw[1], R.BAR_GRAD_SUMS, ("no_sign", "d weight", r), neg)
    _moved_l2(bw["dx"], bm["dx"], ("no_sign", "dx"), neg)


def test_stem_cases_are_not_degenerate(stem):
    case, slope = stem
    zs, dps = _d(case["zs"]), _d(case["dpools"])
    P = [case[n].double() for n in ("weight", "bias", "running_mean", "running_var")]

    def ref(mistake):
        k = R.stem_forward(zs, *P, slope, mistake)
        return k, k["pooled"], R.stem_backward(zs, dps, k, P[0], slope, mistake)
    _check_mistakes(ref)


@pytest.mark.parametrize("act", list(SLOPES))
@pytest.mark.parametrize("mode", [3, 4])
def test_conv_cases_are_not_degenerate(conv, act, mode):
    slope = SLOPES[act]
    rows = _d(conv["ys"])
    w, b, rm, rv = (conv[n].double() for n in ("weight", "bias", "running_mean", "running_var"))
    accs = [g.double() @ conv["wg"].double().t() for g in conv["g"]]

    def ref(mistake):
        k = R.forward_constants(rows, w, rm, rv, True, mistake)
        ys = [R.apply_rows(x, k, b, slope)[1] for x in rows]
        dzs = [R.bf16_round(R.link_dpre(acc, x, k, b, slope, mode, o.double(), s.double()))
               for acc, x, o, s in zip(accs, rows, conv["out"], conv["skip"])]
        return k, ys, R.backward_rows(rows, dzs, k, w, True, mistake)
    _check_mistakes(ref)
    # the mean of the atomic path is k + S / count: count = M moves it too
    s1 = torch.stack([R.shifted_sums(x, conv["shift"])[0] for x in rows]).sum(0)
    true = conv["shift"].double() + s1 / (R.WORLD * conv["M"])
    _moved(true, conv["shift"].double() + s1 / conv["M"], R.BAR_MEAN, ("count_m", "mean of the atomic path"))
