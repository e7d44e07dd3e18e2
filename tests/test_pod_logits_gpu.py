"""GPU: Local POD on the logits (``--pod_logits``) - the kernels of csrc/pod.hip against the float64 reference
(tests/pod_logits_ref.py) on exact operands, and the level inside the UCD and PLOP steps: against the torch composition, replayed
from the whole-step graph, and with the flags off."""
import functools

import numpy as np
import pytest
import torch

import pod_logits_ref as ref
import pod_ref
from test_pod_gpu import NAMES, POD, _steps
from ucd_amd.loss import fused_local_pod_logits, local_pod_logits_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Ctot, K, h, w), scales: VOC 15-5 with an uncovered last row and column; K no multiple of 8 or 4, one new channel, non-square;
# only the background is old, the smallest map; ADE 100-10 step 1 with an odd K and several workgroups per launch; another scale
# list; no merge
CASES = [((2, 21, 16, 9, 9), (1, 2, 4)), ((3, 21, 20, 7, 11), (1, 2, 4)), ((1, 6, 1, 4, 4), (1, 2, 4)),
         ((1, 111, 101, 33, 33), (1, 2, 4)), ((2, 17, 16, 9, 9), (1, 3)), ((2, 16, 16, 5, 5), (1, 2, 4))]
WEIGHT, UPSTREAM = 0.7, 1.5


@functools.lru_cache(maxsize=None)
def _case(case, scales, normalize):
    """Operands and the float64 reference of one case, computed once and shared (read-only) by the tests that need them."""
    s, t = ref.integer_logits(23, *case)
    value = ref.level(s, t, scales, normalize)
    grad = ref.level_grad(s, t, scales, normalize, WEIGHT * UPSTREAM)
    for arr in (s, t, grad):
        arr.setflags(write=False)
    return s, t, value, grad


def _rows(x, pad):
    """The logits as fp32 channels-last rows: dense (pad 0: a row of C floats, 4-byte aligned only for odd C) or as a channel slice
    of a tensor with ``pad`` more channels (row pitch C + pad)."""
    B, Cc, h, w = x.shape
    wide = torch.full((B, h, w, Cc + pad), 77.0, dtype=torch.float32, device=DEV)
    host = torch.from_numpy(np.array(x, dtype=np.float64))          # a copy: the shared operands are read-only
    wide[..., :Cc] = host.permute(0, 2, 3, 1).to(DEV, torch.float32)
    view = wide.permute(0, 3, 1, 2)[:, :Cc]
    assert view.stride() == (h * w * (Cc + pad), 1, w * (Cc + pad), Cc + pad) and torch.equal(view.double().cpu(), host)
    return view


def _run(s, t, scales, normalize, pad):
    xs = _rows(s, pad).detach().requires_grad_(True)
    val = fused_local_pod_logits(xs, _rows(t, pad), scales, WEIGHT, normalize)
    (val * UPSTREAM).backward()
    torch.cuda.synchronize()
    return val.detach(), xs.grad


@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "pitch+3"])
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("case,scales", CASES)
def test_kernels_match_the_reference(case, scales, normalize, pad):
    """Small-integer logits: the merge, the squares and every strip sum are exact in fp32.  The bars of tests/test_pod_gpu.py for
    fp32 maps: level value within 1e-5 ref + 1e-6, dS relative L2 within 1e-5.  Channel 0 and every new-class channel carry the
    same bits."""
    from ucd_amd import hip
    B, Ctot, K, h, w = case
    s, t, want, gref = _case(case, scales, normalize)
    calls = hip.enable_call_timing()
    try:
        val, grad = _run(s, t, scales, normalize, pad)
        assert len(calls.get("ucd_pod_logits_forward", ())) == 1 and len(calls.get("ucd_pod_logits_backward", ())) == 1
    finally:
        hip.disable_call_timing()
    got = val.item() / WEIGHT
    print(f"level {got!r} reference {want!r} diff {abs(got - want):.3e}")
    assert grad.dtype == torch.float32 and grad.shape == (B, Ctot, h, w)
    g = grad.double().cpu().numpy()
    rel = np.linalg.norm(g - gref) / np.linalg.norm(gref)
    print(f"dS relative L2 {rel:.3e}")
    assert abs(got - want) <= 1e-5 * want + 1e-6
    assert rel <= 1e-5
    for c in range(K, Ctot):
        assert torch.equal(grad[:, c], grad[:, 0]), c
    if K == Ctot and normalize:
        assert abs(got - pod_ref.level(s, t, 1.0, scales)) <= 1e-5 * want + 1e-6
        gfeat = pod_ref.level_grad(s, t, 1.0, scales, WEIGHT * UPSTREAM)
        assert np.linalg.norm(g - gfeat) / np.linalg.norm(gfeat) <= 1e-5


@pytest.mark.parametrize("normalize", [1, 0])
def test_torch_composition_on_the_same_operands(normalize):
    """The A/B partner of the kernels (UCD_FUSED_POD=0) is held to the same reference on the device."""
    for case, scales in CASES[:2]:
        s, t, want, gref = _case(case, scales, normalize)
        xs = _rows(s, 0).detach().requires_grad_(True)
        val = local_pod_logits_torch(xs, _rows(t, 0), scales, WEIGHT, normalize)
        (val * UPSTREAM).backward()
        assert abs(val.item() / WEIGHT - want) <= 1e-5 * want + 1e-6
        rel = np.linalg.norm(xs.grad.double().cpu().numpy() - gref) / np.linalg.norm(gref)
        assert rel <= 1e-5, rel


@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "pitch+3"])
@pytest.mark.parametrize("normalize", [1, 0])
def test_degenerate_logits_and_reproducibility(normalize, pad):
    case, scales = CASES[1]
    B, Ctot, K, h, w = case
    s, t, _, _ = _case(case, scales, normalize)
    # a student whose merged logits ARE the teacher's: exactly zero loss and gradient
    same = np.array(s)
    same[:, 0] = t[:, 0] - s[:, K:].sum(1)
    same[:, 1:K] = t[:, 1:]
    val, grad = _run(same, t, scales, normalize, pad)
    assert val.item() == 0.0 and not grad.any()
    # all-zero logits (one map, both): finite
    zs, zt = np.zeros_like(s), np.zeros_like(t)
    for a, b in ((zs, t), (s, zt), (zs, zt)):
        val, grad = _run(a, b, scales, normalize, pad)
        assert torch.isfinite(val).all() and torch.isfinite(grad).all()
    assert val.item() == 0.0 and not grad.any()
    # two runs: the same bits
    a = _run(s, t, scales, normalize, pad)
    b = _run(s, t, scales, normalize, pad)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refused_shape_runs_the_composition():
    x = torch.randn(1, 300, 5, 5, device=DEV, requires_grad=True)            # Ctot = 300: above 256
    t = torch.randn(1, 290, 5, 5, device=DEV)
    assert torch.equal(fused_local_pod_logits(x, t), local_pod_logits_torch(x, t))


# ---- the level inside the step ---------------------------------------------------------------------------------------------------
LOGITS = POD + ("--pod_logits",)


@pytest.mark.usefixtures("deterministic_stats")
def test_step_with_pod_logits_against_the_torch_composition():
    """One UCD step with --pod_factor 0.01 --pod_logits against the same step under UCD_FUSED_POD=0 UCD_BWD_LINK=0: the bars of
    tests/test_pod_gpu.py::test_step_with_pod_against_the_torch_composition.  Five feature levels and the one on the logits, each
    on its own kernels."""
    from ucd_amd import hip
    names = ("ucd_pod_forward", "ucd_pod_backward", "ucd_pod_logits_forward", "ucd_pod_logits_backward")
    calls = hip.enable_call_timing()
    try:
        got, up, _, _, trainer = _steps(LOGITS)
        fused_calls = tuple(len(calls.get(n, ())) for n in names)
        calls.clear()
        want, up_ref, _, _, _ = _steps(LOGITS, flips={"UCD_FUSED_POD": "0", "UCD_BWD_LINK": "0"})
        assert not any(n in calls for n in names)
    finally:
        hip.disable_call_timing()
    assert fused_calls == (5, 5, 1, 1), fused_calls
    assert trainer.pod_flag and trainer.pod_logits and got[0, 4] > 0 and np.isfinite(got).all()
    print("fused:", got, "composition:", want)
    np.testing.assert_allclose(got[:, 3], want[:, 3], rtol=1e-2)
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-2)
    np.testing.assert_allclose(got[:, 1:3], want[:, 1:3], rtol=5e-2, atol=1e-3)
    np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-2)
    for n in NAMES:
        a, b = up_ref[n].flatten().double(), up[n].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(b.norm() / (a.norm() + 1e-300))
        print(f"first update, fused vs composition: {n}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > (0.78 if n.startswith("body.") else 0.98) and 0.85 < ratio < 1.25, (n, cos, ratio)


@pytest.mark.usefixtures("deterministic_stats")
def test_whole_step_graph_replays_the_eager_step_with_pod_logits():
    """Six levels inside the captured iteration: three eager warm-up iterations and three replays give the bits of six eager
    iterations - every loss at every step and every compared parameter afterwards."""
    eager, pe, n_e, _, _ = _steps(LOGITS, "0", steps=6)
    graph, pg, n_g, err, _ = _steps(LOGITS, "1", steps=6)
    assert err is None, err
    assert n_e == 0 and n_g == 6 - 3, (n_e, n_g)
    print("eager", eager, "graph", graph, "max abs difference", np.abs(eager - graph).max())
    assert np.array_equal(eager, graph), (eager, graph)
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


@pytest.mark.usefixtures("deterministic_stats")
def test_flags_that_request_nothing_change_nothing():
    """--pod_logits alone is the plain step; --pod_logits_norm without --pod_logits leaves the five-level term as it is."""
    plain, pp, _, _, t0 = _steps(())
    alone, pa, _, _, t1 = _steps(("--pod_logits",))
    assert not t0.pod_flag and not t1.pod_flag and not t1.pod_logits
    assert np.array_equal(plain, alone), (plain, alone)
    for n in pp:
        assert torch.equal(pp[n], pa[n]), n
    five, p5, _, _, t5 = _steps(POD)
    norm0, pn, _, _, tn = _steps(POD + ("--pod_logits_norm", "0"))
    assert t5.pod_flag and tn.pod_flag and not t5.pod_logits and not tn.pod_logits
    assert np.array_equal(five, norm0), (five, norm0)
    for n in p5:
        assert torch.equal(p5[n], pn[n]), n


def test_plop_with_the_level_on_the_logits():
    """--method PLOP --pod_logits builds and steps (tests/test_pseudo_gpu.py::_steps runs the threshold pass first); its term is
    finite, positive and not the five-level one."""
    from test_pseudo_gpu import _steps as plop_steps
    five, _, _, _, t5 = plop_steps((), method="PLOP")
    six, _, _, _, t6 = plop_steps(("--pod_logits",), method="PLOP")
    assert t5.pod_flag and not t5.pod_logits and t6.pod_flag and t6.pseudo_flag and t6.pod_logits and t6.pod_logits_norm == 1
    print("LPOD of --method PLOP:", five[0, 4], "with --pod_logits:", six[0, 4])
    assert np.isfinite(six).all() and six[0, 4] > 0 and five[0, 4] > 0 and six[0, 4] != five[0, 4]
