"""GPU: SDR's class-prototype feature losses (``--sdr_match`` / ``--sdr_attract`` / ``--sdr_repel``) - the kernels of csrc/proto.hip
against the float64 reference (tests/proto_ref.py) on exact operands, and the terms inside the UCD step: against the torch
composition, replayed from the whole-step graph, with the flags off, and as ``--method SDR``."""
import numpy as np
import pytest
import torch

import proto_ref
from test_pod_gpu import NAMES, _steps
from test_proto_cpu import CASES, UPSTREAM, WEIGHTS, case, tensors
from ucd_amd.loss import fused_proto_losses, proto_classes, proto_losses_torch, proto_update

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _map(x, dtype, pad):
    """The map on the device, channels-last: dense (pad 0) or as a channel slice of a tensor with ``pad`` more channels."""
    B, Cc, h, w = x.shape
    wide = torch.full((B, Cc + pad, h, w), 77.0, dtype=dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    wide[:, :Cc] = x.to(DEV, dtype)
    view = wide[:, :Cc]
    assert view.stride()[3] == Cc + pad and torch.equal(view.double().cpu(), x.double())       # the operands are exact in the map dtype
    return view


def _run(x, cls, state, old, dtype, pad=0, weights=WEIGHTS):
    s = _map(x, dtype, pad).detach().requires_grad_(True)
    total, parts = fused_proto_losses(s, cls.to(DEV), tuple(t.to(DEV) for t in state),
                                      None if old is None else tuple(t.to(DEV) for t in old), weights)
    (total * UPSTREAM).backward()
    torch.cuda.synchronize()
    return total.detach(), parts, s.grad


def _reference(c):
    return proto_ref.losses(c["X"], c["cls"].ravel(), c["state_sum"], c["state_n"], c["O"], c["valid"], WEIGHTS, UPSTREAM)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_class_map_equals_the_reference(i):
    c = case(i)
    B, h, w, Cc, T, K = c["shape"]
    labels = torch.from_numpy(np.array(c["labels"])).to(DEV)
    sem = None if K == 0 else torch.from_numpy(np.array(c["sem_t"])).float().to(DEV)
    got = proto_classes(labels, sem, T, K, (h, w))
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), c["cls"])


@pytest.mark.parametrize("pad", [0, 8], ids=["dense", "pitch+8"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_kernels_match_the_reference(i, dtype, pad):
    """Small-integer maps (exact in bf16; the per-class sums exact in fp32), running prototypes in quarters, old ones in halves.
    Each value within 1e-5 ref + 1e-6; d_x relative L2 within 1e-5 (fp32 maps) or 4e-3 (bf16 maps: the one output rounding); the
    batch sums and counts exactly."""
    c = case(i)
    x, cls, state, old = tensors(c)
    ref_total, ref_parts, ref_dx, S, n = _reference(c)
    total, parts, grad = _run(x, cls, state, old, dtype, pad)
    B, h, w, Cc, T, K = c["shape"]
    assert grad.dtype == dtype and grad.shape == x.shape
    got = [total.item()] + [parts[k].item() for k in ("match", "attract", "repel")]
    for name, g, r in zip(("total", "match", "attract", "repel"), got, (ref_total,) + tuple(ref_parts)):
        print(f"{name} {g!r} reference {r!r} diff {abs(g - r):.3e}")
    gx = grad.double().cpu().permute(0, 2, 3, 1).reshape(-1, Cc).numpy()
    rel = np.linalg.norm(gx - ref_dx) / np.linalg.norm(ref_dx)
    print(f"d_x relative L2 {rel:.3e}")
    for g, r in zip(got, (ref_total,) + tuple(ref_parts)):
        assert abs(g - r) <= 1e-5 * abs(r) + 1e-6
    assert rel <= (1e-5 if dtype == torch.float32 else 4e-3)
    assert np.array_equal(parts["sums"].cpu().numpy(), S) and np.array_equal(parts["n"].cpu().numpy(), n)
    assert not gx[c["cls"].ravel() < 0].any()                           # a pixel without a class has no gradient


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_torch_composition_on_the_same_operands(dtype):
    """The A/B partner of the kernels (UCD_FUSED_PROTO=0) is held to the same reference on the device."""
    for i in (0, 3):
        c = case(i)
        x, cls, state, old = tensors(c)
        ref_total, _, ref_dx, _, _ = _reference(c)
        s = _map(x, dtype, 8).detach().requires_grad_(True)
        total, _ = proto_losses_torch(s, cls.to(DEV), tuple(t.to(DEV) for t in state), None if old is None else tuple(t.to(DEV) for t in old),
                                      WEIGHTS)
        (total * UPSTREAM).backward()
        assert abs(total.item() - ref_total) <= 1e-5 * abs(ref_total) + 1e-6
        gx = s.grad.double().cpu().permute(0, 2, 3, 1).reshape(-1, x.shape[1]).numpy()
        rel = np.linalg.norm(gx - ref_dx) / np.linalg.norm(ref_dx)
        assert rel <= (1e-5 if dtype == torch.float32 else 4e-3), rel


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_degenerate_inputs_and_reproducibility(dtype):
    c = case(1)
    x, cls, state, old = tensors(c)
    B, h, w, Cc, T, K = c["shape"]
    # every pixel ignored: 0 and an all-zero d_x
    total, parts, grad = _run(x, torch.full_like(cls, -1), state, old, dtype)
    assert total.item() == 0.0 and not grad.any() and not parts["n"].any() and not parts["sums"].any()
    assert all(parts[k].item() == 0.0 for k in ("match", "attract", "repel"))
    # X_p = R_c on all rows (quarters up to 32: exact in bf16): L_attr == 0.0 exactly;  mu_c = O_c: L_match == 0.0, finite gradients
    R = torch.from_numpy(np.array(c["state_sum"]) / np.maximum(np.array(c["state_n"]), 1)[:, None])
    rows = R[cls.reshape(-1).clamp_min(0).long()].reshape(B, h, w, Cc).permute(0, 3, 1, 2)
    total, parts, grad = _run(rows, cls, state, (R[:K].float(), old[1]), dtype)
    assert parts["attract"].item() == 0.0 and parts["match"].item() == 0.0
    assert torch.isfinite(total) and torch.isfinite(grad).all()
    # a single present class: L_rep == 0
    one = torch.where(cls >= 0, torch.ones_like(cls), cls)
    assert _run(x, one, state, old, dtype)[1]["repel"].item() == 0.0
    # an empty state (N = 0): no attraction
    empty = (torch.zeros_like(state[0]), torch.zeros_like(state[1]))
    total, parts, grad = _run(x, cls, empty, old, dtype, weights=(0.0, 1.0, 0.0))
    assert parts["attract"].item() == 0.0 and total.item() == 0.0 and not grad.any()
    # two runs: equal bits in every output
    a = _run(x, cls, state, old, dtype, 8)
    b = _run(x, cls, state, old, dtype, 8)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_update_holds_the_float64_sums_exactly():
    c = case(0)
    x, cls, _, old = tensors(c)
    B, h, w, Cc, T, K = c["shape"]
    second = torch.from_numpy(proto_ref.integer_features(77, B * h * w, Cc, T, c["cls"])).reshape(B, h, w, Cc).permute(0, 3, 1, 2)
    state = (torch.zeros(T, Cc, dtype=torch.float64, device=DEV), torch.zeros(T, dtype=torch.int64, device=DEV))
    addr = state[0].data_ptr()
    want_s, want_n = np.zeros((T, Cc)), np.zeros(T, dtype=np.int64)
    for batch in (x, second):
        _, parts = fused_proto_losses(_map(batch, torch.bfloat16, 0), cls.to(DEV), state, None, WEIGHTS)
        proto_update(state, parts)
        rows = batch.permute(0, 2, 3, 1).reshape(-1, Cc).numpy()
        for k in range(T):
            want_s[k] += rows[c["cls"].ravel() == k].sum(axis=0)
            want_n[k] += (c["cls"] == k).sum()
    torch.cuda.synchronize()
    assert state[0].data_ptr() == addr
    assert np.array_equal(state[0].cpu().numpy(), want_s) and np.array_equal(state[1].cpu().numpy(), want_n)


def test_refused_shape_runs_the_composition():
    """C = 12 is no multiple of 8: the entry point makes no library call and returns the composition's value.  On the GPU the
    composition's ``index_add_`` adds with float atomics, in arrival order, so two runs of it agree to the rounding of re-ordered
    fp32 sums only, not bit for bit (the kernels do: test_degenerate_inputs_and_reproducibility): the value is held to the bar of
    the other values, 1e-5 ref + 1e-6, and the path is told by the recorded library calls."""
    from ucd_amd import hip
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 12, 6, 6, generator=g).to(DEV).requires_grad_(True)            # C = 12: not a multiple of 8
    cls = torch.randint(-1, 4, (2, 6, 6), generator=g).to(DEV)
    state = (torch.randn(4, 12, generator=g).double().to(DEV), torch.tensor([3, 0, 2, 5], device=DEV))
    calls = hip.enable_call_timing()
    try:
        got, parts = fused_proto_losses(x, cls, state, None, WEIGHTS)
        got.backward()
        names = set(calls)
    finally:
        hip.disable_call_timing()
    assert not any(k.startswith("ucd_proto") for k in names), names
    want, want_parts = proto_losses_torch(x, cls, state, None, WEIGHTS)
    print(f"entry point {got.item()!r} composition {want.item()!r}")
    assert got.item() > 0 and abs(got.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-6
    assert torch.equal(parts["n"], want_parts["n"]) and got.grad_fn is not None and torch.isfinite(x.grad).all()


# ---- the terms inside the UCD step -------------------------------------------------------------------------------------------------
SDR = ("--sdr_match", "0.5", "--sdr_attract", "0.05", "--sdr_repel", "0.5")


@pytest.fixture
def old_prototypes(monkeypatch):
    """A Trainer built by ``_steps`` has no previous state and no pass over a loader: it gets a closed-form table of old prototypes,
    three of four classes valid, through the setter ``find_prototypes`` uses."""
    from ucd_amd.train import Trainer
    init = Trainer.__init__

    def wrapped(self, *args, **kwargs):
        init(self, *args, **kwargs)
        if self.proto_flag and self.proto_w[0] > 0.:
            g = torch.Generator().manual_seed(5)
            self._set_proto_old(torch.randn(self.old_classes, self.proto_sum.shape[1], generator=g) * 0.5,
                                torch.arange(self.old_classes) % 4 != 3)
    monkeypatch.setattr(Trainer, "__init__", wrapped)


def _state(trainer):
    return trainer.last["PROTO"].item(), trainer.proto_sum.cpu().clone(), trainer.proto_n.cpu().clone()


@pytest.mark.usefixtures("deterministic_stats", "old_prototypes")
def test_step_with_the_terms_against_the_torch_composition():
    """One UCD step with the three flags against the same step under UCD_FUSED_PROTO=0, at the bars of
    tests/test_pod_gpu.py::test_step_with_pod_against_the_torch_composition."""
    from ucd_amd import hip
    calls = hip.enable_call_timing()
    try:
        got, up, _, _, trainer = _steps(SDR)
        fused_calls = tuple(len(calls.get(k, ())) for k in ("ucd_proto_classify", "ucd_proto_forward", "ucd_proto_backward"))
        calls.clear()
        ref, up_ref, _, _, trainer_ref = _steps(SDR, flips={"UCD_FUSED_PROTO": "0"})
        assert not any(k.startswith("ucd_proto") for k in calls)
    finally:
        hip.disable_call_timing()
    assert fused_calls == (1, 1, 1), fused_calls
    term, s, n = _state(trainer)
    term_ref, s_ref, n_ref = _state(trainer_ref)
    assert trainer.proto_flag and trainer.proto_old is not None and term > 0 and np.isfinite(got).all()
    print("fused:", got, term, "composition:", ref, term_ref)
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-2)
    np.testing.assert_allclose(got[:, 0], ref[:, 0], rtol=1e-2)
    np.testing.assert_allclose(got[:, 1:3], ref[:, 1:3], rtol=5e-2, atol=1e-3)
    np.testing.assert_allclose(term, term_ref, rtol=1e-2)
    assert torch.equal(n, n_ref) and n.sum() > 0                       # the update ran: the same classes, the same counts
    np.testing.assert_allclose(s.numpy(), s_ref.numpy(), rtol=1e-2, atol=1e-2 * float(s_ref.abs().max()))
    for name in NAMES:
        a, b = up_ref[name].flatten().double(), up[name].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-300))
        ratio = float(b.norm() / (a.norm() + 1e-300))
        print(f"first update, fused vs composition: {name}: cosine {cos:.4f} length ratio {ratio:.3f}")
        assert cos > (0.78 if name.startswith("body.") else 0.98) and 0.85 < ratio < 1.25, (name, cos, ratio)


@pytest.mark.usefixtures("deterministic_stats", "old_prototypes")
def test_whole_step_graph_replays_the_eager_step_with_the_terms():
    """Classify, the three forward launches, the backward and the update inside the captured iteration: three eager warm-up
    iterations and three replays give the bits of six eager iterations - every loss at every step, the term and the running
    prototypes after them, and every compared parameter."""
    eager, pe, n_e, _, te = _steps(SDR, "0", steps=6)
    graph, pg, n_g, err, tg = _steps(SDR, "1", steps=6)
    assert err is None, err
    assert n_e == 0 and n_g == 6 - 3, (n_e, n_g)
    print("eager", eager, "graph", graph, "max abs difference", np.abs(eager - graph).max())
    assert np.array_equal(eager, graph), (eager, graph)
    (term_e, s_e, c_e), (term_g, s_g, c_g) = _state(te), _state(tg)
    assert term_e == term_g and term_e > 0
    assert torch.equal(s_e, s_g) and torch.equal(c_e, c_g) and c_e.sum() > 0
    for name in pe:
        assert torch.equal(pe[name], pg[name]), name


@pytest.mark.usefixtures("deterministic_stats")
def test_zero_weights_are_the_plain_step():
    """With all three weights 0 nothing is requested: the same launches, the same bits as a Trainer built without the flags."""
    from ucd_amd import hip
    plain, pp, _, _, t0 = _steps((), steps=2)
    calls = hip.enable_call_timing()
    try:
        zero, pz, _, _, t1 = _steps(("--sdr_match", "0", "--sdr_attract", "0", "--sdr_repel", "0"), steps=2)
        names = set(calls)
    finally:
        hip.disable_call_timing()
    assert not t0.proto_flag and not t1.proto_flag and "PROTO" not in t1.last and t1.proto_sum is None
    assert not any(k.startswith("ucd_proto") for k in names)
    assert np.array_equal(plain, zero), (plain, zero)
    for name in pp:
        assert torch.equal(pp[name], pz[name]), name


@pytest.mark.usefixtures("old_prototypes")
def test_method_sdr_builds_and_steps():
    rec, _, _, _, trainer = _steps(("--method", "SDR"), steps=2)
    assert trainer.proto_w == (0.01, 0.001, 0.001) and trainer.pixcon_weight == 0.0 and trainer.lkd_flag and trainer.unce
    assert np.isfinite(rec).all() and trainer.last["PROTO"].item() > 0 and (rec[:, 1] == 0).all()
    assert trainer.proto_n.sum().item() > 0
