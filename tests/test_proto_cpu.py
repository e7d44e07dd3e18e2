"""CPU: the host half of SDR's class-prototype feature losses (``--sdr_match`` / ``--sdr_attract`` / ``--sdr_repel``; csrc/proto.hip,
ucd_amd.loss.fused_proto_losses) - the float64 reference (tests/proto_ref.py) against torch autograd on the composition, the
class map against ``F.interpolate``, the plan, the library's refusals on host buffers, the command line and the Trainer's state."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import proto_ref
from test_pod_cpu import _ToyNet, _toy_batch
from ucd_amd import argparser, hip, switches
from ucd_amd.loss import fused_proto_losses, proto_classes, proto_classes_torch, proto_losses_torch, proto_update

# (B, h, w, C, T, K), (H, W), crowd, single: the cases of tests/test_proto_gpu.py
CASES = [((2, 5, 7, 8, 5, 3), (37, 53), None, None), ((2, 17, 17, 256, 21, 16), (65, 65), 17, 20),
         ((1, 9, 9, 64, 151, 101), (33, 33), None, None), ((1, 4, 4, 16, 2, 0), (16, 16), None, None)]
WEIGHTS, UPSTREAM = (0.7, 0.3, 1.3), 1.5


@functools.lru_cache(maxsize=None)
def case(i):
    (B, h, w, Cc, T, K), (H, W), crowd, single = CASES[i]
    return proto_ref.case(31 + i, B, h, w, Cc, T, K, H, W, crowd, single)


def tensors(c, dtype=torch.float64, device="cpu"):
    """The operands of a case as torch tensors: x [B, C, h, w], cls, state, old."""
    B, h, w, Cc, T, K = c["shape"]
    x = torch.from_numpy(np.array(c["X"])).reshape(B, h, w, Cc).permute(0, 3, 1, 2).to(device=device, dtype=dtype)
    cls = torch.from_numpy(np.array(c["cls"])).to(device)
    state = (torch.from_numpy(np.array(c["state_sum"])).to(device), torch.from_numpy(np.array(c["state_n"])).to(device))
    old = None if K == 0 else (torch.from_numpy(np.array(c["O"])).float().to(device), torch.from_numpy(np.array(c["valid"])).to(device))
    return x, cls, state, old


def test_names_are_registered():
    assert {"ucd_proto_plan", "ucd_proto_classify", "ucd_proto_forward", "ucd_proto_backward", "ucd_proto_update"} <= set(hip.SIGNATURES)
    lib = hip.load()
    for name in ("ucd_proto_plan", "ucd_proto_classify", "ucd_proto_forward", "ucd_proto_backward", "ucd_proto_update"):
        assert getattr(lib, name) is not None
    assert switches.DEFAULTS["UCD_FUSED_PROTO"] == "1" and "UCD_FUSED_PROTO" in switches.snapshot()


def test_the_cases_are_what_they_claim():
    c = case(1)
    counts = np.bincount(c["cls"][c["cls"] >= 0].ravel(), minlength=21)
    assert counts[17] > 256 and counts[20] == 1                     # several pieces per class; a class of one row
    c = case(2)
    assert len(np.unique(c["cls"][c["cls"] >= 0])) < 151 // 2       # most classes are absent
    assert all((case(i)["cls"] == -1).any() for i in range(3))      # ignored and out-of-range pixels
    assert (case(0)["state_n"] == 0).any() and (case(0)["state_n"] > 0).any()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_torch_composition_matches_the_reference_fp64(i):
    c = case(i)
    x, cls, state, old = tensors(c)
    x.requires_grad_(True)
    total, parts = proto_losses_torch(x, cls, state, old, WEIGHTS)
    (total * UPSTREAM).backward()
    ref_total, ref_parts, ref_dx, S, n = proto_ref.losses(c["X"], c["cls"].ravel(), c["state_sum"], c["state_n"], c["O"], c["valid"],
                                                          WEIGHTS, UPSTREAM)
    B, h, w, Cc, T, K = c["shape"]
    assert abs(total.item() - ref_total) <= 1e-12 * abs(ref_total)
    for name, ref in zip(("match", "attract", "repel"), ref_parts):
        assert abs(parts[name].item() - ref) <= 1e-12 * abs(ref) + 1e-300, name
    got = x.grad.permute(0, 2, 3, 1).reshape(-1, Cc).numpy()
    assert np.linalg.norm(got - ref_dx) <= 1e-12 * np.linalg.norm(ref_dx)
    assert np.array_equal(parts["sums"].numpy(), S) and np.array_equal(parts["n"].numpy(), n)
    # the entry point runs the composition on CPU tensors
    again, _ = fused_proto_losses(x.detach(), cls, state, old, WEIGHTS)
    assert again.item() == total.item()


def test_degenerate_inputs_of_the_composition():
    c = case(0)
    x, cls, state, old = tensors(c)
    B, h, w, Cc, T, K = c["shape"]
    # every pixel ignored: 0 and no gradient
    x.requires_grad_(True)
    total, parts = proto_losses_torch(x, torch.full_like(cls, -1), state, old, WEIGHTS)
    total.backward()
    assert total.item() == 0.0 and not x.grad.any() and not parts["n"].any()
    # X_p = R_c on every row: L_attr == 0 exactly;  mu_c = O_c: L_match == 0 with finite gradients
    R = torch.from_numpy(np.array(c["state_sum"]) / np.maximum(np.array(c["state_n"]), 1)[:, None])
    rows = R[cls.reshape(-1).clamp_min(0).long()].reshape(B, h, w, Cc).permute(0, 3, 1, 2).clone().requires_grad_(True)
    total, parts = proto_losses_torch(rows, cls, state, (R[:K].float(), old[1]), WEIGHTS)
    total.backward()
    assert parts["attract"].item() == 0.0 and parts["match"].item() == 0.0 and torch.isfinite(rows.grad).all()
    # a single present class: no repulsion;  an empty state: no attraction
    one = torch.where(cls >= 0, torch.ones_like(cls), cls)
    assert proto_losses_torch(x.detach(), one, state, old, WEIGHTS)[1]["repel"].item() == 0.0
    empty = (torch.zeros_like(state[0]), torch.zeros_like(state[1]))
    assert proto_losses_torch(x.detach(), cls, empty, old, WEIGHTS)[1]["attract"].item() == 0.0


@pytest.mark.parametrize("H,W,h,w", [(37, 53, 5, 7), (513, 513, 33, 33), (513, 513, 65, 65), (512, 512, 64, 64), (768, 768, 48, 48)])
def test_class_map_reads_the_pixels_of_nearest_interpolation(H, W, h, w):
    """Every index: the labels number the pixels, so the class map names the pixel it read."""
    labels = torch.arange(H * W, dtype=torch.int64).reshape(1, H, W)
    want = F.interpolate(labels[None].double(), size=(h, w), mode="nearest")[0].long()
    got = proto_classes_torch(labels, None, H * W, 0, (h, w), ignore_index=-7)
    assert torch.equal(got.long(), want)
    assert np.array_equal(proto_ref.classes(labels.numpy(), None, H * W, 0, (h, w), -7), got.numpy())
    assert torch.equal(proto_classes(labels, None, H * W, 0, (h, w), ignore_index=-7), got)        # CPU tensors: the composition


@pytest.mark.parametrize("i", range(len(CASES)))
def test_class_map_of_the_cases(i):
    c = case(i)
    B, h, w, Cc, T, K = c["shape"]
    sem = None if K == 0 else torch.from_numpy(np.array(c["sem_t"]))
    got = proto_classes_torch(torch.from_numpy(np.array(c["labels"])), sem, T, K, (h, w))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), c["cls"])


@pytest.mark.parametrize("T", [2, 21, 151, 256])
@pytest.mark.parametrize("Cc", [8, 256, 512])
@pytest.mark.parametrize("dtype", [hip.BF16, hip.F32])
def test_plan(T, Cc, dtype):
    M = 24 * 33 * 33
    plan = hip.proto_plan(M, Cc, T, dtype)
    pieces, slots, lanes = math.ceil(M / 64), min(64, T), Cc // (8 if dtype == hip.BF16 else 4)
    assert plan["pieces"] == pieces
    assert all(0 < b <= 160 * 1024 for b in plan["lds_bytes"])
    groups = min(16, 256 // lanes)
    assert plan["grid"] == (math.ceil(pieces / groups), T, T, math.ceil(M * lanes / 256))
    # per-piece slots (sums, squared distances per lane, counts), the slot index, the fp64 means, three values per class, a ticket
    need = pieces * slots * (Cc + lanes + 1) * 4 + T * pieces * 2 + T * Cc * 8 + T * 4 * 8 + 16
    assert need <= plan["workspace_bytes"] <= need + 7 * 16
    assert plan["workspace_bytes"] <= 6 * M * Cc + (1 << 21)


def _rc(fn, **kw):
    """The return code of a library call on HOST buffers: a call that got past its checks would fault, a refusal never touches them."""
    lib = hip.load()
    buf = np.zeros(1 << 16, dtype=np.float64)
    ok = buf.ctypes.data
    a = dict(x=ok, ld=8, dtype=hip.F32, cls=ok, M=16, Cc=8, T=4, K=2, ssum=ok, sn=ok, O=ok, valid=ok, out=ok, tables=ok, bsum=ok, bn=ok,
             ws=ok, ws_bytes=1 << 19, go=ok, d=ok, ld_d=8, labels=ok, B=1, H=16, W=16, h=4, w=4, sem=ok, ld_t=2)
    a.update(kw)
    if fn == "forward":
        return lib.ucd_proto_forward(a["x"], a["ld"], a["dtype"], a["cls"], a["M"], a["Cc"], a["T"], a["K"], a["ssum"], a["sn"], a["O"],
                                     a["valid"], 1.0, 1.0, 1.0, a["out"], a["tables"], a["bsum"], a["bn"], a["ws"], a["ws_bytes"], None)
    if fn == "backward":
        return lib.ucd_proto_backward(a["x"], a["ld"], a["dtype"], a["cls"], a["M"], a["Cc"], a["T"], a["tables"], a["go"], a["d"],
                                      a["ld_d"], None)
    if fn == "classify":
        return lib.ucd_proto_classify(a["labels"], a["B"], a["H"], a["W"], a["h"], a["w"], a["T"], a["K"], 255, a["sem"], a["ld_t"],
                                      a["cls"], None)
    if fn == "update":
        return lib.ucd_proto_update(a["ssum"], a["sn"], a["bsum"], a["bn"], a["T"], a["Cc"], None)
    raise KeyError(fn)


@pytest.mark.parametrize("fn,kwargs,code", [
    ("forward", dict(x=None), hip.EINVAL), ("forward", dict(cls=None), hip.EINVAL), ("forward", dict(ssum=None), hip.EINVAL),
    ("forward", dict(sn=None), hip.EINVAL), ("forward", dict(out=None), hip.EINVAL), ("forward", dict(tables=None), hip.EINVAL),
    ("forward", dict(bsum=None), hip.EINVAL), ("forward", dict(bn=None), hip.EINVAL), ("forward", dict(O=None), hip.EINVAL),
    ("forward", dict(valid=None), hip.EINVAL), ("forward", dict(M=0), hip.EINVAL), ("forward", dict(Cc=0), hip.EINVAL),
    ("forward", dict(T=0), hip.EINVAL), ("forward", dict(K=-1), hip.EINVAL), ("forward", dict(K=5), hip.EINVAL),
    ("forward", dict(ld=4), hip.EINVAL), ("forward", dict(dtype=7), hip.EINVAL),
    ("forward", dict(Cc=12, ld=12), hip.EUNSUPPORTED), ("forward", dict(Cc=520, ld=520), hip.EUNSUPPORTED),
    ("forward", dict(T=257), hip.EUNSUPPORTED), ("forward", dict(M=1 << 31), hip.EUNSUPPORTED),
    ("forward", dict(ld=10), hip.EALIGN), ("forward", dict(x=8), hip.EALIGN), ("forward", dict(ssum=4), hip.EALIGN),
    ("forward", dict(ws=None), hip.EWORKSPACE), ("forward", dict(ws_bytes=64), hip.EWORKSPACE), ("forward", dict(ws=8), hip.EWORKSPACE),
    ("backward", dict(x=None), hip.EINVAL), ("backward", dict(cls=None), hip.EINVAL), ("backward", dict(tables=None), hip.EINVAL),
    ("backward", dict(go=None), hip.EINVAL), ("backward", dict(d=None), hip.EINVAL), ("backward", dict(M=-3), hip.EINVAL),
    ("backward", dict(ld_d=4), hip.EINVAL), ("backward", dict(Cc=20, ld=20, ld_d=20), hip.EUNSUPPORTED),
    ("backward", dict(T=300), hip.EUNSUPPORTED), ("backward", dict(M=1 << 31), hip.EUNSUPPORTED), ("backward", dict(ld_d=10), hip.EALIGN),
    ("classify", dict(labels=None), hip.EINVAL), ("classify", dict(cls=None), hip.EINVAL), ("classify", dict(h=0), hip.EINVAL),
    ("classify", dict(K=5), hip.EINVAL), ("classify", dict(ld_t=1), hip.EINVAL), ("classify", dict(T=257), hip.EUNSUPPORTED),
    ("classify", dict(B=1 << 15, h=1 << 8, w=1 << 8, H=1 << 8, W=1 << 8), hip.EUNSUPPORTED), ("classify", dict(labels=4), hip.EALIGN),
    ("update", dict(ssum=None), hip.EINVAL), ("update", dict(bn=None), hip.EINVAL), ("update", dict(T=0), hip.EINVAL),
    ("update", dict(T=257), hip.EUNSUPPORTED), ("update", dict(sn=4), hip.EALIGN),
])
def test_refusals_on_the_host(fn, kwargs, code):
    assert _rc(fn, **kwargs) == code
    assert hip.load().ucd_last_error()                     # a message was recorded


def test_plan_refuses_like_the_calls():
    for args, what in (((16, 12, 4), "multiple of 8"), ((16, 520, 4), "multiple of 8"), ((16, 8, 257), "classes"),
                       ((1 << 31, 8, 4), "rows"), ((0, 8, 4), "bad sizes")):
        with pytest.raises(RuntimeError, match=what):
            hip.proto_plan(*args)
    assert hip.load().ucd_proto_forward(1 << 12, 8, hip.F32, 1 << 12, 16, 8, 4, 0, 1 << 12, 1 << 12, None, None, 1.0, 1.0, 1.0, 1 << 12,
                                        1 << 12, 1 << 12, 1 << 12, None, 0, None) == hip.EWORKSPACE       # K = 0 needs no old prototypes


def test_argument_rules():
    c = case(0)
    x, cls, state, old = tensors(c)
    with pytest.raises(ValueError, match="feature map"):
        fused_proto_losses(x[0], cls, state, old, WEIGHTS)
    with pytest.raises(ValueError, match="cls must be"):
        fused_proto_losses(x, cls[:, :2], state, old, WEIGHTS)
    with pytest.raises(ValueError, match="the state is"):
        fused_proto_losses(x, cls, (state[0].float(), state[1]), old, WEIGHTS)
    with pytest.raises(ValueError, match="old prototypes"):
        fused_proto_losses(x, cls, state, (old[0], old[1].long()), WEIGHTS)
    with pytest.raises(ValueError, match="weights"):
        fused_proto_losses(x, cls, state, old, (1.0, -1.0, 0.0))
    with pytest.raises(ValueError, match="teacher classes"):
        proto_classes(torch.zeros(1, 8, 8, dtype=torch.int64), None, 4, 5, (2, 2))


def _opts(extra=()):
    return argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--task", "15-5", "--step", "1"] + list(extra)))


def test_flags_and_preset():
    o = _opts()
    assert (o.sdr_match, o.sdr_attract, o.sdr_repel) == (0.0, 0.0, 0.0)
    o = _opts(["--sdr_match", "0.5", "--sdr_attract", "0.25", "--sdr_repel", "2"])
    assert (o.sdr_match, o.sdr_attract, o.sdr_repel) == (0.5, 0.25, 2.0) and (o.loss_kd, o.unce, o.unkd) == (10, True, True)
    for flag in ("--sdr_match", "--sdr_attract", "--sdr_repel"):
        for bad in ("-0.1", "nan", "inf"):
            with pytest.raises(SystemExit):
                _opts([flag, bad])
    o = argparser.modify_command_options(argparser.get_argparser().parse_args(["--method", "SDR", "--task", "15-5", "--step", "1"]))
    assert (o.unce, o.unkd, o.loss_kd, o.init_balanced) == (True, True, 10, True)              # MiB's switches
    assert o.pixcon_weight == 0.0 and (o.sdr_match, o.sdr_attract, o.sdr_repel) == (0.01, 0.001, 0.001)
    assert o.pod_factor == 0.0 and o.pseudo is None and not o.focal_loss
    # next to the other families, BCE included: the terms touch only the features
    for extra in (["--bce"], ["--icarl"], ["--pod_factor", "0.01"], ["--pseudo", "entropy"], ["--focal_loss"], ["--regularizer", "ewc"]):
        o = _opts(["--sdr_attract", "0.1"] + extra)
        assert o.sdr_attract == 0.1


def _toy_trainer(extra, trainer_state=None, teacher=True):
    from ucd_amd.train import Trainer
    opts = _opts(extra)
    opts.pixcon_weight = 0.0                    # the contrastive kernels exist on the GPU only
    student, old = _ToyNet(21, 1), _ToyNet(16, 2)
    old.eval()
    trainer = Trainer(student, old if teacher else None, torch.device("cpu"), opts, trainer_state=trainer_state, classes=[16, 5])
    return trainer, student, old


SDR = ["--sdr_match", "0.5", "--sdr_attract", "0.25", "--sdr_repel", "2"]


def test_flags_request_nothing_when_off():
    trainer, student, _ = _toy_trainer([])
    assert trainer.proto_flag is False
    out = trainer.train_step(*_toy_batch(), torch.optim.SGD(student.parameters(), lr=0.0))
    assert "PROTO" not in out and "proto" not in trainer.state_dict()
    # --sdr_match without a teacher requests nothing; attraction and repulsion run at step 0 too
    assert _toy_trainer(["--sdr_match", "0.5"], teacher=False)[0].proto_flag is False
    t0 = _toy_trainer(["--sdr_match", "0.5", "--sdr_repel", "1"], teacher=False)[0]
    assert t0.proto_flag and t0.proto_w == (0.0, 0.0, 1.0)


def test_cpu_trainer_step_adds_the_term_composed_by_hand():
    plain, student0, _ = _toy_trainer([])
    trainer, student, teacher = _toy_trainer(SDR)
    images, labels = _toy_batch()
    with torch.no_grad():
        _, fs = student(images)
        _, ft = teacher(images)
    x = fs.raw("pre_logits")
    Cc = x.shape[1]
    rng = np.random.RandomState(3)
    prev = {"sum": torch.from_numpy(rng.randn(16, Cc) * 5.0), "n": torch.from_numpy(rng.randint(0, 3, size=16) * 5)}
    assert trainer._old_from_state(prev) and trainer.proto_old[0].shape == (16, Cc)
    r0 = plain.train_step(images, labels, torch.optim.SGD(student0.parameters(), lr=0.0))
    r = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    cls = proto_ref.classes(labels.numpy(), ft["sem"].numpy(), 21, 16, x.shape[-2:])
    rows = x.permute(0, 2, 3, 1).reshape(-1, Cc).double().numpy()
    O = np.where(prev["n"].numpy()[:, None] > 0, prev["sum"].numpy() / np.maximum(prev["n"].numpy(), 1)[:, None], 0.0).astype(np.float32)
    by_hand, _, _, S, n = proto_ref.losses(rows, cls.ravel(), np.zeros((21, Cc)), np.zeros(21, dtype=np.int64), O.astype(np.float64),
                                           prev["n"].numpy() > 0, (0.5, 0.25, 2.0))
    assert by_hand > 0 and abs(r["PROTO"].item() - by_hand) <= 1e-5 * by_hand
    for k in ("loss", "lkd", "ce"):
        assert r[k].item() == r0[k].item()
    assert not torch.equal(student.head.weight.grad, student0.head.weight.grad)
    assert torch.equal(student.cls.weight.grad, student0.cls.weight.grad)          # the classifier sits behind the pre-logits
    # the update ran after the step: the state holds this batch
    assert np.array_equal(trainer.proto_n.numpy(), n) and np.allclose(trainer.proto_sum.numpy(), S, rtol=1e-5, atol=1e-4)
    # a second step uses the state of the first: the attraction term is on
    r2 = trainer.train_step(images, labels, torch.optim.SGD(student.parameters(), lr=0.0))
    assert r2["PROTO"].item() > r["PROTO"].item() and np.array_equal(trainer.proto_n.numpy(), 2 * n)


def test_state_round_trip_and_the_choice_of_old_prototypes():
    trainer, student, _ = _toy_trainer(SDR)
    trainer.train_step(*_toy_batch(), torch.optim.SGD(student.parameters(), lr=0.0))
    state = trainer.state_dict()
    assert set(state["proto"]) == {"sum", "n", "old", "old_valid"} and state["proto"]["old"] is None
    assert state["proto"]["sum"].dtype == torch.float64 and state["proto"]["n"].dtype == torch.int64
    # a resume of the same step: the state comes back into the same tensors
    again, _, _ = _toy_trainer(SDR)
    again._alloc_proto(state["proto"]["sum"].shape[1])
    addr = again.proto_sum.data_ptr()
    again.load_state_dict(state)
    assert again.proto_sum.data_ptr() == addr
    assert torch.equal(again.proto_sum, trainer.proto_sum) and torch.equal(again.proto_n, trainer.proto_n)
    # the next step takes O and valid from rows 0 .. K-1 of the previous step's state
    prev = {"sum": torch.arange(16 * 8, dtype=torch.float64).reshape(16, 8), "n": torch.tensor([2, 0] * 8)}
    nxt, _, _ = _toy_trainer(SDR, trainer_state={"regularizer": None, "proto": prev})
    O, valid = nxt.proto_old
    assert O.dtype == torch.float32 and torch.equal(valid, prev["n"] > 0)
    assert torch.equal(O[0], (prev["sum"][0] / 2).float()) and not O[1].any()
    # and carries them in its own state; a resume restores them
    nxt._alloc_proto(8)                         # (the toy network does not name its head width: the first step would)
    st = nxt.state_dict()
    assert torch.equal(st["proto"]["old"], O) and torch.equal(st["proto"]["old_valid"], valid)
    res, _, _ = _toy_trainer(SDR)
    res.load_state_dict(st)
    assert torch.equal(res.proto_old[0], O) and torch.equal(res.proto_old[1], valid)
    # a previous state with fewer classes than the teacher has is not used
    short, _, _ = _toy_trainer(SDR, trainer_state={"regularizer": None, "proto": {"sum": prev["sum"][:4], "n": prev["n"][:4]}})
    assert short.proto_old is None


def test_find_prototypes_on_the_teacher():
    trainer, _, teacher = _toy_trainer(SDR)
    images, labels = _toy_batch()
    count = trainer.find_prototypes([(images, labels), (images.flip(0), labels.flip(0))])
    with torch.no_grad():
        _, ft = teacher(images)
    x = ft.raw("pre_logits")
    cls = proto_ref.classes(labels.numpy(), ft["sem"].numpy(), 16, 16, x.shape[-2:])
    rows = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).double().numpy()
    _, _, _, S, n = proto_ref.losses(rows, cls.ravel(), np.zeros((16, x.shape[1])), np.zeros(16, dtype=np.int64), None, None, (0, 0, 0))
    O, valid = trainer.proto_old
    assert count == int((n > 0).sum()) and np.array_equal(valid.numpy(), n > 0)
    want = np.where(n[:, None] > 0, S / np.maximum(n, 1)[:, None], 0.0)
    assert np.allclose(O.numpy(), want, rtol=1e-5, atol=1e-6)
    with pytest.raises(RuntimeError, match="sdr_match"):
        _toy_trainer(["--sdr_repel", "1"])[0].find_prototypes([])


def test_update_adds_in_place():
    c = case(0)
    _, _, state, _ = tensors(c)
    state = (state[0].clone(), state[1].clone())
    parts = {"sums": torch.ones_like(state[0]), "n": torch.full_like(state[1], 3)}
    before = (state[0].clone(), state[1].clone())
    proto_update(state, parts)
    assert torch.equal(state[0], before[0] + 1) and torch.equal(state[1], before[1] + 3)
