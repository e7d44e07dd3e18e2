"""Replays the regulariser goldens (tests/golden/make_regularizer_golden.py) through ucd_amd.regularizer: the seeded inputs of
the generator, ``step()`` per iteration (the torch twin or the HIP kernel), and everything the goldens record."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
METHODS = ("ewc", "pi", "rw")
STATES = {"ewc": ("fisher",), "pi": ("delta",), "rw": ("fisher", "score")}


def generator():
    spec = importlib.util.spec_from_file_location("make_regularizer_golden", os.path.join(GOLDEN, "make_regularizer_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def golden(name):
    return np.load(os.path.join(GOLDEN, f"regularizer_{name}.npz"))


def strip(n):
    return n[len("module."):] if n.startswith("module.") else n


def build(name, scen, device, use_kernel, wrap=True, channels_last=False, prefix_state=True):
    """(student, teacher, regulariser): the student wrapped (``module.`` names) like ucd_amd.ddp's, the teacher bare."""
    from ucd_amd.regularizer import get_regularizer
    G = generator()
    teacher_vals, student_vals, old_state, grads, steps = G.inputs(name, scen)
    net = G.make_net(student_vals, True)
    student = G.Wrapped(net) if wrap else net
    teacher = G.make_net(teacher_vals, False) if scen == "s1" else None
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    student = student.to(device)
    if teacher is not None:
        teacher = teacher.to(device)
    if channels_last:
        student = student.to(memory_format=fmt)
        if teacher is not None:
            teacher = teacher.to(memory_format=fmt)
    if old_state is not None and not prefix_state:
        old_state = {a: ({strip(k): v for k, v in d.items()} if isinstance(d, dict) else d) for a, d in old_state.items()}
    reg = get_regularizer(student, teacher, torch.device(device), G.Opts(name), old_state, use_kernel=use_kernel)
    for p in student.parameters():
        if p.requires_grad:
            p.grad = torch.zeros_like(p)          # fixed addresses, like the gradient buckets
    return student, reg, grads, steps


def replay(name, scen, device, use_kernel, **kw):
    """Run the golden's iterations; returns (regulariser, per-iteration records)."""
    student, reg, grads, steps = build(name, scen, device, use_kernel, **kw)
    records = []
    for t in range(len(grads)):
        for n, p in student.named_parameters():
            if p.requires_grad:
                p.grad.copy_(grads[t][strip(n)])
        pen = reg.step()
        rec = {"penalty": float(pen), "grad": {strip(n): p.grad.cpu().numpy().copy()
                                                for n, p in student.named_parameters() if p.grad is not None}}
        for a in STATES[name]:
            rec[a] = {strip(n): v.cpu().numpy().copy() for n, v in getattr(reg, a).items()}
        records.append(rec)
        with torch.no_grad():
            for n, p in student.named_parameters():
                p.add_(steps[t][strip(n)].to(p.device))
    return reg, records


def compare(name, scen, records, z, penalty_rtol=1e-6):
    """Bit-exact state and gradients, penalty within penalty_rtol (exactly 0 where the golden is 0)."""
    for t, rec in enumerate(records):
        want = float(z[f"{scen}|penalty|{t}"])
        if want == 0.0:
            assert rec["penalty"] == 0.0, (name, scen, t, rec["penalty"])
        else:
            assert abs(rec["penalty"] - want) <= penalty_rtol * abs(want), (name, scen, t, rec["penalty"], want)
        for kind in ("grad",) + STATES[name]:
            for k, v in rec[kind].items():
                ref = z[f"{scen}|{kind}{t}|{k}"]
                assert v.shape == ref.shape, (kind, t, k)
                bad = np.flatnonzero(v.view(np.uint32) != ref.view(np.uint32))
                assert bad.size == 0, (name, scen, kind, t, k, bad[:5], v.ravel()[bad[:5]], ref.ravel()[bad[:5]])
        # every recorded key is produced (nothing silently skipped)
        for kind in ("grad",) + STATES[name]:
            keys = {f.split("|")[2] for f in z.files if f.startswith(f"{scen}|{kind}{t}|")}
            assert keys == set(rec[kind]), (name, scen, kind, t, keys ^ set(rec[kind]))


def compare_state_dict(name, scen, sd, z, prefix="module."):
    """The final state_dict(): same entries, key sets and (bit-exact) values as the reference's."""
    entries = {f.split("|")[2] for f in z.files if f.startswith((f"{scen}|sd|", f"{scen}|sdkeys|"))}
    assert set(sd) == entries, (set(sd), entries)
    for a, v in sd.items():
        if isinstance(v, dict):
            want = {k if prefix else strip(k) for k in z[f"{scen}|sdkeys|{a}"]}
            assert set(v) == want, (a, set(v) ^ want)
            for k, x in v.items():
                ref = z[f"{scen}|sd|{a}|module.{strip(k)}"]
                got = x.detach().cpu().numpy()
                assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (a, k)
        else:
            assert np.asarray(v).item() == z[f"{scen}|sd|{a}"].item(), (a, v)
