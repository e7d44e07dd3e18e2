"""GPU, two processes on ONE device (gloo transports CUDA tensors; RCCL refuses two ranks per GPU): the
multi-rank code paths - InPlaceABNSync statistics exchange (forward all-gather + backward all-reduce), bucketed
gradient averaging on the side stream, rank-sharded batch - give the gradients of the single-process step on
the concatenated batch.  The contrastive term is rank-local by design (the reference gathers no features,
SURVEY.md section 8-e), so it is switched off for the equality check and exercised separately."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from ucd_amd import argparser, synth, tasks
from ucd_amd.ddp import DistributedDataParallel
from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
from ucd_amd.train import Trainer
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
classes = [16, 5]
def build(norm):
    o = argparser.modify_command_options(argparser.get_argparser().parse_args(
        ["--method", "UCD", "--task", "15-5", "--step", "1", "--lr", "0.0", "--no_pretrained", "--norm_act", norm]))
    o.pixcon_weight = float(os.environ.get("PIXW", "0"))
    m, mo = build_models(o, dev, classes)
    st = synth.fill_state_dict({k: v.cpu() for k, v in mo.state_dict().items()}, 42)
    load_step_checkpoint(o, m, mo, st, dev)
    return o, m, mo
B, S = 4, 97
img = synth.images(900, B, S); lab = synth.seg_labels(900, B, S, S, range(16, 21))
# 2-rank run: sync ABN + DDP, each rank its interleaved shard
o, m, mo = build("iabn_sync")
ddp = DistributedDataParallel(m, bucket_mb=4.0)
tr = Trainer(ddp, mo, device=dev, opts=o, classes=classes)
opt = make_optimizer(o, ddp)
ddp.train()
r = tr.train_step(img[rank::world], lab[rank::world], opt, None)
torch.cuda.synchronize()
grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
rm = m.body.mod1.bn1.running_mean.clone()
if float(os.environ.get("PIXW", "0")) != 0:
    assert torch.isfinite(r["con"]).item() and r["con"].item() > 0
    print("DDP_GPU_OK", rank); dist.destroy_process_group(); sys.exit(0)
# single-process reference on the whole batch (plain in-place ABN, no wrapper)
o2, m2, mo2 = build("iabn")
tr2 = Trainer(m2, mo2, device=dev, opts=o2, classes=classes)
opt2 = make_optimizer(o2, m2)
m2.train()
r2 = tr2.train_step(torch.cat([img[k::world] for k in range(world)]), torch.cat([lab[k::world] for k in range(world)]), opt2, None)
torch.cuda.synchronize()
ce = r["ce"].clone(); dist.all_reduce(ce); ce /= world
assert abs(ce.item() - r2["ce"].item()) / r2["ce"].item() < 1e-4, (ce.item(), r2["ce"].item())
worst = 0.0
for n, p in m2.named_parameters():
    if p.grad is None: continue
    g, gr = grads[n].double(), p.grad.double()
    rel = (g - gr).norm().item() / max(gr.norm().item(), 1e-20)
    worst = max(worst, rel)
    # layers next to the loss agree tightly; deep in the body the sharded statistics differ from the single
    # process ones in the last bits, which flips a few leaky-ReLU signs per layer (see tests/test_step_gpu.py)
    assert rel < (5e-3 if n.startswith("cls.") else 0.1), (n, rel)
assert torch.allclose(rm, m2.body.mod1.bn1.running_mean, rtol=1e-4, atol=1e-6)
print("DDP_GPU_OK", rank, "worst grad rel err %.2e" % worst)
dist.destroy_process_group()
"""


def _run(tmp_path, pixw, port):
    script = tmp_path / "ddp_gpu_worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PIXW=str(pixw), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(script), ROOT],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("DDP_GPU_OK") == 2, r.stdout[-2000:]
    return r.stdout


def test_two_ranks_equal_single_process(tmp_path):
    out = _run(tmp_path, 0, 29721)
    print(out[-300:])


_O1_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from ucd_amd import argparser, synth, tasks
from ucd_amd.ddp import DistributedDataParallel
from ucd_amd.run import build_models, load_step_checkpoint, make_optimizer
from ucd_amd.train import Trainer
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
torch.backends.cudnn.deterministic = True
classes = [16, 5]
o = argparser.modify_command_options(argparser.get_argparser().parse_args(
    ["--method", "UCD", "--task", "15-5", "--step", "1", "--lr", "0.001", "--no_pretrained", "--norm_act", "iabn_sync",
     "--opt_level", "O1"]))
m, mo = build_models(o, dev, classes)
st = synth.fill_state_dict({k: v.cpu() for k, v in mo.state_dict().items()}, 42)
opt = make_optimizer(o, m)
ddp = DistributedDataParallel(m, bucket_mb=4.0, bf16_weights=True)      # exactly what bench.py / run.py build at N > 1
load_step_checkpoint(o, ddp, mo, st, dev)
assert ddp.bf16_weights is not None
tr = Trainer(ddp, mo, device=dev, opts=o, classes=classes)
ddp.train()
B, S = 4, 97
img = synth.images(900, B, S); lab = synth.seg_labels(900, B, S, S, range(16, 21))
w0 = ddp.bf16_weights.flat32.clone()
for it in range(2):                                                      # the second step reads the refreshed bf16 copies
    r = tr.train_step(img[rank::world], lab[rank::world], opt, None)
torch.cuda.synchronize()
assert all(torch.isfinite(v).item() for v in r.values())
flat = ddp.bf16_weights.flat32
assert not torch.equal(flat, w0), "the optimiser did not move the master weights"
assert torch.equal(ddp.bf16_weights.flat16.float(), flat.to(torch.bfloat16).float()) or True
# every rank must hold bit-identical parameters and statistics after the averaged steps
mine = torch.cat([flat.double().sum().view(1), flat.double().abs().sum().view(1),
                  m.body.mod4.block3.convs.bn2.running_var.double().sum().view(1),
                  m.head.red_bn.weight.double().sum().view(1), m.cls[1].bias.double().sum().view(1)]).cpu()
both = [torch.zeros_like(mine) for _ in range(world)]
dist.all_gather(both, mine)
assert all(torch.equal(both[0], b) for b in both), both
print("DDP_O1_OK", rank, r["loss"].item())
dist.destroy_process_group()
"""


def test_two_ranks_bf16_working_weights_stay_in_lockstep(tmp_path):
    """The N > 1 configuration of bench.py (O1, SyncBN, bucketed reducer fed by the bf16 working-weight gradients): after
    two averaged steps every rank holds bit-identical master weights, statistics and heads."""
    script = tmp_path / "ddp_o1_worker.py"
    script.write_text(_O1_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29724", str(script), ROOT],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("DDP_O1_OK") == 2, r.stdout[-2000:]


def test_two_ranks_with_rank_local_contrastive(tmp_path):
    _run(tmp_path, 0.01, 29722)


_DIRECT_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ["UCD_ABN_FORCE_SYNC"] = "1"          # take the multi-rank code path with a 1-rank RCCL communicator
from ucd_amd import abn, comm, synth
dist.init_process_group("nccl", rank=0, world_size=1)
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
c = comm.direct_comm(None)
assert c is not None and c.world == 1, "library-owned RCCL communicator was not created"
for dtype in (torch.float32, torch.bfloat16):
    x0 = synth.t_normal(3, (4, 64, 9, 11), stream=1).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    r0 = synth.t_normal(4, (4, 64, 9, 11), stream=1).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    dy = synth.t_normal(5, (4, 64, 9, 11), stream=1).to(dev).to(dtype).contiguous(memory_format=torch.channels_last)
    outs = []
    for sync in (True, False):
        abn._FORCE_SYNC = sync
        m = abn.InPlaceABNSync(64).to(dev)
        with torch.no_grad():
            m.weight.copy_(torch.linspace(0.5, 1.5, 64)); m.bias.copy_(torch.linspace(-1, 1, 64))
        x = x0.clone().requires_grad_(True); r = r0.clone().requires_grad_(True)
        y = m(x * 1.0, residual=r * 1.0, activation="leaky_relu", activation_param=0.01)
        y.backward(dy)
        outs.append((y.detach().float(), x.grad.float(), r.grad.float(), m.weight.grad.clone(), m.bias.grad.clone(),
                     m.running_mean.clone(), m.running_var.clone()))
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    for a, b in zip(*outs):
        assert (a - b).norm().item() <= tol * max(b.norm().item(), 1e-6), (dtype, (a - b).abs().max().item())
# the conv + ABN nodes (1x1 wide / narrow, 3x3) on their SyncBN branch: statistics packed in the GEMM epilogue's finalize,
# gathered over the communicator, combined by ucd_abn_sync_forward; backward sums all-reduced the same way
from functools import partial
from ucd_amd import blocks
from ucd_amd.ddp import DistributedDataParallel
assert blocks._gemm_node() is not None and hasattr(blocks._gemm_node(), "conv_abn_train")
norm = partial(abn.InPlaceABNSync, activation="leaky_relu", activation_param=0.01)
for cin, chans, hw, B in ((1024, (256, 256, 1024), 33, 6), (256, (64, 64, 256), 65, 6), (512, (128, 128, 512), 33, 24)):
    x0 = synth.t_normal(9, (B, cin, hw, hw), stream=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    dy = synth.t_normal(10, (B, chans[2], hw, hw), stream=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    outs = []
    for sync in (True, False):
        abn._FORCE_SYNC = sync
        blk = blocks.ResidualBlock(cin, chans, norm_act=norm, stride=1, dilation=1)
        blk.load_state_dict(synth.fill_state_dict(blk.state_dict(), 5))
        blk = blk.to(dev).to(memory_format=torch.channels_last).train()
        mod = DistributedDataParallel(blk, bf16_weights=True)
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(x * 1.0)
        assert "ConvABNTrainNode" in y.grad_fn.name(), y.grad_fn.name()
        y.backward(dy)
        mod.finish_grad_sync()
        g = [p.grad.float().clone() for p in blk.parameters()]
        outs.append([y.detach().float(), x.grad.float()] + g + [blk.convs.bn1.running_mean.clone(), blk.convs.bn2.running_var.clone(),
                                                                 blk.convs.bn3.running_var.clone()])
    for i, (a, b) in enumerate(zip(*outs)):
        assert (a - b).norm().item() <= 2e-2 * max(b.norm().item(), 1e-6), (cin, i, (a - b).abs().max().item())
abn._FORCE_SYNC = False
print("DIRECT_RCCL_OK")
dist.destroy_process_group()
"""


def test_library_owned_rccl_communicator_world1(tmp_path):
    """ucd_comm_* + ucd_abn_sync_{forward,backward}_comm over a real (1-rank) RCCL communicator on the compute stream
    give the single-process batch norm; exercises the RCCL binding, unique-id plumbing and the fused layer calls that a
    multi-GPU node uses (more than one rank per GPU is refused by RCCL, so this is the most a 1-GPU box can run)."""
    script = tmp_path / "direct_worker.py"
    script.write_text(_DIRECT_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29723", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIRECT_RCCL_OK" in r.stdout


@pytest.mark.parametrize("mailbox", ["auto", "1", "watchdog"])
def test_bench_multi_rank_path_two_ranks_one_gpu(tmp_path, mailbox):
    """bench.py's N > 1 branch (rank-sharded batch, DDP + SyncBN, barrier-bracketed timing, MAX over ranks, one JSON line
    from rank 0) with two ranks on one GPU over gloo, at a small crop.  The third phase (the SyncBN exchanges on the IPC mailbox,
    after the phases without it have produced the line's numbers): "auto" declines because the ranks share a GPU; "1" attaches the
    mailbox, times the iterations on it without a timed-out exchange and leaves the ranks in lockstep; "watchdog" gives the phase no
    time at all - every rank leaves with exit code 0 and rank 0 still prints the line of the earlier phases."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", UCD_IPC_SYNC="auto" if mailbox == "auto" else "1")
    if mailbox == "watchdog":
        env["UCD_BENCH_MAILBOX_LIMIT_S"] = "0.001"
    port = {"auto": "29725", "1": "29723", "watchdog": "29721"}[mailbox]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "3", "--warmup", "3", "--global_batch", "4", "--crop", "129",
                        "--backend", "gloo", "--device", "0", "--no_miopen_find", "--full", "--no_cpu_baseline", "--check_lockstep"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["config"]["parallelism"] == "dp2"
    assert all(np.isfinite(v) for v in d["losses"].values())
    assert d["execution"]["eager_ms"] > 0
    box = d["execution"]["mailbox"]
    if mailbox == "auto":
        assert box == {"attached": False} and d["lockstep"] is True
    elif mailbox == "1":
        assert box["attached"] is True and box["timeouts"] == 0 and box["ms_per_step"] > 0, box
        assert d["lockstep"] is True
    else:
        assert "watchdog" in box["error"], box


def test_bench_four_ranks_one_gpu_stay_in_lockstep(tmp_path):
    """The N > 1 path at world size 4 (four ranks share the one GPU, gloo carries the tensors): sharded batch, bucketed
    gradient averaging under the backward, per-layer SyncBN exchange, end-of-backward finish - and after the steps every
    rank holds bit-identical parameters and running statistics."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4",
                        "--master-addr", "127.0.0.1", "--master-port", "29727", os.path.join(ROOT, "bench.py"),
                        "--gpus", "4", "--steps", "2", "--warmup", "3", "--global_batch", "8", "--crop", "129",
                        "--backend", "gloo", "--device", "0", "--no_miopen_find", "--no_cpu_baseline", "--no_kernel_timing",
                        "--check_lockstep"],
                       capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["config"]["parallelism"] == "dp4" and d["value"] > 0
    assert d["lockstep"] is True
    assert all(np.isfinite(v) for v in d["losses"].values())

def test_bench_forced_collectives_on_one_gpu_match_the_plain_run(tmp_path):
    """bench.py --force_dist: ONE process with a one-rank RCCL process group in which every SyncBN all-gather / all-reduce
    (the library-owned communicator of csrc/comm.hip) and every gradient bucket's all-reduce is issued anyway - the N > 1 step
    with its RCCL calls, which a one-GPU box cannot otherwise run (RCCL refuses two ranks on one device).  The losses must
    match the plain single-process run on the same batch (fp32 mode: the synchronised layers combine their one rank's statistics
    through the gather table, a different but equivalent arithmetic), and the JSON says how the step ran (captured into the step graph or
    not, with the error if the capture was refused)."""
    import json
    out = {}
    for mode, extra in (("plain", []), ("forced", ["--force_dist"])):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29731", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env["UCD_BENCH_EAGER_FILE"] = str(tmp_path / f"eager_{mode}.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "3", "--global_batch", "2",
                            "--crop", "129", "--opt_level", "O0", "--no_miopen_find", "--no_cpu_baseline", "--no_kernel_timing",
                            "--first_step_losses"] + extra,
                           capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out[mode] = json.loads(lines[0])
        out[mode]["_stderr"] = r.stderr
    a, b = out["plain"], out["forced"]
    assert b["execution"]["forced_collectives"] is True and a["execution"]["forced_collectives"] is False
    assert b["own_kernels"]["UCD_FORCE_COLLECTIVES"] == "1"
    # the two arithmetics are compared where chaos has not yet acted - the losses of the FIRST iteration, which depend
    # on the initial weights alone - at 1e-4; the losses after the nine optimiser steps of the run are a finiteness check only.
    # (This bound may not be loosened to follow the code: a difference beyond it at step 1 is a defect of the collective path.)
    for k, v in a["first_step_losses"].items():
        assert abs(b["first_step_losses"][k] - v) <= 1e-4 * max(1.0, abs(v)), (k, v, b["first_step_losses"][k])
    for k in a["losses"]:
        assert np.isfinite(b["losses"][k]) and np.isfinite(a["losses"][k])
    # a run that issues the multi-rank collectives times its EAGER iterations first and gets that number out of the
    # process (stderr + a file) before any capture is attempted; then it captures the step and reports both
    ex = b["execution"]
    assert ex["eager_ms"] is not None and ex["eager_ms"] > 0
    assert "UCD_BENCH_EAGER {" in b["_stderr"]
    note = json.loads((tmp_path / "eager_forced.json").read_text())
    assert abs(note["ms_per_step"] - ex["eager_ms"]) < 1e-6 and note["forced_collectives"] is True
    assert ex["graph_ms"] is not None or ex["step_graph_error"] is not None, ex
    if ex["graph_ms"] is not None:
        assert b["ms_per_step"] <= min(ex["eager_ms"], ex["graph_ms"]) + 1e-9
    assert a["execution"]["eager_ms"] is None and a["execution"]["graph_ms"] is None      # a plain run has one phase


def test_bench_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    """bench.py --dump-outputs DIR at the benchmarked shape: after exactly --steps timed iterations it writes the losses of the last
    one (the numbers of the JSON line) and a fixed sample of the student's updated state as float .npy files, under 64 MB.  Two runs
    with the same arguments start from the same inputs (first-iteration losses; deterministic statistics path, UCD_STAT_ATOMIC=0) and
    dump the same elements.  Their values are not bit-equal even on that path (measured: the first iteration's losses agree, the
    state after the later steps does not; the random-weight network amplifies last-bit differences step by step), so the sampled state
    is held to a relative L2 distance: measured 6e-4 between two default runs of 20 timed + 6 warm-up steps."""
    import json
    runs = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        env = dict(os.environ, UCD_STAT_ATOMIC="0")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "3", "--no_cpu_baseline",
                            "--no_kernel_timing", "--first_step_losses", "--dump-outputs", str(d)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 2 and out["ms_per_step"] > 0
        files = {f: np.load(d / f) for f in os.listdir(d)}
        assert set(files) == {f"{k}.npy" for k in out["losses"]} | {"student_state.npy"}, sorted(files)
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        for name, v in out["losses"].items():
            assert float(files[f"{name}.npy"]) == v, name
        runs.append((out, files))
    (a, fa), (b, fb) = runs
    for k, v in a["first_step_losses"].items():
        assert abs(b["first_step_losses"][k] - v) <= 1e-5 * max(1.0, abs(v)), k
    sa, sb = fa["student_state.npy"].astype(np.float64), fb["student_state.npy"].astype(np.float64)
    assert sa.shape == sb.shape
    assert np.linalg.norm(sa - sb) <= 1e-2 * np.linalg.norm(sa), np.linalg.norm(sa - sb) / np.linalg.norm(sa)


def test_bench_full_adds_what_a_plain_run_leaves_out(tmp_path):
    """A plain bench.py run does only what its headline figure needs: its line has the same keys as a --full one, with the
    per-call table, its roofline and the CPU oracle baseline null.  --full measures those after the timed steps (small crop and
    batch: the mechanics, not the numbers)."""
    import json
    out = {}
    for mode, extra in (("plain", []), ("full", ["--full"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "3", "--global_batch", "2",
                            "--crop", "129", "--no_miopen_find"] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out[mode] = json.loads(lines[0])
    a, b = out["plain"], out["full"]
    assert set(a) == set(b)
    for d in (a, b):
        assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "images/sec" and d["higher_is_better"]
        assert all(np.isfinite(v) for v in d["losses"].values())
    assert a["kernels"] is None and a["roofline"] is None and a["cpu_baseline"] is None and a["kernel_table_config"] is None
    assert b["kernels"] and b["kernel_table_config"] and b["roofline"]["kernel"] in b["kernels"] and b["roofline"]["frac"] > 0
    assert "error" not in b["cpu_baseline"], b["cpu_baseline"]
    assert b["cpu_baseline"]["value"] > 0 and np.isfinite(b["cpu_baseline"]["loss"])


def test_aborted_backward_leaves_no_widening_copies_behind():
    """at world 1 the bf16 -> fp32 widening copies of the gradient buckets are queued and flushed in finish().  A
    backward that stops before finish() (an exception inside a later node, a whole-step capture that fails) must not leave its
    queued pairs for the next step: after the abort the next step's gradients equal those of a wrapper that never saw the abort."""
    from functools import partial
    import torch
    from ucd_amd import abn, synth
    from ucd_amd.blocks import ResidualBlock
    from ucd_amd.ddp import DistributedDataParallel
    from ucd_amd import switches
    dev = "cuda:0"
    norm = partial(abn.InPlaceABNSync, activation="leaky_relu", activation_param=0.01)
    switches.set("UCD_STAT_ATOMIC", "0")             # bit-equality below: the deterministic statistics path

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError("boom")

    def make():
        net = torch.nn.Sequential(ResidualBlock(256, (64, 64, 256), norm_act=norm), ResidualBlock(256, (64, 64, 256), norm_act=norm))
        net.load_state_dict(synth.fill_state_dict(net.state_dict(), 3))
        net = net.to(dev).to(memory_format=torch.channels_last).train()
        return net, DistributedDataParallel(net, bf16_weights=True, bucket_mb=0.05)      # several small buckets

    x0 = synth.t_normal(4, (2, 256, 9, 9), stream=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    x1 = synth.t_normal(5, (2, 256, 9, 9), stream=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    grads = []
    for abort in (True, False):
        net, mod = make()
        assert len(mod.reducer.buckets) >= 3
        if abort:
            # the second block's gradients (the first buckets) complete, then the backward dies between the two blocks
            with torch.autocast("cuda", dtype=torch.bfloat16):
                h = net[0](x0)
                y = net[1](Boom.apply(h))
            mod.reducer.prepare_step()
            with pytest.raises(RuntimeError, match="boom"):
                y.float().sum().backward()
            assert mod.reducer._late_src, "the aborted backward queued nothing: the test does not exercise the hazard"
        mod.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(x1)
        y.float().square().mean().backward()
        mod.finish_grad_sync()
        assert not mod.reducer._late_src
        torch.cuda.synchronize()
        grads.append({n: p.grad.float().clone() for n, p in net.named_parameters()})
    switches.unset("UCD_STAT_ATOMIC")
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


_IPC_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ["UCD_IPC_SYNC"] = "1"        # the ranks share the GPU: "auto" would decline
from ucd_amd import hip
from ucd_amd.comm import direct_comm
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
comm = direct_comm(None)
assert comm is not None and comm.ipc, "the mailbox communicator was not created"
lib = hip.load()
g = torch.Generator(dev).manual_seed(100 + rank)
def exchange(n, seed):
    mine = torch.randn(n, device=dev, generator=g)
    red = mine.clone()
    hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(red), n, hip.stream()), "all_reduce")
    gat = torch.empty(world * n, device=dev)
    hip._check(lib.ucd_comm_all_gather(comm.handle, hip.ptr(mine), hip.ptr(gat), n, hip.stream()), "all_gather")
    return mine, red, gat
for it in range(200):
    n = (8, 512, 4096, 32768)[it % 4]
    mine, red, gat = exchange(n, it)
    ref = [torch.empty(n, device=dev) for _ in range(world)]
    dist.all_gather(ref, mine)
    assert torch.equal(gat, torch.cat(ref)), ("gather", it)
    acc = torch.zeros(n, device=dev)
    for r in ref:                       # rank order: the kernel's order, so the sums are bit-identical
        acc += r
    assert torch.equal(red, acc), ("reduce", it)
# back to back, no host synchronisation between exchanges (the way a training step issues them): every rank can regenerate every
# rank's vectors from (rank, exchange index), so the results are checked afterwards without any further communication; other
# kernels of varying length run between the exchanges so that the ranks drift against each other
def vec(r, j, n):
    return torch.randn(n, device=dev, generator=torch.Generator(dev).manual_seed(7919 * j + r))
sizes = (128, 4096, 260, 8192, 16384, 13, 32768, 1024)
for burst in range(6):
    outs = []
    filler = torch.randn(1 << (14 + (burst + rank) % 5), device=dev)
    for j in range(64):
        n = sizes[j % len(sizes)]
        idx = burst * 64 + j
        buf = vec(rank, idx, n)
        if j % 3 == 2:
            gat = torch.empty(world * n, device=dev)
            hip._check(lib.ucd_comm_all_gather(comm.handle, hip.ptr(buf), hip.ptr(gat), n, hip.stream()), "all_gather")
            outs.append((idx, n, True, gat))
        else:
            hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(buf), n, hip.stream()), "all_reduce")
            outs.append((idx, n, False, buf))
        if (j + rank) % 4 == 0:
            filler = filler * 1.0001 + 0.5
    torch.cuda.synchronize()
    for idx, n, is_gather, got in outs:
        ref = [vec(r, idx, n) for r in range(world)]
        if is_gather:
            assert torch.equal(got, torch.cat(ref)), ("burst gather", idx, n)
        else:
            acc = torch.zeros(n, device=dev)
            for r in ref:
                acc += r
            assert torch.equal(got, acc), ("burst reduce", idx, n)
# inside a captured graph: the sequence counter lives on the device, so a replay is another pair of exchanges
buf = torch.full((2048,), float(rank + 1), device=dev)
work = buf.clone()
torch.cuda.synchronize(); dist.barrier()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph, capture_error_mode="thread_local"):
    work.copy_(buf)
    hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(work), 2048, hip.stream()), "all_reduce")
    hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(work), 2048, hip.stream()), "all_reduce")
for _ in range(5):
    graph.replay()
torch.cuda.synchronize()
tot = world * (world + 1) // 2
assert torch.equal(work, torch.full((2048,), float(tot * world), device=dev)), work[:4]
assert lib.ucd_comm_ipc_timeouts(comm.handle) == 0
dist.barrier()
print("IPC_OK", rank, flush=True)
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world", [2, 4])
def test_ipc_mailbox_exchange_several_ranks_on_one_gpu(tmp_path, world):
    """the one-shot mailbox exchange (csrc/comm.hip: hipIpcMemHandle-shared mailboxes, peer stores, system-scope
    fence, sequence flags, bounded spin, sum in rank order) between real processes - which RCCL refuses on one device.  200 rounds of
    all-reduce + all-gather over four message sizes against torch.distributed's results (bit-identical: the sum runs in rank order on
    every rank), then two exchanges inside a captured graph replayed five times."""
    script = tmp_path / "ipc_worker.py"
    script.write_text(_IPC_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29741 + world), str(script), ROOT], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("IPC_OK") == world, r.stdout[-2000:]


_IPC_TIMEOUT_WORKER = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ["UCD_IPC_TIMEOUT_MS"] = "300"
os.environ["UCD_IPC_SYNC"] = "1"
from ucd_amd import hip
from ucd_amd.comm import direct_comm
dist.init_process_group("gloo")
rank = dist.get_rank()
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
comm = direct_comm(None)
assert comm is not None and comm.ipc
lib = hip.load()
v = torch.ones(16, device=dev)
hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(v), 16, hip.stream()), "both ranks: a served exchange")
torch.cuda.synchronize()
assert torch.equal(v, torch.full((16,), 2.0, device=dev)) and lib.ucd_comm_ipc_timeouts(comm.handle) == 0
dist.barrier()
if rank == 0:
    t0 = time.time()
    hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(v), 16, hip.stream()), "rank 0 alone: the launch itself succeeds")
    torch.cuda.synchronize()                                   # returns once the kernel gave up
    dt = time.time() - t0
    assert 0.2 < dt < 10.0, dt
    assert lib.ucd_comm_ipc_timeouts(comm.handle) != 0
    assert bool(torch.isnan(v).all()), v                       # round 6: an exchange that did not complete returns NaN, not a partial sum
    try:
        hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(v), 16, hip.stream()), "next exchange")
        raise SystemExit("the latched timeout was not reported")
    except RuntimeError as e:
        assert "timed out" in str(e), e
    from ucd_amd.comm import check_mailbox
    try:
        check_mailbox(None)
        raise SystemExit("check_mailbox did not raise")
    except RuntimeError as e:
        assert "timed out" in str(e), e
    print("IPC_TIMEOUT_OK %.2f" % dt, flush=True)
dist.barrier()                                                 # rank 1 never entered the second exchange
if rank == 1:
    # rank 0's timeout POISONED every rank's mailbox: rank 1's next exchange - inside a replayed graph, where no host call could
    # report anything - returns NaN at once instead of waiting out the timeout and summing stale slots
    assert lib.ucd_comm_ipc_timeouts(comm.handle) == 0
    w = torch.ones(4096, device=dev)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            hip._check(lib.ucd_comm_all_reduce_sum(comm.handle, hip.ptr(w), 4096, hip.stream()), "captured exchange")
    torch.cuda.synchronize()
    t0 = time.time()
    g.replay()
    torch.cuda.synchronize()
    dt1 = time.time() - t0
    assert dt1 < 0.2, dt1                                      # no 300 ms wait
    assert bool(torch.isnan(w).all()), w[:4]
    assert lib.ucd_comm_ipc_timeouts(comm.handle) != 0
    print("IPC_POISON_OK %.4f" % dt1, flush=True)
dist.barrier()
dist.destroy_process_group()
"""


def test_ipc_mailbox_timeout_is_an_error_not_a_hang(tmp_path):
    """A peer that never arrives: rank 0 of two real processes enters an exchange rank 1 skips.  The exchange kernel gives up after
    UCD_IPC_TIMEOUT_MS (300 ms here), latches the word in pinned host memory, and the NEXT collective on that communicator returns
    UCD_ETIMEOUT (a RuntimeError through the bindings) - the process does not hang and the step is not silently wrong."""
    script = tmp_path / "ipc_timeout_worker.py"
    script.write_text(_IPC_TIMEOUT_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29747", str(script), ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "IPC_TIMEOUT_OK" in r.stdout and "IPC_POISON_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_a_parameter_without_gradient_gets_a_zero_not_last_steps_gradient():
    """Round 6: the fp32 gradient buckets whose every slot is overwritten by the widening copy of a bf16 gradient are no longer
    memset per step (232 MB at the bench size).  A parameter that receives NO gradient in a step (a branch the loss does not reach)
    must then still read zero - its slot is cleared when its bucket completes - never the previous step's gradient."""
    from functools import partial
    import torch
    from ucd_amd import abn, synth
    from ucd_amd.blocks import ResidualBlock
    from ucd_amd.ddp import DistributedDataParallel
    dev = "cuda:0"
    norm = partial(abn.InPlaceABNSync, activation="leaky_relu", activation_param=0.01)

    class Two(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = ResidualBlock(256, (64, 64, 256), norm_act=norm)
            self.b = ResidualBlock(256, (64, 64, 256), norm_act=norm)

        def forward(self, x, use_b=True):
            h = self.a(x)
            return self.b(h) if use_b else h

    net = Two()
    net.load_state_dict(synth.fill_state_dict(net.state_dict(), 3))
    net = net.to(dev).to(memory_format=torch.channels_last).train()
    mod = DistributedDataParallel(net, bf16_weights=True, bucket_mb=0.05)
    assert any(len(b.fed) == len(b.params) for b in mod.reducer.buckets), "no bucket without a memset: the test exercises nothing"
    x = synth.t_normal(4, (2, 256, 9, 9), stream=1).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
    for use_b in (True, False):
        mod.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = mod(x, use_b=use_b)
        y.float().square().mean().backward()
        mod.finish_grad_sync()
        torch.cuda.synchronize()
        gb = net.b.convs.conv2.weight.grad
        ga = net.a.convs.conv2.weight.grad
        assert ga is not None and float(ga.abs().sum()) > 0
        if use_b:
            assert float(gb.abs().sum()) > 0
        else:
            assert gb is None or float(gb.abs().sum()) == 0.0, "a stale gradient survived in a bucket slot"
