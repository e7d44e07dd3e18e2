"""GPU: the MULTI-RANK (SyncBN) forms of the fused norm kernels, three "ranks" held in one process, against float64.

One process per GPU with InPlaceABNSync everywhere is the product, and under SyncBN every norm layer runs another kernel sequence
than the single-process one: per-rank moments -> gather / all-reduce -> a finalise with count = world * M, and a backward whose
per-element term takes the GLOBAL sums while the parameter gradients take THIS RANK's.  Here the ranks run one after another on
the default stream and the collectives are torch ops (``torch.stack`` = all-gather, an elementwise sum of the per-rank buffers -
every replica of an accumulator - = all-reduce); each rank owns its running statistics.  The reference (oracle/syncbn_forms.py)
is training-mode batch norm over the concatenated batch, the activation and the stem's max pool in float64 on the CPU, computed
from the values the kernels read (the bf16 activations; for the conv paths the bf16 product the conv call STORED - the GEMM has
its own tests).  Inputs: rank offsets of +0 / +2 / -3 channel stds (the between-rank term is most of the variance), one channel
with a negative stored weight, every layer under UCD_NORM_ABS_GAMMA.

Bars (oracle/syncbn_forms.py): fp32 quantities - statistics, constants, running statistics, packs, parameter-gradient sums - at
those of test_abn_gpu.py::test_sync_forward_backward_kernels_match_global_batch (fp32 case); bf16 tensors per element within one
bf16 ulp of the float64 value plus what the fp32 bars of the constants may move it by, and below 2^-9 in relative L2; the atomic
sums about a shift within 4 x the error of a sequential fp32 restatement on the CPU.  tests/test_syncbn_forms_cpu.py shows that
dropping the between-rank term, count = M, parameter gradients from the global sums and a lost sign of the negative weight each
move the reference by >= 10 x these bars.  Measured errors: profiles/syncbn_forms.md (every check prints its figure)."""
import functools

import pytest
import torch

from oracle import syncbn_forms as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = R.WORLD
ACTS = {"leaky_relu": R.SLOPE, "identity": 1.0}
STEM_SHAPES = [(2, 64, 9, 11), (1, 64, 8, 8)]          # pooled 5 x 6 (odd and even edge) and 4 x 4 (even map)


def _code(act):
    from ucd_amd import hip
    return hip.ACT_CODES[act] | hip.NORM_ABS_GAMMA


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _close(got, ref, bar_, what):
    got = got.detach().double().cpu()
    err, allow = (got - ref).abs(), R.bar(ref, **bar_)
    print("syncbn-forms | %s | max err %.3e | worst err / bar %.3f" % (what, err.max().item(), (err / allow).max().item()))
    assert (err <= allow).all(), (what, (err / allow).max().item())


def _bf16_close(got, ref, prop, what):
    """Per element one bf16 ulp of the float64 value + the propagated fp32 bars; relative L2 below 2^-9."""
    got = got.detach().double().cpu()
    err, allow = (got - ref).abs(), R.BF16_ULP * ref.abs() + prop
    l2 = ((got - ref).norm() / ref.norm()).item()
    print("syncbn-forms | %s | rel L2 %.3e (bar %.3e) | worst err / bar %.3f" % (what, l2, R.BF16_L2, (err / allow).max().item()))
    assert (err <= allow).all(), (what, (err / allow).max().item(), int((err > allow).sum()))
    assert l2 < R.BF16_L2, (what, l2)


def _constants(bufs, rms, rvs, k, C, what):
    """mean | invstd | scale in buf[3C:6C] and the running statistics of every rank against float64; ranks bit-identical."""
    for r, (buf, rm, rv) in enumerate(zip(bufs, rms, rvs)):
        _close(buf[3 * C:4 * C], k["mean"], R.BAR_MEAN, what + " mean r%d" % r)
        _close(buf[4 * C:5 * C], k["invstd"], R.BAR_INVSTD, what + " invstd r%d" % r)
        _close(buf[5 * C:6 * C], k["scale"], R.BAR_SCALE, what + " scale r%d" % r)
        _close(rm, k["running_mean"], R.BAR_RMEAN, what + " running mean r%d" % r)      # one update: a second one would be 0.9 x off
        _close(rv, k["running_var"], R.BAR_RVAR, what + " running var r%d" % r)
        assert torch.equal(buf[3 * C:6 * C], bufs[0][3 * C:6 * C]), (what, "constants differ between ranks", r)


def _packs(packs, k, M, what):
    C = packs[0].numel() // 2
    for r, p in enumerate(packs):
        _close(p[:C], k["packs"][r][0], R.BAR_MEAN, what + " pack mean r%d" % r)
        _close(p[C:], k["packs"][r][1], dict(rtol=R.BAR_VAR["rtol"], atol=R.BAR_VAR["atol"] * M), what + " pack M2 r%d" % r)


def _params(case):
    return [case[n].to(DEV) for n in ("weight", "bias")], [case[n].double() for n in ("weight", "bias", "running_mean", "running_var")]


# ---------------------------------------------------------------------------------------------
# the stem
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem(shape, act):
    """Sequence 1 on the device + its float64 reference, shared by the forward and the backward test."""
    from ucd_amd import hip
    slope = ACTS[act]
    case = R.stem_case(shape, slope)
    B, C, H, Wd = shape
    M = B * H * Wd
    (weight, bias), P = _params(case)
    zs = [_cl(z) for z in case["zs"]]
    packs, bufs = [], []
    for z in zs:
        buf = torch.zeros(8 * C, device=DEV)
        hip.abn_sync_stats(z, C, M, C, None, H * Wd, buf[:2 * C], buf[2 * C:3 * C], buf[6 * C:])
        packs.append(buf[6 * C:].clone()); bufs.append(buf)
    gathered = torch.stack(packs).contiguous()
    rms, rvs, outs, idxs = [], [], [], []
    for z, buf in zip(zs, bufs):
        rm, rv = case["running_mean"].to(DEV), case["running_var"].to(DEV)
        hip.abn_sync_finalize(gathered, W, M, C, weight, rm, rv, R.MOMENTUM, R.EPS, buf, _code(act))
        out, idx = hip.stem_apply_pool(z, buf[3 * C:4 * C], buf[5 * C:6 * C], bias, _code(act), slope, True)
        rms.append(rm); rvs.append(rv); outs.append(out); idxs.append(idx)
    z64 = [z.double() for z in case["zs"]]
    k = R.stem_forward(z64, *P, slope)
    return dict(case=case, zs=zs, z64=z64, packs=packs, bufs=bufs, rms=rms, rvs=rvs, outs=outs, idxs=idxs, k=k, weight=weight,
                bias=bias, P=P, M=M, slope=slope)


@pytest.mark.parametrize("shape", STEM_SHAPES)
@pytest.mark.parametrize("act", list(ACTS))
def test_stem_forward_per_rank_moments_gather_finalize_and_pool(shape, act):
    """Sequence 1: ucd_abn_sync_stats per rank -> gather -> ucd_abn_sync_finalize on every rank -> ucd_stem_apply_pool (the ``sync``
    arm of ucd_amd.abn's stem function)."""
    s = _stem(shape, act)
    k, C, what = s["k"], shape[1], "stem fwd %s %s" % (shape, act)
    _packs(s["packs"], k, s["M"], what)
    _constants(s["bufs"], s["rms"], s["rvs"], k, C, what)
    for r, (z, out) in enumerate(zip(s["z64"], s["outs"])):
        allow = R.maps_of(R.y_allowance(R.rows_of(z), k), z).flatten(2).gather(2, k["idx"][r])
        assert out.shape == (shape[0], C, (shape[2] + 1) // 2, (shape[3] + 1) // 2)
        _bf16_close(out.flatten(2), k["pooled"][r], allow, what + " pooled r%d" % r)


@pytest.mark.parametrize("shape", STEM_SHAPES)
@pytest.mark.parametrize("act", list(ACTS))
def test_stem_backward_phase_one_all_reduce_phase_two(shape, act):
    """Sequence 2: ucd_stem_pool_backward phase 1 per rank -> sum of the sums over the ranks -> phase 2 with count = world * M.  A
    rank's phase-1 sums are ITS [d bias | d weight * sign(weight)]; dz takes the summed ones."""
    from ucd_amd import hip
    s = _stem(shape, act)
    case, k, C, M, slope = s["case"], s["k"], shape[1], s["M"], s["slope"]
    what = "stem bwd %s %s" % (shape, act)
    dps = [_cl(dp.view(shape[0], C, *s["outs"][0].shape[2:])) for dp in case["dpools"]]
    bw = R.stem_backward(s["z64"], [dp.double() for dp in case["dpools"]], k, s["P"][0], slope)

    def phase(r, sums, count, dz, ph):
        buf = s["bufs"][r]
        hip.stem_pool_backward(s["zs"][r], dps[r], s["idxs"][r], buf[3 * C:4 * C], buf[4 * C:5 * C], buf[5 * C:6 * C], s["bias"],
                               s["weight"], sums, count, _code(act), slope, dz, ph)
    local = [torch.empty(2 * C, device=DEV) for _ in range(W)]
    for r in range(W):
        phase(r, local[r], float(W * M), None, 1)
        _close(local[r], torch.cat(bw["local"][r]), R.BAR_GRAD_SUMS, what + " phase-1 sums r%d" % r)
    total = torch.stack(local).sum(0)
    for r in range(W):
        dz = torch.empty_like(s["zs"][r])
        phase(r, total, float(W * M), dz, 2)
        x = R.rows_of(s["z64"][r])
        _bf16_close(R.rows_of(dz), bw["dx"][r], R.dx_allowance(x, bw["dx"][r], k, bw), what + " dz r%d" % r)


@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_backward_phase_three_is_phase_one_then_two(shape):
    """world = 1: the single launch sequence (phase 3) equals phase 1 followed by phase 2 BIT FOR BIT - csrc/stem.hip reduces in a
    fixed order (per-workgroup partial rows, a fixed tree over them; no atomics), and phase 3 is the same two kernels."""
    from ucd_amd import hip
    s = _stem(shape, "leaky_relu")
    C, M, r = shape[1], s["M"], 1
    z, idx, buf = s["zs"][r], s["idxs"][r], s["bufs"][r]
    dp = _cl(s["case"]["dpools"][r].view(shape[0], C, *s["outs"][0].shape[2:]))
    args = (z, dp, idx, buf[3 * C:4 * C], buf[4 * C:5 * C], buf[5 * C:6 * C], s["bias"], s["weight"])
    s3, s12 = torch.empty(2 * C, device=DEV), torch.empty(2 * C, device=DEV)
    dz3, dz12 = torch.empty_like(z), torch.empty_like(z)
    hip.stem_pool_backward(*args, s3, float(M), _code("leaky_relu"), R.SLOPE, dz3, 3)
    hip.stem_pool_backward(*args, s12, float(M), _code("leaky_relu"), R.SLOPE, None, 1)
    hip.stem_pool_backward(*args, s12, float(M), _code("leaky_relu"), R.SLOPE, dz12, 2)
    assert torch.equal(s3, s12) and torch.equal(dz3, dz12)
    assert dz3.float().abs().sum() > 0


# ---------------------------------------------------------------------------------------------
# the conv paths
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv():
    case = R.conv_case()
    case.update(R.link_case(case))
    return case


def _applied(ys, outs, k, bias64, slope, what):
    for r, (y, out) in enumerate(zip(ys, outs)):
        y64 = y.double().cpu()
        _bf16_close(out, R.apply_rows(y64, k, bias64, slope)[1], R.y_allowance(y64, k), what + " y r%d" % r)


@pytest.mark.parametrize("act", list(ACTS))
def test_row_partial_path_pack_gather_sync_forward(act):
    """Sequence 3: ucd_conv1x1 out_mode 2 with per-tile partial rows (no accumulator) -> ucd_conv1x1_stats_finalize with a pack ->
    gather -> ucd_abn_sync_forward.  286 rows per rank = three row tiles, the last one ragged."""
    from ucd_amd import hip
    case, slope = _conv(), ACTS[act]
    M, N = case["M"], case["N"]
    (weight, bias), P = _params(case)
    w = case["w"].to(DEV)
    assert hip.conv1x1_row_tiles(M) == 3
    ys, packs, bufs = [], [], []
    for a in case["a"]:
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        part = hip.conv1x1_stats_partial(M, N, DEV)
        hip.conv1x1(a.to(DEV), w, y, out_mode=2, partial=part)
        buf, pack = torch.zeros(6 * N, device=DEV), torch.empty(2 * N, device=DEV)
        hip.conv1x1_stats_finalize(part, M, N, None, None, None, R.MOMENTUM, R.EPS, buf, pack)
        ys.append(y); packs.append(pack); bufs.append(buf)
    gathered = torch.stack(packs).contiguous()
    rms, rvs, outs = [], [], []
    for y, buf in zip(ys, bufs):
        rm, rv = case["running_mean"].to(DEV), case["running_var"].to(DEV)
        out = torch.empty_like(y)
        hip.abn_sync_forward(y, N, out, N, None, 0, M, N, None, 1, gathered, W, weight, bias, rm, rv, R.MOMENTUM, R.EPS, buf,
                             _code(act), slope)
        rms.append(rm); rvs.append(rv); outs.append(out)
    k = R.forward_constants([y.double().cpu() for y in ys], *P[:1], *P[2:])
    what = "row-partial [%d, %d] x3 %s" % (M, N, act)
    _packs(packs, k, M, what)
    _constants(bufs, rms, rvs, k, N, what)
    _applied(ys, outs, k, P[1], slope, what)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("reps", ["library", 2])
def test_atomic_path_summed_accumulators_and_the_finalising_apply(act, reps):
    """Sequence 4: ucd_conv1x1 out_mode 2 into an atomic accumulator about a shift that all ranks share -> sum of the accumulators
    (every replica) over the ranks -> ucd_abn_apply_stats with count = world * M on every rank.  The sums themselves are held to 4 x
    the error of a sequential fp32 restatement (the factor covers the unordered adds of at most world * row tiles terms per
    address)."""
    from ucd_amd import hip
    case, slope = _conv(), ACTS[act]
    M, N = case["M"], case["N"]
    (weight, bias), P = _params(case)
    w, shift = case["w"].to(DEV), case["shift"].to(DEV)
    rep = hip.load().ucd_conv1x1_stat_replicas(M) if reps == "library" else reps
    ys, accs, bufs = [], [], []
    for a in case["a"]:
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        acc, buf = torch.zeros(rep, 2 * N, device=DEV), torch.zeros(6 * N, device=DEV)
        hip.conv1x1(a.to(DEV), w, y, out_mode=2, partial=buf[2 * N:3 * N], stat_acc=acc, stat_shift=shift, stat_rep=rep)
        assert torch.equal(buf[2 * N:3 * N], shift)                    # the snapshot of the shift
        assert rep == 1 or acc[rep - 1].abs().sum() > 0                # every replica took adds
        ys.append(y); accs.append(acc); bufs.append(buf)
    total = torch.stack(accs).sum(0)                                   # the all-reduce: [rep, 2 N]
    rms, rvs, outs = [], [], []
    for y, buf in zip(ys, bufs):
        rm, rv = case["running_mean"].to(DEV), case["running_var"].to(DEV)
        out = torch.empty_like(y)
        hip.abn_apply_stats(y, out, None, M, N, total, buf[2 * N:3 * N], float(W * M), weight, bias, rm, rv, R.MOMENTUM, R.EPS, buf,
                            _code(act), slope, reps=rep)
        rms.append(rm); rvs.append(rv); outs.append(out)
    y64 = [y.double().cpu() for y in ys]
    what = "atomic fwd [%d, %d] x3 reps %d %s" % (M, N, rep, act)
    for name, rows, got in [("r%d" % r, y64[r], accs[r].sum(0)) for r in range(W)] + [("all ranks", torch.cat(y64), total.sum(0))]:
        ref, f32 = R.shifted_sums(rows, case["shift"]), R.shifted_sums(rows, case["shift"], torch.float32)
        for j, part in enumerate(("sum (y - k)", "sum (y - k)^2")):
            allow = 4 * (f32[j].double() - ref[j]).abs().max().item()
            _close(got[j * N:(j + 1) * N], ref[j], dict(rtol=0.0, atol=allow), "%s %s %s" % (what, part, name))
    k = R.forward_constants(y64, *P[:1], *P[2:])
    _constants(bufs, rms, rvs, k, N, what)
    _applied(ys, outs, k, P[1], slope, what)


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("mode", [3, 4])
def test_atomic_path_backward_global_sums_and_local_parameter_gradients(act, mode):
    """Sequence 5: the link epilogue (out_mode 3: d pre from the layer's own pre-activation; out_mode 4: the block link - sign from
    the block output, the shortcut's gradient folded in) adds its sums into ``stat_acc`` (summed over the ranks afterwards) and
    ``stat_acc2`` (stays local); ucd_abn_bwd_apply_raw then takes sums = global, grad_sums = local, count = world * M and writes
    this rank's [d bias | d weight * sign(weight)] to grad_out."""
    from ucd_amd import hip
    case, slope = _conv(), ACTS[act]
    M, N = case["M"], case["N"]
    (weight, bias), P = _params(case)
    x64 = [y.double() for y in case["ys"]]                             # the layer's pre-norm input (what the epilogue reads)
    k = R.forward_constants(x64, *P[:1], *P[2:])
    mean, invstd, scale = (k[n].float().to(DEV) for n in ("mean", "invstd", "scale"))
    wg = case["wg"].to(DEV)
    rep = hip.load().ucd_conv1x1_stat_replicas(M)
    tiles = hip.conv1x1_row_tiles(M)
    plain = hip.ACT_CODES[act]
    what = "atomic bwd out_mode %d [%d, %d] x3 %s" % (mode, M, N, act)
    xs, dzs, acc1, acc2 = [], [], [], []
    for r in range(W):
        x, g = case["ys"][r].to(DEV), case["g"][r].to(DEV)
        a1, a2 = torch.zeros(rep, 2 * N, device=DEV), torch.zeros(rep, 2 * N, device=DEV)
        part = torch.empty(tiles, 2, N, device=DEV)
        if mode == 3:
            dz = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            hip.conv1x1(g, wg, dz, out_mode=3, out_norm=(mean, scale, bias, invstd, plain, slope), residual=x, partial=part,
                        stat_acc=a1, stat_acc2=a2, stat_rep=rep)
            pre = (x64[r] - k["mean"]) * k["scale"] + P[1]
            assert pre.abs().min() > 1e-5                              # no derivative hangs on the last fp32 bit
        else:
            dz = case["skip"][r].to(DEV).clone()
            hip.conv1x1(g, wg, dz, out_mode=4, out_norm=(mean, None, None, invstd, plain, slope), residual=case["out"][r].to(DEV),
                        side2=x, accumulate=True, partial=part, stat_acc=a1, stat_acc2=a2, stat_rep=rep)
        # the stored d pre against float64 (fp32 accumulation of 192 products on top of the bf16 rounding)
        g64, w64 = case["g"][r].double(), case["wg"].double()
        ref = R.link_dpre(g64 @ w64.t(), x64[r], k, P[1], slope, mode, case["out"][r].double(), case["skip"][r].double())
        _bf16_close(dz, ref, R.LINK_K * 2.0 ** -24 * (g64.abs() @ w64.abs().t()), what + " d pre r%d" % r)
        xs.append(x); dzs.append(dz); acc1.append(a1); acc2.append(a2)
    dz64 = [dz.double().cpu() for dz in dzs]
    bw = R.backward_rows(x64, dz64, k, P[0])
    for r in range(W):
        # both accumulators took the same <= row-tiles adds per address, each in its own order: two orders of n adds differ by at
        # most 2 n roundings of the running magnitude, 8 x 2^-24 x sum |term| covers three tiles (five 64-row tiles: 10 < 16)
        xh = (x64[r] - k["mean"]) * k["invstd"]
        mag = torch.cat([dz64[r].abs().sum(0), (dz64[r] * xh).abs().sum(0)])
        gap = (acc1[r].sum(0) - acc2[r].sum(0)).abs().double().cpu()
        assert (gap <= 16 * 2.0 ** -24 * mag).all(), (what, "stat_acc / stat_acc2", r, (gap / mag).max().item())
        raw = torch.cat([dz64[r].sum(0), (dz64[r] * xh).sum(0)])      # no sign on the accumulators
        _close(acc1[r].sum(0), raw, R.BAR_GRAD_SUMS, what + " stat_acc r%d" % r)
        _close(acc2[r].sum(0), raw, R.BAR_GRAD_SUMS, what + " stat_acc2 r%d" % r)
    total = torch.stack(acc1).sum(0)                                   # the all-reduce of stat_acc; stat_acc2 stays
    _close(total.sum(0), torch.cat(bw["total"]), R.BAR_GRAD_SUMS, what + " summed stat_acc")
    for r in range(W):
        gout = torch.full((2 * N,), float("nan"), device=DEV)
        dx, dzo = torch.empty_like(dzs[r]), torch.empty_like(dzs[r])
        hip.abn_bwd_apply_raw(xs[r], dzs[r], None, dx, dzo, M, N, mean, invstd, scale, bias, weight, total, acc2[r], gout,
                              float(W * M), hip.ACT_IDENTITY | hip.NORM_ABS_GAMMA, 0.0, reps=rep)
        _close(gout, torch.cat(bw["local"][r]), R.BAR_GRAD_SUMS, what + " grad_out r%d" % r)
        _bf16_close(dx, bw["dx"][r], R.dx_allowance(x64[r], bw["dx"][r], k, bw), what + " dx r%d" % r)
        assert torch.equal(dzo, dzs[r])                                # identity activation: dz_out is d pre itself
