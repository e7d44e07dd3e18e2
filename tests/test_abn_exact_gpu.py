"""GPU: every ABN pass of ucd_amd/csrc/abn.hip against float64 on operands where fp32 is exact, once per launch geometry class.

The operands (abn_exact_ref.operands) are small integers and powers of two, so every fp32 partial sum and every element-wise
result is exact whatever the order of summation (tests/test_abn_exact_cpu.py proves it for each case): the comparisons are
``torch.equal`` against the float64 reference cast to the output type, and one dropped, repeated or misplaced row, band, lane or
replica fails them at any size.  Three things cannot be exact and are compared under bounds written next to the assertion: the
finalised constants (1 / M, rsqrt), window means whose area is no power of two (one rounded multiply), and the one real-valued
case that holds the shifted sums to the precision they exist for.
"""
import functools

import pytest
import torch

import abn_exact_ref as R
from ucd_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.0
MOMENTUM = 0.125          # a power of two: 1 - momentum and momentum * mean are exact
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))      # the eps the library receives (a C float)


# ---------------------------------------------------------------------------------------------------------------------
# operands on the device: dense, or channel slices of a wider buffer
# ---------------------------------------------------------------------------------------------------------------------
class Rows:
    """An [M, C] activation on the device.  pad = 0: dense (ld = C).  pad = k > 0: columns 8 .. 8 + C of a buffer that is 8 (k + 1)
    columns wider - every operand of a call gets another k, so no two share an ld - whose other columns hold `fill`."""

    def __init__(self, M, C, td, pad, fill, value=None):
        self.C, self.ld, self.td = C, C + (8 * (pad + 1) if pad else 0), td
        self.buf = torch.full((M, self.ld), fill, dtype=td, device=DEV)
        self.t = self.buf[:, 8:8 + C] if pad else self.buf
        if value is not None:
            self.t.copy_(value.to(td))

    def assert_is(self, ref64, what):
        """The slice equals the float64 reference cast to the storage type, and nothing outside the slice changed."""
        torch.cuda.synchronize()
        got, ref = self.t.cpu(), ref64.to(self.td)
        assert torch.equal(got, ref), f"{what}: {(got != ref).sum().item()} of {ref.numel()} elements differ, first row {(got != ref).any(1).nonzero()[0].item()}"
        if self.ld != self.C:
            assert (self.buf[:, :8] == SENTINEL).all() and (self.buf[:, 8 + self.C:] == SENTINEL).all(), f"{what}: wrote outside its slice"


def rows_in(t64, td, pad):
    return Rows(t64.shape[0], t64.shape[1], td, pad, float("nan"), t64)


def vec(t64):
    return None if t64 is None else t64.to(torch.float32).contiguous().to(DEV)


def f64(t):
    return t.detach().cpu().to(torch.float64)


class CaseData:
    def __init__(self, name):
        self.name, self.cs, self.o = name, R.CASES[name], R.operands(name)
        o, cs = self.o, self.cs
        self.td = R.torch_dtype(cs.dtype)
        self.M, self.C, self.HW, self.slope, self.act = o["M"], o["C"], o["HW"], o["slope"], cs.act
        p = 1 if cs.pad else 0
        self.x, self.dy, self.res = rows_in(o["x"], self.td, 1 * p), rows_in(o["dy"], self.td, 2 * p), rows_in(o["res"], self.td, 3 * p)
        self.pb = vec(o["pb"])
        for k in ("mean", "invstd", "scale", "shift", "weight", "sums_in"):
            setattr(self, k, vec(o[k]))

    @functools.cached_property
    def y_res64(self):
        """the stored output of the layer with its residual: the sign source of the from-y backward forms"""
        o = self.o
        return R.apply(o["x"], o["pb"], self.HW, o["mean"], o["scale"], o["shift"], o["res"], self.slope)

    @functools.cached_property
    def y_res(self):
        return rows_in(self.y_res64, self.td, 4 if self.cs.pad else 0)

    def out(self, k):
        return Rows(self.M, self.C, self.td, k if self.cs.pad else 0, SENTINEL)


_data = {}


def _case_data(name):
    if name not in _data:          # one case on the device at a time
        _data.clear()
        _data[name] = CaseData(name)
    return _data[name]


@pytest.fixture(scope="module", params=list(R.CASES))
def case(request):
    return _case_data(request.param)


@pytest.fixture(scope="module", params=[n for n, c in R.CASES.items() if c.passes == "all"])
def full_case(request):
    return _case_data(request.param)


@pytest.fixture(scope="module", params=[n for n, c in R.CASES.items() if c.passes == "all" and c.dtype == "bf16"])
def bf16_case(request):
    return _case_data(request.param)


def _nan_workspace(M, C):
    nbytes = hip.load().ucd_abn_workspace_bytes(M, C)
    assert nbytes == R.K_MAX_BANDS * 2 * C * 4
    return torch.full((R.K_MAX_BANDS, 2 * C), float("nan"), dtype=torch.float32, device=DEV), nbytes


def _rows_written(ws):
    """number of leading workspace rows the kernel wrote in full; nothing behind them may be touched"""
    written = ~torch.isnan(ws)
    n = int(written.all(1).sum().item())
    assert written[:n].all() and not written[n:].any()
    return n


# ---------------------------------------------------------------------------------------------------------------------
# forward statistics and the backward reduction
# ---------------------------------------------------------------------------------------------------------------------
def test_stats_sums_and_shift_are_exact(case):
    d, o = case, case.o
    sums, ks = torch.zeros(2 * d.C, device=DEV), torch.zeros(d.C, device=DEV)
    hip.abn_stats(d.x.t, d.x.ld, d.M, d.C, d.pb, d.HW, sums, ks)
    s, ss, k = R.stats(o["x"], o["pb"], d.HW)
    assert torch.equal(ks.cpu(), k.to(torch.float32))
    assert torch.equal(sums.cpu(), torch.cat([s, ss]).to(torch.float32))


def test_stats_band_count_and_partial_rows(case):
    """The one place where the Python restatement of make_geom meets the library: the kernel writes exactly the predicted number
    of partial rows into a NaN-filled workspace, and each row holds its band's sums."""
    d, o = case, case.o
    lib = hip.load()
    ws, nbytes = _nan_workspace(d.M, d.C)
    sums, ks = torch.zeros(2 * d.C, device=DEV), torch.zeros(d.C, device=DEV)
    hip._check(lib.ucd_abn_stats(hip.ptr(d.x.t), d.x.ld, hip.dtype_code(d.x.t), d.M, d.C, hip.ptr(d.pb), d.HW, hip.ptr(sums), hip.ptr(ks),
                                 hip.ptr(ws), nbytes, hip.stream()), "ucd_abn_stats")
    torch.cuda.synchronize()
    g = R.reduce_geom(d.M, d.C, d.cs.dtype)
    assert _rows_written(ws) == g.gy
    f = R.biased(o["x"], o["pb"], d.HW) - R.biased(o["x"], o["pb"], d.HW)[0]
    total, partial = R.two_stage_sum(torch.cat([f, f * f], 1), g)
    assert torch.equal(ws[:g.gy].cpu(), partial.to(torch.float32))
    assert torch.equal(sums.cpu(), total.to(torch.float32))


@pytest.mark.parametrize("abs_gamma", [False, True], ids=["gamma", "abs_gamma"])
@pytest.mark.parametrize("from_y", [False, True], ids=["sign_from_x", "sign_from_y"])
def test_bwd_reduce_is_exact(case, from_y, abs_gamma):
    d, o = case, case.o
    y, y64 = (d.y_res, d.y_res64) if from_y else (None, None)
    sums = torch.zeros(2 * d.C, device=DEV)
    hip.abn_bwd_reduce(d.x.t, d.x.ld, d.dy.t, d.dy.ld, y.t if y else None, y.ld if y else 0, d.M, d.C, d.pb, d.HW, d.mean, d.invstd,
                       d.scale, d.shift, d.act | (R.ABS_GAMMA if abs_gamma else 0), d.slope, sums, d.weight)
    ref = R.bwd_reduce(o["x"], o["pb"], d.HW, o["dy"], y64, o["mean"], o["invstd"], o["scale"], o["shift"], d.slope, o["weight"], abs_gamma)
    assert torch.equal(sums.cpu(), ref.to(torch.float32))


def test_bwd_reduce_band_count(case):
    d = case
    lib = hip.load()
    ws, nbytes = _nan_workspace(d.M, d.C)
    sums = torch.zeros(2 * d.C, device=DEV)
    hip._check(lib.ucd_abn_bwd_reduce(hip.ptr(d.x.t), d.x.ld, hip.ptr(d.dy.t), d.dy.ld, None, 0, hip.dtype_code(d.x.t), d.M, d.C,
                                      hip.ptr(d.pb), d.HW, hip.ptr(d.mean), hip.ptr(d.invstd), hip.ptr(d.scale), hip.ptr(d.shift), None,
                                      d.act, float(d.slope), hip.ptr(sums), hip.ptr(ws), nbytes, hip.stream()), "ucd_abn_bwd_reduce")
    torch.cuda.synchronize()
    assert _rows_written(ws) == R.reduce_geom(d.M, d.C, d.cs.dtype).gy


# ---------------------------------------------------------------------------------------------------------------------
# the element-wise passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["residual", "no_shift", "plain"])
def test_apply_is_exact(full_case, variant):
    """(the plane-bias form runs in the cases that have one)"""
    d, o = full_case, full_case.o
    res, res64 = (d.res, o["res"]) if variant == "residual" else (None, None)
    shift, shift64 = (None, None) if variant == "no_shift" else (d.shift, o["shift"])
    y = d.out(5)
    hip.abn_apply(d.x.t, d.x.ld, y.t, y.ld, res.t if res else None, res.ld if res else 0, d.M, d.C, d.pb, d.HW, d.mean, d.scale, shift,
                  d.act, d.slope)
    y.assert_is(R.apply(o["x"], o["pb"], d.HW, o["mean"], o["scale"], shift64, res64, d.slope), "y")


@pytest.mark.parametrize("variant", ["plain", "dz_out_abs_gamma", "dz_out", "frozen"])
def test_bwd_apply_is_exact(full_case, variant):
    d, o = full_case, full_case.o
    from_y = variant != "plain"
    want_dz = variant.startswith("dz_out")
    abs_gamma, frozen = variant == "dz_out_abs_gamma", variant == "frozen"
    y, y64 = (d.y_res, d.y_res64) if from_y else (None, None)
    dx, dz = d.out(5), d.out(6) if want_dz else None
    hip.abn_bwd_apply(d.x.t, d.x.ld, d.dy.t, d.dy.ld, y.t if y else None, y.ld if y else 0, dx.t, dx.ld, dz.t if dz else None,
                      dz.ld if dz else 0, d.M, d.C, d.pb, d.HW, d.mean, d.invstd, d.scale, d.shift, d.weight, d.sums_in, R.COUNT,
                      1 if frozen else 0, d.act | (R.ABS_GAMMA if abs_gamma else 0), d.slope)
    rdx, rdz = R.bwd_apply(o["x"], o["pb"], d.HW, o["dy"], y64, o["mean"], o["invstd"], o["scale"], o["shift"], d.slope, o["weight"],
                           o["sums_in"], R.COUNT, abs_gamma, frozen)
    dx.assert_is(rdx, "dx")
    if dz:
        dz.assert_is(rdz, "dz")


# ---------------------------------------------------------------------------------------------------------------------
# the forms that finalise in their prologue, from `reps` replicas
# ---------------------------------------------------------------------------------------------------------------------
def _apply_stats(x, y, res, M, C, acc, reps, ks, count, w, b, rm, rv, eps, buf, act, slope):
    if x.ld == C:
        hip.abn_apply_stats(x.t, y.t, res.t if res else None, M, C, acc, ks, count, w, b, rm, rv, MOMENTUM, eps, buf, act, slope, reps)
        return
    p = hip.ptr           # the wrapper takes dense rows only
    hip._check(hip.load().ucd_abn_apply_stats(p(x.t), x.ld, p(y.t), y.ld, p(res.t) if res else None, res.ld if res else 0, M, C, p(acc),
                                              reps, p(ks), float(count), p(w), p(b), p(rm), p(rv), MOMENTUM, float(eps), p(buf[3 * C:]),
                                              p(buf[4 * C:]), p(buf[5 * C:]), act, float(slope), hip.stream()), "ucd_abn_apply_stats")


def _assert_within(got, ref64, bound, what):
    err = (f64(got) - ref64).abs()
    worst = (err / bound.clamp_min(2.0 ** -200)).max().item()
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert (err <= bound).all(), f"{what}: error up to {worst:.2f} of its bound"


@pytest.mark.parametrize("reps", R.REPS)
@pytest.mark.parametrize("variant", ["gamma_plain", "abs_gamma_residual"])
def test_apply_stats_y_is_exact_from_the_constants_it_wrote(bf16_case, variant, reps):
    d, o, C = bf16_case, bf16_case.o, bf16_case.C
    abs_gamma = variant == "abs_gamma_residual"
    res, res64 = (d.res, o["res"]) if abs_gamma else (None, None)
    acc = vec(R.replica_split(o["fin_total"], reps))
    buf = torch.zeros(6 * C, device=DEV)
    rm0, rv0 = o["fin_kshift"] * 0.5, torch.ones(C, dtype=torch.float64)
    rm, rv = vec(rm0), vec(rv0)
    y = d.out(5)
    _apply_stats(d.x, y, res, d.M, C, acc, reps, vec(o["fin_kshift"]), R.FIN_COUNT, d.weight, d.shift, rm, rv, R.FIN_EPS, buf,
                 d.act | (R.ABS_GAMMA if abs_gamma else 0), d.slope)
    torch.cuda.synchronize()
    mean, scale = f64(buf[3 * C:4 * C]), f64(buf[5 * C:])
    y.assert_is(R.apply(o["x"], None, 0, mean, scale, o["shift"], res64, d.slope), "y")
    # the constants themselves: under the bounds of abn_exact_ref.finalize_bounds (exact operands leave them little to miss)
    _, c = R.apply_fin(o["x"], res64, o["fin_total"][None], o["fin_kshift"], R.FIN_COUNT, o["weight"], o["shift"], R.FIN_EPS, abs_gamma,
                       d.slope, rm0, rv0, MOMENTUM)
    b = R.finalize_bounds(o["fin_total"][:C], o["fin_total"][C:], o["fin_kshift"], R.FIN_COUNT, R.FIN_EPS, c, MOMENTUM, c.running_mean,
                          c.running_var)
    for what, got, ref in (("mean", buf[3 * C:4 * C], c.mean), ("invstd", buf[4 * C:5 * C], c.invstd), ("scale", buf[5 * C:], c.scale),
                           ("running_mean", rm, c.running_mean), ("running_var", rv, c.running_var)):
        _assert_within(got, ref, b[what], f"FIN {what}")


def _bwd_apply_raw(d, y, dx, dz, sums, grad_sums, reps, grad_out, act):
    M, C = d.M, d.C
    if d.x.ld == C:
        hip.abn_bwd_apply_raw(d.x.t, d.dy.t, y.t if y else None, dx.t, dz.t if dz else None, M, C, d.mean, d.invstd, d.scale, d.shift,
                              d.weight, sums, grad_sums, grad_out, R.COUNT, act, d.slope, reps)
        return
    p = hip.ptr
    hip._check(hip.load().ucd_abn_bwd_apply_raw(p(d.x.t), d.x.ld, p(d.dy.t), d.dy.ld, p(y.t) if y else None, y.ld if y else 0, p(dx.t), dx.ld,
                                                p(dz.t) if dz else None, dz.ld if dz else 0, M, C, p(d.mean), p(d.invstd), p(d.scale),
                                                p(d.shift), p(d.weight), p(sums), p(grad_sums), reps, p(grad_out), R.COUNT, act,
                                                float(d.slope), hip.stream()), "ucd_abn_bwd_apply_raw")


@pytest.mark.parametrize("reps", R.REPS)
@pytest.mark.parametrize("variant", ["x_same_sums", "y_dz_separate_sums_abs_gamma", "y_dz_same_sums"])
def test_bwd_apply_raw_is_exact(bf16_case, variant, reps):
    d, o = bf16_case, bf16_case.o
    from_y, abs_gamma, separate = variant != "x_same_sums", variant.endswith("abs_gamma"), "separate" in variant
    y, y64 = (d.y_res, d.y_res64) if from_y else (None, None)
    sums64 = R.replica_split(o["sums_in"], reps)
    grad64 = R.replica_split(o["sums_in"].roll(1), reps) if separate else None
    dx, dz = d.out(5), d.out(6) if from_y else None
    grad_out = torch.full((2 * d.C,), SENTINEL, device=DEV)
    _bwd_apply_raw(d, y, dx, dz, vec(sums64), vec(grad64), reps, grad_out, d.act | (R.ABS_GAMMA if abs_gamma else 0))
    rdx, rdz, rgrad = R.bwd_apply_raw(o["x"], o["dy"], y64, o["mean"], o["invstd"], o["scale"], o["shift"], d.slope, o["weight"], sums64,
                                      grad64, R.COUNT, abs_gamma)
    dx.assert_is(rdx, "dx")
    if dz:
        dz.assert_is(rdz, "dz")
    assert torch.equal(grad_out.cpu(), rgrad.to(torch.float32))


# ---------------------------------------------------------------------------------------------------------------------
# finalised constants: bounds from the formula (abn_exact_ref.finalize_bounds holds the derivation)
# ---------------------------------------------------------------------------------------------------------------------
FINALIZE_CASES = ["f32_six_groups_pb", "f32_80_groups", "bf16_9_bands", "bf16_60_bands", "f32_96_bands_ragged", "bf16_100_bands"]


@pytest.mark.parametrize("abs_gamma", [False, True], ids=["gamma", "abs_gamma"])
@pytest.mark.parametrize("name", FINALIZE_CASES)
def test_finalised_constants_meet_their_rounding_bounds(name, abs_gamma):
    """count = M here, so 1 / M and the rsqrt are rounded.  Row 0 (the shift k) is set to the channel's integer offset, which
    keeps |mean - k| below |k| and (mean - k)^2 below var / 2 - the two conditions under which the bounds of finalize_bounds cover every
    rounded operation - and are asserted first.  The sums themselves stay exact."""
    d = _case_data(name)
    o, M, C, HW = d.o, d.M, d.C, d.HW
    x64 = o["x"].clone()
    x64[0] = R.channel_offset(C)
    pb64 = None if o["pb"] is None else o["pb"].clone()
    if pb64 is not None:
        pb64[0] = 0
    x, pb = rows_in(x64, d.td, 1 if d.cs.pad else 0), vec(pb64)
    s, ss, k = R.stats(x64, pb64, HW)
    assert ((s / M).abs() <= k.abs()).all() and (2 * s * s / M <= ss).all()
    rm0, rv0 = R.channel_offset(C) * 0.5, torch.ones(C, dtype=torch.float64)
    c = R.finalize(s, ss, k, M, o["weight"], EPS32, abs_gamma, rm0, rv0, MOMENTUM)
    b = R.finalize_bounds(s, ss, k, M, EPS32, c, MOMENTUM, c.running_mean, c.running_var)
    flags = R.ABS_GAMMA if abs_gamma else 0

    buf, rm, rv = torch.zeros(6 * C, device=DEV), vec(rm0), vec(rv0)
    sums, ks, mean, invstd, scale = buf[:2 * C], buf[2 * C:3 * C], buf[3 * C:4 * C], buf[4 * C:5 * C], buf[5 * C:]
    hip.abn_stats_finalize(x.t, x.ld, M, C, pb, HW, sums, ks, d.weight, rm, rv, MOMENTUM, EPS32, mean, invstd, scale, flags)
    torch.cuda.synchronize()
    assert torch.equal(sums.cpu(), torch.cat([s, ss]).to(torch.float32)) and torch.equal(ks.cpu(), k.to(torch.float32))
    for what, got, ref in (("mean", mean, c.mean), ("invstd", invstd, c.invstd), ("scale", scale, c.scale), ("running_mean", rm, c.running_mean),
                           ("running_var", rv, c.running_var)):
        _assert_within(got, ref, b[what], f"stats_finalize {what}")
    # the kernel's variance, read back through invstd^-2 - eps, would carry the rsqrt's error: the biased variance is held to
    # its own bound through the running variance of a second call with momentum 1 (running_var = var * n / (n - 1), two more
    # rounded operations: 2u of the result)
    rv1 = torch.zeros(C, device=DEV)
    hip.abn_stats_finalize(x.t, x.ld, M, C, pb, HW, sums, ks, d.weight, torch.zeros(C, device=DEV), rv1, 1.0, EPS32, mean, invstd, scale, flags)
    corr = M / (M - 1)
    _assert_within(rv1, c.var * corr, b["var"] * corr + 2 * R.U * c.var * corr, "stats_finalize var")

    if d.cs.dtype == "bf16" and pb64 is None:
        # the FIN form on the same sums (one replica: M is no power of two, a split would not add back exactly)
        fbuf, frm, frv = torch.zeros(6 * C, device=DEV), vec(rm0), vec(rv0)
        y = Rows(M, C, d.td, 2 if d.cs.pad else 0, SENTINEL)
        _apply_stats(x, y, None, M, C, vec(torch.cat([s, ss]))[None], 1, vec(k), M, d.weight, d.shift, frm, frv, EPS32, fbuf, d.act | flags, d.slope)
        torch.cuda.synchronize()
        for what, got, ref in (("mean", fbuf[3 * C:4 * C], c.mean), ("invstd", fbuf[4 * C:5 * C], c.invstd), ("scale", fbuf[5 * C:], c.scale),
                               ("running_mean", frm, c.running_mean), ("running_var", frv, c.running_var)):
            _assert_within(got, ref, b[what], f"FIN {what}")


def test_shifted_sums_hold_the_variance_of_offset_channels():
    """The numerical regime the shifted sums exist for, on real values: bf16, 100 row bands (64 band-lanes), channels whose
    |mean| / std runs from 0 to 30.  The kernel's biased variance meets the finalize bound 4u (ss + |s d|) / n against float64
    (sums about k = row 0, as the kernel takes them); E[x^2] - E[x]^2 would miss it by about u mean^2 / var = 900 u."""
    B, H, W, C = 2, 100, 128, 64
    M = B * H * W
    g = R.reduce_geom(M, C, "bf16")
    assert g.gy >= R.WIDE_STAGE2_FROM
    ratio = torch.linspace(-30, 30, C, dtype=torch.float64)
    std = 2.0 ** (torch.arange(C) % 3 - 1).to(torch.float64)
    z = R.ihash(M * C, 77, -32768, 32767).view(M, C) / 8192 / 2.3094          # uniform in [-4, 4): unit variance
    x = (ratio * std + std * z).to(torch.bfloat16)
    x64 = x.to(torch.float64)
    s, ss, k = R.stats(x64, None, H * W)
    c = R.finalize(s, ss, k, M, None, EPS32, False)
    b = R.finalize_bounds(s, ss, k, M, EPS32, c, 1.0)
    assert ((c.mean.abs() / c.var.sqrt()).max() > 25)
    xd = x.to(DEV)
    buf, rm, rv = torch.zeros(6 * C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    hip.abn_stats_finalize(xd, C, M, C, None, H * W, buf[:2 * C], buf[2 * C:3 * C], None, rm, rv, 1.0, EPS32, buf[3 * C:4 * C], buf[4 * C:5 * C],
                           buf[5 * C:], 0)
    torch.cuda.synchronize()
    # the kernel's variance two ways: its fp32 sums finalised here in float64, and its own finalize through running_var at
    # momentum 1 (= var n / (n - 1): 2u of the result more)
    ks, kss = f64(buf[:C]), f64(buf[C:2 * C])
    var_of_sums = (kss - ks * ks / M) / M
    corr = M / (M - 1)
    naive = (x64 * x64).sum(0) / M - (x64.sum(0) / M) ** 2
    print(f"|mean|/std up to {(c.mean.abs() / c.var.sqrt()).max():.1f}; u mean^2 / var up to {(R.U * c.mean ** 2 / c.var).max() / R.U:.0f} u; "
          f"bound / var between {(b['var'] / c.var).min() / R.U:.1f} u and {(b['var'] / c.var).max() / R.U:.1f} u; float64 E[x^2]-E[x]^2 sanity {((naive - c.var).abs() / c.var).max():.1e}")
    _assert_within(var_of_sums, c.var, b["var"], "variance from the kernel's sums")
    _assert_within(rv, c.var * corr, b["var"] * corr + 2 * R.U * c.var * corr, "variance from the kernel's finalize")
    _assert_within(buf[4 * C:5 * C], c.invstd, b["invstd"], "invstd")


# ---------------------------------------------------------------------------------------------------------------------
# plane sums and window means
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.PLANE_CASES))
def test_plane_sum_is_exact(name):
    dtype, B, HW, C, alpha, pad = R.PLANE_CASES[name]
    x64 = R.small_rows(B * HW, C, sum(name.encode()))
    x = rows_in(x64, R.torch_dtype(dtype), 2 if pad else 0)
    out = torch.full((B + 1, C), SENTINEL, device=DEV)
    hip.plane_sum(x.t, x.ld, B, HW, C, alpha, out)
    torch.cuda.synchronize()
    assert torch.equal(out[:B].cpu(), R.plane_sum(x64, B, HW, alpha).to(torch.float32))
    assert (out[B] == SENTINEL).all()


@pytest.mark.parametrize("name", list(R.WINDOW_CASES))
def test_window_mean_against_avg_pool2d(name):
    dtype, B, H, W, C, ph, pw, pad = R.WINDOW_CASES[name]
    td = R.torch_dtype(dtype)
    x64 = R.small_rows(B * H * W, C, sum(name.encode()))
    ref = R.window_mean(x64, B, H, W, ph, pw)
    OH, OW = H - ph + 1, W - pw + 1
    if pad:
        lib = hip.load()
        x, out = rows_in(x64, td, 1), Rows(B * OH * OW, C, td, 2, SENTINEL)
        nbytes = lib.ucd_window_mean_workspace_bytes(B, H, W, C, ph)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        hip._check(lib.ucd_window_mean(hip.ptr(x.t), x.ld, hip.dtype_code(x.t), B, H, W, C, ph, pw, hip.ptr(out.t), out.ld, hip.ptr(ws), nbytes,
                                       hip.stream()), "ucd_window_mean")
        torch.cuda.synchronize()
        got = out.t.cpu()
        assert (out.buf[:, :8] == SENTINEL).all() and (out.buf[:, 8 + C:] == SENTINEL).all()
    else:
        x4 = x64.to(td).to(DEV).view(B, H, W, C).permute(0, 3, 1, 2)
        got = hip.window_mean(x4, ph, pw).permute(0, 2, 3, 1).reshape(-1, C).cpu()
    if R.window_area_exact(ph, pw):
        assert torch.equal(got, ref.to(td))
        return
    # exact integer sums, then ONE rounded multiply by the rounded 1 / area: fl(1 / area) is off by a relative e1, the product
    # by half an ulp more.  While |e1| <= u / 2 (plain arithmetic on the area, checked here) that is within one fp32 ulp of the
    # float64 value v - |e1| |v| < 2^-25 2^(e+1) = ulp(v) / 2 for v in [2^e, 2^(e+1)) - before the store rounds to the output
    # type, which keeps the order of the two ends of that interval
    inv32 = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(ph * pw), dtype=torch.float32))
    assert abs(inv32 * ph * pw - 1.0) <= R.U / 2
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -100))) - 23)
    lo, hi = (ref - ulp).to(td), (ref + ulp).to(td)
    assert ((got >= lo) & (got <= hi)).all(), f"{((got < lo) | (got > hi)).sum().item()} window means more than one fp32 ulp off"
