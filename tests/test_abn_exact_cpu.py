"""CPU: the float64 reference of the ABN passes (abn_exact_ref.py) against autograd, the exactness of the operands that
tests/test_abn_exact_gpu.py compares with torch.equal, and the geometry class every case of its table is there for."""
import pytest
import torch
import torch.nn.functional as F

import abn_exact_ref as R

EXACT = 2.0 ** 24


def _is_fp32(t):
    return torch.equal(t.to(torch.float32).to(torch.float64), t)


def _stored(t, dtype):
    """t survives the case's storage type unchanged"""
    return torch.equal(t.to(R.torch_dtype(dtype)).to(torch.float64), t)


def _sum_is_exact(terms, gran):
    """Every term is an integer multiple of `gran` and the absolute terms of a column add to less than 2^24 of them: any partial
    sum, in any order and over any subset of the rows (a band, a lane, a replica), is exact in fp32."""
    units = terms / gran
    return bool(torch.equal(units, units.round()) and units.abs().sum(0).max() < EXACT)


# ---------------------------------------------------------------------------------------------------------------------
# the reference against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abs_gamma", [False, True])
@pytest.mark.parametrize("with_pb,with_res", [(False, False), (True, True), (False, True)])
def test_reference_matches_autograd_through_batch_norm(with_pb, with_res, abs_gamma):
    g = torch.Generator().manual_seed(3)
    B, HW, C, eps, slope = 3, 14, 8, 1e-5, 0.01
    M = B * HW
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.5 + torch.arange(C) - 3.0
    dy = torch.randn(M, C, generator=g, dtype=torch.float64)
    pb = torch.randn(B, C, generator=g, dtype=torch.float64) if with_pb else None
    res = torch.randn(M, C, generator=g, dtype=torch.float64) if with_res else None
    w = torch.randn(C, generator=g, dtype=torch.float64)
    w[1] = -0.7
    b = torch.randn(C, generator=g, dtype=torch.float64) * 0.3

    xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = xa if pb is None else xa + pb.repeat_interleave(HW, 0)
    z = F.batch_norm(xin, None, None, wa.abs() + eps if abs_gamma else wa, ba, True, 0.0, eps)
    out = F.leaky_relu(z if res is None else z + res, slope)
    (out * dy).sum().backward()

    s, ss, k = R.stats(x, pb, HW)
    c = R.finalize(s, ss, k, M, w, eps, abs_gamma)
    y = R.apply(x, pb, HW, c.mean, c.scale, b, res, slope)
    assert (y - out.detach()).abs().max() < 1e-12
    for from_y in ([True] if with_res else [True, False]):          # the sign of z + res is not that of z
        yy = y if from_y else None
        sums = R.bwd_reduce(x, pb, HW, dy, yy, c.mean, c.invstd, c.scale, b, slope, w, abs_gamma)
        dx, _ = R.bwd_apply(x, pb, HW, dy, yy, c.mean, c.invstd, c.scale, b, slope, w, sums, M, abs_gamma)
        assert (dx - xa.grad).abs().max() < 1e-12
        assert (sums[:C] - ba.grad).abs().max() < 1e-12
        assert (sums[C:] - wa.grad).abs().max() < 1e-12
    if pb is None:
        # the FIN / RAW forms: the same layer from replicas of the raw (unsigned) sums
        raw = R.bwd_reduce(x, None, HW, dy, y, c.mean, c.invstd, c.scale, b, slope)
        for reps in R.REPS:
            y2, c2 = R.apply_fin(x, res, R.replica_split(torch.cat([s, ss]), reps), k, M, w, b, eps, abs_gamma, slope)
            assert (y2 - out.detach()).abs().max() < 1e-12 and (c2.invstd - c.invstd).abs().max() < 1e-12
            dx, _, grad = R.bwd_apply_raw(x, dy, y, c.mean, c.invstd, c.scale, b, slope, w, R.replica_split(raw, reps), None, M,
                                          abs_gamma)
            assert (dx - xa.grad).abs().max() < 1e-12
            assert (grad - torch.cat([ba.grad, wa.grad])).abs().max() < 1e-12


def test_window_mean_and_plane_sum_references():
    x = R.small_rows(2 * 5 * 6, 8, 1)
    out = R.window_mean(x, 2, 5, 6, 2, 3).view(2, 4, 4, 8)
    xi = x.view(2, 5, 6, 8)
    assert torch.equal(out[1, 2, 1], xi[1, 2:4, 1:4].sum((0, 1)) / 6)
    assert torch.equal(R.plane_sum(x, 2, 30, 0.5)[1], xi[1].sum((0, 1)) * 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# the operands make every pass exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_operands_are_exact_in_fp32_and_in_storage(name):
    cs, o = R.CASES[name], R.operands(name)
    x, pb, HW, dy, res, slope, C = o["x"], o["pb"], o["HW"], o["dy"], o["res"], o["slope"], o["C"]
    for t in (x, dy, res):
        assert _stored(t, cs.dtype)
    # forward statistics: integers, |x' - k| <= 4
    f = R.biased(x, pb, HW) - R.biased(x, pb, HW)[0]
    assert f.abs().max() <= 4 and _sum_is_exact(f, 1.0) and _sum_is_exact(f * f, 1.0)
    s, ss, k = R.stats(x, pb, HW)
    mean = k + s / o["M"]
    assert (mean != 0).all() and (mean[1:] != mean[:-1]).all()          # channel means non-zero and different between channels
    # the constants handed to the other passes
    for t in (o["mean"], o["shift"], o["sums_in"] / R.COUNT):
        assert torch.equal(t, t.round())
    for t in (o["invstd"], o["scale"], o["weight"].abs()):
        assert torch.equal(torch.log2(t), torch.log2(t).round()) and (t[1:] != t[:-1]).all()
    assert (o["weight"] < 0).any() and (o["weight"] > 0).any()
    # backward reductions: dz in quarters, dz * xhat in sixteenths, for either source of the sign
    y_res = R.apply(x, pb, HW, o["mean"], o["scale"], o["shift"], res, slope)
    for y in (None, y_res):
        dz, xh = R.dz_xhat(x, pb, HW, dy, y, o["mean"], o["invstd"], o["scale"], o["shift"], slope)
        assert _sum_is_exact(dz, 0.25) and _sum_is_exact(dz * xh, 1.0 / 16)
    if cs.passes != "all":
        return
    # element-wise outputs: exact in fp32 and unchanged by the storage type
    outs = [y_res, R.apply(x, pb, HW, o["mean"], o["scale"], None, None, slope), R.apply(x, pb, HW, o["mean"], o["scale"], o["shift"], None, slope)]
    for y, abs_gamma, frozen in ((None, False, False), (y_res, True, False), (y_res, False, False), (y_res, False, True)):
        outs += R.bwd_apply(x, pb, HW, dy, y, o["mean"], o["invstd"], o["scale"], o["shift"], slope, o["weight"], o["sums_in"], R.COUNT,
                            abs_gamma, frozen)
    if cs.dtype == "bf16":
        for reps in R.REPS:
            raw = R.replica_split(o["sums_in"], reps)
            assert _sum_is_exact(raw, 1.0) and torch.equal(raw.sum(0), o["sums_in"])
            for abs_gamma in (False, True):
                outs += R.bwd_apply_raw(x, dy, y_res, o["mean"], o["invstd"], o["scale"], o["shift"], slope, o["weight"], raw, None, R.COUNT,
                                        abs_gamma)[:2]
    for t in outs:
        assert _is_fp32(t) and _stored(t, cs.dtype)
    if cs.dtype == "bf16":
        # FIN: the replicas add back exactly (in 64ths), the constants they give are an integer mean and a power-of-two invstd,
        # and z is exact in fp32 before the one rounding of the store
        for reps in R.REPS:
            acc = R.replica_split(o["fin_total"], reps)
            assert _sum_is_exact(acc, 1.0 / 64) and torch.equal(acc.sum(0), o["fin_total"])
        for abs_gamma in (False, True):
            yf, c = R.apply_fin(x, res, o["fin_total"][None], o["fin_kshift"], R.FIN_COUNT, o["weight"], o["shift"], R.FIN_EPS, abs_gamma, slope)
            assert torch.equal(c.mean, c.mean.round()) and torch.equal(torch.log2(c.invstd), torch.log2(c.invstd).round())
            assert _is_fp32(c.scale) and _is_fp32(o["fin_total"][:C] / R.FIN_COUNT * o["fin_total"][:C])
            z = (x - c.mean) * c.scale
            assert _is_fp32(z) and _is_fp32(z + o["shift"]) and _is_fp32(z + o["shift"] + res) and _is_fp32(yf)
            if not abs_gamma:
                assert _stored(yf, cs.dtype)


@pytest.mark.parametrize("name", list(R.PLANE_CASES))
def test_plane_sum_cases_are_exact(name):
    dtype, B, HW, C, alpha, _ = R.PLANE_CASES[name]
    x = R.small_rows(B * HW, C, sum(name.encode()))
    assert _stored(x, dtype) and _sum_is_exact(x.view(B, HW, C).permute(1, 0, 2).reshape(HW, -1), 1.0)
    assert _is_fp32(R.plane_sum(x, B, HW, alpha)) and alpha == 2.0 ** round(torch.log2(torch.tensor(alpha)).item())


@pytest.mark.parametrize("name", list(R.WINDOW_CASES))
def test_window_mean_cases_are_exact(name):
    dtype, B, H, W, C, ph, pw, _ = R.WINDOW_CASES[name]
    x = R.small_rows(B * H * W, C, sum(name.encode()))
    # the running sums hold sums of at most H x W integers of one image
    assert _stored(x, dtype) and _sum_is_exact(x.view(B, H * W, C).permute(1, 0, 2).reshape(H * W, -1), 1.0)
    if R.window_area_exact(ph, pw):
        assert _stored(R.window_mean(x, B, H, W, ph, pw), dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the geometry
# ---------------------------------------------------------------------------------------------------------------------
def _geoms(cs):
    M = cs.B * cs.H * cs.W
    return M, R.reduce_geom(M, cs.C, cs.dtype), R.apply_geom(M, cs.C, cs.dtype)


def test_every_case_reaches_the_classes_it_is_there_for():
    """When the geometry changes, this says which rows of the table need new shapes."""
    reached = set()
    for name, cs in R.CASES.items():
        M, r, a = _geoms(cs)
        for cls in cs.classes:
            assert R.CLASSES[cls](cs, M, r, a), f"{name} no longer reaches '{cls}': reduce {r}, apply {a}"
        reached.update(cs.classes)
    assert reached == set(R.CLASSES), set(R.CLASSES) - reached
    # both types, where both have the class: the replica forms are bf16 only, and at the band cap (25 MB at the least) the two
    # types differ in nothing the 60- to 200-band cases of both do not show - the second stage reads fp32 partial rows either way
    for cls in R.CLASSES:
        types = {cs.dtype for cs in R.CASES.values() if cls in cs.classes}
        assert types == {"bf16", "f32"} or cls in ("replicas_ty4", "band_cap"), (cls, types)


def test_restated_geometry_on_known_launches():
    """make_geom on shapes whose launch the kernel comments and the recorded-bits cases spell out"""
    assert R.reduce_geom(3 * 33 * 32, 64, "bf16") == R.Geom(8, 32, 1, 9, 384)
    assert R.apply_geom(3 * 33 * 32, 64, "bf16") == R.Geom(8, 32, 1, 13, 256)       # "13 row bands of 256 rows, the last one 96"
    assert R.apply_geom(3 * 33 * 32, 64, "f32")[:2] + R.apply_geom(3 * 33 * 32, 64, "f32")[3:] == (16, 16, 25, 128)   # "25 bands"
    assert R.apply_geom(2 * 9 * 11, 24, "f32")[:2] == (6, 42)
    assert R.apply_geom(3 * 17 * 19, 1024, "bf16")[:3] == (64, 4, 2)
    assert R.stage2_lanes(95) == 16 and R.stage2_lanes(96) == 64


def test_plane_and_window_cases_cover_their_classes():
    seen = set()
    for dtype, B, HW, C, alpha, pad in R.PLANE_CASES.values():
        g = R.plane_geom(HW, C, dtype)
        four, tail = R.lane_walk(0, HW, g.TY)
        seen.add((dtype, "hw_below_ty" if HW < g.TY else "four_and_tail" if four and tail else "other"))
        assert B > 1
        if pad:
            seen.add((dtype, "ld"))
    assert seen >= {(d, k) for d in ("bf16", "f32") for k in ("hw_below_ty", "four_and_tail", "ld")}, seen
    assert {a for _, _, _, _, a, _ in R.PLANE_CASES.values()} >= {1.0, 0.125}
    seen = set()
    for dtype, B, H, W, C, ph, pw, pad in R.WINDOW_CASES.values():
        for k, hit in (("ph_ne_pw", ph != pw and ph > 1 and pw > 1), ("full_height", ph == H), ("pw_1", pw == 1 and ph > 1),
                       ("identity", ph == pw == 1), ("exact_area", R.window_area_exact(ph, pw) and ph * pw > 1),
                       ("rounded_area", not R.window_area_exact(ph, pw)), ("ld", pad)):
            if hit:
                seen.add((dtype, k))
    need = {(d, k) for d in ("bf16", "f32") for k in ("ph_ne_pw", "full_height", "identity", "exact_area", "rounded_area", "ld")}
    assert seen >= need | {("bf16", "pw_1")}, need - seen


@pytest.mark.parametrize("name", list(R.CASES))
def test_restated_walk_reads_every_row_once_and_adds_to_the_plain_sums(name):
    """The restatement of the band walk, the second stage and the plane-bias index against the plain float64 reference: a slip in
    either (a band that starts a row late, a dropped tail loop, 16 of 64 band-lanes, r / (HW + 1)) breaks the equality."""
    cs, o = R.CASES[name], R.operands(name)
    M, r, a = _geoms(cs)
    for g in (r, a):
        rows = [i for four, tail in R.band_rows(M, g) for i in four + tail]
        assert sorted(rows) == list(range(M))
    x, pb, HW = o["x"], o["pb"], o["HW"]
    if pb is not None:
        assert torch.equal(R.biased(x, pb, HW), x + pb.repeat_interleave(HW, 0))
    s, ss, k = R.stats(x, pb, HW)
    f = R.biased(x, pb, HW) - k
    total, partial = R.two_stage_sum(torch.cat([f, f * f], 1), r)
    assert partial.shape[0] == r.gy and torch.equal(total, torch.cat([s, ss]))


@pytest.mark.parametrize("TY", [4, 8, 32])
def test_restated_replica_walk_reads_every_replica_once(TY):
    for reps in R.REPS + (16,):
        assert sorted(R.replica_walk(reps, TY)) == list(range(max(reps, 1)))
        total = (R.ihash(16, reps, -4, 4) + 5) * 256
        split = R.replica_split(total, reps)
        assert torch.equal(split[torch.tensor(R.replica_walk(reps, TY))].sum(0), total)
        assert len({float(v) for v in split[:, 0]}) == reps          # all different: no replica can stand in for another
