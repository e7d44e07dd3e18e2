"""Float64 reference of the ABN passes (ucd_amd/csrc/abn.hip), operands on which those passes are exact in fp32, a restatement
of the launch geometry, and the case table of tests/test_abn_exact_cpu.py and tests/test_abn_exact_gpu.py.

Why exact operands: on small integers every fp32 partial sum of a reduction is an integer below 2^24, so the result does not
depend on the order of summation and a kernel can be compared with ``torch.equal`` - one dropped, repeated or misplaced row
fails at any size, which no tolerance that admits a reordering can promise.  Everything that would make a pass inexact (mean,
invstd, scale, the sums, 1 / count) is an argument of the C ABI, so the operands below choose integers and powers of two for
them.  Only the finalised constants (1 / M and an rsqrt are rounded) are compared under a bound, derived in ``finalize_bounds``.

The reference is plain torch in float64 on the CPU, one function per pass, written from the definitions in include/ucd_hip.h
and the kernel comments - it never walks bands.  The band walk is restated separately (``make_geom``, ``lane_walk``,
``two_stage_sum``, ``replica_walk``); the CPU test checks the restated walk against the plain sums, the GPU test checks the
restated band count against the library.
"""
import collections
import functools

import torch
import torch.nn.functional as F

IDENTITY, LEAKY, ABS_GAMMA = 0, 1, 0x100          # include/ucd_hip.h: UCD_ACT_*, UCD_NORM_ABS_GAMMA
SLOPE = 0.25                                      # leaky_relu slope of every exact case (identity: 1)
U = 2.0 ** -24                                    # unit roundoff of fp32

K_BLOCK = 256                                     # abn.hip: kBlock
K_MAX_BANDS = 512                                 # abn.hip: kMaxBands
WIDE_STAGE2_FROM = 96                             # abn.hip: UCD_REDUCE_BANDS takes 64 band-lanes from 96 bands up

Geom = collections.namedtuple("Geom", "TX TY gx gy rows_per_band")


def ceil_div(a, b):
    return -(-a // b)


def vec_of(dtype):
    """Channels per thread: a lane moves 16 bytes."""
    return 8 if dtype == "bf16" else 4


def torch_dtype(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry, restated from abn.hip (make_geom, geom_for, UCD_REDUCE_BANDS, replica_sum)
# ---------------------------------------------------------------------------------------------------------------------
def make_geom(M, C, vec, target_blocks, min_iters, max_bands=4096):
    CG = C // vec
    TX = min(CG, 64)
    TY = K_BLOCK // TX
    gx = ceil_div(CG, TX)
    by_rows = M // (TY * min_iters)
    gy = max(1, min(target_blocks // gx, by_rows, max_bands))
    rows_per_band = ceil_div(ceil_div(M, gy), 4 * TY) * 4 * TY
    return Geom(TX, TY, gx, ceil_div(M, rows_per_band), rows_per_band)


def reduce_geom(M, C, dtype):
    """ucd_abn_stats, ucd_abn_bwd_reduce"""
    return make_geom(M, C, vec_of(dtype), 512, 8, K_MAX_BANDS)


def apply_geom(M, C, dtype):
    """ucd_abn_apply, ucd_abn_bwd_apply and their FIN / RAW forms"""
    return make_geom(M, C, vec_of(dtype), 512, 4)


def plane_geom(HW, C, dtype):
    """ucd_plane_sum: TX and TY only, one block column per image"""
    return make_geom(HW, C, vec_of(dtype), 1, 1)


def stage2_lanes(bands):
    return 64 if bands >= WIDE_STAGE2_FROM else 16


def lane_walk(r, r_end, step):
    """The indices r, r + step, ... below r_end as walk_band (and the second stage, and plane_sum) visits them:
    (those of the four-in-flight loop, those of the one-at-a-time tail)."""
    four, tail = [], []
    while r + 3 * step < r_end:
        four += [r, r + step, r + 2 * step, r + 3 * step]
        r += 4 * step
    while r < r_end:
        tail.append(r)
        r += step
    return four, tail


def band_rows(M, g):
    """Per row band: (rows read by the four-in-flight loop, rows read by the tail loop), over the band's TY lanes."""
    out = []
    for b in range(g.gy):
        r_begin = b * g.rows_per_band
        r_end = min(M, r_begin + g.rows_per_band)
        four, tail = [], []
        for ty in range(g.TY):
            f, t = lane_walk(r_begin + ty, r_end, g.TY)
            four += f
            tail += t
        out.append((four, tail))
    return out


def two_stage_sum(v, g):
    """Column sums of v [M, K] the way the two-stage reductions take them: per-band partial rows, then `stage2_lanes` band-lanes.
    Returns (sums [K], partial [gy, K])."""
    partial = torch.stack([v[torch.tensor(four + tail, dtype=torch.long)].sum(0) for four, tail in band_rows(v.shape[0], g)])
    lanes = stage2_lanes(g.gy)
    total = torch.zeros_like(partial[0])
    for lane in range(lanes):
        four, tail = lane_walk(lane, g.gy, lanes)
        if four or tail:
            total = total + partial[torch.tensor(four + tail, dtype=torch.long)].sum(0)
    return total, partial


def replica_walk(reps, TY):
    """The replicas replica_sum adds, over its TY row threads (reps <= 1: one plain load)."""
    if reps <= 1:
        return [0]
    seen = []
    for ty in range(TY):
        r = ty
        while r < reps:
            seen += [r + u * TY for u in range(4) if r + u * TY < reps]
            r += 4 * TY
    return seen


def plane_bias_image(r, HW):
    """Row r of an activation belongs to image r / HW (the plane bias is one row per image)."""
    return r // HW


# ---------------------------------------------------------------------------------------------------------------------
# the passes in float64
# ---------------------------------------------------------------------------------------------------------------------
def biased(x, pb, HW):
    """x' = x + plane_bias[row / HW]"""
    if pb is None:
        return x
    return x + pb[plane_bias_image(torch.arange(x.shape[0]), HW)]


def act(z, slope):
    return torch.where(z > 0, z, z * slope)


def stats(x, pb, HW):
    """(sum (x' - k), sum (x' - k)^2, k) with k = row 0 of x'"""
    xp = biased(x, pb, HW)
    k = xp[0].clone()
    f = xp - k
    return f.sum(0), (f * f).sum(0), k


def gamma_eff(weight, eps, abs_gamma, like):
    if weight is None:
        return torch.ones_like(like)
    return weight.abs() + eps if abs_gamma else weight


Consts = collections.namedtuple("Consts", "mean var invstd scale running_mean running_var")


def finalize(s, ss, k, n, weight, eps, abs_gamma, running_mean=None, running_var=None, momentum=0.0):
    d = s / n
    mean = k + d
    var = ((ss - s * d) / n).clamp_min(0)
    invstd = (var + eps) ** -0.5
    scale = gamma_eff(weight, eps, abs_gamma, invstd) * invstd
    unbiased = var * (n / (n - 1)) if n > 1 else var
    rm = None if running_mean is None else (1 - momentum) * running_mean + momentum * mean
    rv = None if running_var is None else (1 - momentum) * running_var + momentum * unbiased
    return Consts(mean, var, invstd, scale, rm, rv)


def apply(x, pb, HW, mean, scale, shift, res, slope):
    z = (biased(x, pb, HW) - mean) * scale
    if shift is not None:
        z = z + shift
    if res is not None:
        z = z + res
    return act(z, slope)


def dz_xhat(x, pb, HW, dy, y, mean, invstd, scale, shift, slope):
    """dz = dy * act'(z), the sign of z from the stored output y or recomputed from x; xhat = (x' - mean) * invstd"""
    d = biased(x, pb, HW) - mean
    sgn = y if y is not None else d * scale + (0 if shift is None else shift)
    return torch.where(sgn > 0, dy, dy * slope), d * invstd


def weight_sign(weight):
    """sign(weight) with sign(0) = +1"""
    return torch.where(weight < 0, -torch.ones_like(weight), torch.ones_like(weight))


def bwd_reduce(x, pb, HW, dy, y, mean, invstd, scale, shift, slope, weight=None, abs_gamma=False):
    """[sum dz | sum dz * xhat]; abs-gamma: the second row is d weight = sign(weight) * sum dz * xhat"""
    dz, xh = dz_xhat(x, pb, HW, dy, y, mean, invstd, scale, shift, slope)
    s0, s1 = dz.sum(0), (dz * xh).sum(0)
    if abs_gamma and weight is not None:
        s1 = s1 * weight_sign(weight)
    return torch.cat([s0, s1])


def bwd_apply(x, pb, HW, dy, y, mean, invstd, scale, shift, slope, weight, sums, count, abs_gamma=False, frozen=False,
              raw=False):
    """(dx, dz).  Training: dx = ((dz - s0 / count) - xhat * s1 / count) * gw with gw = weight * invstd, or scale under
    abs-gamma, where s1 = sums[C:] carries sign(weight) (undone here) unless the sums are RAW.  Frozen: dx = dz * scale."""
    dz, xh = dz_xhat(x, pb, HW, dy, y, mean, invstd, scale, shift, slope)
    if frozen:
        return dz * scale, dz
    C = x.shape[1]
    k0, k1 = sums[:C] / count, sums[C:] / count
    if abs_gamma:
        if weight is not None and not raw:
            k1 = k1 * weight_sign(weight)
        gw = scale
    else:
        gw = invstd if weight is None else weight * invstd
    return ((dz - k0) - xh * k1) * gw, dz


def apply_fin(x, res, acc, kshift, count, weight, bias, eps, abs_gamma, slope, running_mean=None, running_var=None,
              momentum=0.0):
    """FIN: statistics arrive as `reps` replicas of raw sums [reps][2 C] about kshift.  Returns (y, Consts)."""
    C = x.shape[1]
    tot = acc.sum(0)
    c = finalize(tot[:C], tot[C:], kshift, count, weight, eps, abs_gamma, running_mean, running_var, momentum)
    return apply(x, None, 0, c.mean, c.scale, bias, res, slope), c


def bwd_apply_raw(x, dy, y, mean, invstd, scale, shift, slope, weight, sums, grad_sums, count, abs_gamma):
    """RAW: sums / grad_sums are `reps` replicas [reps][2 C] with no sign applied.  Returns (dx, dz, grad_out = [d bias | d weight])."""
    C = x.shape[1]
    dx, dz = bwd_apply(x, None, 0, dy, y, mean, invstd, scale, shift, slope, weight, sums.sum(0), count, abs_gamma, raw=True)
    grad = (sums if grad_sums is None else grad_sums).sum(0).clone()
    if abs_gamma and weight is not None:
        grad[C:] = grad[C:] * weight_sign(weight)
    return dx, dz, grad


def plane_sum(x, B, HW, alpha):
    """x [B * HW, C] -> alpha * sum over each image's pixels, [B, C]"""
    return x.view(B, HW, -1).sum(1) * alpha


def window_mean(x, B, H, W, ph, pw):
    """x [B * H * W, C] -> the stride-1, unpadded ph x pw window means as rows [B * OH * OW, C]"""
    C = x.shape[1]
    out = F.avg_pool2d(x.view(B, H, W, C).permute(0, 3, 1, 2), (ph, pw), stride=1)
    return out.permute(0, 2, 3, 1).reshape(-1, C)


def finalize_bounds(s, ss, k, n, eps, c, momentum, running_mean_out=None, running_var_out=None):
    """Bounds on |kernel - float64| for the finalised constants, from the formula (all arguments float64; s, ss exact in the
    kernel because the operands are).  With u = 2^-24 and d = s * (1 / n):

      mean = k + d             1 / n and the product are rounded, then the sum: 2u |d| + u |k + d| <= 2u (|k| + |s / n|)
                               (the cases keep |d| <= |k|: k is a row of the channel and the channel mean is far from 0)
      var = (ss - s d) / n     the product, the difference, 1 / n and the last product: 4u (ss + |s d|) / n
                               (d carries 2u of its own into s d; the cases keep s d <= ss / 2, which pays for it)
      invstd = rsqrt(var+eps)  a relative 8u for the sum, the 1-ulp seed and the Newton step of the FIN form (five rounded
                               operations; its quadratic term is below u) or the IEEE sqrt and division, and the product with
                               gamma for `scale` - plus the variance's error through -1/2 dvar / (var + eps)
      running statistics       the same bounds scaled by the momentum, plus 2u of the result (the two products, one of them by
                               a power of two in the cases, and the sum; the operands of the sum have one sign); the unbiased
                               correction n / (n - 1) is a rounded quotient and a rounded product, 2u of the unbiased variance more
    Returns a dict of tensors."""
    d = s / n
    b_mean = 2 * U * (k.abs() + d.abs())
    b_var = 4 * U * (ss + (s * d).abs()) / n
    rel = 8 * U + 0.5 * b_var / (c.var + eps)
    out = {"mean": b_mean, "var": b_var, "invstd": rel * c.invstd, "scale": rel * c.scale.abs()}
    if running_mean_out is not None:
        out["running_mean"] = momentum * b_mean + 2 * U * running_mean_out.abs()
    if running_var_out is not None:
        corr = n / (n - 1) if n > 1 else 1.0
        out["running_var"] = momentum * (b_var * corr + 2 * U * c.var * corr) + 2 * U * running_var_out.abs()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# exact operands
# ---------------------------------------------------------------------------------------------------------------------
def ihash(n, seed, lo, hi):
    """n integers in [lo, hi] from an integer hash of the index (int64 arithmetic below 2^63, no random generator): the same
    bytes everywhere.  The mixing steps are those of tests/golden/make_abn_bits_golden._hash."""
    h = (torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 40503 + 12345) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return (lo + (h >> 4) % (hi - lo + 1)).to(torch.float64)


def channel_offset(C):
    """Integer channel means: 5 .. 11 in magnitude, alternating sign - non-zero, and no two neighbours alike."""
    c = torch.arange(C)
    return ((5 + c % 7) * (1 - 2 * (c % 2))).to(torch.float64)


def replica_split(total, reps):
    """`reps` replicas [reps][2 C] that add back to `total` exactly: replica r holds total * n_r / 256 with n_r = r + 1 and the
    last one the rest (all different, so a dropped or repeated replica changes the sum)."""
    if reps == 1:
        return total[None].clone()
    n = list(range(1, reps))
    n.append(256 - sum(n))
    assert n[-1] > 0
    return total[None] * (torch.tensor(n, dtype=torch.float64) / 256)[:, None]


COUNT = 1024.0           # `count` of the passes that take their sums as arguments: a power of two, not M
FIN_COUNT = 4096.0
FIN_EPS = 2.0 ** -10


@functools.lru_cache(maxsize=2)
def operands(name):
    """Float64 operands of one case (a dict of CPU tensors; activations are [M, C] rows).  Read-only: shared between tests.

    x' = x + pb stays within 2 of the channel's integer offset, so |x' - k| <= 4 and |x' - mean| <= 3; dy and the residual are
    integers within 4.  mean / shift are integers, invstd / scale / weight powers of two (weight of both signs), all different
    between neighbouring channels, and the sums handed to bwd_apply are integer multiples of COUNT."""
    cs = CASES[name]
    B, H, W, C = cs.B, cs.H, cs.W, cs.C
    M, HW = B * H * W, H * W
    seed = sum(name.encode())
    c = torch.arange(C)
    cm = channel_offset(C)
    o = {"M": M, "HW": HW, "C": C, "slope": 1.0 if cs.act == IDENTITY else SLOPE}
    spread = 1 if cs.pb else 2
    o["x"] = cm + ihash(M * C, seed, -spread, spread).view(M, C)
    o["pb"] = ihash(B * C, seed + 5, -1, 1).view(B, C) if cs.pb else None
    o["dy"] = ihash(M * C, seed + 1, -4, 4).view(M, C)
    o["res"] = ihash(M * C, seed + 2, -4, 4).view(M, C)
    o["mean"] = cm + (c % 3 - 1).to(torch.float64)
    o["invstd"] = 2.0 ** -(c % 3).to(torch.float64)
    o["scale"] = 2.0 ** (1 - c % 4).to(torch.float64)
    o["shift"] = (c % 5 - 2).to(torch.float64)
    o["weight"] = 2.0 ** (c % 3 - 1).to(torch.float64) * (1 - 2 * (c % 4 == 1).to(torch.float64))
    o["sums_in"] = COUNT * torch.cat([(c % 5 - 2), ((c + 1) % 3 - 1)]).to(torch.float64)
    # FIN: raw sums about kshift = the channel offset whose mean is an integer and whose var + eps is a power of four
    a, e = (c % 5 - 2).to(torch.float64), (c % 3 - 1).to(torch.float64)
    o["fin_kshift"] = cm
    o["fin_total"] = torch.cat([FIN_COUNT * a, FIN_COUNT * (4.0 ** e - FIN_EPS + a * a)])
    return o


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# classes: the geometry classes a row is in the table FOR (tests/test_abn_exact_cpu.py proves that it reaches each of them);
# passes: "all", or the reductions only for the maps that are there for the band count alone; pad: every operand is a channel
# slice of a wider buffer (ld > C)
Case = collections.namedtuple("Case", "dtype B H W C pb act pad passes classes")


def _case(dtype, B, H, W, C, classes, pb=False, act=LEAKY, pad=False, passes="all"):
    return Case(dtype, B, H, W, C, pb, act, pad, passes, tuple(classes.split()))


CASES = {
    # one channel group: TX = 1, TY = 256 - rows only.  35 rows: fewer than TY, every lane at most one tail row
    "bf16_tx1_35": _case("bf16", 1, 5, 7, 8, "tx1 m_below_ty tail_only"),
    "f32_tx1_35": _case("f32", 1, 5, 7, 4, "tx1 m_below_ty tail_only"),
    # 1311 rows = 5 row steps of 256 and 31 rows: one band, four-in-flight and tail, and it ends inside a row step
    "f32_tx1_1311": _case("f32", 3, 19, 23, 4, "tx1 one_band_partial_step four_and_tail"),
    "bf16_tx1_1311": _case("bf16", 3, 19, 23, 8, "tx1 one_band_partial_step four_and_tail", act=IDENTITY),
    # six channel groups: TX = 6 does not divide 256, TY = 42 and four idle threads.  Plane bias: HW = 35 / 99 is no multiple of
    # TY and the image index changes 6 / 2 times inside the one band.  Every operand is a slice of a wider buffer
    "bf16_six_groups_pb": _case("bf16", 7, 5, 7, 48, "idle_threads plane_bias_steps four_and_tail ld_pad", pb=True, pad=True),
    "f32_six_groups_pb": _case("f32", 3, 9, 11, 24, "idle_threads plane_bias_steps four_and_tail ld_pad", pb=True, pad=True),
    # 80 channel groups: gx = 2, the second block column has 16 live groups of 64; TY = 4 - the replica forms' wide geometry
    "bf16_80_groups": _case("bf16", 3, 5, 7, 640, "ragged_gx replicas_ty4"),
    "f32_80_groups": _case("f32", 3, 5, 7, 320, "ragged_gx"),
    # one row
    "bf16_one_row": _case("bf16", 1, 1, 1, 64, "m1 m_below_ty"),
    "f32_one_row": _case("f32", 1, 1, 1, 64, "m1 m_below_ty"),
    # 9 bands of 384 rows, the last one 96 rows = 3 row steps; second stage on 16 lanes below its four-in-flight loop.  Padded
    "bf16_9_bands": _case("bf16", 3, 33, 32, 64, "stage2_16_tail short_last_band ld_pad", pad=True),
    "f32_9_bands_pb": _case("f32", 3, 17, 19, 64, "stage2_16_tail short_last_band", pb=True),
    # 60 bands: the 16 lanes run their four-in-flight loop; the last band is 45 / 8 rows
    "bf16_60_bands": _case("bf16", 3, 161, 47, 64, "stage2_16_four short_last_band"),
    "f32_60_bands": _case("f32", 8, 5, 71, 256, "stage2_16_four short_last_band"),
    # 100 bands, M an exact multiple of rows_per_band: 64 lanes, tail loop only
    "bf16_100_bands": _case("bf16", 2, 100, 128, 64, "stage2_64_exact"),
    "f32_100_bands": _case("f32", 2, 40, 40, 256, "stage2_64_exact"),
    # 96 bands of 48 rows, the last one 5 rows: shorter than a four-row batch (16 rows) and it ends inside a row step
    "bf16_96_bands_ragged": _case("bf16", 5, 11, 83, 512, "stage2_64_ragged short_last_band replicas_ty4"),
    "f32_96_bands_ragged": _case("f32", 5, 11, 83, 256, "stage2_64_ragged short_last_band"),
    # 200 bands: the 64 lanes enter their own four-in-flight loop (more than 192 bands)
    "bf16_200_bands": _case("bf16", 2, 160, 160, 64, "stage2_64_four", passes="reduce"),
    # 512 bands of 48 rows: kMaxBands, where the band count stops following M (768 bands of 32 rows without the cap)
    "f32_512_bands": _case("f32", 4, 64, 96, 256, "band_cap stage2_64_four", passes="reduce"),
}

# what a class means, as a predicate on (case, M, reduce geometry, apply geometry)
def _last_band(M, g):
    return M - (g.gy - 1) * g.rows_per_band


def _lane_loops(M, g):
    """(some lane runs the four-in-flight loop, some lane runs the tail loop), over all bands"""
    rows = band_rows(M, g)
    return any(f for f, _ in rows), any(t for _, t in rows)


CLASSES = {
    "tx1": lambda cs, M, r, a: r.TX == 1 and cs.C == vec_of(cs.dtype),
    "idle_threads": lambda cs, M, r, a: K_BLOCK % r.TX != 0 and cs.C // vec_of(cs.dtype) == 6,
    "ragged_gx": lambda cs, M, r, a: r.gx >= 2 and (cs.C // vec_of(cs.dtype)) % r.TX != 0,
    "m1": lambda cs, M, r, a: M == 1,
    "m_below_ty": lambda cs, M, r, a: M < r.TY,
    "tail_only": lambda cs, M, r, a: _lane_loops(M, r) == (False, True) and _lane_loops(M, a) == (False, True),
    "four_and_tail": lambda cs, M, r, a: _lane_loops(M, r) == (True, True) and _lane_loops(M, a) == (True, True),
    "one_band_partial_step": lambda cs, M, r, a: r.gy == 1 and a.gy == 1 and M % r.TY != 0,
    "short_last_band": lambda cs, M, r, a: r.gy > 1 and _last_band(M, r) < r.rows_per_band and a.gy > 1 and _last_band(M, a) < a.rows_per_band,
    "stage2_16_tail": lambda cs, M, r, a: 1 < r.gy < 49,
    "stage2_16_four": lambda cs, M, r, a: 49 <= r.gy < WIDE_STAGE2_FROM,
    "stage2_64_exact": lambda cs, M, r, a: r.gy >= WIDE_STAGE2_FROM and M % r.rows_per_band == 0,
    "stage2_64_ragged": lambda cs, M, r, a: r.gy >= WIDE_STAGE2_FROM and _last_band(M, r) < 4 * r.TY and _last_band(M, r) % r.TY != 0,
    "stage2_64_four": lambda cs, M, r, a: r.gy > 192,
    "band_cap": lambda cs, M, r, a: r.gy == K_MAX_BANDS and M // (r.TY * 8) > K_MAX_BANDS,
    "plane_bias_steps": lambda cs, M, r, a: cs.pb and (cs.H * cs.W) % r.TY != 0 and min(r.rows_per_band, M) // (cs.H * cs.W) >= 2,
    "replicas_ty4": lambda cs, M, r, a: cs.dtype == "bf16" and a.TY == 4 and max(REPS) > 4 * a.TY and any(a.TY < n <= 4 * a.TY for n in REPS),
    "ld_pad": lambda cs, M, r, a: cs.pad,
}

# replica counts of the FIN / RAW forms: one (a plain load), three (fewer than TY = 4), five (more than TY: a second replica
# for row thread 0 inside one batch), seventeen (more than 4 TY: a second trip of the loop)
REPS = (1, 3, 5, 17)

# name: (dtype, B, HW, C, alpha, pad) - ucd_plane_sum
PLANE_CASES = {
    "bf16_hw_below_ty": ("bf16", 3, 5, 64, 1.0, False),              # TY = 32 > HW = 5
    "f32_hw_below_ty": ("f32", 3, 5, 64, 0.125, False),              # TY = 16
    "bf16_2048_tail": ("bf16", 2, 273, 2048, 0.125, False),          # the ASPP input's width: gx = 4, TY = 4; 68 rows per lane and one more for lane 0
    "f32_six_groups_tail": ("f32", 2, 200, 24, 1.0, True),           # TY = 42: one four-row batch and a tail row for the first 32 lanes
    "bf16_six_groups_tail": ("bf16", 4, 200, 48, 0.5, True),
}

# name: (dtype, B, H, W, C, ph, pw, pad) - ucd_window_mean
WINDOW_CASES = {
    "bf16_4x2": ("bf16", 2, 9, 11, 16, 4, 2, False),                 # ph != pw, area 8: exact
    "f32_4x2": ("f32", 2, 9, 11, 8, 4, 2, False),
    "bf16_full_height": ("bf16", 2, 9, 11, 16, 9, 3, False),         # ph = H: one output row; area 27
    "f32_full_height": ("f32", 2, 9, 11, 8, 9, 3, False),
    "bf16_2x1": ("bf16", 2, 9, 11, 16, 2, 1, False),                 # pw = 1
    "f32_1x1": ("f32", 2, 9, 11, 8, 1, 1, False),                    # the identity
    "bf16_1x1": ("bf16", 1, 5, 7, 8, 1, 1, False),
    "bf16_3x7": ("bf16", 3, 9, 11, 24, 3, 7, False),                 # area 21: one rounded multiply
    "f32_3x7": ("f32", 3, 9, 11, 12, 3, 7, False),
    "bf16_4x4_ld": ("bf16", 2, 9, 11, 16, 4, 4, True),               # input and output are channel slices
    "f32_3x7_ld": ("f32", 2, 9, 11, 8, 3, 7, True),
}


def window_area_exact(ph, pw):
    area = ph * pw
    return area & (area - 1) == 0


def small_rows(n_rows, C, seed):
    """Integer rows for plane_sum / window_mean: the channel offset plus a hash within 4."""
    return channel_offset(C) + ihash(n_rows * C, seed, -4, 4).view(n_rows, C)
