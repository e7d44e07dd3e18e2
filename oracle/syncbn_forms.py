"""TEST INFRASTRUCTURE - float64 reference of the multi-rank (SyncBN) forms of the fused norm kernels, and the seeded inputs of
tests/test_syncbn_forms_gpu.py.

The reference is training-mode batch norm over the CONCATENATED batch of all ranks (what InPlaceABNSync computes,
oracle/syncbn.py), the activation, and for the stem the 3x3 / 2 max pool, in float64 torch on the CPU.  It is written the way
the ranks see it - per-rank (mean_r, M2_r), Chan's combination, count = world * M, global sums in the per-element term of the
backward and this rank's sums in the parameter gradients - so that each of the four mistakes a multi-rank kernel sequence can
make is one switch (``MISTAKES``); tests/test_syncbn_forms_cpu.py asserts that every switch moves the reference by at least ten
times the bar the GPU tests apply, i.e. that a pass of the GPU tests excludes the mistake.

Stored weight convention of the in-place layers (``abs_gamma``): gamma~ = |weight| + eps, d weight = sign(weight) * sum dz xhat.
"""
import torch
import torch.nn.functional as F

WORLD = 3
EPS = 1e-5
MOMENTUM = 0.1
SLOPE = 0.01
NEG_CHANNEL = 5                         # the channel whose stored weight is negative
RANK_OFFSETS = (0.0, 2.0, -3.0)         # per-rank offset of the activations in units of the per-channel std

MISTAKES = ("no_between", "count_m", "global_grads", "no_sign")

# ---- the bars of the GPU tests (fp32 quantities: those of tests/test_abn_gpu.py::test_sync_forward_backward_kernels_match_global_batch
# in its fp32 case; scale = gamma~ * invstd takes invstd's, a pack's M2_r the variance's times M) ----
BAR_MEAN = dict(rtol=1e-5, atol=1e-5)
BAR_VAR = dict(rtol=1e-4, atol=1e-5)
BAR_INVSTD = dict(rtol=1e-4, atol=0.0)
BAR_SCALE = dict(rtol=1e-4, atol=0.0)
BAR_RMEAN = dict(rtol=1e-5, atol=1e-6)
BAR_RVAR = dict(rtol=1e-4, atol=0.0)
BAR_GRAD_SUMS = dict(rtol=1e-3, atol=1e-3)
BF16_ULP = 2.0 ** -8                    # per element: one bf16 ulp of the float64 value (+ the propagated bars of the constants)
BF16_L2 = 2.0 ** -9                     # relative L2 over a bf16 tensor


def bar(ref, rtol, atol):
    """The allowance |got - ref| <= atol + rtol |ref| as a tensor."""
    return atol + rtol * ref.abs()


def bf16_round(t):
    return t.float().bfloat16().double()


def act_fn(pre, slope):
    return torch.where(pre > 0, pre, pre * slope)


def act_grad(pre, slope):
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))


# ---------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------
def rank_pack(x):
    """x [M, C] float64 rows of one rank -> (mean_r, M2_r)."""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).sum(0)


def combine(packs, m_local, mistake=None):
    """packs: list of (mean_r, M2_r) -> (mean, M2) of the global batch: Chan's combination for equal counts."""
    means = torch.stack([p[0] for p in packs])
    mean = means.mean(0)
    m2 = torch.stack([p[1] for p in packs]).sum(0)
    if mistake != "no_between":
        m2 = m2 + m_local * ((means - mean) ** 2).sum(0)
    return mean, m2


def gamma_eff(weight, abs_gamma):
    return weight.abs() + EPS if abs_gamma else weight


def forward_constants(rows, weight, running_mean, running_var, abs_gamma=True, mistake=None):
    """rows: list over ranks of [M, C] float64 -> dict(packs, mean, var, invstd, scale, running_mean, running_var, count)."""
    m_local = rows[0].shape[0]
    packs = [rank_pack(x) for x in rows]
    mean, m2 = combine(packs, m_local, mistake)
    count = float(m_local if mistake == "count_m" else len(rows) * m_local)
    var = m2 / count
    invstd = 1.0 / torch.sqrt(var + EPS)
    return dict(packs=packs, mean=mean, var=var, invstd=invstd, scale=gamma_eff(weight, abs_gamma) * invstd, count=count,
                running_mean=(1 - MOMENTUM) * running_mean + MOMENTUM * mean,
                running_var=(1 - MOMENTUM) * running_var + MOMENTUM * var * count / (count - 1))


def apply_rows(x, k, bias, slope, residual=None):
    """act((x - mean) scale + bias [+ residual]) -> (pre-activation, output)."""
    pre = (x - k["mean"]) * k["scale"] + bias
    if residual is not None:
        pre = pre + residual
    return pre, act_fn(pre, slope)


def backward_rows(rows, dzs, k, weight, abs_gamma=True, mistake=None):
    """The norm's backward on d pre (``dzs``: list over ranks of [M, C], the gradient w.r.t. the pre-activation):
    -> dict(local [per rank (d bias_r, d weight_r)], total (sum dz, sum dz xhat), dx [per rank]).  dx takes the global sums over
    count = world * M, the parameter gradients this rank's sums with the sign of the stored weight."""
    sign = torch.where(weight < 0, -1.0, 1.0).double() if abs_gamma else torch.ones_like(weight)
    xhat = [(x - k["mean"]) * k["invstd"] for x in rows]
    raw = [(dz.sum(0), (dz * xh).sum(0)) for dz, xh in zip(dzs, xhat)]
    total = (torch.stack([r[0] for r in raw]).sum(0), torch.stack([r[1] for r in raw]).sum(0))
    gsign = torch.ones_like(sign) if mistake == "no_sign" else sign
    if mistake == "global_grads":
        local = [(total[0], total[1] * gsign) for _ in raw]
    else:
        local = [(r[0], r[1] * gsign) for r in raw]
    count = k["count"]
    k0 = total[0] / count
    # one side of the all-reduce without the sign: the kernel that undoes it then flips the term of the negative channels
    k1 = total[1] / count * (sign if mistake == "no_sign" else 1.0)
    dx = [(dz - k0 - xh * k1) * k["scale"] for dz, xh in zip(dzs, xhat)]
    return dict(local=local, total=total, dx=dx, k0=k0, k1=k1)


def rows_of(t):
    """[B, C, H, W] -> [B H W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def maps_of(rows, like):
    B, C, H, W = like.shape
    return rows.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------
# the stem: norm + activation + 3x3 / 2 max pool
# ---------------------------------------------------------------------------------------------
def _windows(a):
    """[B, C, H, W] -> the 3x3 / stride 2 / padding 1 windows [B, C, 9, L] (-inf outside the map) and the flat pixel index of every
    window slot [9, L] (-1 outside)."""
    B, C, H, W = a.shape
    win = F.unfold(F.pad(a, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
    pix = torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W)
    pos = F.unfold(F.pad(pix, (1, 1, 1, 1), value=-1.0), 3, stride=2).view(9, -1).long()
    return win, pos


def pool_argmax(a):
    """The pool's decision on the bf16-ROUNDED activation (what a separate apply pass stores and what the fused kernel compares):
    -> flat pixel index [B, C, L] of every window's maximum (first maximum of a tie, like max_pool2d)."""
    win, pos = _windows(bf16_round(a))
    slot = win.argmax(2)                                   # ties are excluded by the inputs (stem_case)
    return pos.t()[torch.arange(pos.shape[1]), slot]       # [B, C, L]


def window_margin(a):
    """(top - runner-up) of every window of the bf16-rounded activation, in units of the bf16 spacing at the top value, and the
    runner-up's flat pixel index."""
    win, pos = _windows(bf16_round(a))
    top, slot = win.topk(2, dim=2)
    ulp = 2.0 ** (torch.floor(torch.log2(top[:, :, 0].abs().clamp_min(1e-30))) - 7)
    return (top[:, :, 0] - top[:, :, 1]) / ulp, pos.t()[torch.arange(pos.shape[1]), slot[:, :, 1]]


def stem_forward(zs, weight, bias, running_mean, running_var, slope, mistake=None):
    """zs: list over ranks of [B, C, H, W] float64 (the bf16 activations) -> constants + per-rank pre-activation, pooled output and
    arg-max index."""
    k = forward_constants([rows_of(z) for z in zs], weight, running_mean, running_var, True, mistake)
    k["pre"], k["pooled"], k["idx"] = [], [], []
    for z in zs:
        pre, a = apply_rows(rows_of(z), k, bias, slope)
        pre, a = maps_of(pre, z), maps_of(a, z)
        idx = pool_argmax(a)
        k["pre"].append(pre); k["idx"].append(idx)
        k["pooled"].append(a.flatten(2).gather(2, idx))    # float64 value at the position the bf16 comparison chose [B, C, L]
    return k


def stem_backward(zs, dpools, k, weight, slope, mistake=None):
    """dpools: list over ranks of [B, C, L] float64 -> backward_rows' dict on d pre = scatter(dpool) * act'(pre)."""
    dzs = []
    for z, dp, pre, idx in zip(zs, dpools, k["pre"], k["idx"]):
        g = torch.zeros_like(z).flatten(2).scatter_add_(2, idx, dp).view_as(z)
        dzs.append(rows_of(g * act_grad(pre, slope)))
    return backward_rows([rows_of(z) for z in zs], dzs, k, weight, True, mistake)


# ---------------------------------------------------------------------------------------------
# seeded inputs (CPU)
# ---------------------------------------------------------------------------------------------
def _params(g, C):
    weight = torch.rand(C, generator=g) + 0.5
    weight[NEG_CHANNEL] = -0.8
    bias = torch.randn(C, generator=g) * 0.3
    running_mean = torch.randn(C, generator=g) * 0.2
    running_var = torch.rand(C, generator=g) + 0.5
    return weight, bias, running_mean, running_var


def stem_case(shape, slope, seed=7):
    """Stem inputs: per rank a bf16 map [B, C, H, W] (channel std 1.5 .. 3, rank offsets RANK_OFFSETS), the layer's parameters and a
    pooled-map gradient with a per-rank mean.

    A random draw cannot be tie free: ~0.6 % of the 3x3 windows have their two largest values in one bf16 bucket, and the three ranks
    hold thousands of windows - re-seeding would never end.  So the draw is REPAIRED: while a window's top two bf16 activations are
    closer than two bf16 steps (a tie, or a pair that the last fp32 bit of a constant could turn into one), the runner-up's z is
    lowered by a quarter of the channel std; likewise a pre-activation closer to zero than 1e-3 (the leaky_relu derivative must not
    hang on the last bit either).  Every pass recomputes the float64 statistics of the changed maps; the loop ends when a pass finds
    nothing."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    weight, bias, rm, rv = _params(g, C)
    std = 1.5 + 1.5 * torch.rand(C, generator=g)
    base = 0.3 * torch.randn(C, generator=g)
    zs = [((torch.randn(B, C, H, W, generator=g) + off) * std.view(1, C, 1, 1) + base.view(1, C, 1, 1)).bfloat16()
          for off in RANK_OFFSETS]
    for _ in range(200):
        k = stem_forward([z.double() for z in zs], weight.double(), bias.double(), rm.double(), rv.double(), slope)
        dirty = False
        for z, pre in zip(zs, k["pre"]):
            a = act_fn(pre, slope)
            margin, runner = window_margin(a)
            flat = z.flatten(2)
            bad = margin < 2
            if bad.any():
                cur = flat.double()
                # a pixel that is the runner-up of several windows takes one step (the minimum), the others keep their value
                low = torch.where(bad, cur.gather(2, runner) - (0.25 * std).view(1, C, 1), torch.full_like(margin, float("inf")))
                flat.copy_(cur.scatter_reduce(2, runner, low, "amin", include_self=True).bfloat16())
                dirty = True
            near = pre.abs().flatten(2) < 1e-3
            if near.any():
                flat.copy_(torch.where(near, flat.double() - (0.05 * std).view(1, C, 1), flat.double()).bfloat16())
                dirty = True
        if not dirty:
            break
    else:
        raise AssertionError("stem_case: the tie repair did not converge")
    L = k["idx"][0].shape[2]
    # per-rank means of different size and sign: no rank's sums vanish, and no two ranks' sums cancel
    dpools = [(0.15 * torch.randn(B, C, L, generator=g) + m).bfloat16() for m in (0.6, 0.9, -0.3)]
    return dict(zs=zs, dpools=dpools, weight=weight, bias=bias, running_mean=rm, running_var=rv, shape=shape)


def conv_case(M=286, K=64, N=128, seed=3):
    """Operands of the conv paths: per rank a [M, K] bf16, one weight [N, K] bf16.  Column 0 of ``a`` is constant per rank and
    carries the rank offset (RANK_OFFSETS times the channel's std through w[:, 0]), column 1 is 1 and carries a small channel mean,
    the rest is noise; ``product`` restates the stored bf16 product on the CPU (the GPU tests read the kernel's own)."""
    g = torch.Generator().manual_seed(seed)
    weight, bias, rm, rv = _params(g, N)
    w = torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5
    std = w[:, 2:].norm(dim=1)
    w[:, 0] = std
    w[:, 1] = 0.3 * std * torch.randn(N, generator=g)
    w = w.bfloat16()
    a = []
    for off in RANK_OFFSETS:
        t = torch.randn(M, K, generator=g)
        t[:, 0] = off
        t[:, 1] = 1.0
        a.append(t.bfloat16())
    ys = [(x.float() @ w.float().t()).bfloat16() for x in a]
    full = torch.cat(ys).double()
    shift = (full.mean(0) + 0.1 * full.std(0) * torch.randn(N, generator=g)).float()
    # gradients w.r.t. the layer's output: noise + a mean + a part along the activation, so that every rank's two sums are far
    # from zero and from the other ranks'
    dys = []
    for y in ys:
        u = (y.double() - y.double().mean(0)) / y.double().std(0)
        dys.append((0.5 * torch.randn(M, N, generator=g) + 0.25 + u.float()).bfloat16())
    res = [torch.randn(M, N, generator=g).bfloat16() for _ in RANK_OFFSETS]
    return dict(a=a, w=w, ys=ys, dys=dys, res=res, shift=shift, weight=weight, bias=bias, running_mean=rm, running_var=rv,
                M=M, K=K, N=N)


def shifted_sums(rows, shift, dtype=torch.float64):
    """[sum (y - k) | sum (y - k)^2] per channel over the rows in ``dtype``, one row after another (in float32: a plain sequential
    restatement of what an accumulator about a shift holds - its error against float64 sizes the bar of the atomic sums)."""
    d = rows.to(dtype) - shift.to(dtype)
    if dtype == torch.float64:
        return d.sum(0), (d * d).sum(0)
    s1, s2 = torch.zeros_like(d[0]), torch.zeros_like(d[0])
    for r in d:
        s1 += r
        s2 += r * r
    return s1, s2


# ---------------------------------------------------------------------------------------------
# the conv paths: forward apply of the stored product, backward link epilogue + apply on raw sums
# ---------------------------------------------------------------------------------------------
LINK_K = 192            # depth of the gradient product: N columns that carry the activation's direction, a ones column, noise


def link_case(case, seed=5):
    """Operands of the backward link (out_mode 3 / 4) on top of conv_case: the gradient product g [M, 192] . wg [N, 192]^T =
    (normalised activation of the channel) + 0.25 + noise, the block-link's sign tensor and shortcut gradient."""
    g = torch.Generator().manual_seed(seed)
    M, N = case["M"], case["N"]
    wg = torch.zeros(N, LINK_K)
    wg[:, :N] = torch.eye(N)
    wg[:, N] = 0.25
    wg[:, N + 1:] = torch.randn(N, LINK_K - N - 1, generator=g) * 0.5 / (LINK_K - N - 1) ** 0.5
    gs = []
    for y in case["ys"]:
        t = torch.randn(M, LINK_K, generator=g)
        t[:, :N] = ((y.double() - y.double().mean(0)) / y.double().std(0)).float()
        t[:, N] = 1.0
        gs.append(t.bfloat16())
    out = [torch.randn(M, N, generator=g).bfloat16() for _ in gs]          # out_mode 4: the block output (its sign)
    skip = [(0.3 * torch.randn(M, N, generator=g)).bfloat16() for _ in gs]  # out_mode 4: the shortcut's gradient
    assert all((o != 0).all() for o in out)
    return dict(g=gs, wg=wg.bfloat16(), out=out, skip=skip)


def link_dpre(acc, x, k, bias, slope, mode, out=None, skip=None):
    """d pre of the link epilogue in float64: mode 3 acc * act'((x - mean) scale + bias), mode 4 (acc + skip) * act'(out)."""
    if mode == 3:
        return acc * act_grad((x - k["mean"]) * k["scale"] + bias, slope)
    return (acc + skip) * act_grad(out, slope)


def y_allowance(x, k):
    """What the fp32 bars of mean and scale may move an applied element by."""
    return bar(k["mean"], **BAR_MEAN) * k["scale"] + (x - k["mean"]).abs() * bar(k["scale"], **BAR_SCALE)


def dx_allowance(x, dx, k, b):
    """What the fp32 bars of the constants and of the two sums may move an element of dx by."""
    xh = (x - k["mean"]) * k["invstd"]
    dk0, dk1 = bar(b["total"][0], **BAR_GRAD_SUMS) / k["count"], bar(b["total"][1], **BAR_GRAD_SUMS) / k["count"]
    dxh = bar(k["mean"], **BAR_MEAN) * k["invstd"] + xh.abs() * BAR_INVSTD["rtol"]
    return k["scale"] * (dk0 + xh.abs() * dk1 + b["k1"].abs() * dxh) + dx.abs() * BAR_SCALE["rtol"]
