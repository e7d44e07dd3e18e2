"""Float64 reference of Local POD (PLOP's ``_local_pod``, on maps of any aspect), written from the formulas with explicit loops over
scales and regions.  Independent of ``ucd_amd.loss.local_pod_torch``: numpy only, the gradient from the closed form, not autograd.

    P = X >= 0 ? X : X / a,  Q = P^2
    scale s: kh = h // s, kw = w // s; region (i, j) = rows [i kh, (i+1) kh) x columns [j kw, (j+1) kw)
    E = all (mean of Q over the region's columns per (channel, row), mean over its rows per (channel, column))
    E^ = E / max(|E|, 1e-12);  l_b = |E^_s - E^_t|;  level = mean_b l_b
"""
import numpy as np

EPS = 1e-12


def n_embed(C, h, w, scales):
    return sum(s * s * C * (h // s + w // s) for s in scales)


def _pre(x, a):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x >= 0, x, x / a)


def embed(x, a, scales):
    """E of one sample: x [C, h, w]."""
    q = _pre(x, a) ** 2
    C, h, w = q.shape
    out = []
    for s in scales:
        kh, kw = h // s, w // s
        for i in range(s):
            for j in range(s):
                reg = q[:, i * kh:(i + 1) * kh, j * kw:(j + 1) * kw]
                out.append(reg.mean(axis=2).reshape(-1))        # [C, kh]: over the region's columns
                out.append(reg.mean(axis=1).reshape(-1))        # [C, kw]: over the region's rows
    return np.concatenate(out)


def distances(x_s, x_t, a, scales):
    """l_b for every sample of [B, C, h, w] maps."""
    ls = []
    for xs, xt in zip(np.asarray(x_s, dtype=np.float64), np.asarray(x_t, dtype=np.float64)):
        es, et = embed(xs, a, scales), embed(xt, a, scales)
        es = es / max(np.linalg.norm(es), EPS)
        et = et / max(np.linalg.norm(et), EPS)
        ls.append(np.linalg.norm(es - et))
    return np.asarray(ls)


def level(x_s, x_t, a, scales):
    return float(distances(x_s, x_t, a, scales).mean())


def level_grad(x_s, x_t, a, scales, weight=1.0):
    """d(weight * level) / d x_s, [B, C, h, w] float64."""
    x_s, x_t = np.asarray(x_s, dtype=np.float64), np.asarray(x_t, dtype=np.float64)
    B, C, h, w = x_s.shape
    grad = np.zeros_like(x_s)
    for b in range(B):
        es, et = embed(x_s[b], a, scales), embed(x_t[b], a, scales)
        ns = max(np.linalg.norm(es), EPS)
        eh_s, eh_t = es / ns, et / max(np.linalg.norm(et), EPS)
        l = np.linalg.norm(eh_s - eh_t)
        u = (eh_s - eh_t) / l if l > 0 else np.zeros_like(eh_s)
        g = (weight / B) * (u - eh_s * np.dot(eh_s, u)) / ns
        dq = np.zeros((C, h, w))
        off = 0
        for s in scales:
            kh, kw = h // s, w // s
            for i in range(s):
                for j in range(s):
                    g_row = g[off:off + C * kh].reshape(C, kh)
                    off += C * kh
                    g_col = g[off:off + C * kw].reshape(C, kw)
                    off += C * kw
                    dq[:, i * kh:(i + 1) * kh, j * kw:(j + 1) * kw] += g_row[:, :, None] / kw + g_col[:, None, :] / kh
        assert off == g.size
        grad[b] = 2.0 * _pre(x_s[b], a) * dq * np.where(x_s[b] >= 0, 1.0, 1.0 / a)
    return grad


def integer_maps(seed, shape, a):
    """Student and teacher maps of small integers |x| <= 8 (exact in bf16).  With a = 1 negative entries stay as they are; with
    another slope a negative entry is stored as ``a * integer`` where that product is exact in float32 and in bfloat16 (a power of
    two slope), else as the integer itself - the stored value is then what every implementation reads."""
    rng = np.random.RandomState(seed)
    maps = []
    for _ in range(2):
        k = rng.randint(-8, 9, size=shape).astype(np.float64)
        if a != 1.0:
            m, _e = np.frexp(a)
            if m == 0.5:                                   # a power of two: the product is exact
                k = np.where(k < 0, k * a, k)
        maps.append(k)
    return maps[0], maps[1]
