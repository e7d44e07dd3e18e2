"""Float64 reference of Local POD on the logits (PLOP's last level, ``extra_channels: "sum"``): numpy only, explicit loops over
scales and regions, the gradient from the closed form, not autograd.  Independent of ``ucd_amd.loss.local_pod_logits_torch``.

    merge (as PLOP writes it): M = zeros [B, K, h, w];  M[:, 0] = S[:, 0] + S[:, K:].sum(1);  M[:, 1:] = S[:, 1:K]
    Q_s = M^2, Q_t = T^2;  the pools of tests/pod_ref.py at slope 1 on K channels:  n_E = sum_s s^2 K (h // s + w // s)
    normalize = 1: E^ = E / max(|E|, 1e-12), l_b = |E^_s - E^_t|;   normalize = 0: l_b = |E_s - E_t|;   level = mean_b l_b
    dS[c] = 2 M[k(c)] dQ[k(c)],  k(c) = c below K, 0 from K on
"""
import numpy as np

import pod_ref

EPS = 1e-12


def n_embed(K, h, w, scales):
    return sum(s * s * K * (h // s + w // s) for s in scales)


def merge(s, K):
    """[B, Ctot, h, w] -> [B, K, h, w]."""
    b = np.asarray(s, dtype=np.float64)
    if K == b.shape[1]:
        return b.copy()
    m = np.zeros((b.shape[0], K) + b.shape[2:])
    m[:, 0] = b[:, 0] + b[:, K:].sum(1)
    m[:, 1:] = b[:, 1:K]
    return m


def distances(s, t, scales, normalize):
    t = np.asarray(t, dtype=np.float64)
    m = merge(s, t.shape[1])
    ls = []
    for ms, mt in zip(m, t):
        es, et = pod_ref.embed(ms, 1.0, scales), pod_ref.embed(mt, 1.0, scales)
        if normalize:
            es = es / max(np.linalg.norm(es), EPS)
            et = et / max(np.linalg.norm(et), EPS)
        ls.append(np.linalg.norm(es - et))
    return np.asarray(ls)


def level(s, t, scales, normalize):
    return float(distances(s, t, scales, normalize).mean())


def level_grad(s, t, scales, normalize, weight=1.0):
    """d(weight * level) / d s, [B, Ctot, h, w] float64."""
    s, t = np.asarray(s, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, Ctot, h, w = s.shape
    K = t.shape[1]
    m = merge(s, K)
    grad = np.zeros_like(s)
    for b in range(B):
        es, et = pod_ref.embed(m[b], 1.0, scales), pod_ref.embed(t[b], 1.0, scales)
        if normalize:
            ns = max(np.linalg.norm(es), EPS)
            eh_s, eh_t = es / ns, et / max(np.linalg.norm(et), EPS)
            l = np.linalg.norm(eh_s - eh_t)
            u = (eh_s - eh_t) / l if l > 0 else np.zeros_like(eh_s)
            g = (weight / B) * (u - eh_s * np.dot(eh_s, u)) / ns
        else:
            l = np.linalg.norm(es - et)
            g = (weight / B) * (es - et) / l if l > 0 else np.zeros_like(es)
        dq = np.zeros((K, h, w))
        off = 0
        for sc in scales:
            kh, kw = h // sc, w // sc
            for i in range(sc):
                for j in range(sc):
                    g_row = g[off:off + K * kh].reshape(K, kh)
                    off += K * kh
                    g_col = g[off:off + K * kw].reshape(K, kw)
                    off += K * kw
                    dq[:, i * kh:(i + 1) * kh, j * kw:(j + 1) * kw] += g_row[:, :, None] / kw + g_col[:, None, :] / kh
        assert off == g.size
        dm = 2.0 * m[b] * dq
        grad[b, :K] = dm
        grad[b, K:] = dm[0]
    return grad


def integer_logits(seed, B, Ctot, K, h, w):
    """Student [B, Ctot, h, w] and teacher [B, K, h, w] logits of small integers |x| <= 8: every merge, square and strip sum of
    the kernels is exact in fp32."""
    rng = np.random.RandomState(seed)
    s = rng.randint(-8, 9, size=(B, Ctot, h, w)).astype(np.float64)
    t = rng.randint(-8, 9, size=(B, K, h, w)).astype(np.float64)
    return s, t
