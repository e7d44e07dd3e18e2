"""Float64 numpy reference of SDR's class-prototype feature losses (csrc/proto.hip): the class of a
low-resolution pixel, the three values and the gradient w.r.t. the map - and the exact operands the tests feed to it."""
import numpy as np

EPS = 1e-6


def nearest_index(src, dst):
    """F.interpolate(mode='nearest'): min(floor(i * (float)src / dst), src - 1), the product in fp32."""
    scale = np.float32(src) / np.float32(dst)
    idx = np.floor(np.arange(dst, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, src - 1)


def classes(labels, sem_t, T, K, hw, ignore_index=255):
    """int32 [B, h, w]: the nearest down-sampled label; -1 where ignored or outside [0, T); with teacher logits [B, K, h, w] a
    background pixel takes their first arg-max."""
    h, w = hw
    B, H, W = labels.shape
    y = labels[:, nearest_index(H, h)][:, :, nearest_index(W, w)]
    cls = np.where((y == ignore_index) | (y < 0) | (y >= T), -1, y)
    if sem_t is not None:
        cls = np.where(cls == 0, np.argmax(sem_t[:, :K], axis=1), cls)        # numpy's arg-max is the first maximum too
    return cls.astype(np.int32)


def losses(X, cls, state_sum, state_n, O, valid, weights, upstream=1.0):
    """X [M, C] float64, cls [M].  Returns (total, (L_match, L_attr, L_rep), d total * upstream / d X [M, C], S [T, C], n [T])."""
    w_m, w_a, w_r = weights
    X = np.asarray(X, dtype=np.float64)
    M, C = X.shape
    T = state_sum.shape[0]
    K = 0 if O is None else O.shape[0]
    n = np.zeros(T, dtype=np.int64)
    S = np.zeros((T, C))
    for c in range(T):
        rows = cls == c
        n[c] = rows.sum()
        S[c] = X[rows].sum(axis=0)
    P = [c for c in range(T) if n[c] > 0]
    mu = {c: S[c] / n[c] for c in P}
    G = {c: np.zeros(C) for c in P}
    d_x = np.zeros_like(X)
    # matching
    A = [c for c in P if c < K and valid[c]]
    l_match = 0.0
    for c in A:
        diff = mu[c] - O[c]
        d = np.sqrt((diff * diff).sum())
        l_match += d / len(A)
        if d > 0:
            G[c] += w_m / len(A) * diff / d
    # attraction
    Bs = [c for c in P if state_n[c] > 0]
    l_attr = 0.0
    for c in Bs:
        R = state_sum[c] / state_n[c]
        rows = cls == c
        diff = X[rows] - R
        l_attr += (diff * diff).sum() / n[c] / len(Bs)
        d_x[rows] += 2.0 * w_a / (len(Bs) * n[c]) * diff
    # repulsion
    l_rep = 0.0
    if len(P) >= 2:
        for c in P:
            for k in P:
                if k == c:
                    continue
                diff = mu[c] - mu[k]
                d = np.sqrt((diff * diff).sum())
                l_rep += 1.0 / (d + EPS) / len(P)
                if d > 0:
                    G[c] += w_r / len(P) * 2.0 * (-1.0 / (d + EPS) ** 2) * diff / d        # the pair counts as (c, k) and as (k, c)
    for c in P:
        d_x[cls == c] += G[c] / n[c]
    total = w_m * l_match + w_a * l_attr + w_r * l_rep
    return total, (l_match, l_attr, l_rep), d_x * upstream, S, n


def case(seed, B, h, w, C, T, K, H, W, crowd=None, single=None, ignore_index=255):
    """Exact operands of one case.  ``labels`` [B, H, W] int64 carry a designed low-resolution class map at exactly the pixels the
    nearest rule reads and other classes everywhere else; ``sem_t`` [B, K, h, w] are small-integer teacher logits with ties;
    ``X`` [B h w, C] small integers with |x| <= 64 (exact in bf16, every sum exact in fp32) around class centres that keep the class
    means at least 1 apart; the running prototypes are multiples of 1/4 (``state_sum = N R`` exactly), the old ones of 1/2.
    ``crowd``: a class that takes more than half of the pixels; ``single``: a class that takes exactly one."""
    rng = np.random.RandomState(seed)
    M = B * h * w
    pool = np.concatenate([np.arange(T), [0] * (T // 2 + 1) if K else [], [ignore_index, T + 3]]).astype(np.int64)
    if single is not None:
        pool = pool[pool != single]
    low = pool[rng.randint(0, len(pool), size=M)]
    if crowd is not None:
        low[rng.rand(M) < 0.55] = crowd
    low[0], low[1] = ignore_index, T + 3                  # an ignored and an out-of-range pixel in every case
    if single is not None:
        low[rng.randint(2, M)] = single
    low = low.reshape(B, h, w)
    labels = rng.randint(0, T, size=(B, H, W)).astype(np.int64)
    if single is not None:
        labels[labels == single] = ignore_index
    labels[np.ix_(np.arange(B), nearest_index(H, h), nearest_index(W, w))] = low
    sem_t = rng.randint(-3, 4, size=(B, K, h, w)).astype(np.float64) if K else None
    cls = classes(labels, sem_t, T, K, (h, w), ignore_index)
    assert (cls[low != 0] == np.where((low == ignore_index) | (low >= T), -1, low)[low != 0]).all()
    centres = rng.randint(-40, 41, size=(T, C)).astype(np.float64)
    flat = cls.reshape(M)
    X = rng.randint(-8, 9, size=(M, C)).astype(np.float64) + centres[np.where(flat >= 0, flat, 0)]
    assert np.abs(X).max() <= 64
    state_n = rng.randint(0, 50, size=T).astype(np.int64)
    state_n[rng.rand(T) < 0.25] = 0
    R = rng.randint(-128, 129, size=(T, C)) / 4.0
    state_sum = R * state_n[:, None]
    O = rng.randint(-64, 65, size=(K, C)) / 2.0 if K else None
    valid = rng.rand(K) < 0.75 if K else None
    present = [c for c in range(T) if (flat == c).any()]
    means = np.stack([X[flat == c].mean(axis=0) for c in present]) if present else np.zeros((0, C))
    if len(present) >= 2:
        gaps = np.sqrt(((means[:, None] - means[None]) ** 2).sum(axis=2)) + np.eye(len(present)) * 1e9
        assert gaps.min() >= 1.0, gaps.min()
    out = dict(labels=labels, sem_t=sem_t, cls=cls, X=X, state_sum=state_sum, state_n=state_n, O=O, valid=valid,
               shape=(B, h, w, C, T, K))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def integer_features(seed, M, C, T, cls):
    """Small-integer rows with |x| <= 64 around integer class centres (exact in bf16; all sums exact in fp32)."""
    rng = np.random.RandomState(seed)
    centres = rng.randint(-40, 41, size=(T, C)).astype(np.float64)
    flat = np.asarray(cls).reshape(M)
    return rng.randint(-8, 9, size=(M, C)).astype(np.float64) + centres[np.where(flat >= 0, flat, 0)]
