"""Checker for var_policy_dist (include/var_hip.h), numpy only: a Philox4x32-10 restatement, the generator's uniform /
Box-Muller mapping, and the two distributions' action and log-probability in float64."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: (..., 4) and key: (..., 2) unsigned 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def words(key0, key1, step, rows):
    """The four words of every row in `rows` at the 64-bit `step`: counter {step_lo, step_hi, row, 0}."""
    rows = np.asarray(rows, dtype=np.uint64)
    ctr = np.zeros(rows.shape + (4,), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = step & MASK, (step >> 32) & MASK, rows
    return philox4x32_10(ctr, np.array([key0, key1], dtype=np.uint64))


def uniform(x):
    """u = ((x >> 8) + 0.5) * 2^-24 as the kernel holds it: a float32.  The sum needs 25 bits from 2^23 on, so it rounds to
    even there (the largest word gives 1.0); rounding the exact float64 value to float32 is the same rounding."""
    exact = ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return exact.astype(np.float32)


def categorical_noise(key0, key1, step, B):
    return uniform(words(key0, key1, step, np.arange(B))[:, 0])


def gaussian_noise(key0, key1, step, B, n):
    """float64 Box-Muller on the float32 uniforms: (x0, x1) -> z0, z1 and (x2, x3) -> z2, z3; the first n per row."""
    u = uniform(words(key0, key1, step, np.arange(B))).astype(np.float64)
    z = np.empty((B, 4))
    for a in (0, 2):
        r, t = np.sqrt(-2.0 * np.log(u[:, a])), 2.0 * np.pi * u[:, a + 1]
        z[:, a], z[:, a + 1] = r * np.cos(t), r * np.sin(t)
    return z[:, :n]


def softmax_cdf(logits):
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p, np.cumsum(p, axis=1)


def dist(kind, head, logstd, noise, deterministic):
    """kind 0: head = mean (B,n), logstd (n), noise = z (B,n) -> action (B,n), logp (B,1).
    kind 1: head = logits (B,n), noise = u (B,) -> action (B,1) int64, logp (B,1).  float64 throughout."""
    head = np.asarray(head, dtype=np.float64)
    if kind == 0:
        ls = np.asarray(logstd, dtype=np.float64).reshape(1, -1)
        std = np.exp(ls)
        a = head.copy() if deterministic else head + std * np.asarray(noise, dtype=np.float64)
        logp = (-(a - head) ** 2 / (2.0 * std ** 2) - ls - 0.5 * np.log(2.0 * np.pi)).sum(axis=1, keepdims=True)
        return a, logp
    n = head.shape[1]
    _, cdf = softmax_cdf(head)
    if deterministic:
        a = head.argmax(axis=1)                                   # numpy: the first index of the maximum
    else:
        u = np.asarray(noise, dtype=np.float64).reshape(-1, 1)
        a = (cdf[:, :n - 1] <= u).sum(axis=1)
    mx = head.max(axis=1, keepdims=True)
    logsm = head - mx - np.log(np.exp(head - mx).sum(axis=1, keepdims=True))
    return a.reshape(-1, 1).astype(np.int64), np.take_along_axis(logsm, a.reshape(-1, 1), axis=1)


def near_boundary(logits, u, eps=1e-5):
    """Rows whose u lies within eps of a float64 CDF boundary: an fp32 CDF may fall on the other side there."""
    n = np.asarray(logits).shape[1]
    _, cdf = softmax_cdf(logits)
    return (np.abs(cdf[:, :n - 1] - np.asarray(u, dtype=np.float64).reshape(-1, 1)) < eps).any(axis=1)
