"""TEST INFRASTRUCTURE: the numpy restatement of var_reward_norm_step (csrc/env_step.hip) in the kernel's own order -- scalar
float64 operations, one rounding each, the sums over the envs walked as the kernel's single thread walks them -- and the seeded
input sequences the host and GPU tests share.  `pairwise=False` (sums left to right) and `zero_first=True` (ret zeroed before
the update instead of after) are the two faults the tests inject to show that the comparison can fail."""
import numpy as np

NS = (1, 7, 8, 9, 16, 17, 64, 128)
STEPS = 50
ALL_DONE_STEP = 23
SEED = 21


def numpy_order_sum(a, n, mean=None, pairwise=True):
    """np.add.reduce of a contiguous float64 vector of n <= 128 elements, element by element; mean: sum (a - mean)^2 instead."""
    f = np.float64

    def at(i):
        if mean is None:
            return f(a[i])
        d = f(a[i]) - mean
        return d * d
    if n < 8 or not pairwise:
        res = f(0.0)
        for i in range(n):
            res = res + at(i)
        return res
    r = [at(k) for k in range(8)]
    i = 8
    while i < n - (n % 8):
        for k in range(8):
            r[k] = r[k] + at(i + k)
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        res = res + at(i)
        i += 1
    return res


class NormStep:
    """State and one step of the kernel: ret (N), rms [mean, var, count], episode (3, N), slot [2]."""

    def __init__(self, n, gamma=0.99, cliprew=10.0, epsilon=1e-8, normalise=True, num_steps=1, pairwise=True, zero_first=False):
        self.n, self.gamma, self.cliprew, self.epsilon = n, np.float64(gamma), np.float64(cliprew), np.float64(epsilon)
        self.normalise, self.num_steps, self.pairwise, self.zero_first = normalise, num_steps, pairwise, zero_first
        self.ret = np.zeros(n, np.float64)
        self.rms = np.array([0.0, 1.0, 1e-4], np.float64)
        self.episode = np.zeros((3, n), np.float64)
        self.slot = np.zeros(2, np.int32)

    def __call__(self, dot, env_reward, done, bad=None):
        """-> reward (N,1) f32, masks (N,1) f32, bad_masks (N,1) f32, orig_reward (N) f64."""
        n, f = self.n, np.float64
        done = np.asarray(done).astype(bool)
        rews = np.array([(f(dot[i]) if dot is not None else f(0.0)) + f(env_reward[i]) for i in range(n)], np.float64)
        if self.zero_first:
            self.ret[done] = 0.0
        ret = np.array([self.ret[i] * self.gamma + rews[i] for i in range(n)], np.float64)
        out = rews.copy()
        if self.normalise:
            cnt = f(n)
            bmean = numpy_order_sum(ret, n, None, self.pairwise) / cnt
            bvar = numpy_order_sum(ret, n, bmean, self.pairwise) / cnt
            mean, var, count = self.rms
            delta = bmean - mean
            total = count + cnt
            m2 = (var * count + bvar * cnt) + (((delta * delta) * count) * cnt) / total
            self.rms[:] = (mean + (delta * cnt) / total, m2 / total, total)
            den = np.sqrt(self.rms[1] + self.epsilon)
            for i in range(n):
                o = rews[i] / den
                out[i] = -self.cliprew if o < -self.cliprew else (self.cliprew if o > self.cliprew else o)
        self.slot[1] = self.slot[0]
        self.slot[0] = (self.slot[0] + 1) % self.num_steps
        if not self.zero_first:
            ret[done] = 0.0
        self.ret = ret
        run = self.episode[0] + rews
        self.episode[1][done] = run[done]
        self.episode[2][done] += 1.0
        run[done] = 0.0
        self.episode[0] = run
        masks = np.where(done, 0.0, 1.0).astype(np.float32).reshape(n, 1)
        bm = np.ones((n, 1), np.float32) if bad is None else np.where(np.asarray(bad).astype(bool), 0.0, 1.0).astype(np.float32).reshape(n, 1)
        return out.astype(np.float32).reshape(n, 1), masks, bm, rews, out


def sequence(n, seed=SEED, steps=STEPS):
    """Seeded inputs of `steps` env steps: dot (steps, n) f32, env_reward (steps, n) f64, done (steps, n) bool drawn at p = 0.1
    with one all-done step, bad (steps, n) bool at p = 0.05."""
    rng = np.random.default_rng(1000 * seed + n)
    dot = rng.uniform(-1.0, 1.0, size=(steps, n)).astype(np.float32)
    env = rng.normal(0.0, 2.0, size=(steps, n)) * (rng.random((steps, n)) < 0.5)
    done = rng.random((steps, n)) < 0.1
    done[ALL_DONE_STEP % steps] = True
    bad = rng.random((steps, n)) < 0.05
    return dot, env, done, bad


def run_restatement(n, seq, **kw):
    """All outputs of the restatement over a sequence, stacked per step (rms: the running moments after every step), and
    the final episode block and slot words."""
    dot, env, done, bad = seq
    st = NormStep(n, **kw)
    out32, out64, rets, rms = [], [], [], []
    for t in range(dot.shape[0]):
        r32, _, _, _, o64 = st(dot[t], env[t], done[t], bad[t])
        out32.append(r32)
        out64.append(o64)
        rets.append(st.ret.copy())
        rms.append(st.rms.copy())
    return {"reward": np.stack(out32), "out64": np.stack(out64), "ret": np.stack(rets), "rms": np.stack(rms),
            "episode": st.episode.copy(), "slot": st.slot.copy()}


def run_host_normalizer(var_amd, n, seq, **kw):
    """The same sequence through var_amd.ReturnNormalizer (rews = float64(dot) + env_reward, calcReward's sum)."""
    dot, env, done, _ = seq
    norm = var_amd.ReturnNormalizer(n, **kw)
    out64, rets, rms = [], [], []
    for t in range(dot.shape[0]):
        out64.append(norm(dot[t].astype(np.float64) + env[t], done[t]))
        rets.append(norm.ret.copy())
        rms.append([norm.ret_rms.mean, norm.ret_rms.var, norm.ret_rms.count])
    return {"out64": np.stack(out64), "ret": np.stack(rets), "rms": np.array(rms, np.float64)}
