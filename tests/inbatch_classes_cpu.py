"""CPU restatement of the class-aware in-batch head (csrc/inbatch.hip: var_inbatch_loss_fwd_bwd_ex) in float64 through torch
autograd, its seeded inputs and the yardstick of tests/test_gpu_inbatch_classes.py, by the convention of tests/step_tail_cpu.py
for the label-blind head: per output (loss, ga, gc), D is the largest over SEEDS draws of max |torch fp32 - float64| /
scale(float64) of the SAME restatement at the same case, and the GPU has to stay within 4 D.

With l_ij = -d_ij / tau, d_ij = pairwise_distance(a_i, c_j, eps = PD_EPS), t(i) = target[i], y_i = anchor class, z_j = candidate
class, the loss is inv_count * sum_i L_i:
    ALL             L_i = logsumexp_j l_ij - l_{i,t(i)}
    OTHER_CLASS     L_i = logsumexp_{j in N_i} l_ij - l_{i,t(i)},             N_i = { j : z_j != y_i } + { t(i) }
                    (the logits outside N_i are set to -inf)
    MULTI_POSITIVE  L_i = logsumexp_j l_ij - (1/|P_i|) sum_{p in P_i} l_ip,   P_i = { j : z_j = y_i } + { t(i) }

Inputs: step_tail_cpu.inbatch_inputs(B, M, seed) gives a, cand, t; then z = rng.integers(0, 5, M) from
default_rng(CLASS_SEED + seed) -- five classes, as taskNum + 1 of the data -- and y = z[t].  A yardstick case asserts
min_i |N_i| >= MIN_NEGATIVES: a row left alone with its positive is the case fp32 log-softmax cannot resolve
(inbatch_inputs' docstring), and a yardstick measured there would pin nothing."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests.step_tail_cpu import PD_EPS, SEEDS, _head_distance, f32, inbatch_inputs

ALL, OTHER_CLASS, MULTI_POSITIVE = 0, 1, 2          # VAR_INBATCH_* of include/var_hip.h
MODES = {"all": ALL, "other_class": OTHER_CLASS, "multi_positive": MULTI_POSITIVE}
N_CLASSES = 5
CLASS_SEED = 90000
MIN_NEGATIVES = 8
FAULTS = ("mask_dropped", "positives_off_by_one", "target_masked")


def class_inputs(B, M, seed):
    """(a, cand, t, y, z): inbatch_inputs plus int32 candidate classes z in [0, 5) and anchor classes y = z[t]."""
    a, cand, t = inbatch_inputs(B, M, seed)
    z = np.random.default_rng(CLASS_SEED + seed).integers(0, N_CLASSES, M).astype(np.int32)
    return a, cand, t, z[t].copy(), z


def negatives_mask(t, y, z):
    """(B, M) bool: j in N_i."""
    m = z[None, :] != y[:, None]
    m[np.arange(len(t)), t] = True
    return m


def positives_mask(t, y, z):
    """(B, M) bool: j in P_i."""
    m = z[None, :] == y[:, None]
    m[np.arange(len(t)), t] = True
    return m


def classes_loss(ta, tc, t, y, z, tau, inv_count, mode, fault=None):
    """The loss of the three modes as a torch scalar of (ta (B,3), tc (M,3)); t, y, z numpy.  fault: one of FAULTS, a wrong
    restatement for tests/test_inbatch_classes_host.py to tell from the right one."""
    assert fault is None or fault in FAULTS
    t, y, z = (np.asarray(x) for x in (t, y, z))
    tt = torch.from_numpy(t).long()
    l = -F.pairwise_distance(ta[:, None, :], tc[None, :, :], p=2, eps=PD_EPS) / tau
    l_pos = l.gather(1, tt[:, None])[:, 0]
    if mode == ALL:
        rows = torch.logsumexp(l, 1) - l_pos
    elif mode == OTHER_CLASS:
        keep = negatives_mask(t, y, z)
        if fault == "mask_dropped":
            keep[:] = True
        if fault == "target_masked":
            keep = z[None, :] != y[:, None]
        masked = torch.where(torch.from_numpy(keep), l, torch.full_like(l, -float("inf")))
        rows = torch.logsumexp(masked, 1) - l_pos
    else:
        assert mode == MULTI_POSITIVE
        pos = torch.from_numpy(positives_mask(t, y, z))
        n_pos = pos.sum(1).to(l.dtype) + (1 if fault == "positives_off_by_one" else 0)
        rows = torch.logsumexp(l, 1) - torch.where(pos, l, torch.zeros_like(l)).sum(1) / n_pos
    return rows.sum() * inv_count


def classes_torch(a, cand, t, y, z, tau, inv_count, mode, dtype, fault=None):
    """classes_loss through torch autograd on the CPU in `dtype`: {'loss', 'ga', 'gc'} (numpy)."""
    ta, tc = (torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_() for x in (a, cand))
    loss = classes_loss(ta, tc, t, y, z, tau, inv_count, mode, fault)
    loss.backward()
    return {"loss": loss.detach().numpy().reshape(1), "ga": ta.grad.numpy(), "gc": tc.grad.numpy()}


def classes64(a, cand, t, y, z, tau, inv_count, mode, fault=None):
    return classes_torch(a, cand, t, y, z, tau, inv_count, mode, torch.float64, fault)


def loops64(a, cand, t, y, z, tau, inv_count, mode):
    """The same losses and gradients with plain double loops and the closed-form gradient (include/var_hip.h): for small shapes."""
    a, cand = np.asarray(a, np.float64), np.asarray(cand, np.float64)
    B, M = a.shape[0], cand.shape[0]
    ga, gc, loss = np.zeros((B, 3)), np.zeros((M, 3)), 0.0
    for i in range(B):
        u = [a[i] - cand[j] + PD_EPS for j in range(M)]
        d = [float(np.sqrt((u[j] ** 2).sum())) for j in range(M)]
        l = [-d[j] / tau for j in range(M)]
        in_n = [mode != OTHER_CLASS or z[j] != y[i] or j == t[i] for j in range(M)]
        in_p = [(z[j] == y[i] or j == t[i]) if mode == MULTI_POSITIVE else j == t[i] for j in range(M)]
        n_p = sum(in_p)
        mx = max(l[j] for j in range(M) if in_n[j])
        lse = mx + np.log(sum(np.exp(l[j] - mx) for j in range(M) if in_n[j]))
        loss += lse - sum(l[j] for j in range(M) if in_p[j]) / n_p
        for j in range(M):
            s = (np.exp(l[j] - lse) if in_n[j] else 0.0) - (1.0 / n_p if in_p[j] else 0.0)
            g = -s / tau * inv_count / max(d[j], 1e-12) * u[j]                 # dL/da_i through d_ij
            ga[i] += g
            gc[j] -= g
    return {"loss": np.array([loss * inv_count]), "ga": ga, "gc": gc}


def min_negatives(t, y, z):
    return int(negatives_mask(t, y, z).sum(1).min())


@functools.lru_cache(maxsize=None)
def classes_distance(B, M, tau, inv_count, mode):
    """Per output, the largest over SEEDS draws of max |torch fp32 - float64| / max |float64| of classes_torch at this case."""
    worst = {}
    for s in range(SEEDS):
        a, cand, t, y, z = class_inputs(B, M, 7000 + s)
        assert min_negatives(t, y, z) >= MIN_NEGATIVES, (B, M, s)
        for k, x in _head_distance(classes64(a, cand, t, y, z, f32(tau), f32(inv_count), mode),
                                   classes_torch(a, cand, t, y, z, f32(tau), f32(inv_count), mode, torch.float32)).items():
            worst[k] = max(worst.get(k, 0.0), x)
    return worst
