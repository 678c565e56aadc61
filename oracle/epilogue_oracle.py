"""fp64 restatement of the step-epilogue formulas (TEST INFRASTRUCTURE — oracle).

Plain numpy float64 functions of what include/isg.h documents for isg_sum_replicas,
isg_bn_finalize, isg_grad_finalize, isg_bn_update_running and one Adam step
(isg_adam / isg_adam_dev / isg_step_tail). Nothing here imports the product package; the
formulas are pinned to torch itself (BatchNorm2d autograd and torch.optim.Adam in float64)
by tests/test_epilogue_oracle_cpu.py.

Statistics of one BatchNorm layer over M = N*H*W values per channel (isg.h isg_bn):
  sum   = sum y            sumsq = sum y^2           (y: the raw conv output, bias included)
  gsum  = sum g            gxsum = sum g*(y - mean)  (g: gradient w.r.t. the BN output)
Every function takes and returns float64 arrays; callers holding float32 values (gamma,
running statistics, eps) pass them converted, which is exact.
"""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def replica_sum(rep):
    """Sum over axis 0 (the replicas) in replica order: rep[0] + rep[1] + ... in float64."""
    rep = _f64(rep)
    acc = rep[0].copy()
    for r in range(1, rep.shape[0]):
        acc = acc + rep[r]
    return acc


def raw_stats(y, g):
    """(sum, sumsq, gsum, gxsum, M) per channel of y, g: [N, C, H, W] — the four statistics
    as the kernels accumulate them, gxsum centred on the batch mean."""
    y, g = _f64(y), _f64(g)
    M = y.shape[0] * y.shape[2] * y.shape[3]
    s = y.sum((0, 2, 3))
    mean = s / M
    return (s, (y * y).sum((0, 2, 3)), g.sum((0, 2, 3)),
            (g * (y - mean[None, :, None, None])).sum((0, 2, 3)), M)


def batch_mean_var(s, sumsq, M):
    """Batch mean and BIASED variance (clamped at 0: sumsq/M - mean^2 can round below)."""
    s, sumsq = _f64(s), _f64(sumsq)
    mean = s / M
    var = np.maximum(sumsq / M - mean * mean, 0.0)
    return mean, var


def rstd_of(var, eps):
    return 1.0 / np.sqrt(_f64(var) + float(eps))


def bn_fwd_coef(mean, rstd, gamma, beta):
    """[C, 4] = (mean, gamma*rstd, beta, 0) of BN(y) = (y - mean)*gamma*rstd + beta."""
    mean, rstd, gamma, beta = map(_f64, (mean, rstd, gamma, beta))
    return np.stack([mean, gamma * rstd, beta, np.zeros_like(mean)], 1)


def bn_bwd_coef(mean, rstd, gamma, gsum, gxsum, M, train=True):
    """[C, 4] = (A, B, mean, C) of dy = A*g + B*(y - mean) + C, the BatchNorm2d input
    gradient. Train: A = gamma*rstd, B = -gamma*rstd^2*mean(g*xhat), C = -gamma*rstd*mean(g)
    with mean(g*xhat) = rstd*gxsum/M. Eval (running statistics are constants): B = C = 0."""
    mean, rstd, gamma, gsum, gxsum = map(_f64, (mean, rstd, gamma, gsum, gxsum))
    A = gamma * rstd
    if not train:
        z = np.zeros_like(A)
        return np.stack([A, z, mean, z], 1)
    mg = gsum / M
    mgx = rstd * gxsum / M
    return np.stack([A, -gamma * rstd * rstd * mgx, mean, -gamma * rstd * mg], 1)


def dgamma_dbeta(rstd, gsum, gxsum):
    return _f64(rstd) * _f64(gxsum), _f64(gsum).copy()


def dconv_bias_eval(gamma, rstd, gsum):
    """Gradient of a conv bias ahead of an eval-mode BN: sum of dy = gamma*rstd*g."""
    return _f64(gamma) * _f64(rstd) * _f64(gsum)


def dconv_bias_train(gamma, rstd, s, gsum, gxsum, M):
    """Gradient of a conv bias ahead of a train-mode BN. Mathematically ZERO (the batch
    mean removes the bias); what is returned is the documented expression
      gamma*rstd*(gsum - M*(gsum/M)) - gamma*rstd^2*(rstd*gxsum/M)*(sum - M*mean)
    evaluated in float64 without contraction — its rounding residue — and a bound on the
    residue of ANY float64 evaluation of it (contracted or not): each bracket is two
    roundings of a value of the bracket's first term's size, times 2 of margin:
      8 * 2^-53 * (|gamma*rstd*gsum| + |gamma*rstd^2*(rstd*gxsum/M)*sum|)."""
    gamma, rstd, s, gsum, gxsum = map(_f64, (gamma, rstd, s, gsum, gxsum))
    mean = s / M
    mg = gsum / M
    mgx = rstd * gxsum / M
    db = gamma * rstd * (gsum - M * mg) - gamma * rstd * rstd * mgx * (s - M * mean)
    bound = 8.0 * 2.0 ** -53 * (np.abs(gamma * rstd * gsum) + np.abs(gamma * rstd * rstd * mgx * s))
    return db, bound


def running_update(rm, rv, nbt, mean, var, M, momentum):
    """torch BatchNorm2d train semantics: rm' = (1-m) rm + m mean;
    rv' = (1-m) rv + m var*M/(M-1) (var biased; left unscaled when M == 1); nbt' = nbt + 1."""
    rm, rv, mean, var = map(_f64, (rm, rv, mean, var))
    m = float(momentum)
    unb = var * M / (M - 1.0) if M > 1 else var
    return (1.0 - m) * rm + m * mean, (1.0 - m) * rv + m * unb, int(nbt) + 1


def adam_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """One torch.optim.Adam step (1-based `step`, L2 weight decay added to the gradient):
    returns (p', m', v')."""
    p, g, m, v = map(_f64, (p, g, m, v))
    if weight_decay != 0.0:
        g = g + weight_decay * p
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v
