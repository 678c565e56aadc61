"""Pin oracle/epilogue_oracle.py to torch itself in float64 (CPU only): the BatchNorm
formulas against torch.nn.BatchNorm2d driven by autograd through `conv bias -> BN`, the Adam
step against torch.optim.Adam.

Bar: 1e-12 relative — both sides are float64 evaluations of the same formulas (unit
roundoff 1.1e-16; the sums run over a few hundred values). Per-channel quantities are held
element by element; the input gradient, whose elements are themselves differences of
terms of the tensor's size, relative to the channel's largest element.
"""
import numpy as np
import pytest
import torch

from oracle import epilogue_oracle as E

RTOL = 1e-12
EPS = 1e-5


def _close(got, ref, what, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = RTOL * (np.abs(ref) if scale is None else scale)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{what}: worst |err| / bar = {worst:.3g}")
    assert (err <= tol).all(), (what, worst)


def _case(train, momentum=0.1, seed=5):
    """y = y0 + conv_bias, BN(y), loss = sum(out * g): autograd's gradients and the updated
    running statistics, with the tensors the oracle needs."""
    gen = torch.Generator().manual_seed(seed)
    N, C, H, W = 3, 5, 7, 6
    y0 = torch.randn(N, C, H, W, dtype=torch.float64, generator=gen) * 1.7 + \
        torch.linspace(-2.0, 3.0, C, dtype=torch.float64)[None, :, None, None]
    g = torch.randn(N, C, H, W, dtype=torch.float64, generator=gen) + 0.3
    bias = torch.randn(C, dtype=torch.float64, generator=gen).requires_grad_()
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, dtype=torch.float64, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(C, dtype=torch.float64, generator=gen))
        bn.running_mean.copy_(torch.randn(C, dtype=torch.float64, generator=gen))
        bn.running_var.copy_(torch.rand(C, dtype=torch.float64, generator=gen) + 0.5)
    bn.train(train)
    old = (bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(),
           int(bn.num_batches_tracked))
    y = y0 + bias[None, :, None, None]
    y.retain_grad()
    out = bn(y)
    (out * g).sum().backward()
    return bn, y, g.numpy(), bias, out, old


@pytest.mark.parametrize("momentum", [0.1, 0.25])
def test_train_formulas_match_batchnorm2d_autograd(momentum):
    bn, y, g, bias, out, (rm0, rv0, nbt0) = _case(True, momentum)
    yv = y.detach().numpy()
    s, sq, gs, gxs, M = E.raw_stats(yv, g)
    mean, var = E.batch_mean_var(s, sq, M)
    rstd = E.rstd_of(var, EPS)
    gamma, beta = bn.weight.detach().numpy(), bn.bias.detach().numpy()

    rm, rv, nbt = E.running_update(rm0, rv0, nbt0, mean, var, M, momentum)
    _close(rm, bn.running_mean.numpy(), "running_mean")
    _close(rv, bn.running_var.numpy(), "running_var")
    assert nbt == int(bn.num_batches_tracked) == nbt0 + 1

    f = E.bn_fwd_coef(mean, rstd, gamma, beta)
    assert (f[:, 3] == 0).all()
    fwd = (yv - f[None, :, 0, None, None]) * f[None, :, 1, None, None] + f[None, :, 2, None, None]
    ref = out.detach().numpy()
    _close(fwd, ref, "BN forward from (mean, gamma*rstd, beta)",
           scale=np.abs(ref).max((0, 2, 3))[None, :, None, None])

    dgamma, dbeta = E.dgamma_dbeta(rstd, gs, gxs)
    _close(dgamma, bn.weight.grad.numpy(), "dgamma")
    _close(dbeta, bn.bias.grad.numpy(), "dbeta")

    k = E.bn_bwd_coef(mean, rstd, gamma, gs, gxs, M)
    dy = (k[None, :, 0, None, None] * g + k[None, :, 1, None, None]
          * (yv - k[None, :, 2, None, None]) + k[None, :, 3, None, None])
    ref = y.grad.numpy()
    _close(dy, ref, "input gradient A*g + B*(y-mean) + C",
           scale=np.abs(ref).max((0, 2, 3))[None, :, None, None])

    # the conv-bias gradient ahead of a train-mode BN is zero up to rounding, in torch's
    # evaluation and in the documented expression alike
    db, bound = E.dconv_bias_train(gamma, rstd, s, gs, gxs, M)
    assert (np.abs(db) <= bound).all()
    assert (np.abs(bias.grad.numpy()) <= 1e-12 * np.abs(ref).sum((0, 2, 3))).all()


def test_eval_formulas_match_batchnorm2d_autograd():
    bn, y, g, bias, out, (rm0, rv0, nbt0) = _case(False)
    yv = y.detach().numpy()
    s, sq, gs, _, M = E.raw_stats(yv, g)
    gxs = (g * (yv - rm0[None, :, None, None])).sum((0, 2, 3))  # centred on the running mean
    rstd = E.rstd_of(rv0, EPS)
    gamma = bn.weight.detach().numpy()
    np.testing.assert_array_equal(bn.running_mean.numpy(), rm0)  # eval: no update
    assert int(bn.num_batches_tracked) == nbt0

    _close(E.dconv_bias_eval(gamma, rstd, gs), bias.grad.numpy(), "eval dconv_bias")
    dgamma, dbeta = E.dgamma_dbeta(rstd, gs, gxs)
    _close(dgamma, bn.weight.grad.numpy(), "eval dgamma")
    _close(dbeta, bn.bias.grad.numpy(), "eval dbeta")
    k = E.bn_bwd_coef(rm0, rstd, gamma, gs, gxs, M, train=False)
    assert (k[:, 1] == 0).all() and (k[:, 3] == 0).all()
    _close(k[None, :, 0, None, None] * g, y.grad.numpy(), "eval input gradient A*g")


def test_replica_sum_is_in_replica_order():
    rep = np.array([[1.0, 2.0 ** 60], [2.0 ** -60, -2.0 ** 60], [1.0, 1.0]])
    # ((1 + 2^-60) + 1) = 2 and ((2^60 - 2^60) + 1) = 1; another order gives other bits
    np.testing.assert_array_equal(E.replica_sum(rep), [2.0, 1.0])
    np.testing.assert_array_equal(E.replica_sum(rep[::-1]), [2.0, 0.0])


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["nowd", "wd"])
def test_adam_step_matches_torch_adam(wd):
    gen = torch.Generator().manual_seed(11)
    p = torch.randn(97, dtype=torch.float64, generator=gen).requires_grad_()
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    po = p.detach().numpy().copy()
    mo, vo = np.zeros_like(po), np.zeros_like(po)
    for step in (1, 2):
        g = torch.randn(97, dtype=torch.float64, generator=gen) * 10.0 ** float(step - 2)
        p.grad = g.clone()
        opt.step()
        po, mo, vo = E.adam_step(po, g.numpy(), mo, vo, step, 1e-3, 0.9, 0.999, 1e-8, wd)
        st = opt.state[p]
        _close(po, p.detach().numpy(), f"adam step {step} param")
        _close(mo, st["exp_avg"].numpy(), f"adam step {step} exp_avg")
        _close(vo, st["exp_avg_sq"].numpy(), f"adam step {step} exp_avg_sq")
