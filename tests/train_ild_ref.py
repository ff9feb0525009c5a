"""float64 torch restatement of the stereo (ILD) DSD100 trainer (test infrastructure): build_ca of
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:66-113 with explicit transposed convolutions (so that autograd reaches the
weights through the InverseLayers), the stage-1 loss of :183-198 and the ILD term of :210-228 with Theano's gradient
conventions -- rectify = 0.5 (x + |x|) so r'(0) = 0.5, abs'(0) = 0 -- and lasagne.updates.adadelta."""
import numpy as np
import torch
import torch.nn.functional as Fnn

from train_ref import _t, adadelta, autograd, rectify  # noqa: F401  (adadelta is shared with the DSD restatement)

EPS, ILD_WEIGHT = 1e-12, 1.0 / 500.0
NCH, NSRC = 2, 4


def forward(P, x):
    """p = rectify(concat_s(InverseLayer(conv1, InverseLayer(conv2, fc_s(z)))) + bo), [B, 8, tc, F]: channel 2 s + c is
    source s in input channel c (:106-111)."""
    W1, b1, b1b, W2, b2, b2b, Wfc, bfc = P[:8]
    W1c, W2c = torch.flip(W1, dims=(2, 3)), torch.flip(W2, dims=(2, 3))
    a1b = Fnn.conv2d(x, W1c) + b1.view(1, -1, 1, 1) + b1b.view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1b, W2c) + b2.view(1, -1, 1, 1)
    a2b = a2 + b2b.view(1, -1, 1, 1)
    B = x.shape[0]
    z = rectify(a2b.reshape(B, -1) @ Wfc + bfc)
    ys = []
    for k in range(NSRC):
        d = rectify(z @ P[8 + 2 * k] + P[9 + 2 * k]).reshape(a2.shape)
        g = Fnn.conv_transpose2d(d, W2c)
        ys.append(Fnn.conv_transpose2d(g, W1c))
    return rectify(torch.cat(ys, dim=1) + P[16].view(1, -1, 1, 1))


def components(p, x, tgt, r, eps=EPS, ild_weight=ILD_WEIGHT, stage=1):
    """(loss, errors_insts of mic 0's four sources, of mic 1's, the weighted ILD term): :183-198, and for ``stage`` 2
    :210-228.  ``r`` is ``[2, B, 4, tc, F]``: rand_num, rand_num2.  In stage 1 the last value is 0."""
    r1, r2 = r[0], r[1]
    loss = 0
    sources, errors = [], []
    for j in range(NCH):
        pj = p[:, j::NCH]
        den = pj.sum(dim=1, keepdim=True) + eps * r1
        source = pj / den * x[:, j:j + 1] + eps * r1
        sources.append(source)
        se = (source - tgt[:, j::NCH]) ** 2
        errors += list(torch.abs(se.sum(dim=(0, 2, 3))))
        loss = loss + torch.abs(se.sum())
    ild = torch.zeros((), dtype=p.dtype, device=p.device)
    if stage == 2:
        a_est = 20 * torch.log10(torch.abs(sources[0] / (sources[1] + eps * r2) + eps * r2))
        a_gt = 20 * torch.log10(torch.abs(tgt[:, 0::NCH] / (tgt[:, 1::NCH] + eps * r2) + eps * r2))
        d = a_est.mean(dim=(0, 1, 2)) - a_gt.mean(dim=(0, 1, 2))
        ild = ild_weight * torch.abs((d ** 2).sum())
        loss = loss + ild
    return [loss] + errors + [ild]


def loss_and_grads(params, x, tgt, r, **kw):
    """float64: the ten values of ``components`` and the 17 gradients of the loss (ndarrays).  Keywords: eps, ild_weight,
    stage and those of ``train_ref.autograd`` (tie, dtype, device)."""
    return autograd(forward, components, params, x, tgt, r, **kw)


def components_np(p, x, tgt, r, **kw):
    with torch.no_grad():
        return np.array([float(v) for v in components(_t(p), _t(x), _t(tgt), _t(r), **kw)])


def forward_np(params, x):
    with torch.no_grad():
        return forward([_t(p) for p in params], _t(x)).numpy()
