"""float64 torch restatement of the Bach10 trainer (test infrastructure): build_ca of examples/bach10/trainCNNbach10.py:66-123
with explicit transposed convolutions (so that autograd reaches the weights through the InverseLayers), the loss of :160-198
with Theano's gradient conventions -- rectify = 0.5 (x + |x|) so r'(0) = 0.5, abs'(0) = 0 -- and lasagne.updates.adadelta."""
import numpy as np
import torch
import torch.nn.functional as Fnn

from train_ref import _t, adadelta, autograd, rectify  # noqa: F401  (adadelta is shared with the DSD restatement)

EPS = 1e-18


def forward(P, x):
    """p = rectify(concat(InverseLayer(conv1, InverseLayer(conv2, fc_k(z)))) + bo), [B, 4, tc, F].  conv1^T leaves the
    last (F - 30) % 4 columns without a tap: they are padded with zeros (the VJP of a valid strided convolution)."""
    W1, b1, b1b, W2, b2, b2b, Wfc, bfc = P[:8]
    W1c, W2c = torch.flip(W1, dims=(2, 3)), torch.flip(W2, dims=(2, 3))
    a1b = Fnn.conv2d(x, W1c, stride=(1, 4)) + b1.view(1, -1, 1, 1) + b1b.view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1b, W2c) + b2.view(1, -1, 1, 1)
    a2b = a2 + b2b.view(1, -1, 1, 1)
    B, F = x.shape[0], x.shape[3]
    z = rectify(a2b.reshape(B, -1) @ Wfc + bfc)
    ys = []
    for k in range(4):
        d = rectify(z @ P[8 + 2 * k] + P[9 + 2 * k]).reshape(a2.shape)
        g = Fnn.conv_transpose2d(d, W2c)
        y = Fnn.conv_transpose2d(g, W1c, stride=(1, 4))
        ys.append(Fnn.pad(y, (0, F - y.shape[3])))
    return rectify(torch.cat(ys, dim=1) + P[16].view(1, -1, 1, 1))


def components(p, x, tgt, r, eps=EPS):
    """bach10/trainCNNbach10.py:173-198: (loss, error1, error2, error3, error4).  eps * r is in the denominator only."""
    den = p[:, 0:1] + p[:, 1:2] + p[:, 2:3] + p[:, 3:4] + eps * r
    errors = [(((p[:, k:k + 1] / den) * x - tgt[:, k:k + 1]) ** 2).sum() for k in range(4)]
    loss = torch.abs(errors[0] + errors[1] + errors[2] + errors[3])
    return [loss] + errors


def loss_and_grads(params, x, tgt, r, **kw):
    """float64: the five values of ``components`` and the 17 gradients of the loss (ndarrays).  Keywords: eps (bach10/trainCNNbach10.py:160)
    and those of ``train_ref.autograd`` (tie, dtype, device)."""
    return autograd(forward, components, params, x, tgt, r, **kw)


def forward_np(params, x):
    with torch.no_grad():
        return forward([_t(p) for p in params], _t(x)).numpy()
