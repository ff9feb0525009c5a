"""float64 torch restatement of the score-informed Bach10 trainer (test infrastructure): build_ca of
examples/bach10_scoreinformed/trainCNNrwc.py:134-193 (17 arrays) and its single-branch form trainCNNrwc_samp.py:195-235 (11
arrays) with explicit transposed convolutions, as tests/train_bach10_ref.py restates the Bach10 graph; the loss of
trainCNNrwc.py:246-275 with Theano's gradient conventions -- rectify = 0.5 (x + |x|) so r'(0) = 0.5, abs'(0) = 0 -- and
lasagne.updates.adadelta.  The layout is told from the number of arrays."""
import numpy as np
import torch
import torch.nn.functional as Fnn

from train_ref import _t, adadelta, autograd, rectify  # noqa: F401

EPS = 1e-18
DEAD = (10, 11, 12, 13, 14, 15)      # fc12, fc13, fc14 of the 17-array layout; and bo[4:16]


def forward(P, x):
    """p = rectify(concat_k(InverseLayer(conv1, InverseLayer(conv2, fc_1k(z)))) + bo): [B, 16, tc, F] for 17 arrays, [B, 4, tc,
    F] for 11.  conv1 has four input channels, so each branch's InverseLayer of conv1 gives four channels."""
    W1, b1, b1b, W2, b2, b2b, Wfc, bfc = P[:8]
    nb = (len(P) - 9) // 2
    W1c, W2c = torch.flip(W1, dims=(2, 3)), torch.flip(W2, dims=(2, 3))
    a1b = Fnn.conv2d(x, W1c, stride=(1, 4)) + b1.view(1, -1, 1, 1) + b1b.view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1b, W2c) + b2.view(1, -1, 1, 1)
    a2b = a2 + b2b.view(1, -1, 1, 1)
    B, F = x.shape[0], x.shape[3]
    z = rectify(a2b.reshape(B, -1) @ Wfc + bfc)
    ys = []
    for k in range(nb):
        d = rectify(z @ P[8 + 2 * k] + P[9 + 2 * k]).reshape(a2.shape)
        g = Fnn.conv_transpose2d(d, W2c)
        y = Fnn.conv_transpose2d(g, W1c, stride=(1, 4))
        ys.append(Fnn.pad(y, (0, F - y.shape[3])))
    return rectify(torch.cat(ys, dim=1) + P[8 + 2 * nb].view(1, -1, 1, 1))


def components(p, x, tgt, r, eps=EPS):
    """trainCNNrwc.py:248-275: (loss, error1, error2, error3, error4) from prediction2[:, 0:4] and the sum of the four input
    channels.  eps * r is in the denominator only."""
    den = p[:, 0:1] + p[:, 1:2] + p[:, 2:3] + p[:, 3:4] + eps * r
    mix = x[:, 0:1] + x[:, 1:2] + x[:, 2:3] + x[:, 3:4]
    errors = [(((p[:, k:k + 1] / den) * mix - tgt[:, k:k + 1]) ** 2).sum() for k in range(4)]
    loss = torch.abs(errors[0] + errors[1] + errors[2] + errors[3])
    return [loss] + errors


def loss_and_grads(params, x, tgt, r, **kw):
    """float64: the five values of ``components`` and the gradients of the loss, one per array (ndarrays).  Keywords: eps and
    those of ``train_ref.autograd`` (tie, dtype, device)."""
    return autograd(forward, components, params, x, tgt, r, **kw)


def live(params):
    """The 11 live arrays of a 17-array list (``arch.live_params``): arrays 0 .. 9 and bo[0:4]."""
    return list(params[:10]) + [np.asarray(params[16])[:4]]


def forward_np(params, x):
    with torch.no_grad():
        return forward([_t(p) for p in params], _t(x)).numpy()
