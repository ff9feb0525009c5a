"""float64 torch restatement of the iKala trainer (test infrastructure): build_ca of examples/ikala/trainCNN.py:66-118 with
explicit transposed convolutions (so that autograd reaches the weights through the InverseLayers), the loss of :155-189 with
Theano's gradient conventions -- rectify = 0.5 (x + |x|) so r'(0) = 0.5, abs'(0) = 0 -- and lasagne.updates.adadelta."""
import numpy as np
import torch
import torch.nn.functional as Fnn

from train_ref import _t, adadelta, autograd, rectify  # noqa: F401  (adadelta is shared with the DSD restatement)

EPS, ALPHA, BETA_ACC, BETA_VOC = 1e-8, 0.9, 0.005, 0.02


def forward(P, x):
    """p = rectify(concat(InverseLayer(conv1, InverseLayer(conv2, fc_k(z)))) + bo), [B, 2, tc, F].  conv1^T leaves the
    last (F - 30) % 3 columns without a tap: they are padded with zeros (the VJP of a valid strided convolution)."""
    W1, b1, b1b, W2, b2, b2b, Wfc, bfc = P[:8]
    W1c, W2c = torch.flip(W1, dims=(2, 3)), torch.flip(W2, dims=(2, 3))
    a1b = Fnn.conv2d(x, W1c, stride=(1, 3)) + b1.view(1, -1, 1, 1) + b1b.view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1b, W2c) + b2.view(1, -1, 1, 1)
    a2b = a2 + b2b.view(1, -1, 1, 1)
    B, F = x.shape[0], x.shape[3]
    z = rectify(a2b.reshape(B, -1) @ Wfc + bfc)
    ys = []
    for k in range(2):
        d = rectify(z @ P[8 + 2 * k] + P[9 + 2 * k]).reshape(a2.shape)
        g = Fnn.conv_transpose2d(d, W2c)
        y = Fnn.conv_transpose2d(g, W1c, stride=(1, 3))
        ys.append(Fnn.pad(y, (0, F - y.shape[3])))
    return rectify(torch.cat(ys, dim=1) + P[12].view(1, -1, 1, 1))


def components(p, x, tgt, r, eps=EPS, alpha=ALPHA, beta_acc=BETA_ACC, beta_voc=BETA_VOC):
    """ikala/trainCNN.py:170-189: (loss, vocals_error, acc_error, negative_error_voc, negative_error_acc)."""
    voc = p[:, 0:1] + eps * r
    acco = p[:, 1:2] + eps * r
    mask1 = voc / (voc + acco)
    mask2 = acco / (voc + acco)
    vocals = mask1 * x
    acc = mask2 * x
    vocals_error = ((vocals - tgt[:, 0:1]) ** 2).sum()
    acc_error = (alpha * (acc - tgt[:, 1:2]) ** 2).sum()
    negative_error_voc = (beta_voc * (vocals - tgt[:, 1:2]) ** 2).sum()
    negative_error_acc = (beta_acc * (acc - tgt[:, 0:1]) ** 2).sum()
    loss = torch.abs(vocals_error + acc_error - negative_error_voc)
    return [loss, vocals_error, acc_error, negative_error_voc, negative_error_acc]


def loss_and_grads(params, x, tgt, r, **kw):
    """float64: the five values of ``components`` and the 13 gradients of the loss (ndarrays).  Keywords: eps, alpha, beta_acc, beta_voc (ikala/trainCNN.py:152-155)
    and those of ``train_ref.autograd`` (tie, dtype, device)."""
    return autograd(forward, components, params, x, tgt, r, **kw)


def forward_np(params, x):
    with torch.no_grad():
        return forward([_t(p) for p in params], _t(x)).numpy()
