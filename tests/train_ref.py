"""float64 torch restatement of the DSD trainer (test infrastructure): build_ca of examples/dsd100/trainCNN.py:66-130 with
explicit transposed convolutions (so that autograd reaches the weights through the InverseLayers), the loss of :167-219 with
Theano's gradient conventions -- rectify = 0.5 (x + |x|) so r'(0) = 0.5, abs'(0) = 0 -- and lasagne.updates.adadelta.

``relu_tie(d)`` is a switch for the controls of tests/test_train_edges_cpu.py: inside it rectify's derivative at exactly 0 is
``d`` (0 or 1: the conventions a kernel could carry by mistake) in all three restatements; the values are unchanged."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as Fnn

EPS, ALPHA, BETA, BETA_VOC = 1e-8, 0.001, 0.01, 0.03


_TIE = [0.5]


@contextlib.contextmanager
def relu_tie(d):
    """rectify'(0) = d inside the block (0.5 is Theano's and the trainers')."""
    old, _TIE[0] = _TIE[0], float(d)
    try:
        yield
    finally:
        _TIE[0] = old


def rectify(v):
    y = 0.5 * (v + torch.abs(v))
    if _TIE[0] != 0.5:   # a term that is 0 everywhere and has derivative (d - 0.5) where v == 0
        y = y + (_TIE[0] - 0.5) * torch.where(v == 0, v, torch.zeros_like(v))
    return y


def _t(a, grad=False, dtype=torch.float64, device="cpu"):
    t = torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype=dtype, device=device).clone()
    return t.requires_grad_(grad)


def forward(P, x):
    """p = rectify(concat(InverseLayer(conv1, InverseLayer(conv2, fc_k(z)))) + bo), [B, 4, tc, F]."""
    W1, b1, b1b, W2, b2, b2b, Wfc, bfc = P[:8]
    W1c, W2c = torch.flip(W1, dims=(2, 3)), torch.flip(W2, dims=(2, 3))
    a1b = Fnn.conv2d(x, W1c) + b1.view(1, -1, 1, 1) + b1b.view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1b, W2c) + b2.view(1, -1, 1, 1)
    a2b = a2 + b2b.view(1, -1, 1, 1)
    B = x.shape[0]
    z = rectify(a2b.reshape(B, -1) @ Wfc + bfc)
    ys = []
    for k in range(3):
        d = rectify(z @ P[8 + 2 * k] + P[9 + 2 * k]).reshape(a2.shape)
        g = Fnn.conv_transpose2d(d, W2c)
        ys.append(Fnn.conv_transpose2d(g, W1c))
    y = torch.cat([ys[0], ys[1], ys[2], ys[1]], dim=1) + P[14].view(1, -1, 1, 1)
    return rectify(y)


def components(p, x, tgt, r, eps=EPS, alpha=ALPHA, beta=BETA, beta_voc=BETA_VOC):
    """trainCNN.py:180-217: (loss, vocals, bass, drums, negative, alpha, negative_voc)."""
    s = [p[:, i:i + 1] + eps * r for i in range(4)]
    den = s[0] + s[1] + s[2] + s[3]
    voc, bas, dru = (s[0] / den) * x, (s[1] / den) * x, (s[2] / den) * x
    t = [tgt[:, i:i + 1] for i in range(4)]

    def se(a, b):
        return (a - b) ** 2
    vocals = se(voc, t[0]).sum()
    bass = se(bas, t[1]).sum()
    drums = se(dru, t[2]).sum()
    negative = (beta * se(bas, t[3]) + beta * se(dru, t[3])).sum()
    alpha_c = (alpha * se(voc, t[1]) + alpha * se(voc, t[2]) + alpha * se(bas, t[0]) + alpha * se(bas, t[2])
               + alpha * se(dru, t[0]) + alpha * se(dru, t[1])).sum()
    negative_voc = (beta_voc * se(voc, t[3])).sum()
    loss = torch.abs(vocals + drums + bass - negative - alpha_c - negative_voc)
    return [loss, vocals, bass, drums, negative, alpha_c, negative_voc]


def autograd(forward_fn, components_fn, params, x, tgt, r, tie=0.5, dtype=torch.float64, device="cpu", **hyper):
    """The values of ``components_fn`` and the gradients of the loss, as float64 ndarrays, computed in ``dtype`` on
    ``device`` with rectify'(0) = ``tie``.  float32 gives the restatement's own float32 error (the yardstick of the
    elementwise gradient bound); the values are still summed in float64 from the ``dtype`` squared errors."""
    kw = dict(dtype=dtype, device=device)
    P = [_t(p, True, **kw) for p in params]
    with relu_tie(tie):
        out = components_fn(forward_fn(P, _t(x, **kw)), _t(x, **kw), _t(tgt, **kw), _t(r, **kw), **hyper)
        grads = torch.autograd.grad(out[0], P, allow_unused=True)
    grads = [np.zeros(p.shape) if g is None else g.detach().cpu().numpy().astype(np.float64) for p, g in zip(P, grads)]
    return np.array([float(v.detach()) for v in out]), grads


def loss_and_grads(params, x, tgt, r, **kw):
    """float64: the seven values of ``components`` and the 15 gradients of the loss (ndarrays).  Keywords: eps, alpha,
    beta, beta_voc (trainCNN.py:167-170) and those of :func:`autograd`."""
    return autograd(forward, components, params, x, tgt, r, **kw)


def adadelta(params, grads, accu, delta, lr=1.0, rho=0.95, eps=1e-6):
    """lasagne.updates.adadelta, one step (float64): new params, accu, delta_accu."""
    P, A, D = [], [], []
    for p, g, a, d in zip(params, grads, accu, delta):
        g = np.asarray(g, np.float64)
        a = rho * np.asarray(a, np.float64) + (1 - rho) * g * g
        u = g * np.sqrt(np.asarray(d, np.float64) + eps) / np.sqrt(a + eps)
        P.append(np.asarray(p, np.float64) - lr * u)
        A.append(a)
        D.append(rho * np.asarray(d, np.float64) + (1 - rho) * u * u)
    return P, A, D


def forward_np(params, x):
    with torch.no_grad():
        return forward([_t(p) for p in params], _t(x)).numpy()
