"""float64 torch restatement of build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132), the oracle of the
deep score-informed graph's tests.

Written out layer by layer with explicit ``conv2d`` / ``conv_transpose2d``: an ``InverseLayer`` of a rectified convolution
is ``theano.grad`` through the rectify, and Lasagne's rectify is Theano's ``0.5 * (x + |x|)`` whose derivative at 0 is 0.5
-- ``torch.relu`` autograd would give 0 there.  ``rprime0`` exists so that the fixture generator can show the fixtures tell
the conventions apart.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

STRIDE = (1, 2)


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def rect(x):
    return 0.5 * (x + x.abs())


def rect_grad(pre, rprime0=0.5):
    return torch.where(pre > 0, torch.ones_like(pre), torch.where(pre == 0, torch.full_like(pre, rprime0), torch.zeros_like(pre)))


def forward(params, x, rprime0=0.5, branches=None):
    """params: the 22 arrays (or the live-only layout), x ``[n, 4, tc, F]`` -> ``p [n, 4 k, tc, F]`` float64 ndarray,
    k = the branches the 1x1 layer holds (``branches`` limits how many are evaluated)."""
    P = [_t(p) for p in params]
    h = _t(x)
    shapes, pres = [], []
    for k in range(6):
        W, b, bl = P[3 * k], P[3 * k + 1], P[3 * k + 2]
        shapes.append(tuple(h.shape))
        pre = Fn.conv2d(h, W.flip(2, 3), b, stride=STRIDE)        # Lasagne flip_filters=True: a true convolution
        pres.append(pre)
        h = rect(pre) + bl.view(1, -1, 1, 1)
    W11, b11, bl11, fb = P[18], P[19], P[20], P[21]
    src = rect(Fn.conv2d(h, W11, b11)) + bl11.view(1, -1, 1, 1)
    nb = W11.shape[0] // 200 if branches is None else branches
    outs = []
    for br in range(nb):
        g = src[:, 200 * br:200 * (br + 1)]
        for k in range(5, -1, -1):
            W = P[3 * k]
            d = g * rect_grad(pres[k], rprime0)
            # the gradient of a valid stride-2 convolution w.r.t. its input: the input columns no tap reaches get 0
            n, c, hh, ww = shapes[k]
            ho, wo = d.shape[2], d.shape[3]
            out_pad = (hh - ((ho - 1) * STRIDE[0] + W.shape[2]), ww - ((wo - 1) * STRIDE[1] + W.shape[3]))
            g = Fn.conv_transpose2d(d, W.flip(2, 3), stride=STRIDE, output_padding=out_pad)
        outs.append(g)
    o = torch.cat(outs, dim=1)
    return rect(o + fb[:4 * nb].view(1, -1, 1, 1)).numpy()


def masked(p, x, eps_mode, mixture='ch0'):
    """The soft masks of predict_function2 on the first 4 output channels: ``[4, n, tc, F]``.  eps_mode 0 (A) / 1 (B)
    as oracle.net_ref; mixture 'ch0' (separate script) or 'sum' (trainCNNrwc.py:258-263)."""
    p = np.asarray(p, dtype=np.float64)[:, :4]
    x = np.asarray(x, dtype=np.float64)
    eps = 5e-19
    mix = x[:, 0] if mixture == 'ch0' else x.sum(axis=1)
    if eps_mode == 0:
        q = p + eps
        den = q.sum(axis=1)
    else:
        q = p
        den = p.sum(axis=1) + eps
    return np.stack([q[:, s] / den * mix for s in range(4)])
