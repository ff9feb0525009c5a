"""float64 torch autograd restatement of the deep score-informed trainer (test infrastructure): build_ca_1x1 of
examples/bach10_scoreinformed/trainCNNrwc.py:66-132, the loss of :246-275 (``train_si_ref.components``) and
``lasagne.updates.adadelta`` (``train_ref.adadelta``).

The graph has thirteen rectifier layers (seven in the encoder, six InverseLayers that reuse the encoder's) and its gradient
jumps wherever a pre-activation crosses zero, so a gradient is compared at a *given* sign pattern: with ``codes`` (seven
arrays ``[B, C_l, H_l, W_l]`` of 0 / 0.5 / 1, the device's ``ScoreTrainer.rectify_codes()``) every rectify is ``pre * c`` and
every InverseLayer multiplies by ``c``; ``c`` is a constant of the gradient, as Theano's derivative of ``sgn`` is zero.
Without ``codes`` the restatement uses its own: rectify = 0.5 (x + |x|), r'(0) = ``tie``.  The output rectify is always the
restatement's own, on its own q."""
import numpy as np
import torch
import torch.nn.functional as Fn

import train_ref
from train_ref import _t, adadelta  # noqa: F401
from train_si_ref import EPS, components  # noqa: F401

STRIDE = (1, 2)
NF = 200
LAYERS = 6


def rect_grad(pre, tie):
    return torch.where(pre > 0, torch.ones_like(pre), torch.where(pre == 0, torch.full_like(pre, tie), torch.zeros_like(pre)))


def graph(P, x, codes=None, tie=0.5):
    """q ``[B, 4, tc, F]`` (branch 0 before the output rectify), the seven pre-activations and the seven codes used."""
    h = x
    shapes, pres, cs = [], [], []

    def act(pre, k):
        pres.append(pre)
        if codes is not None:
            c = codes[k]
            y = pre * c
        else:
            c = rect_grad(pre.detach(), tie)
            y = train_ref.rectify(pre)
        cs.append(c)
        return y

    for k in range(LAYERS):
        W, b, bl = P[3 * k], P[3 * k + 1], P[3 * k + 2]
        shapes.append(tuple(h.shape))
        h = act(Fn.conv2d(h, W.flip(2, 3), b, stride=STRIDE), k) + bl.view(1, -1, 1, 1)
    W11, b11, bl11, fb = P[18], P[19], P[20], P[21]
    src = act(Fn.conv2d(h, W11, b11), LAYERS) + bl11.view(1, -1, 1, 1)
    g = src[:, 0:NF]
    for k in range(LAYERS - 1, -1, -1):
        W = P[3 * k]
        d = g * cs[k]
        n, c, hh, ww = shapes[k]
        out_pad = (hh - (d.shape[2] - 1 + W.shape[2]), ww - ((d.shape[3] - 1) * STRIDE[1] + W.shape[3]))
        g = Fn.conv_transpose2d(d, W.flip(2, 3), stride=STRIDE, output_padding=out_pad)
    return g + fb[0:4].view(1, -1, 1, 1), pres, cs


def loss_and_grads(params, x, tgt, r, codes=None, tie=0.5, dtype=torch.float64, eps=EPS):
    """(loss, error1 .. error4), the 22 gradients (float64 ndarrays; exact zeros for what no loss term reaches), and a dict
    with ``q``, ``pres`` (the seven pre-activations) and ``codes`` (those used, all rows of the 1x1 layer) as ndarrays."""
    kw = dict(dtype=dtype)
    P = [_t(p, True, **kw) for p in params]
    cd = None if codes is None else [_t(c, **kw) for c in codes]
    if cd is not None and cd[LAYERS].shape[1] < P[18].shape[0]:       # the device keeps the live rows' codes only
        pad = torch.zeros((cd[LAYERS].shape[0], P[18].shape[0] - cd[LAYERS].shape[1]) + tuple(cd[LAYERS].shape[2:]), **kw)
        cd[LAYERS] = torch.cat([cd[LAYERS], pad], dim=1)
    with train_ref.relu_tie(tie):
        q, pres, cs = graph(P, _t(x, **kw), cd, tie)
        out = components(train_ref.rectify(q), _t(x, **kw), _t(tgt, **kw), _t(r, **kw), eps=eps)
        grads = torch.autograd.grad(out[0], P, allow_unused=True)
    grads = [np.zeros(p.shape) if g is None else g.detach().numpy().astype(np.float64) for p, g in zip(P, grads)]
    info = dict(q=q.detach().numpy(), pres=[p.detach().numpy() for p in pres], codes=[c.detach().numpy() for c in cs])
    return np.array([float(v.detach()) for v in out]), grads, info


def forward_np(params, x):
    """p ``[B, 4, tc, F]``: the live channels after the output rectify."""
    with torch.no_grad():
        q, _, _ = graph([_t(p) for p in params], _t(x))
        return train_ref.rectify(q).numpy()


def live(params):
    """The live-only layout (k = 1) of a 22-array list."""
    return list(params[:18]) + [np.asarray(params[18])[:NF], np.asarray(params[19])[:NF], np.asarray(params[20])[:NF],
                                np.asarray(params[21])[:4]]


def setup(B, tc, F, seed, branches=4):
    """He-uniform weights and biases in +-0.05 (``synth.synth_params('bach10_si_1x1')``), a live final bias of 0.5 + |.| (it
    keeps min |q| / max |q| well above the 1e-3 the tests ask for: the output rectify stays out of the comparison), inputs as
    tests/test_gpu_train_si.py::_setup."""
    from deepconvsep_amd.synth import synth_params
    rs = np.random.RandomState(seed)
    params = [np.asarray(p, np.float32) for p in synth_params('bach10_si_1x1', tc, F, seed=seed)]
    params[21] = (np.float32(0.5) + np.abs(params[21])).astype(np.float32)
    if branches < 4:
        params = params[:18] + [params[18][:NF * branches], params[19][:NF * branches], params[20][:NF * branches],
                                params[21][:4 * branches]]
    x = (0.3 * rs.uniform(0, 0.25, size=(B, 4, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 4, tc, F))).astype(np.float32)
    return params, x, r, tgt


def check_codes(dev_codes, pres64, label=""):
    """Part 2 of the criterion: per layer, the device's codes differ from the float64 sign pattern on at most a 1e-4 share of
    the units, and only where |pre64| <= 1e-5 max |pre64| of the layer.  Returns the number of differing units."""
    total = 0
    for k, (c, pre) in enumerate(zip(dev_codes, pres64)):
        pre = pre[:, :c.shape[1]]
        own = np.where(pre > 0, 1.0, np.where(pre == 0, 0.5, 0.0))
        diff = own != c
        n = int(diff.sum())
        total += n
        if n:
            worst = np.abs(pre[diff]).max() / np.abs(pre).max()
            print("%s layer %d: %d of %d codes differ, worst |pre| / max %.2e" % (label, k + 1, n, c.size, worst))
            assert n <= 1e-4 * c.size, (label, k, n, c.size)
            assert worst <= 1e-5, (label, k, worst)
    return total
