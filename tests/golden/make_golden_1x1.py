"""Writes tests/golden/net_bach10si1x1_f257_*.npz: the reference's own build_ca_1x1 (examples/bach10_scoreinformed/
trainCNNrwc.py:66-132) evaluated on seeded inputs.  CPU only; needs the reference tree (DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_1x1.py

The graph source is executed as the reference wrote it, on the Lasagne stand-in oracle/lasagne_np.py extended HERE by
subclassing with the two things build_ca_1x1 needs beyond the other graphs: a SliceLayer and the InverseLayer of a rectified
convolution (theano.grad through Theano's relu = 0.5 (x + |x|): r'(0) = 0.5).

The weights are not stored (they would be ~13 MB at 257 bins): each fixture keeps the seed that regenerates them
(``params_for``) and a checksum of the regenerated arrays.  Stored: the input tiles ``x``, the whole graph's 16-channel
output ``p``, the soft masks under both mixtures (channel 0 / channel sum, eps convention B), and the parameter shapes.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lasagne_np as L  # noqa: E402
from oracle import ref_exec  # noqa: E402

TRAINER = "examples/bach10_scoreinformed/trainCNNrwc.py"
# A fixture holds ~3.4e5 pre-activations, ~200 of which lie within 1e-4 of their scale in any draw; within 1e-6 lie ~2, so
# a few seeds give a draw with none.  The kernels' float32 error on a pre-activation is ~1e-7 of its scale.
MARGIN = 1e-6
RPRIME0 = [0.5]          # r'(0) of the stand-in's rectified InverseLayer (0.5 = Theano; the checks below try 0 and 1)
F_BINS = 257

# name -> (first seed tried, tiles, time_context, zero biases on conv1..conv2 + a silent region)
CASES = {
    "zero": (11, 2, 20, True),
    "rand": (23, 1, 30, False),
}


class Conv2DLayer(L.Conv2DLayer):
    """The stand-in's convolution with the gradient through its nonlinearity (InverseLayer of a rectified layer)."""

    def pre(self, x):
        y = self.linear(x)
        return y + self.b.value.reshape(1, -1, 1, 1) if self.b is not None else y

    def vjp(self, x, g):
        if self.nonlinearity is L.identity:
            d = g
        else:
            pre = self.pre(x)
            d = g * np.where(pre > 0, 1.0, np.where(pre == 0, RPRIME0[0], 0.0))
        gx = np.zeros(x.shape, dtype=np.float64)
        W = self.W.value
        for u, v, rows, cols in self._taps(x.shape):
            gx[:, :, rows, cols] += np.einsum('boyx,oc->bcyx', d, W[:, :, u, v])
        return gx


class SliceLayer(L.Layer):
    def __init__(self, incoming, indices, axis=-1, **kwargs):
        super(SliceLayer, self).__init__(incoming, kwargs.get('name'))
        self.slice, self.axis = indices, axis

    def get_output_shape_for(self, s):
        s = list(s)
        s[self.axis] = len(range(*self.slice.indices(s[self.axis])))
        return tuple(s)

    def forward(self, x):
        idx = [slice(None)] * x.ndim
        idx[self.axis] = self.slice
        return x[tuple(idx)]


class _NS(object):
    pass


def stand_in():
    lasagne = _NS()
    lasagne.layers = _NS()
    for k, v in vars(L.layers).items():
        setattr(lasagne.layers, k, v)
    lasagne.layers.Conv2DLayer = Conv2DLayer
    lasagne.layers.SliceLayer = SliceLayer
    lasagne.nonlinearities = L.nonlinearities
    return lasagne


def build(x):
    src, first = ref_exec._def_block(ref_exec._file_lines(TRAINER), "build_ca_1x1")
    ns = dict(np=np, lasagne=stand_in(), __name__="make_golden_1x1")
    exec(compile("\n" * (first - 1) + src, TRAINER, "exec"), ns)
    B, C, tc, F = x.shape
    return ns["build_ca_1x1"](input_var=x, batch_size=B, time_context=tc, feat_size=F, nchannels=C)


def param_shapes(tc, F=F_BINS):
    out = build(np.zeros((1, 4, tc, F)))
    return [tuple(p.shape) for p in L.get_all_params(out)]


def params_for(seed, tc, zero, shapes=None):
    """A fixture's weights, regenerated from its seed (He-uniform filters as synth_params('bach10_si_1x1'), biases
    uniform +-0.05; ``zero``: b and BiasLayer.b of conv1 and conv2 exactly 0).  The inputs come from the same seed."""
    if shapes is None:
        from deepconvsep_amd.arch import ARCHS
        shapes = ARCHS['bach10_si_1x1'].param_shapes(tc, F_BINS)
    rs = np.random.RandomState(seed)
    params = []
    for i, s in enumerate(shapes):
        if len(s) == 1:
            p = rs.uniform(-0.05, 0.05, s)
            if zero and i in (1, 2, 4, 5):
                p[:] = 0.0
        else:
            lim = np.sqrt(6.0 / (s[1] * s[2] * s[3]))
            p = rs.uniform(-lim, lim, s)
        params.append(p.astype(np.float32))
    return params


def inputs_for(seed, n, tc, zero):
    rs = np.random.RandomState(seed + 1000)
    x = rs.uniform(0.0, 1.0, (n, 4, tc, F_BINS)) * rs.uniform(0.0, 1.0, (n, 4, 1, F_BINS)) ** 2
    if zero:
        x[:, :, 5:9, :] = 0.0       # digital silence: four frames, every channel
        x[:, :, :, 200:] = 0.0      # and the top bins (the library tiler's zero padding looks the same)
    return x.astype(np.float32)


def checksum(params):
    h = hashlib.sha256()
    for p in params:
        h.update(np.ascontiguousarray(p, dtype=np.float32).tobytes())
    return h.hexdigest()


def run(params, x, rprime0=0.5):
    RPRIME0[0] = rprime0
    try:
        out = build(np.asarray(x, dtype=np.float64))
        L.set_all_param_values(out, [np.asarray(p, dtype=np.float64) for p in params])
        return L.get_output(out), out
    finally:
        RPRIME0[0] = 0.5


def near_zero(out, x):
    """Smallest |pre| / sum |w x| over the nonzero pre-activations of every rectified convolution.  A draw is rejected when
    it is below MARGIN: float32 arithmetic could flip that pre-activation's sign, and with it r' in the decoder."""
    worst = np.inf
    vals = {}
    for layer in L.get_all_layers(out):
        if isinstance(layer, L.InputLayer):
            vals[id(layer)] = np.asarray(x, dtype=np.float64)
        elif isinstance(layer, L.MergeLayer):
            continue
        elif id(layer.input_layer) in vals:
            vals[id(layer)] = layer.forward(vals[id(layer.input_layer)])
            if isinstance(layer, Conv2DLayer) and layer.nonlinearity is not L.identity:
                xin = vals[id(layer.input_layer)]
                pre = layer.pre(xin)
                W = layer.W.value
                layer.W.set_value(np.abs(W))
                scale = layer.linear(np.abs(xin)) + np.abs(layer.b.value).reshape(1, -1, 1, 1)
                layer.W.set_value(W)
                nz = pre != 0
                if nz.any():
                    worst = min(worst, float(np.min(np.abs(pre[nz]) / np.maximum(scale[nz], 1e-300))))
    return worst


def masks(p, x):
    sys.path.insert(0, os.path.dirname(HERE))
    import deep1x1_ref
    return deep1x1_ref.masked(p, x, 1, 'ch0'), deep1x1_ref.masked(p, x, 1, 'sum')


def main():
    if not ref_exec.available():
        raise SystemExit("reference tree not found (DCS_REFERENCE_ROOT)")
    for name, (seed0, n, tc, zero) in CASES.items():
        shapes = param_shapes(tc)
        for seed in range(seed0, seed0 + 200):
            params = params_for(seed, tc, zero, shapes)
            x = inputs_for(seed, n, tc, zero)
            p, out = run(params, x)
            worst = near_zero(out, x)
            if worst > MARGIN:
                break
        assert worst > MARGIN, "no draw of case %s keeps its pre-activations %g away from zero" % (name, MARGIN)
        if zero:
            for alt in (0.0, 1.0):
                pa, _ = run(params, x, alt)
                moved = float(np.max(np.abs(pa - p)))
                assert moved > 1e-3, "r'(0) = %g moves p by only %g: the fixture cannot tell the conventions apart" % (alt, moved)
        mch0, msum = masks(p, x)
        path = os.path.join(HERE, "net_bach10si1x1_f%d_%s.npz" % (F_BINS, name))
        np.savez_compressed(path, x=x, p=p, masked_ch0=mch0, masked_sum=msum, seed=seed, tc=tc,
                            shapes=np.array([list(s) + [1] * (4 - len(s)) for s in shapes], dtype=np.int64),
                            ndims=np.array([len(s) for s in shapes], dtype=np.int64), checksum=checksum(params),
                            min_rel_preact=worst)
        print("wrote %s: p %s, max %.4g, min |pre|/scale %.3g" % (path, p.shape, float(p.max()), worst))


if __name__ == "__main__":
    main()
