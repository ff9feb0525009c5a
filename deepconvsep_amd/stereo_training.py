"""Training of the stereo (ILD) DSD100 graph on the MI355X: the first half of ``train_auto`` of
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py (:117-289) and the data feed of ``dataset.LargeDatasetMulti``
(dataset.py:903-1119).

``StereoTrainer`` has the surface of :class:`deepconvsep_amd.training.Trainer` for arch ``'dsd_ild'``: 17 parameters, two
input channels, eight output channels (channel ``2 s + c``: source s in input channel c), the stage-1 loss of
``train_fn_mse`` / ``train_fn1`` and, with ``ild=True``, the stage-2 loss of ``train_fn_ILD`` (csrc/train_dsdild.hip on the
shared core csrc/train_core.hip).  It is a class of its own because the graph differs from the three mono ones in its input
channels, its two draws and its second loss; ``training.TRAINABLE`` lists the mono graphs only.

The draws: the reference's ``rand_num`` / ``rand_num2`` are ``RandomStreams(128).normal(std=0.1)`` and are redrawn by Theano
on every call.  The trainer holds one pair ``[2, B, 4, tc, F]`` until :meth:`StereoTrainer.set_rand` replaces it (the
training script does so before every step); Theano's MRG31k3p stream itself is not reproduced.

``StereoFeatureWindows`` keeps the ``*_in_m_.data [2, T, F]`` / ``*_out_m_.data [8, T, F]`` pairs resident on the device
and cuts the reference's windows from them.  There is no CPU fallback.
"""
import os
from ctypes import byref, c_double, c_int, c_int64, c_void_p

import numpy as np

from . import _lib
from .arch import ARCHS
from .runtime import _on_ctx_stream, _ptr, default_context, require_gpu
from .separation import save_model as _save_model
from .training import ADA_EPSILON, LEARNING_RATE, RHO, all_slots, reference_slots
from .transform import read_shape_file

ARCH = 'dsd_ild'
# trainCNN_ILD_DSD100.py:152 and :228 (the ILD term is divided by 500); the draws' std (:164, :210)
ILD_EPS, ILD_WEIGHT, RAND_STD = 1e-12, 1.0 / 500.0, 0.1
SOURCES = ('vocals', 'bass', 'drums', 'other')
CHANNELS, N_SOURCES = 2, 4


def param_shapes(tc, F):
    """The 17 .pkl shapes of build_ca (trainCNN_ILD_DSD100.py:66-113)."""
    return [tuple(s) for s in ARCHS[ARCH].param_shapes(tc, F)]


def glorot_init(tc=30, F=513, seed=0):
    """Lasagne's defaults for build_ca: every W ``GlorotUniform(gain=1)`` -- uniform in +-sqrt(3) * sqrt(2 / ((n1 + n2) *
    receptive field)) with (n1, n2) the first two axes -- and every bias ``Constant(0)``; float32."""
    rs = np.random.RandomState(seed)
    out = []
    for shp in param_shapes(tc, F):
        if len(shp) == 1:
            out.append(np.zeros(shp, dtype=np.float32))
            continue
        rf = int(np.prod(shp[2:])) if len(shp) > 2 else 1
        a = np.sqrt(3.0) * np.sqrt(2.0 / ((shp[0] + shp[1]) * rf))
        out.append(rs.uniform(-a, a, size=shp).astype(np.float32))
    return out


class StereoTrainer(object):
    """``train_fn_mse`` / ``train_fn1`` (trainCNN_ILD_DSD100.py:204-206) and ``train_fn_ILD`` (:268), resident on one GPU.

    ``params``: the 17 arrays in .pkl order, default :func:`glorot_init`.  ``rand``: ``[2, B, 4, tc, F]``, rand_num then
    rand_num2; default ``0.1 * RandomState(seed).randn``.  ``ild_weight`` is the 1 / 500 of :228.  The batch size is fixed,
    as in the reference's compiled graph."""

    def __init__(self, ctx=None, params=None, batch_size=32, time_context=30, feat_size=513, seed=0, rand=None,
                 eps=ILD_EPS, ild_weight=ILD_WEIGHT, learning_rate=LEARNING_RATE, rho=RHO, epsilon=ADA_EPSILON):
        torch = require_gpu()
        self.ctx = ctx if ctx is not None else default_context()
        self.arch = ARCH
        self.C, self.S = CHANNELS, N_SOURCES
        self.B, self.tc, self.F = int(batch_size), int(time_context), int(feat_size)
        self.rand_shape = (2, self.B, self.S, self.tc, self.F)
        if params is None:
            params = glorot_init(self.tc, self.F, seed)
        params = [np.asarray(p, dtype=np.float32) for p in params]
        if rand is None:
            rand = RAND_STD * np.random.RandomState(seed).randn(*self.rand_shape)
        rand = np.asarray(rand)
        if rand.shape != self.rand_shape:
            raise ValueError("rand has shape %r, the trainer takes %r" % (rand.shape, self.rand_shape))
        self.shapes = [tuple(p.shape) for p in params]
        with self.ctx.stream_scope():
            dev = [self.ctx.to_device(p, np.float32) for p in params]
            rand_d = self.ctx.to_device(rand, np.float32)
        n = len(dev)
        ptrs = (c_void_p * n)(*[p.data_ptr() for p in dev])
        shapes = (c_int64 * (4 * n))()
        for i, p in enumerate(params):
            if p.ndim > 4:
                raise ValueError("mismatch: parameter %d has %d axes" % (i, p.ndim))
            shp = list(p.shape) + [1] * (4 - p.ndim)
            for k in range(4):
                shapes[4 * i + k] = shp[k]
        hyper = (c_double * 7)(eps, ild_weight, 0.0, 0.0, learning_rate, rho, epsilon)
        h = c_void_p()
        _lib.check(self.ctx._lib.dcs_trainer_create(self.ctx._h, ARCHS[ARCH].code, self.tc, self.F, self.B, ptrs, shapes, n,
                                                    _ptr(rand_d), hyper, byref(h)))
        self._h = h
        count = c_int()
        _lib.check(self.ctx._lib.dcs_trainer_out_count(self._h, byref(count)))
        with self.ctx.stream_scope():
            self._out = torch.zeros(count.value, dtype=torch.float64, device=self.ctx.device)
        self._keep = (dev, rand_d)   # released after create's copies have run (stream order)

    def _io(self, inputs, targets):
        torch = require_gpu()
        x = inputs if isinstance(inputs, torch.Tensor) else self.ctx.to_device(inputs, np.float32)
        t = targets if isinstance(targets, torch.Tensor) else self.ctx.to_device(targets, np.float32)
        x = x.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        t = t.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        want_x, want_t = (self.B, self.C, self.tc, self.F), (self.B, self.C * self.S, self.tc, self.F)
        if tuple(x.shape) != want_x or tuple(t.shape) != want_t:
            raise ValueError("inputs %r / targets %r, the trainer takes %r / %r" % (tuple(x.shape), tuple(t.shape), want_x,
                                                                                     want_t))
        return x, t

    @_on_ctx_stream
    def run(self, inputs, targets, mode, ild=False):
        """``dcs_trainer_step``; returns the device tensor of 16 doubles (loss, the eight errors, the weighted ILD term,
        zeros) before any update."""
        x, t = self._io(inputs, targets)
        _lib.check(self.ctx._lib.dcs_trainer_step(self._h, _ptr(x), _ptr(t), int(mode) + (4 if ild else 0), _ptr(self._out)))
        self._last_io = (x, t)
        return self._out

    def step(self, inputs, targets, ild=False):
        """``train_fn_mse`` (:204), with ``ild`` ``train_fn_ILD`` (:268): the loss at the current parameters, then one
        Adadelta update."""
        return float(self.ctx.to_host(self.run(inputs, targets, 2, ild))[0])

    def losses(self, inputs, targets):
        """``train_fn1`` (:206): ``errors_insts`` as a 2 x 4 array, ``[mic][source]``."""
        return np.array(self.ctx.to_host(self.run(inputs, targets, 0))[1:9], dtype=np.float64).reshape(self.C, self.S)

    def loss_and_gradients(self, inputs, targets, ild=False):
        """Testing aid: the 16 outputs and the gradients of the loss (one per parameter), no update."""
        out = self.ctx.to_host(self.run(inputs, targets, 1, ild)).copy()
        return out, self.gradients()

    @_on_ctx_stream
    def set_rand(self, rand):
        """Replace the two draws (``[2, B, 4, tc, F]``, an ndarray or a device tensor) in stream order."""
        torch = require_gpu()
        r = rand if isinstance(rand, torch.Tensor) else self.ctx.to_device(np.asarray(rand), np.float32)
        if tuple(r.shape) != self.rand_shape:
            raise ValueError("rand has shape %r, the trainer takes %r" % (tuple(r.shape), self.rand_shape))
        r = r.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        _lib.check(self.ctx._lib.dcs_trainer_set_rand(self._h, _ptr(r)))
        self._rand_keep = r

    @_on_ctx_stream
    def _get(self, which):
        torch = require_gpu()
        outs = [torch.empty(s, dtype=torch.float32, device=self.ctx.device) for s in self.shapes]
        ptrs = (c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        _lib.check(self.ctx._lib.dcs_trainer_get(self._h, int(which), ptrs, len(outs)))
        return [o.cpu().numpy() for o in outs]

    def params(self):
        """``lasagne.layers.get_all_param_values`` (:59): float32 arrays in .pkl order."""
        return self._get(0)

    def gradients(self):
        """Gradients of the last step (testing aid), .pkl order."""
        return self._get(1)

    def adadelta_state(self):
        """(accu, delta_accu) of lasagne.updates.adadelta, .pkl order."""
        return self._get(2), self._get(3)

    @_on_ctx_stream
    def forward(self, inputs):
        """``lasagne.layers.get_output(network)`` (:172): ``[B, 8, tc, F]`` before masking (device tensor)."""
        torch = require_gpu()
        shape = (self.B, self.C * self.S, self.tc, self.F)
        x, _ = self._io(inputs, torch.zeros(shape, dtype=torch.float32, device=self.ctx.device))
        p = torch.empty(shape, dtype=torch.float32, device=self.ctx.device)
        _lib.check(self.ctx._lib.dcs_trainer_forward(self._h, _ptr(x), _ptr(p)))
        return p

    def save_model(self, path):
        """:58-63: the pickled list ``Network(ctx, 'dsd_ild', ...)`` and ``Separator('dsd_ild', ...)`` load."""
        _save_model(path, self.params())

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def feature_pairs(paths, prefix_in='in', prefix_out='out'):
    """The ``(in, out)`` file pairs of ``LargeDatasetMulti.updatePath`` (dataset.py:1098-1100): every file of ``paths`` (files
    or directories) that ends in ``<prefix_in>_m_.data`` and has its ``<prefix_out>_m_.data`` next to it, sorted."""
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in os.listdir(p)]
        else:
            files.append(p)
    tail = prefix_in + '_m_.data'
    pairs = []
    for f in sorted(files):
        if not f.endswith(tail):
            continue
        d, name = os.path.split(f)
        out = os.path.join(d, name.replace(prefix_in + '_m_', prefix_out + '_m_'))
        if os.path.isfile(out):
            pairs.append((f, out))
    return pairs


class StereoFeatureWindows(object):
    """The training data of ``LargeDatasetMulti`` (dataset.py:903-1119) resident on the device.

    ``paths``: feature directories or ``*_in_m_.data`` files; each ``[cin, T, F]`` input file is paired with the
    ``*_out_m_.data [cout, T, F]`` next to it (examples/dsd100_2ch_ILD/compute_features.py writes ``[2, T, 513]`` and ``[8,
    T, 513]``).  Slots as for :class:`deepconvsep_amd.training.FeatureWindows`: ``windows='reference'`` reproduces
    loadFile's slots (:931-1007), zero slots included, ``'all'`` takes every full window.  ``mult_factor_in`` /
    ``mult_factor_out`` scale the two tensors (:964-972).  ``batches(epoch)`` yields ``total // batch_size`` batches in the
    order of ``RandomState(seed + epoch).permutation`` -- seeded, where the reference's shuffle is not."""

    def __init__(self, paths, time_context=30, overlap=25, mult_factor_in=0.3, mult_factor_out=0.3, windows='reference',
                 batch_size=32, seed=0, ctx=None, prefix_in='in', prefix_out='out'):
        if windows not in ('reference', 'all'):
            raise ValueError("windows must be 'reference' or 'all'")
        self.tc, self.overlap, self.batch_size, self.seed = int(time_context), int(overlap), int(batch_size), int(seed)
        self.mult_in, self.mult_out = float(mult_factor_in), float(mult_factor_out)
        self.pairs = feature_pairs([paths] if isinstance(paths, str) else list(paths), prefix_in, prefix_out)
        slots = reference_slots if windows == 'reference' else all_slots
        self.shapes, table = [], []
        for i, (pin, pout) in enumerate(self.pairs):
            sin = read_shape_file(pin.replace('.data', '.shape'))
            sout = read_shape_file(pout.replace('.data', '.shape'))
            if len(sin) != 3 or len(sout) != 3 or tuple(sin[1:]) != tuple(sout[1:]):
                raise ValueError("%s: shapes %r / %r, expected (cin, T, F) / (cout, T, F)" % (pin, sin, sout))
            self.shapes.append((tuple(sin), tuple(sout)))
            table += [(i if s is not None else -1, s if s is not None else 0) for s in slots(sin[1], self.tc, self.overlap)]
        for k, what in ((0, "input channels"), (2, "F")):
            if len(set(s[0][k] for s in self.shapes)) > 1:
                raise ValueError("feature files disagree on %s" % what)
        if len(set(s[1][0] for s in self.shapes)) > 1:
            raise ValueError("feature files disagree on output channels")
        self.channels_in = self.shapes[0][0][0] if self.shapes else 0
        self.channels_out = self.shapes[0][1][0] if self.shapes else 0
        if self.shapes and (not 1 <= self.channels_in <= 4 or not 1 <= self.channels_out <= 16):
            raise ValueError("channels_in %d (1 .. 4), channels_out %d (1 .. 16)" % (self.channels_in, self.channels_out))
        if self.shapes and self.channels_out % self.channels_in:      # dataset.py:1066
            raise ValueError("number of outputs is not multiple of number of inputs")
        self.F = self.shapes[0][0][2] if self.shapes else 0
        self.table = np.asarray(table, dtype=np.int32).reshape(-1, 2)
        self.total = len(self.table)
        self.iteration_size = self.total // self.batch_size
        self._ctx = ctx

    def _upload(self):
        if getattr(self, "_data", None) is not None:
            return
        self.ctx = self._ctx if self._ctx is not None else default_context()
        blocks, files, off = [], [], 0
        for (pin, pout), (sin, sout) in zip(self.pairs, self.shapes):
            for p, shp in ((pin, sin), (pout, sout)):
                blocks.append(np.fromfile(p, dtype=np.float64).reshape(shp).astype(np.float32).ravel())
            files.append((off, sin[1]))
            off += blocks[-1].size + blocks[-2].size
        self._data = self.ctx.to_device(np.concatenate(blocks) if blocks else np.zeros(1, np.float32), np.float32)
        with self.ctx.stream_scope():
            import torch
            self._files = torch.from_numpy(np.asarray(files, dtype=np.int64).reshape(-1, 2)).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, cin, tc, F]`` and targets ``[B, cout, tc, F]`` (device tensors) of the window-table rows ``rows``."""
        self._upload()
        import torch
        win = np.ascontiguousarray(self.table[np.asarray(rows, dtype=np.int64)])
        B = len(win)
        with self.ctx.stream_scope():
            win_d = torch.from_numpy(win).to(self.ctx.device)
            x = torch.empty((B, self.channels_in, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
            t = torch.empty((B, self.channels_out, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
            _lib.check(self.ctx._lib.dcs_trainer_gather_channels(self.ctx._h, _ptr(self._data), _ptr(self._files), _ptr(win_d),
                                                                 B, self.tc, self.F, self.channels_in, self.channels_out,
                                                                 self.mult_in, self.mult_out, _ptr(x), _ptr(t)))
        return x, t

    def batches(self, epoch=0):
        perm = np.random.RandomState(self.seed + epoch).permutation(self.total)
        for b in range(self.iteration_size):
            yield self.gather(perm[b * self.batch_size:(b + 1) * self.batch_size])
