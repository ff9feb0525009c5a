"""Training of the stereo (ILD) DSD100 graph on the MI355X: the first half of ``train_auto`` of
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py (:117-289) and the data feed of ``dataset.LargeDatasetMulti``
(dataset.py:903-1119).

``StereoTrainer`` has the surface of :class:`deepconvsep_amd.training.Trainer` for arch ``'dsd_ild'``: 17 parameters, two
input channels, eight output channels (channel ``2 s + c``: source s in input channel c), the stage-1 loss of
``train_fn_mse`` / ``train_fn1`` and, with ``ild=True``, the stage-2 loss of ``train_fn_ILD`` (csrc/train_dsdild.hip on
csrc/train_dsd_graph.hip and the shared core csrc/train_core.hip).  The handle itself is
:class:`deepconvsep_amd.training.TrainerHandle`; the class adds what only this graph knows: its channels, its two draws and
the ``ild`` flag of its second loss.  ``training.TRAINABLE`` lists the mono graphs only.

The draws: the reference's ``rand_num`` / ``rand_num2`` are ``RandomStreams(128).normal(std=0.1)`` and are redrawn by Theano
on every call.  The trainer holds one pair ``[2, B, 4, tc, F]`` until :meth:`StereoTrainer.set_rand` replaces it (the
training script does so before every step); Theano's MRG31k3p stream itself is not reproduced.

``StereoFeatureWindows`` keeps the ``*_in_m_.data [2, T, F]`` / ``*_out_m_.data [8, T, F]`` pairs resident on the device
and cuts the reference's windows from them (slot table and epoch order: :class:`deepconvsep_amd.training.WindowFeed`).  There
is no CPU fallback.
"""
import os

import numpy as np

from . import _lib
from .arch import ARCHS
from .runtime import _ptr
from .training import ADA_EPSILON, LEARNING_RATE, RHO, TrainerHandle, WindowFeed, glorot_arrays, listed_files
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
    return glorot_arrays(param_shapes(tc, F), seed)


class StereoTrainer(TrainerHandle):
    """``train_fn_mse`` / ``train_fn1`` (trainCNN_ILD_DSD100.py:204-206) and ``train_fn_ILD`` (:268), resident on one GPU.

    ``params``: the 17 arrays in .pkl order, default :func:`glorot_init`.  ``rand``: ``[2, B, 4, tc, F]``, rand_num then
    rand_num2; default ``0.1 * RandomState(seed).randn``.  ``ild_weight`` is the 1 / 500 of :228.  The batch size is fixed,
    as in the reference's compiled graph."""

    def __init__(self, ctx=None, params=None, batch_size=32, time_context=30, feat_size=513, seed=0, rand=None,
                 eps=ILD_EPS, ild_weight=ILD_WEIGHT, learning_rate=LEARNING_RATE, rho=RHO, epsilon=ADA_EPSILON):
        self.C, self.S = CHANNELS, N_SOURCES
        TrainerHandle.__init__(self, ctx, ARCH, self.C, self.C * self.S, batch_size, time_context, feat_size,
                               (2, int(batch_size), self.S, int(time_context), int(feat_size)), params, rand, seed,
                               (eps, ild_weight, 0.0, 0.0, learning_rate, rho, epsilon))

    def _default_params(self, seed):
        return glorot_init(self.tc, self.F, seed)

    def _default_rand(self, seed):
        return RAND_STD * np.random.RandomState(seed).randn(*self.rand_shape)

    def run(self, inputs, targets, mode, ild=False):
        """``dcs_trainer_step``; returns the device tensor of 16 doubles (loss, the eight errors, the weighted ILD term,
        zeros) before any update.  ``ild``: the stage-2 loss, the library's modes 4 .. 6."""
        return TrainerHandle.run(self, inputs, targets, int(mode) + (4 if ild else 0))

    def step(self, inputs, targets, ild=False):
        """``train_fn_mse`` (:204), with ``ild`` ``train_fn_ILD`` (:268): the loss at the current parameters, then one
        step of the selected update (Adadelta unless ``set_optimizer`` chose another)."""
        return float(self.ctx.to_host(self.run(inputs, targets, 2, ild))[0])

    def losses(self, inputs, targets):
        """``train_fn1`` (:206): ``errors_insts`` as a 2 x 4 array, ``[mic][source]``."""
        return np.array(self.ctx.to_host(self.run(inputs, targets, 0))[1:9], dtype=np.float64).reshape(self.C, self.S)

    def loss_and_gradients(self, inputs, targets, ild=False):
        """Testing aid: the 16 outputs and the gradients of the loss (one per parameter), no update."""
        out = self.ctx.to_host(self.run(inputs, targets, 1, ild)).copy()
        return out, self.gradients()


def feature_pairs(paths, prefix_in='in', prefix_out='out'):
    """The ``(in, out)`` file pairs of ``LargeDatasetMulti.updatePath`` (dataset.py:1098-1100): every file of ``paths`` (files
    or directories) that ends in ``<prefix_in>_m_.data`` and has its ``<prefix_out>_m_.data`` next to it, sorted."""
    tail = prefix_in + '_m_.data'
    pairs = []
    for f in sorted(listed_files(paths)):
        if not f.endswith(tail):
            continue
        d, name = os.path.split(f)
        out = os.path.join(d, name.replace(prefix_in + '_m_', prefix_out + '_m_'))
        if os.path.isfile(out):
            pairs.append((f, out))
    return pairs


class StereoFeatureWindows(WindowFeed):
    """The training data of ``LargeDatasetMulti`` (dataset.py:903-1119) resident on the device.

    ``paths``: feature directories or ``*_in_m_.data`` files; each ``[cin, T, F]`` input file is paired with the
    ``*_out_m_.data [cout, T, F]`` next to it (examples/dsd100_2ch_ILD/compute_features.py writes ``[2, T, 513]`` and ``[8,
    T, 513]``).  Slots as for :class:`deepconvsep_amd.training.FeatureWindows`: ``windows='reference'`` reproduces
    loadFile's slots (:931-1007), zero slots included, ``'all'`` takes every full window.  ``mult_factor_in`` /
    ``mult_factor_out`` scale the two tensors (:964-972).  ``batches(epoch)`` yields ``total // batch_size`` batches in the
    order of ``RandomState(seed + epoch).permutation`` -- seeded, where the reference's shuffle is not."""

    def __init__(self, paths, time_context=30, overlap=25, mult_factor_in=0.3, mult_factor_out=0.3, windows='reference',
                 batch_size=32, seed=0, ctx=None, prefix_in='in', prefix_out='out'):
        WindowFeed.__init__(self, windows, time_context, overlap, batch_size, seed, ctx)
        self.mult_in, self.mult_out = float(mult_factor_in), float(mult_factor_out)
        self.pairs = feature_pairs([paths] if isinstance(paths, str) else list(paths), prefix_in, prefix_out)
        self.shapes = []
        for pin, pout in self.pairs:
            sin = read_shape_file(pin.replace('.data', '.shape'))
            sout = read_shape_file(pout.replace('.data', '.shape'))
            if len(sin) != 3 or len(sout) != 3 or tuple(sin[1:]) != tuple(sout[1:]):
                raise ValueError("%s: shapes %r / %r, expected (cin, T, F) / (cout, T, F)" % (pin, sin, sout))
            self.shapes.append((tuple(sin), tuple(sout)))
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
        self._set_table(s[0][1] for s in self.shapes)

    def _upload(self):
        if getattr(self, "_data", None) is not None:
            return
        self._open()
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
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, self.channels_in, self.channels_out)
            _lib.check(self.ctx._lib.dcs_trainer_gather_channels(self.ctx._h, _ptr(self._data), _ptr(self._files), _ptr(win_d),
                                                                 B, self.tc, self.F, self.channels_in, self.channels_out,
                                                                 self.mult_in, self.mult_out, _ptr(x), _ptr(t)))
        return x, t
