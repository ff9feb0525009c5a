"""Training on the MI355X: the first half of the reference's ``train_auto`` for the DSD100 graph
(examples/dsd100/trainCNN.py:132-263), for the iKala singing-voice graph (examples/ikala/trainCNN.py:120-235, arch
``'ikala_nopool'``) and for the Bach10 graph (examples/bach10/trainCNNbach10.py:126-254, the graph trainCNNrwc.py and
trainCNNSibelius.py train too), and the data feed of ``dataset.LargeDataset`` (dataset.py:383-602).

``Trainer`` holds the parameters (15 for DSD, 13 for iKala, 17 for Bach10), Adadelta's state and the baked-in uniform draw on
the device and runs ``train_fn`` (forward, loss, gradients, Adadelta) and ``train_fn1`` (the loss components) as HIP kernels
(the shared core csrc/train_core.hip behind ``dcs_trainer_*``, the graphs in csrc/train_dsd.hip, csrc/train_ikala.hip and
csrc/train_bach10.hip, the last two descriptions of the shared build_ca graph csrc/train_ca.hip).
``FeatureWindows`` keeps the ``.data`` / ``.shape`` feature files resident on the device and cuts the reference's windows
from them.  There is no CPU fallback.
"""
import math
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np

from . import _lib
from .arch import ARCHS
from .runtime import _on_ctx_stream, _ptr, default_context, require_gpu
from .separation import save_model as _save_model
from .transform import read_shape_file

# trainCNN.py:167-170 and lasagne.updates.adadelta's defaults
EPS, ALPHA, BETA, BETA_VOC = 1e-8, 0.001, 0.01, 0.03
LEARNING_RATE, RHO, ADA_EPSILON = 1.0, 0.95, 1e-6
COMPONENTS = ("vocals", "bass", "drums", "negative", "alpha", "negative_voc")
# examples/ikala/trainCNN.py:152-155; train_fn1's four components (:197)
IKALA_EPS, IKALA_ALPHA, IKALA_BETA_ACC, IKALA_BETA_VOC = 1e-8, 0.9, 0.005, 0.02
IKALA_COMPONENTS = ("vocals", "acc", "negative_voc", "negative_acc")
# examples/bach10/trainCNNbach10.py:160 (alpha of :161 is never used); train_fn1's four errors (:206, :249-252)
BACH10_EPS = 1e-18
BACH10_COMPONENTS = ('bassoon', 'clarinet', 'saxophone', 'violin')
TRAINABLE = ('dsd', 'ikala_nopool', 'bach10')


def n_sources(arch):
    """Targets / output channels of a trainable graph: 4 for DSD and Bach10, 2 for iKala."""
    return 2 if arch == 'ikala_nopool' else 4


def param_shapes(arch, tc, F):
    """The .pkl shapes of build_ca: 15 for DSD (dsd100/trainCNN.py:66-130), 13 for 'ikala_nopool' (ikala/trainCNN.py:
    66-118), 17 for 'bach10' (bach10/trainCNNbach10.py:66-123).  Only these three graphs train here."""
    if arch in ('ikala_nopool', 'bach10'):
        return [tuple(s) for s in ARCHS[arch].param_shapes(tc, F)]
    if arch != 'dsd':
        raise NotImplementedError("training is built for the DSD, 'ikala_nopool' and 'bach10' graphs only, not %r" % (arch,))
    kh = int(tc / 2)
    flat = 50 * (tc - kh + 1)
    shapes = [(50, 1, 1, F), (50,), (50,), (50, 50, kh, 1), (50,), (50,), (flat, 128), (128,)]
    for _ in range(3):
        shapes += [(128, flat), (flat,)]
    return shapes + [(4,)]


def glorot_init(arch='dsd', tc=30, F=513, seed=0):
    """Lasagne's defaults for build_ca (any of the trainers): every W ``GlorotUniform(gain=1)`` -- uniform in +-sqrt(3) *
    sqrt(2 / ((n1 + n2) * receptive field)) with (n1, n2) the first two axes -- and every bias ``Constant(0)``; float32."""
    rs = np.random.RandomState(seed)
    out = []
    for shp in param_shapes(arch, tc, F):
        if len(shp) == 1:
            out.append(np.zeros(shp, dtype=np.float32))
            continue
        rf = int(np.prod(shp[2:])) if len(shp) > 2 else 1
        a = math.sqrt(3.0) * math.sqrt(2.0 / ((shp[0] + shp[1]) * rf))
        out.append(rs.uniform(-a, a, size=shp).astype(np.float32))
    return out


class Trainer(object):
    """``train_fn`` / ``train_fn1`` of trainCNN.py:262-263 for the DSD graph, resident on one GPU; ``arch='ikala_nopool'``:
    the same pair of examples/ikala/trainCNN.py:195-197 for the iKala graph; ``arch='bach10'``: that of
    examples/bach10/trainCNNbach10.py:204-206 for the Bach10 graph.

    ``params``: the 15 (DSD), 13 (iKala) or 17 (Bach10) arrays in .pkl order (``load_model``), default :func:`glorot_init`.  ``rand``: the
    uniform draw of trainCNN.py:180 ``[batch, 1, tc, F]``; default ``RandomState(seed).uniform``.  The batch size is fixed,
    as in the reference's compiled graph.  For iKala, ``beta`` is beta_acc, and loss hyper-parameters left at their DSD
    defaults take iKala's values (ikala/trainCNN.py:152-155: eps 1e-8, alpha 0.9, beta_acc 0.005, beta_voc 0.02).  For
    Bach10, eps left at its default is 1e-18 (bach10/trainCNNbach10.py:160) and alpha, beta and beta_voc are ignored: the
    loss has no such terms."""

    def __init__(self, ctx=None, arch='dsd', params=None, batch_size=32, time_context=30, feat_size=513, seed=0,
                 rand=None, eps=EPS, alpha=ALPHA, beta=BETA, beta_voc=BETA_VOC, learning_rate=LEARNING_RATE, rho=RHO,
                 epsilon=ADA_EPSILON):
        torch = require_gpu()
        self.ctx = ctx if ctx is not None else default_context()
        self.arch = arch
        self.S = n_sources(arch)
        if arch == 'ikala_nopool':
            eps = IKALA_EPS if eps is EPS else eps
            alpha = IKALA_ALPHA if alpha is ALPHA else alpha
            beta = IKALA_BETA_ACC if beta is BETA else beta
            beta_voc = IKALA_BETA_VOC if beta_voc is BETA_VOC else beta_voc
        elif arch == 'bach10':
            eps = BACH10_EPS if eps is EPS else eps
        self.B, self.tc, self.F = int(batch_size), int(time_context), int(feat_size)
        if params is None:
            params = glorot_init(arch, self.tc, self.F, seed)
        params = [np.asarray(p, dtype=np.float32) for p in params]
        if rand is None:
            rand = np.random.RandomState(seed).uniform(size=(self.B, 1, self.tc, self.F))
        rand = np.asarray(rand)
        if rand.shape != (self.B, 1, self.tc, self.F):
            raise ValueError("rand has shape %r, the trainer takes %r" % (rand.shape, (self.B, 1, self.tc, self.F)))
        self.shapes = [tuple(p.shape) for p in params]
        code = ARCHS[arch].code if arch in ARCHS else -1
        with self.ctx.stream_scope():
            dev = [self.ctx.to_device(p, np.float32) for p in params]
            rand_d = self.ctx.to_device(rand, np.float32)
            self._out7 = torch.zeros(7, dtype=torch.float64, device=self.ctx.device)
        n = len(dev)
        ptrs = (c_void_p * n)(*[p.data_ptr() for p in dev])
        shapes = (c_int64 * (4 * n))()
        for i, p in enumerate(params):
            shp = list(p.shape) + [1] * (4 - p.ndim)
            for k in range(4):
                shapes[4 * i + k] = shp[k]
        hyper = (c_double * 7)(eps, alpha, beta, beta_voc, learning_rate, rho, epsilon)
        h = c_void_p()
        _lib.check(self.ctx._lib.dcs_trainer_create(self.ctx._h, code, self.tc, self.F, self.B, ptrs, shapes, n,
                                                    _ptr(rand_d), hyper, byref(h)))
        self._h = h
        self._keep = (dev, rand_d)   # released after create's copies have run (stream order)

    def _io(self, inputs, targets):
        torch = require_gpu()
        x = inputs if isinstance(inputs, torch.Tensor) else self.ctx.to_device(inputs, np.float32)
        t = targets if isinstance(targets, torch.Tensor) else self.ctx.to_device(targets, np.float32)
        x = x.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        t = t.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        if tuple(x.shape) != (self.B, 1, self.tc, self.F) or tuple(t.shape) != (self.B, self.S, self.tc, self.F):
            raise ValueError("inputs %r / targets %r, the trainer takes (%d, 1, %d, %d) / (%d, %d, %d, %d)"
                             % (tuple(x.shape), tuple(t.shape), self.B, self.tc, self.F, self.B, self.S, self.tc, self.F))
        return x, t

    @_on_ctx_stream
    def run(self, inputs, targets, mode):
        """``dcs_trainer_step``; returns the device tensor of (loss, components, zeros to 7) before any update."""
        x, t = self._io(inputs, targets)
        _lib.check(self.ctx._lib.dcs_trainer_step(self._h, _ptr(x), _ptr(t), int(mode), _ptr(self._out7)))
        self._last_io = (x, t)
        return self._out7

    def step(self, inputs, targets):
        """``train_fn`` (trainCNN.py:262): the loss at the current parameters, then one Adadelta update."""
        return float(self.ctx.to_host(self.run(inputs, targets, 2))[0])

    def losses(self, inputs, targets):
        """``train_fn1`` (trainCNN.py:263): vocals, bass, drums, negative, alpha, negative_voc at the current parameters;
        iKala (ikala/trainCNN.py:197): vocals_error, acc_error, negative_error_voc, negative_error_acc; Bach10
        (bach10/trainCNNbach10.py:206): error1 .. error4 (bassoon, clarinet, saxophone, violin)."""
        n = {'dsd': len(COMPONENTS), 'bach10': len(BACH10_COMPONENTS)}.get(self.arch, len(IKALA_COMPONENTS))
        return [float(v) for v in self.ctx.to_host(self.run(inputs, targets, 0))[1:1 + n]]

    def loss_and_gradients(self, inputs, targets):
        """Testing aid: loss and the gradients of |E| (one per parameter) at the current parameters, no update."""
        out = self.ctx.to_host(self.run(inputs, targets, 1)).copy()
        return out, self.gradients()

    @_on_ctx_stream
    def _get(self, which):
        torch = require_gpu()
        outs = [torch.empty(s, dtype=torch.float32, device=self.ctx.device) for s in self.shapes]
        ptrs = (c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        _lib.check(self.ctx._lib.dcs_trainer_get(self._h, int(which), ptrs, len(outs)))
        return [o.cpu().numpy() for o in outs]

    def params(self):
        """``lasagne.layers.get_all_param_values`` (trainCNN.py:60): float32 arrays in .pkl order."""
        return self._get(0)

    def gradients(self):
        """Gradients of the last step (testing aid), .pkl order."""
        return self._get(1)

    def adadelta_state(self):
        """(accu, delta_accu) of lasagne.updates.adadelta, .pkl order."""
        return self._get(2), self._get(3)

    @_on_ctx_stream
    def forward(self, inputs):
        """``lasagne.layers.get_output(network2)``: ``[B, 4, tc, F]`` (iKala ``[B, 2, tc, F]``) before masking (device
        tensor)."""
        torch = require_gpu()
        x, _ = self._io(inputs, torch.zeros((self.B, self.S, self.tc, self.F), dtype=torch.float32, device=self.ctx.device))
        p = torch.empty((self.B, self.S, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
        _lib.check(self.ctx._lib.dcs_trainer_forward(self._h, _ptr(x), _ptr(p)))
        return p

    def save_model(self, path):
        """trainCNN.py:59-64: the pickled list ``Network('dsd', ...)`` and separate_dsd.py load (iKala: ``Network('ikala',
        ...)``, ``Separator('ikala', ...)`` and separate_ikala.py, which resolve it to the no-pool graph; Bach10:
        ``Network('bach10', ...)``, ``Separator('bach10', ...)`` and separate_bach10.py)."""
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


def reference_slots(T, tc, overlap):
    """Window starts of one file as ``LargeDataset`` fills them (dataset.py:596-602 getNum, :383-488 loadFile): getNum(T)
    slots; the first windows start = 0, tc - ov, ... while start + tc < T; a file shorter than tc gives one padded
    window; None = a slot loadFile never reaches (all zero, initOutput :509-516)."""
    n = max(1, int(np.floor((T + np.floor(float(T) / tc) * overlap) / tc)))
    if tc > T:
        return [0] + [None] * (n - 1)
    starts = []
    start = 0
    while start + tc < T and len(starts) < n:
        starts.append(start)
        start = start - overlap + tc
    return starts + [None] * (n - len(starts))


def all_slots(T, tc, overlap):
    """Every full window start = 0, tc - ov, ... with start + tc <= T (a file shorter than tc: one padded window)."""
    if tc > T:
        return [0]
    return list(range(0, T - tc + 1, tc - overlap))


class FeatureWindows(object):
    """The training data of ``LargeDataset`` (dataset.py) resident on the device.

    ``paths``: ``.data`` files of float64 ``[1 + sources, T, F]`` (each with its ``.shape``): by default ``[5, T, F]``
    (mixture, vocals, bass, drums, other) as examples/dsd100/compute_features.py writes them; ``sources=2``: ``[3, T, F]``
    (mixture, voice, accompaniment) as examples/ikala/compute_features.py writes them.  ``windows='reference'`` reproduces loadFile's slots, zero slots
    included (at tc 30 / overlap 25 only about the first third of each 30 s chunk is used); ``'all'`` takes every full
    window.  ``batches(epoch)`` yields ``total // batch_size`` batches in the order of ``RandomState(seed + epoch)
    .permutation`` -- seeded, where the reference's shuffle is not."""

    def __init__(self, paths, time_context=30, overlap=25, mult_factor=0.3, windows='reference', batch_size=32, seed=0,
                 ctx=None, sources=4):
        if windows not in ('reference', 'all'):
            raise ValueError("windows must be 'reference' or 'all'")
        self.sources = int(sources)
        if not 1 <= self.sources <= 8:
            raise ValueError("sources must be 1 .. 8, got %r" % (sources,))
        self.tc, self.overlap, self.mult, self.batch_size, self.seed = int(time_context), int(overlap), float(mult_factor), \
            int(batch_size), int(seed)
        self.paths = list(paths)
        slots = reference_slots if windows == 'reference' else all_slots
        self.shapes, table = [], []
        for i, p in enumerate(self.paths):
            shp = read_shape_file(p.replace('.data', '.shape'))
            if len(shp) != 3 or shp[0] != 1 + self.sources:
                raise ValueError("%s: shape %r, expected (%d, T, F)" % (p, shp, 1 + self.sources))
            self.shapes.append(shp)
            table += [(i if s is not None else -1, s if s is not None else 0) for s in slots(shp[1], self.tc, self.overlap)]
        if len(set(s[2] for s in self.shapes)) > 1:
            raise ValueError("feature files disagree on F: %r" % sorted(set(s[2] for s in self.shapes)))
        self.F = self.shapes[0][2] if self.shapes else 0
        self.table = np.asarray(table, dtype=np.int32).reshape(-1, 2)
        self.total = len(self.table)
        self.iteration_size = self.total // self.batch_size
        self._ctx = ctx

    def _upload(self):
        if getattr(self, "_data", None) is not None:
            return
        self.ctx = self._ctx if self._ctx is not None else default_context()
        blocks, files, off = [], [], 0
        for p, shp in zip(self.paths, self.shapes):
            a = np.fromfile(p, dtype=np.float64).reshape(shp).astype(np.float32)
            blocks.append(a.ravel())
            files.append((off, shp[1]))
            off += a.size
        self._data = self.ctx.to_device(np.concatenate(blocks) if blocks else np.zeros(1, np.float32), np.float32)
        with self.ctx.stream_scope():
            import torch
            self._files = torch.from_numpy(np.asarray(files, dtype=np.int64).reshape(-1, 2)).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, 1, tc, F]`` and targets ``[B, sources, tc, F]`` (device tensors) of the window-table rows ``rows``."""
        self._upload()
        import torch
        win = np.ascontiguousarray(self.table[np.asarray(rows, dtype=np.int64)])
        B = len(win)
        with self.ctx.stream_scope():
            win_d = torch.from_numpy(win).to(self.ctx.device)
            x = torch.empty((B, 1, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
            t = torch.empty((B, self.sources, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
            if self.sources == 4:
                _lib.check(self.ctx._lib.dcs_trainer_gather(self.ctx._h, _ptr(self._data), _ptr(self._files), _ptr(win_d), B,
                                                            self.tc, self.F, self.mult, _ptr(x), _ptr(t)))
            else:
                _lib.check(self.ctx._lib.dcs_trainer_gather_sources(self.ctx._h, _ptr(self._data), _ptr(self._files),
                                                                    _ptr(win_d), B, self.tc, self.F, self.sources,
                                                                    self.mult, _ptr(x), _ptr(t)))
        return x, t

    def batches(self, epoch=0):
        perm = np.random.RandomState(self.seed + epoch).permutation(self.total)
        for b in range(self.iteration_size):
            yield self.gather(perm[b * self.batch_size:(b + 1) * self.batch_size])
