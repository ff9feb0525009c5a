"""Training on the MI355X: the first half of the reference's ``train_auto`` for the DSD100 graph
(examples/dsd100/trainCNN.py:132-263), for the iKala singing-voice graph (examples/ikala/trainCNN.py:120-235, arch
``'ikala_nopool'``) and for the Bach10 graph (examples/bach10/trainCNNbach10.py:126-254, the graph trainCNNrwc.py and
trainCNNSibelius.py train too), and the data feed of ``dataset.LargeDataset`` (dataset.py:383-602).

``TrainerHandle`` is the one Python handle on ``dcs_trainer_*`` (the shared core csrc/train_core.hip): upload of the
parameters and the baked-in draw, the optimiser's state, ``train_fn`` (forward, loss, gradients, and Adadelta or -- after
``set_optimizer('adam')`` -- Adam) and ``train_fn1`` (the loss components) as HIP kernels; ``set_params``,
``optimizer_state`` / ``load_optimizer_state`` and ``save_checkpoint`` / ``load_checkpoint`` rewrite and resume a live
trainer.  ``Trainer`` describes the three mono graphs to it (15 parameters for DSD, 13 for iKala, 17
for Bach10: csrc/train_dsd.hip, a description of the full-width graph csrc/train_dsd_graph.hip, and csrc/train_ikala.hip and
csrc/train_bach10.hip, descriptions of the shared build_ca graph csrc/train_ca.hip); ``stereo_training.StereoTrainer`` and
``score_training.ScoreTrainer`` describe theirs.
``WindowFeed`` is what the window feeds share: the slot table, the seeded epoch order and the lazily opened context;
``RenderedFeed`` adds what the feeds of augment and score_render share, which transform their windows per batch.
``FeatureWindows`` keeps the ``.data`` / ``.shape`` feature files resident on the device and cuts the reference's windows
from them; the feeds of stereo_training, score_training, augment and score_render derive from the same base.
:func:`glorot_arrays` is Lasagne's initialisation for any of the layouts.  There is no CPU fallback.
"""
import math
import os
import pickle
from ctypes import byref, c_double, c_int, c_int64, c_void_p

import numpy as np

from . import _lib
from .arch import ARCHS
from .runtime import StftPlan, _on_ctx_stream, _ptr, default_context, require_gpu
from .separation import blackmanharris, save_model as _save_model
from .transform import read_shape_file

# trainCNN.py:167-170 and lasagne.updates.adadelta's defaults
EPS, ALPHA, BETA, BETA_VOC = 1e-8, 0.001, 0.01, 0.03
LEARNING_RATE, RHO, ADA_EPSILON = 1.0, 0.95, 1e-6
# dcs_trainer_set_optimizer: kind -> (DCS_OPT_* code, the names of hyper_h, lasagne.updates' defaults)
OPTIMIZERS = {'adadelta': (0, ('learning_rate', 'rho', 'epsilon'), (LEARNING_RATE, RHO, ADA_EPSILON)),
              'adam': (1, ('learning_rate', 'beta1', 'beta2', 'epsilon'), (1e-3, 0.9, 0.999, 1e-8))}
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


def glorot_arrays(shapes, seed):
    """Lasagne's defaults for a list of parameter shapes: every W ``GlorotUniform(gain=1)`` -- uniform in +-sqrt(3) *
    sqrt(2 / ((n1 + n2) * receptive field)) with (n1, n2) the first two axes -- and every bias ``Constant(0)``; float32,
    drawn from one ``RandomState(seed)`` in parameter order."""
    rs = np.random.RandomState(seed)
    out = []
    for shp in shapes:
        if len(shp) == 1:
            out.append(np.zeros(shp, dtype=np.float32))
            continue
        rf = int(np.prod(shp[2:])) if len(shp) > 2 else 1
        a = math.sqrt(3.0) * math.sqrt(2.0 / ((shp[0] + shp[1]) * rf))
        out.append(rs.uniform(-a, a, size=shp).astype(np.float32))
    return out


def glorot_init(arch='dsd', tc=30, F=513, seed=0):
    """Lasagne's defaults for build_ca (any of the trainers): every W ``GlorotUniform(gain=1)`` -- uniform in +-sqrt(3) *
    sqrt(2 / ((n1 + n2) * receptive field)) with (n1, n2) the first two axes -- and every bias ``Constant(0)``; float32."""
    return glorot_arrays(param_shapes(arch, tc, F), seed)


class TrainerHandle(object):
    """One ``dcs_trainer`` handle: what ``Trainer``, ``stereo_training.StereoTrainer`` and ``score_training.ScoreTrainer``
    share.  The parameters, the optimiser's state and the baked-in draw live on the device; the batch size is fixed, as in the
    reference's compiled graph.

    A subclass describes its graph to ``__init__`` -- the arch name, input and output channels, the draw's shape and the
    seven ``hyper`` values of ``dcs_trainer_create`` -- and supplies ``_default_params(seed)`` and, where the draw is not
    uniform, ``_default_rand(seed)``; both are only called once a GPU is known to be there.  ``params``: float32 arrays in
    .pkl order, at most four axes each."""

    def __init__(self, ctx, arch, channels_in, channels_out, batch_size, time_context, feat_size, rand_shape, params, rand,
                 seed, hyper, code=None):
        torch = require_gpu()
        self.ctx = ctx if ctx is not None else default_context()
        self.arch = arch
        self.B, self.tc, self.F = int(batch_size), int(time_context), int(feat_size)
        self.rand_shape = tuple(rand_shape)
        self._x_shape = (self.B, channels_in, self.tc, self.F)
        self._t_shape = (self.B, channels_out, self.tc, self.F)
        if params is None:
            params = self._default_params(seed)
        params = [np.asarray(p, dtype=np.float32) for p in params]
        if rand is None:
            rand = self._default_rand(seed)
        rand = np.asarray(rand)
        if rand.shape != self.rand_shape:
            raise ValueError("rand has shape %r, the trainer takes %r" % (rand.shape, self.rand_shape))
        self.shapes = [tuple(p.shape) for p in params]
        n = len(params)
        shapes = (c_int64 * (4 * n))()
        for i, p in enumerate(params):
            if p.ndim > 4:
                raise ValueError("mismatch: parameter %d has %d axes" % (i, p.ndim))
            shp = list(p.shape) + [1] * (4 - p.ndim)
            for k in range(4):
                shapes[4 * i + k] = shp[k]
        with self.ctx.stream_scope():
            dev = [self.ctx.to_device(p, np.float32) for p in params]
            rand_d = self.ctx.to_device(rand, np.float32)
        ptrs = (c_void_p * n)(*[p.data_ptr() for p in dev])
        h = c_void_p()
        _lib.check(self.ctx._lib.dcs_trainer_create(self.ctx._h, ARCHS[arch].code if code is None else code, self.tc, self.F,
                                                    self.B, ptrs, shapes, n, _ptr(rand_d), (c_double * 7)(*hyper), byref(h)))
        self._h = h
        count = c_int()
        _lib.check(self.ctx._lib.dcs_trainer_out_count(self._h, byref(count)))
        with self.ctx.stream_scope():
            self._out = torch.zeros(count.value, dtype=torch.float64, device=self.ctx.device)
        self._keep = (dev, rand_d)   # released after create's copies have run (stream order)

    def _default_rand(self, seed):
        return np.random.RandomState(seed).uniform(size=self.rand_shape)

    def _io(self, inputs, targets=None):
        """``inputs`` (and ``targets``, where given) as contiguous float32 device tensors of the trainer's shapes."""
        torch = require_gpu()
        x = inputs if isinstance(inputs, torch.Tensor) else self.ctx.to_device(inputs, np.float32)
        x = x.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        if targets is None:
            if tuple(x.shape) != self._x_shape:
                raise ValueError("inputs %r, the trainer takes %r" % (tuple(x.shape), self._x_shape))
            return x, None
        t = targets if isinstance(targets, torch.Tensor) else self.ctx.to_device(targets, np.float32)
        t = t.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        if tuple(x.shape) != self._x_shape or tuple(t.shape) != self._t_shape:
            raise ValueError("inputs %r / targets %r, the trainer takes %r / %r" % (tuple(x.shape), tuple(t.shape),
                                                                                     self._x_shape, self._t_shape))
        return x, t

    @_on_ctx_stream
    def run(self, inputs, targets, mode):
        """``dcs_trainer_step``; returns the device tensor of ``dcs_trainer_out_count`` doubles (loss, components, zeros)
        before any update."""
        x, t = self._io(inputs, targets)
        _lib.check(self.ctx._lib.dcs_trainer_step(self._h, _ptr(x), _ptr(t), int(mode), _ptr(self._out)))
        self._last_io = (x, t)
        return self._out

    def step(self, inputs, targets):
        """``train_fn``: the loss at the current parameters, then one step of the selected update (Adadelta unless
        :meth:`set_optimizer` chose another)."""
        return float(self.ctx.to_host(self.run(inputs, targets, 2))[0])

    def loss_and_gradients(self, inputs, targets):
        """Testing aid: the outputs of ``run`` and the gradients of the loss (one per parameter; exact zeros for parameters
        the loss does not reach) at the current parameters, no update."""
        out = self.ctx.to_host(self.run(inputs, targets, 1)).copy()
        return out, self.gradients()

    @_on_ctx_stream
    def set_rand(self, rand):
        """Replace the draw (``rand_shape``, an ndarray or a device tensor) in stream order."""
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
        """``lasagne.layers.get_all_param_values``: float32 arrays in .pkl order."""
        return self._get(0)

    def gradients(self):
        """Gradients of the last step (testing aid), .pkl order."""
        return self._get(1)

    def adadelta_state(self):
        """(accu, delta_accu) of lasagne.updates.adadelta, .pkl order."""
        return self._get(2), self._get(3)

    @_on_ctx_stream
    def _set(self, which, arrays):
        """``dcs_trainer_set``: ``arrays`` in .pkl order with the trainer's shapes into the parameters (0) or one of the two
        accumulators (2, 3), in stream order."""
        arrays = [np.asarray(a, dtype=np.float32) for a in arrays]
        if len(arrays) == len(self.shapes):    # a wrong count goes to the library, which words it; the shapes only Python knows
            self._check_shapes(arrays)
        dev = [self.ctx.to_device(a, np.float32) for a in arrays]
        ptrs = (c_void_p * max(len(dev), 1))(*[d.data_ptr() for d in dev])
        _lib.check(self.ctx._lib.dcs_trainer_set(self._h, int(which), ptrs, len(dev)))
        self._set_keep = dev   # released after the copies have run (stream order)

    def _check_shapes(self, arrays):
        """``ValueError`` in the library's "mismatch: ..." wording unless ``arrays`` has the trainer's count and shapes."""
        if len(arrays) != len(self.shapes):
            raise ValueError("mismatch: got %d values to set %d parameters" % (len(arrays), len(self.shapes)))
        for i, (a, want) in enumerate(zip(arrays, self.shapes)):
            if tuple(np.shape(a)) != want:
                raise ValueError("mismatch: parameter %d has shape %r but value to set has shape %r"
                                 % (i, want, tuple(np.shape(a))))

    def set_params(self, params):
        """``lasagne.layers.set_all_param_values`` on the live trainer: the optimiser's state and step count stay."""
        self._set(0, params)

    def set_optimizer(self, kind='adadelta', **hyper):
        """Select the update of :meth:`step`, as calling ``lasagne.updates.adadelta`` / ``lasagne.updates.adam`` again does:
        fresh (zero) accumulators and step count.  ``hyper``: ``learning_rate``, ``rho``, ``epsilon`` for ``'adadelta'``
        (Lasagne's 1, 0.95, 1e-6), ``learning_rate``, ``beta1``, ``beta2``, ``epsilon`` for ``'adam'`` (1e-3, 0.9, 0.999,
        1e-8)."""
        if kind not in OPTIMIZERS:
            raise ValueError("optimizer %r: one of %r" % (kind, sorted(OPTIMIZERS)))
        code, names, defaults = OPTIMIZERS[kind]
        unknown = sorted(set(hyper) - set(names))
        if unknown:
            raise TypeError("set_optimizer(%r) takes %r, not %r" % (kind, names, unknown))
        vals = [float(hyper.get(n, d)) for n, d in zip(names, defaults)]
        self._set_optimizer(code, vals)

    def _set_optimizer(self, code, vals):
        vals = list(vals) + [0.0] * (4 - len(vals))
        _lib.check(self.ctx._lib.dcs_trainer_set_optimizer(self._h, int(code), (c_double * 4)(*vals)))

    def optimizer_state(self):
        """The selected update and its state: ``kind``, ``hyper`` (a dict by name), ``steps`` (updates since it was selected;
        Adam's t) and the two accumulators ``slots`` = (accu, delta_accu) or (m, v), each in .pkl order."""
        kind, vals, steps = c_int(), (c_double * 4)(), c_int64()
        _lib.check(self.ctx._lib.dcs_trainer_get_optimizer(self._h, byref(kind), vals, byref(steps)))
        name = [k for k, v in OPTIMIZERS.items() if v[0] == kind.value][0]
        return {'kind': name, 'hyper': dict(zip(OPTIMIZERS[name][1], list(vals))), 'steps': int(steps.value),
                'slots': (self._get(2), self._get(3))}

    def load_optimizer_state(self, d):
        """Put back what :meth:`optimizer_state` returned (of a trainer with the same shapes): the update, its
        hyper-parameters, both accumulators and the step count."""
        slots = d['slots']
        if len(slots) != 2:
            raise ValueError("mismatch: an optimiser state holds two slots, got %d" % len(slots))
        if int(d['steps']) < 0:
            raise ValueError("load_optimizer_state: %d steps" % int(d['steps']))
        for arrays in slots:      # before the optimiser is replaced
            self._check_shapes(arrays)
        self.set_optimizer(d['kind'], **d['hyper'])
        self._set(2, slots[0])
        self._set(3, slots[1])
        _lib.check(self.ctx._lib.dcs_trainer_set_steps(self._h, int(d['steps'])))

    def save_checkpoint(self, path):
        """The parameters and :meth:`optimizer_state` in one protocol-2 pickle: what :meth:`load_checkpoint` resumes
        from, bit for bit.  (:meth:`save_model` writes the parameter list alone, the reference's format.)"""
        with open(path, 'wb') as f:
            pickle.dump({'params': self.params(), 'optimizer': self.optimizer_state()}, f, protocol=2)

    def load_checkpoint(self, path):
        """Resume from :meth:`save_checkpoint`'s file; the shapes must be the trainer's (``ValueError`` "mismatch: ...")."""
        with open(path, 'rb') as f:
            d = pickle.load(f)
        if not isinstance(d, dict) or 'params' not in d or 'optimizer' not in d:
            raise ValueError("%s is not a trainer checkpoint (a parameter list goes to set_params)" % path)
        # every shape is checked before anything is written
        for arrays in (d['params'],) + tuple(d['optimizer']['slots']):
            self._check_shapes(arrays)
        self.set_params(d['params'])
        self.load_optimizer_state(d['optimizer'])

    @_on_ctx_stream
    def forward(self, inputs):
        """``lasagne.layers.get_output`` of the network: the output channels ``[B, channels_out, tc, F]`` before masking
        (device tensor)."""
        torch = require_gpu()
        x, _ = self._io(inputs)
        p = torch.empty(self._t_shape, dtype=torch.float32, device=self.ctx.device)
        _lib.check(self.ctx._lib.dcs_trainer_forward(self._h, _ptr(x), _ptr(p)))
        return p

    def save_model(self, path):
        """The reference's ``save_model``: the pickled parameter list that ``Network(arch, ...)``, ``Separator(arch, ...)``
        and the separate_*.py scripts load (``arch.resolve`` tells the layouts apart by their shapes)."""
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


class Trainer(TrainerHandle):
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
        if arch == 'ikala_nopool':
            eps = IKALA_EPS if eps is EPS else eps
            alpha = IKALA_ALPHA if alpha is ALPHA else alpha
            beta = IKALA_BETA_ACC if beta is BETA else beta
            beta_voc = IKALA_BETA_VOC if beta_voc is BETA_VOC else beta_voc
        elif arch == 'bach10':
            eps = BACH10_EPS if eps is EPS else eps
        self.S = n_sources(arch)
        # an arch without a code goes to the library as -1: dcs_trainer_create refuses what it cannot train
        TrainerHandle.__init__(self, ctx, arch, 1, self.S, batch_size, time_context, feat_size,
                               (int(batch_size), 1, int(time_context), int(feat_size)), params, rand, seed,
                               (eps, alpha, beta, beta_voc, learning_rate, rho, epsilon),
                               code=ARCHS[arch].code if arch in ARCHS else -1)

    def _default_params(self, seed):
        return glorot_init(self.arch, self.tc, self.F, seed)

    def losses(self, inputs, targets):
        """``train_fn1`` (trainCNN.py:263): vocals, bass, drums, negative, alpha, negative_voc at the current parameters;
        iKala (ikala/trainCNN.py:197): vocals_error, acc_error, negative_error_voc, negative_error_acc; Bach10
        (bach10/trainCNNbach10.py:206): error1 .. error4 (bassoon, clarinet, saxophone, violin)."""
        n = {'dsd': len(COMPONENTS), 'bach10': len(BACH10_COMPONENTS)}.get(self.arch, len(IKALA_COMPONENTS))
        return [float(v) for v in self.ctx.to_host(self.run(inputs, targets, 0))[1:1 + n]]


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


def listed_files(paths):
    """``paths`` (files or directories) as a list of files: a directory stands for the files in it."""
    files = []
    for p in paths:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in os.listdir(p)]
        else:
            files.append(p)
    return files


class WindowFeed(object):
    """What the window feeds share: the slot table over a list of files (real or virtual), the seeded epoch order and the
    context that is only opened when the first batch is cut.

    A subclass validates its files, hands their frame counts to :meth:`_set_table`, uploads its data in ``_upload`` (which
    starts with :meth:`_open`) and cuts a batch in ``gather(rows)`` with one library call on the tensors of
    :meth:`_batch`."""

    def __init__(self, windows, time_context, overlap, batch_size, seed, ctx):
        if windows not in ('reference', 'all'):
            raise ValueError("windows must be 'reference' or 'all'")
        self._slots = reference_slots if windows == 'reference' else all_slots
        self.tc, self.overlap, self.batch_size, self.seed = int(time_context), int(overlap), int(batch_size), int(seed)
        self._ctx = ctx

    def _set_table(self, frames):
        """``table`` [total, 2] int32 = (file, window start) of every slot of files of ``frames`` frames each; file -1: a
        slot the reference never fills (an all-zero window)."""
        table = []
        for i, T in enumerate(frames):
            table += [(i if s is not None else -1, s if s is not None else 0) for s in self._slots(int(T), self.tc, self.overlap)]
        self.table = np.asarray(table, dtype=np.int32).reshape(-1, 2)
        self.total = len(self.table)
        self.iteration_size = self.total // self.batch_size

    def _open(self):
        self.ctx = self._ctx if self._ctx is not None else default_context()

    def _batch(self, rows, channels_in, channels_out):
        """Inside ``ctx.stream_scope()``: the table rows ``rows`` on the device, their count B, and uninitialised inputs
        ``[B, channels_in, tc, F]`` and targets ``[B, channels_out, tc, F]``."""
        import torch
        win = np.ascontiguousarray(self.table[np.asarray(rows, dtype=np.int64)])
        B = len(win)
        win_d = torch.from_numpy(win).to(self.ctx.device)
        x = torch.empty((B, channels_in, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
        t = torch.empty((B, channels_out, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
        return win_d, B, x, t

    def batches(self, epoch=0):
        perm = np.random.RandomState(self.seed + epoch).permutation(self.total)
        for b in range(self.iteration_size):
            yield self.gather(perm[b * self.batch_size:(b + 1) * self.batch_size])


class RenderedFeed(WindowFeed):
    """What the feeds share that render and transform their windows per batch (``augment.RenderedWindows``,
    ``score_render.ScoreRenderedWindows``): the scale, the track count ``sources`` of the virtual files ``files``, ``F``, and
    the ``StftPlan``, made with the context (``window``: an array or a function of the frame size, default blackmanharris)."""

    def __init__(self, files, mult_factor, frameSize, hopSize, window, *feed):
        WindowFeed.__init__(self, *feed)
        self.mult = float(mult_factor)
        self.frame, self.hop, self._window = int(frameSize), int(hopSize), window
        counts = set(len(f.tracks) for f in files)
        if len(counts) != 1:
            raise ValueError("virtual files disagree on the number of tracks: %r" % sorted(counts))
        self.sources = counts.pop()
        if not 1 <= self.sources <= 8:
            raise ValueError("1 .. 8 tracks per virtual file, got %d" % self.sources)
        self.F = self.frame // 2 + 1

    def _open(self):
        WindowFeed._open(self)
        win = self._window if self._window is not None else blackmanharris
        self._plan = StftPlan(self.ctx, self.frame, self.hop, win(self.frame) if callable(win) else win)


class FeatureWindows(WindowFeed):
    """The training data of ``LargeDataset`` (dataset.py) resident on the device.

    ``paths``: ``.data`` files of float64 ``[1 + sources, T, F]`` (each with its ``.shape``): by default ``[5, T, F]``
    (mixture, vocals, bass, drums, other) as examples/dsd100/compute_features.py writes them; ``sources=2``: ``[3, T, F]``
    (mixture, voice, accompaniment) as examples/ikala/compute_features.py writes them.  ``windows='reference'`` reproduces loadFile's slots, zero slots
    included (at tc 30 / overlap 25 only about the first third of each 30 s chunk is used); ``'all'`` takes every full
    window.  ``batches(epoch)`` yields ``total // batch_size`` batches in the order of ``RandomState(seed + epoch)
    .permutation`` -- seeded, where the reference's shuffle is not."""

    def __init__(self, paths, time_context=30, overlap=25, mult_factor=0.3, windows='reference', batch_size=32, seed=0,
                 ctx=None, sources=4):
        WindowFeed.__init__(self, windows, time_context, overlap, batch_size, seed, ctx)
        self.sources = int(sources)
        if not 1 <= self.sources <= 8:
            raise ValueError("sources must be 1 .. 8, got %r" % (sources,))
        self.mult = float(mult_factor)
        self.paths = list(paths)
        self.shapes = []
        for p in self.paths:
            shp = read_shape_file(p.replace('.data', '.shape'))
            if len(shp) != 3 or shp[0] != 1 + self.sources:
                raise ValueError("%s: shape %r, expected (%d, T, F)" % (p, shp, 1 + self.sources))
            self.shapes.append(shp)
        if len(set(s[2] for s in self.shapes)) > 1:
            raise ValueError("feature files disagree on F: %r" % sorted(set(s[2] for s in self.shapes)))
        self.F = self.shapes[0][2] if self.shapes else 0
        self._set_table(s[1] for s in self.shapes)

    def _upload(self):
        if getattr(self, "_data", None) is not None:
            return
        self._open()
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
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, 1, self.sources)
            if self.sources == 4:
                _lib.check(self.ctx._lib.dcs_trainer_gather(self.ctx._h, _ptr(self._data), _ptr(self._files), _ptr(win_d), B,
                                                            self.tc, self.F, self.mult, _ptr(x), _ptr(t)))
            else:
                _lib.check(self.ctx._lib.dcs_trainer_gather_sources(self.ctx._h, _ptr(self._data), _ptr(self._files),
                                                                    _ptr(win_d), B, self.tc, self.F, self.sources,
                                                                    self.mult, _ptr(x), _ptr(t)))
        return x, t
