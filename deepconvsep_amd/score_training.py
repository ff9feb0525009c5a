"""Training of the score-informed Bach10 graph on the MI355X: the first half of ``train_auto`` of
examples/bach10_scoreinformed/trainCNNrwc.py (``--function build_ca``, :134-193 and :225-344; trainCNNrwc_samp.py trains the
single-branch form of the same graph with the same loss) and the data feed of ``dataset.LargeDatasetMask2`` (dataset.py:
819-879 on :383-488) with the products of trainCNNrwc.py:309-320.

``ScoreTrainer`` has the surface of :class:`deepconvsep_amd.training.Trainer`: four input channels (the mixture times the four
harmonic masks), four targets, ``branches=4`` the 17-array ``.pkl`` layout ``'bach10_si'``, ``branches=1`` the 11-array layout
``'bach10_si1'`` (csrc/train_bach10si.hip on the shared build_ca graph csrc/train_ca.hip and the core csrc/train_core.hip).  Both train the
same live computation: the loss reads ``prediction2[:, 0:4]``, the four channels of decoder branch 0.  The 17-array layout's ``fc12``, ``fc13``, ``fc14``
(arrays 10 .. 15) and ``bo[4:16]`` get an exactly zero gradient in the reference, so Adadelta never moves them: the trainer
returns them as they were given, and zeros for their gradients and accumulators.  The handle itself is
:class:`deepconvsep_amd.training.TrainerHandle`; the class adds the choice of layout (``arch_name``) and ``rectify_codes``.
``training.TRAINABLE`` lists the mono graphs only.

``function='build_ca_1x1'`` trains the deep graph of trainCNNrwc.py:66-132 instead (csrc/train_deep1x1.hip): 22 arrays, the
``.pkl`` layout ``'bach10_si_1x1'`` that ``arch.resolve`` tells apart, with ``branches`` 4 (the whole graph) or 1 .. 3 (the
live-only layouts).  Its loss reads branch 0 too: rows 200 .. 799 of the 1x1 layer and ``fb[4:16]`` are dead in the same sense.

``ScoreFeatureWindows`` keeps the ``[5, T, F]`` feature files and their note tables resident on the device and cuts the
reference's windows, masks included, in one launch per batch (slot table and epoch order:
:class:`deepconvsep_amd.training.WindowFeed`).  There is no CPU fallback.
"""
import os
from ctypes import c_void_p

import numpy as np

from . import _lib
from .arch import ARCHS
from .runtime import _on_ctx_stream, _ptr, require_gpu
from .training import (ADA_EPSILON, BACH10_COMPONENTS, BACH10_EPS, LEARNING_RATE, RHO, TrainerHandle, WindowFeed,
                       glorot_arrays, listed_files)
from .transform import read_shape_file

CHANNELS, N_SOURCES = 4, 4
COMPONENTS = BACH10_COMPONENTS           # trainCNNrwc.py:336-339
SI_EPS = BACH10_EPS                      # trainCNNrwc.py:235


FUNCTIONS = ('build_ca', 'build_ca_1x1')     # trainCNNrwc.py --function


def arch_name(branches, function='build_ca'):
    if function not in FUNCTIONS:
        raise ValueError("function must be one of %r, got %r" % (FUNCTIONS, function))
    if function == 'build_ca_1x1':
        if branches not in (1, 2, 3, 4):
            raise ValueError("branches must be 4 (the whole graph) or 1 .. 3 (live-only layouts), got %r" % (branches,))
        return 'bach10_si_1x1'
    if branches not in (1, 4):
        raise ValueError("branches must be 4 (the 17-array layout) or 1 (the 11-array layout), got %r" % (branches,))
    return 'bach10_si' if branches == 4 else 'bach10_si1'


def param_shapes(tc, F, branches=4, function='build_ca'):
    """The .pkl shapes of build_ca: 17 arrays (trainCNNrwc.py:134-193) or, ``branches=1``, 11 (trainCNNrwc_samp.py:195-235);
    of build_ca_1x1: 22 arrays (:66-132), the 1x1 layer and the final bias cut to ``branches`` branches."""
    if arch_name(branches, function) == 'bach10_si_1x1':
        return [tuple(s) for s in ARCHS['bach10_si_1x1'].param_shapes(tc, F, branches=branches)]
    return [tuple(s) for s in ARCHS[arch_name(branches)].param_shapes(tc, F)]


def glorot_init(tc=30, F=2049, seed=0, branches=4, function='build_ca'):
    """Lasagne's defaults for build_ca: every W ``GlorotUniform(gain=1)`` -- uniform in +-sqrt(3) * sqrt(2 / ((n1 + n2) *
    receptive field)) with (n1, n2) the first two axes -- and every bias ``Constant(0)``; float32."""
    return glorot_arrays(param_shapes(tc, F, branches, function), seed)


class ScoreTrainer(TrainerHandle):
    """``train_fn`` / ``train_fn1`` of trainCNNrwc.py:281-283, resident on one GPU.

    ``params``: the 17 (``branches=4``) or 11 (``branches=1``) arrays in .pkl order, default :func:`glorot_init`.  ``rand``:
    the uniform draw of :246 ``[batch, 1, tc, F]``; default ``RandomState(seed).uniform``.  The batch size is fixed, as in
    the reference's compiled graph.  ``forward`` returns ``get_output(network2)[:, 0:4]`` (:244-251), the live channels;
    ``save_model`` (:59-64) writes the list ``Separator('bach10_si', ...)`` and
    examples/bach10_scoreinformed/separate_bach10.py load (17 arrays, or 11: resolved to ``'bach10_si1'``)."""

    def __init__(self, ctx=None, params=None, branches=4, batch_size=32, time_context=30, feat_size=2049, seed=0, rand=None,
                 eps=SI_EPS, learning_rate=LEARNING_RATE, rho=RHO, epsilon=ADA_EPSILON, function='build_ca'):
        self.branches = int(branches)
        self.function = function
        self.arch = arch_name(self.branches, function)
        if self.arch == 'bach10_si_1x1':
            ARCHS[self.arch].dims(int(time_context), int(feat_size))   # ValueError below time_context 19 / feat_size 253
        self.C, self.S = CHANNELS, N_SOURCES
        TrainerHandle.__init__(self, ctx, self.arch, self.C, self.S, batch_size, time_context, feat_size,
                               (int(batch_size), 1, int(time_context), int(feat_size)), params, rand, seed,
                               (eps, 0.0, 0.0, 0.0, learning_rate, rho, epsilon))

    def _default_params(self, seed):
        return glorot_init(self.tc, self.F, seed, self.branches, self.function)

    def losses(self, inputs, targets):
        """``train_fn1`` (trainCNNrwc.py:283): error1 .. error4 (bassoon, clarinet, saxophone, violin)."""
        return [float(v) for v in self.ctx.to_host(self.run(inputs, targets, 0))[1:1 + self.S]]

    @_on_ctx_stream
    def rectify_codes(self):
        """``build_ca_1x1`` only: r'(pre) of the last step's seven rectified layers (conv1 .. conv6, the live rows of the 1x1
        layer) as float32 arrays ``[B, C, H, W]`` of 0 / 0.5 / 1 (0.5: a pre-activation of exactly 0)."""
        torch = require_gpu()
        if self.arch != 'bach10_si_1x1':
            raise NotImplementedError("rectify_codes: only the build_ca_1x1 trainer keeps its rectifier codes")
        a = ARCHS[self.arch]
        d = a.dims(self.tc, self.F)
        shapes = [(self.B, l['cout'], l['ho'], l['wo']) for l in d['layers']] + [(self.B, a.nf, d['h6'], d['w6'])]
        outs = [torch.empty(s, dtype=torch.float32, device=self.ctx.device) for s in shapes]
        ptrs = (c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        _lib.check(self.ctx._lib.dcs_trainer_rectify_codes(self._h, ptrs, len(outs)))
        return [o.cpu().numpy() for o in outs]


def score_pairs(paths, pitch_code='e'):
    """The ``(features, note table)`` file pairs of ``LargeDataset`` (dataset.py:617-619 and loadPitch :361-364): every file
    of ``paths`` (files or directories) that ends in ``_m_.data``, with ``_m_`` replaced by ``_<pitch_code>_`` for its note
    table; sorted."""
    pairs = []
    for f in sorted(listed_files(paths)):
        if not f.endswith('_m_.data'):
            continue
        d, name = os.path.split(f)
        notes = os.path.join(d, name.replace('_m_', '_' + pitch_code + '_'))
        if not os.path.isfile(notes):
            raise IOError("%s: no note table %s" % (f, notes))
        pairs.append((f, notes))
    return pairs


def pack_notes(lib, notes, F):
    """``dcs_trainer_pack_score``: one file's ``[ninst, P, W]`` note table as the feed kernel's ``[ninst, P, W - 1]`` int32
    table.  A harmonic band outside ``[0, F)`` raises ValueError (DCS_ESHAPE)."""
    notes = np.ascontiguousarray(notes, dtype=np.float64)
    if notes.ndim != 3:
        raise ValueError("notes must be [instruments, notes, 2*nharmonics+3]")
    ninst, P, W = notes.shape
    out = np.zeros((ninst, P, max(W - 1, 1)), dtype=np.int32)
    _lib.check(lib.dcs_trainer_pack_score(notes.ctypes.data_as(c_void_p), ninst, P, W, int(F), out.ctypes.data_as(c_void_p)))
    return out


class ScoreFeatureWindows(WindowFeed):
    """The training data of ``LargeDatasetMask2`` (dataset.py:819-879) resident on the device.

    ``paths``: feature directories or ``*_m_.data`` files, float64 ``[5, T, F]`` (mixture, bassoon, clarinet, saxophone,
    violin), each with its note table ``*_<pitch_code>_.data`` ``[4, P, 2 * nharmonics + 3]`` next to it, as
    examples/bach10_scoreinformed/compute_features.py writes them (trainCNNrwc.py:658 trains from ``'e'``).  Slots as for
    :class:`deepconvsep_amd.training.FeatureWindows`.  ``gather(rows)`` returns the network's inputs ``[B, 4, tc, F]`` --
    ``mask_j * (mult_factor * mixture)``, the masks those of ``filterSpec`` for the window -- and the targets
    ``[B, 4, tc, F]``; ``batches(epoch)`` yields ``total // batch_size`` batches in the order of ``RandomState(seed + epoch)
    .permutation`` -- seeded, where the reference's shuffle is not.  The timbre-model branch of ``filterSpec`` is not part of
    the feed (``score.timbre_masks`` computes it on the host)."""

    def __init__(self, paths, pitch_code='e', time_context=30, overlap=25, mult_factor=0.3, windows='reference',
                 batch_size=32, seed=0, ctx=None):
        WindowFeed.__init__(self, windows, time_context, overlap, batch_size, seed, ctx)
        self.mult = float(mult_factor)
        self.pitch_code = pitch_code
        self.pairs = score_pairs([paths] if isinstance(paths, str) else list(paths), pitch_code)
        self.shapes, self.note_shapes = [], []
        for p, q in self.pairs:
            shp = read_shape_file(p.replace('.data', '.shape'))
            nshp = read_shape_file(q.replace('.data', '.shape'))
            if len(shp) != 3 or len(nshp) != 3 or shp[0] != 1 + nshp[0]:
                raise ValueError("%s: shapes %r / %r, expected (1 + ninst, T, F) / (ninst, P, W)" % (p, shp, nshp))
            self.shapes.append(tuple(shp))
            self.note_shapes.append(tuple(nshp))
        for k, what in ((0, "channels"), (2, "F")):
            if len(set(s[k] for s in self.shapes)) > 1:
                raise ValueError("feature files disagree on %s" % what)
        if len(set(s[2] for s in self.note_shapes)) > 1:
            raise ValueError("note tables disagree on their width")
        self.ninst = self.note_shapes[0][0] if self.shapes else 0
        self.width = self.note_shapes[0][2] if self.shapes else 0
        if self.shapes and (not 1 <= self.ninst <= 32 or self.width < 5 or self.width % 2 == 0):
            raise ValueError("ninst %d (1 .. 32), note table width %d (odd, from 5)" % (self.ninst, self.width))
        self.F = self.shapes[0][2] if self.shapes else 0
        self._set_table(s[1] for s in self.shapes)

    def _upload(self):
        if getattr(self, "_data", None) is not None:
            return
        self._open()
        blocks, files, off = [], [], 0
        packed, note_files, noff = [], [], 0
        for (p, q), shp, nshp in zip(self.pairs, self.shapes, self.note_shapes):
            a = np.fromfile(p, dtype=np.float64).reshape(shp).astype(np.float32)
            blocks.append(a.ravel())
            files.append((off, shp[1]))
            off += a.size
            t = pack_notes(self.ctx._lib, np.fromfile(q, dtype=np.float64).reshape(nshp), self.F)
            packed.append(t.ravel())
            note_files.append((noff, nshp[1]))
            noff += t.size
        self._data = self.ctx.to_device(np.concatenate(blocks) if blocks else np.zeros(1, np.float32), np.float32)
        with self.ctx.stream_scope():
            import torch
            self._files = torch.from_numpy(np.asarray(files, dtype=np.int64).reshape(-1, 2)).to(self.ctx.device)
            self._notes = torch.from_numpy(np.concatenate(packed + [np.zeros(1, np.int32)])).to(self.ctx.device)
            self._note_files = torch.from_numpy(np.asarray(note_files, dtype=np.int64).reshape(-1, 2)).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, ninst, tc, F]`` and targets ``[B, ninst, tc, F]`` (device tensors) of the window-table rows ``rows``."""
        self._upload()
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, self.ninst, self.ninst)
            _lib.check(self.ctx._lib.dcs_trainer_gather_score(self.ctx._h, _ptr(self._data), _ptr(self._files),
                                                              _ptr(self._notes), _ptr(self._note_files), _ptr(win_d), B,
                                                              self.tc, self.F, self.ninst, self.width, self.mult, _ptr(x),
                                                              _ptr(t)))
        return x, t
