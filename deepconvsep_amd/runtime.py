"""Thin object layer over the C ABI: Context, StftPlan, Network.

PyTorch-ROCm is used for exactly three things here: allocating device memory
(``torch.empty(..., device='cuda')``), host<->device copies, and naming the HIP
stream the kernels run on.  No torch operator computes anything on the path.
"""
import ctypes
from ctypes import POINTER, byref, c_double, c_int64, c_void_p

import numpy as np

from . import _lib
from .arch import (ARCHS, EPS_A, EPS_B, TIE_ALL, TIE_FIRST, TILER_LIBRARY, TILER_SCRIPT, check_params, live_params,
                   resolve as resolve_arch)
from .streaming import stereo_ld


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("deepconvsep_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                           "and there is no CPU fallback")
    return torch


def _on_ctx_stream(method):
    """Run a method of an object with a ``.ctx`` inside ``torch.cuda.stream(ctx.torch_stream)``: the tensors it
    allocates belong to that stream in torch's caching allocator and the copies it issues are ordered with the
    kernels libdcs enqueues there, whatever stream is current in the caller."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with self.ctx.stream_scope():
            return method(self, *args, **kwargs)
    return wrapper


class Context(object):
    """One device + one HIP stream (``dcs_ctx``).

    The stream is the one current on ``device`` when the context is made (or ``stream=``); it is kept as a
    ``torch.cuda.Stream`` so that every host<->device copy, allocation and ``.cpu()`` the package issues runs on the
    stream the kernels run on (:meth:`stream_scope`).  A caller that produces inputs or consumes outputs on another
    stream synchronises with :attr:`torch_stream` as with any torch stream."""

    def __init__(self, device=None, stream=None):
        torch = require_gpu()
        lib = _lib.load()
        if device is None:
            device = stream.device.index if stream is not None else torch.cuda.current_device()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self.torch_stream = stream if stream is not None else torch.cuda.current_stream(self.device_index)
        if self.torch_stream.device.index != self.device_index:
            raise ValueError("stream belongs to device %d, context to device %d"
                             % (self.torch_stream.device.index, self.device_index))
        h = c_void_p()
        _lib.check(lib.dcs_create(self.device_index, c_void_p(self.torch_stream.cuda_stream), byref(h)))
        self._h = h
        self._lib = lib

    def stream_scope(self):
        """``with ctx.stream_scope():`` makes the context's stream torch's current stream."""
        return _torch().cuda.stream(self.torch_stream)

    # -- memory plumbing ------------------------------------------------------------------
    def to_device(self, array, dtype):
        torch = _torch()
        a = np.ascontiguousarray(array, dtype=dtype)
        with self.stream_scope():
            return torch.from_numpy(a).to(self.device)

    def to_host(self, tensor):
        """Device tensor -> ndarray, ordered after everything enqueued on the context's stream."""
        with self.stream_scope():
            return tensor.cpu().numpy()

    def empty(self, shape, dtype):
        torch = _torch()
        tdt = {np.float32: torch.float32, np.float64: torch.float64}[dtype]
        with self.stream_scope():
            return torch.empty(tuple(int(s) for s in shape), dtype=tdt, device=self.device)

    def synchronize(self):
        _lib.check(self._lib.dcs_synchronize(self._h))

    def check_guards(self):
        """``dcs_debug_check_guards``: with ``DCS_WS_GUARD=<bytes>`` in the environment, verify the red zones around every
        device block libdcs holds -- scratch, model weights and their packed copies, plan tables, ramps (raises on damage,
        naming the block); returns the number of guarded blocks."""
        n = c_int64()
        _lib.check(self._lib.dcs_debug_check_guards(self._h, byref(n)))
        return n.value

    # -- multichannel Wiener filter ----------------------------------------------------------------
    def mwf(self, mag, phase, src, niter, pre_div=1.0, eps=1e-10):
        """``dcs_mwf_f32``: ``niter`` EM iterations of the multichannel Wiener filter (time-invariant full-rank spatial
        covariances) on float32 device tensors.  ``mag``, ``phase`` ``[2, T, F]`` (the mixture), ``src`` ``[2, J, T, F]``
        (per-channel source magnitudes, divided by ``pre_div`` before use) -> (magnitudes, phases), both ``[2, J, T, F]``.
        ``niter=0`` returns ``src / pre_div`` and the mixture's phases."""
        torch = _torch()
        if mag.dim() != 3 or src.dim() != 4 or mag.shape[0] != 2 or src.shape[0] != 2 or tuple(phase.shape) != tuple(mag.shape) \
                or tuple(src.shape[2:]) != tuple(mag.shape[1:]):
            raise ValueError("mwf expects mag, phase [2, T, F] and src [2, J, T, F], got %r, %r, %r"
                             % (tuple(mag.shape), tuple(phase.shape), tuple(src.shape)))
        if any(t.dtype != torch.float32 or t.device != self.device for t in (mag, phase, src)):
            raise ValueError("mwf expects float32 tensors on %s" % (self.device,))
        with self.stream_scope():
            mag, phase, src = mag.contiguous(), phase.contiguous(), src.contiguous()
            J, T, F = (int(x) for x in src.shape[1:])
            out_mag = torch.empty((2, J, T, F), dtype=torch.float32, device=src.device)
            out_phase = torch.empty((2, J, T, F), dtype=torch.float32, device=src.device)
            _lib.check(self._lib.dcs_mwf_f32(self._h, _ptr(mag), _ptr(phase), T * F, _ptr(src), J * T * F, T * F, F, T, F, J,
                                             int(niter), float(pre_div), float(eps), _ptr(out_mag), _ptr(out_phase)))
        return out_mag, out_phase

    # -- sample-rate conversion ----------------------------------------------------------------------
    def resampler(self, fi, fo, **design):
        """The :class:`deepconvsep_amd.resample.Resampler` of ``fi -> fo`` Hz (``design``: ``zero_crossings``, ``beta``,
        ``rolloff``), made on first use and kept with the context."""
        from .resample import Resampler
        key = (int(fi), int(fo)) + tuple(sorted(design.items()))
        cache = self.__dict__.setdefault("_resamplers", {})
        if key not in cache:
            cache[key] = Resampler(self, fi, fo, **design)
        return cache[key]

    # -- kernel timing (bench.py) ---------------------------------------------------------------
    def timing_stride(self, stride):
        _lib.check(self._lib.dcs_timing_stride(self._h, int(stride)))

    def timing(self, tags):
        """Bracket the kernels of the named tags (``_lib.TAGS`` keys; ``'all'``; ``None`` = off) with HIP events.  ``'all'``
        is every tag ``_lib.TAGS`` names: not ``DCS_TAG_BSS_CORR`` / ``DCS_TAG_BSS_CHOL`` (15, 16), which
        ``scripts/bench_bsseval.py`` enables by number."""
        if not tags:
            mask = 0
        elif tags == 'all':
            mask = 0
            for t in _lib.TAGS.values():
                mask |= 1 << t
        else:
            mask = 0
            for t in tags:
                mask |= 1 << _lib.TAGS[t]
        _lib.check(self._lib.dcs_timing_enable(self._h, mask))

    def timing_reset(self):
        _lib.check(self._lib.dcs_timing_reset(self._h))

    def timing_query(self, tag):
        ms, cnt = c_double(), c_int64()
        _lib.check(self._lib.dcs_timing_query(self._h, _lib.TAGS[tag], byref(ms), byref(cnt)))
        return ms.value, cnt.value

    def close(self):
        if getattr(self, "_h", None):
            for rs in self.__dict__.pop("_resamplers", {}).values():
                rs.close()
            self._lib.dcs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=None):
    torch = require_gpu()
    idx = torch.cuda.current_device() if device is None else int(device)
    if idx not in _default_ctx:
        _default_ctx[idx] = Context(idx)
    return _default_ctx[idx]


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(None)


class StftPlan(object):
    """``dcs_stft``: window + twiddle tables for one (frameSize, hopSize, window)."""

    def __init__(self, ctx, frame, hop, window):
        self.ctx = ctx
        self.frame, self.hop = int(frame), int(hop)
        self.bins = self.frame // 2 + 1
        w = np.ascontiguousarray(window, dtype=np.float64)
        if w.shape != (self.frame,):
            raise ValueError("window must have frameSize=%d samples, got %r" % (self.frame, w.shape))
        self.window = w
        h = c_void_p()
        _lib.check(ctx._lib.dcs_stft_plan(ctx._h, self.frame, self.hop, w.ctypes.data_as(POINTER(c_double)), byref(h)))
        self._h = h

    @_on_ctx_stream
    def forward(self, audio_t, phase=True, rows_out=None, ld=None):
        """audio_t: 1-D float32/float64 device tensor.  Returns (mag, phase|None) device tensors
        ``[rows_out, ld]`` (defaults: the reference's dense ``[T, bins]``)."""
        torch = _torch()
        L = int(audio_t.numel())
        T = _lib.frame_count(L, self.hop)
        rows = T if rows_out is None else int(rows_out)
        ld = self.bins if ld is None else int(ld)
        f64 = audio_t.dtype == torch.float64
        mag = torch.empty((rows, ld), dtype=audio_t.dtype, device=audio_t.device)
        ph = torch.empty((rows, ld), dtype=audio_t.dtype, device=audio_t.device) if phase else None
        fn = self.ctx._lib.dcs_stft_forward_f64 if f64 else self.ctx._lib.dcs_stft_forward_f32
        _lib.check(fn(self._h, _ptr(audio_t), L, _ptr(mag), _ptr(ph), ld, rows))
        return mag, ph

    @_on_ctx_stream
    def forward_clips(self, audio_t, phase=True, mag_out=None, phase_out=None):
        """``compute_transform`` (transform.py:80-131): audio_t ``[clips, samples]`` float32 / float64 device tensor (rows
        contiguous) -> (mag, phase|None) ``[clips, T, bins]`` from ONE launch (``dcs_stft_forward_f32/f64_clips``)."""
        torch = _torch()
        if audio_t.dim() != 2 or audio_t.stride(1) != 1:
            raise ValueError("forward_clips expects a [clips, samples] tensor with contiguous rows")
        B, L = int(audio_t.shape[0]), int(audio_t.shape[1])
        T = _lib.frame_count(L, self.hop)
        f64 = audio_t.dtype == torch.float64
        mag = mag_out if mag_out is not None else torch.empty((B, T, self.bins), dtype=audio_t.dtype, device=audio_t.device)
        ph = None
        if phase:
            ph = phase_out if phase_out is not None else torch.empty((B, T, self.bins), dtype=audio_t.dtype, device=audio_t.device)
        fn = self.ctx._lib.dcs_stft_forward_f64_clips if f64 else self.ctx._lib.dcs_stft_forward_f32_clips
        _lib.check(fn(self._h, _ptr(audio_t), L, B, int(audio_t.stride(0)), _ptr(mag), _ptr(ph), self.bins, T))
        return mag, ph

    @_on_ctx_stream
    def inverse(self, mag_t, phase_t, n_out=None, pre_div=1.0, out=None):
        """mag_t ``[S, T, ld]`` or ``[T, ld]``, phase_t ``[T, ld]`` (same ld).  Returns ``[S, n_out]``
        (or ``[n_out]``), written into ``out`` (contiguous ``[S, n_out]``, same dtype) when given."""
        torch = _torch()
        squeeze = mag_t.dim() == 2
        if squeeze:
            mag_t = mag_t.unsqueeze(0)
        S, T, ld = (int(x) for x in mag_t.shape)
        if tuple(phase_t.shape) != (T, ld):
            raise ValueError("phase shape %r does not match magnitude %r" % (tuple(phase_t.shape), (T, ld)))
        mag_t = mag_t.contiguous()
        phase_t = phase_t.contiguous()
        full = _lib.inverse_length(T, self.hop, self.frame)
        n_out = full if n_out is None else min(int(n_out), full)
        if out is None:
            out = torch.empty((S, n_out), dtype=mag_t.dtype, device=mag_t.device)
        elif tuple(out.shape) != (S, n_out) or out.dtype != mag_t.dtype or not out.is_contiguous():
            raise ValueError("out must be a contiguous %r tensor of the magnitudes' dtype" % ((S, n_out),))
        if mag_t.dtype == torch.float64:
            _lib.check(self.ctx._lib.dcs_stft_inverse_f64(self._h, _ptr(mag_t), T * ld, _ptr(phase_t), ld, T, S,
                                                          float(pre_div), _ptr(out), n_out))
        else:
            _lib.check(self.ctx._lib.dcs_stft_inverse_f32(self._h, _ptr(mag_t), T * ld, _ptr(phase_t), ld, T, S,
                                                          float(pre_div), _ptr(out), n_out))
        return out[0] if squeeze else out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_stft_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Network(object):
    """``dcs_model``: one ``build_ca`` graph with its parameters resident in HBM.

    ``params`` is the list ``lasagne.layers.get_all_param_values`` pickled by the reference's
    trainers (examples/dsd100/trainCNN.py:59-64); a count/shape mismatch raises ``ValueError``
    like ``set_all_param_values`` does (examples/dsd100/separate_dsd.py:250).
    """

    def __init__(self, ctx, arch, params, time_context=30, feat_size=513, live_only=True):
        self.ctx = ctx
        self.tc, self.F = int(time_context), int(feat_size)
        params = [np.asarray(p) for p in params]
        # 'ikala': pooled or trainer (no-pool) graph by fc.W; 'bach10_si': 17-array or single-branch 11-array graph by count
        self.arch = resolve_arch(arch, params, self.tc, self.F)
        check_params(self.arch, params, self.tc, self.F)
        self.graph_arch = self.arch                                  # the graph the .pkl belongs to
        if live_only:
            # the 17-array score-informed graph: three of its four decoder branches never reach predict_function2 -- they are
            # neither uploaded nor allocated (3 x 171 MB of dense weights at 2049 bins); forward_raw then returns the four
            # live channels.  live_only=False keeps the whole graph (what lasagne.layers.get_output would evaluate).
            self.arch, params = live_params(self.arch, params)
        # weight tensors hosted by torch (float32, as the pickles store them)
        self._params = [ctx.to_device(p, np.float32) for p in params]
        n = len(self._params)
        ptrs = (c_void_p * n)(*[p.data_ptr() for p in self._params])
        shapes = (c_int64 * (4 * n))()
        for i, p in enumerate(params):
            shp = list(p.shape) + [1] * (4 - p.ndim)
            for k in range(4):
                shapes[4 * i + k] = shp[k]
        h = c_void_p()
        _lib.check(ctx._lib.dcs_model_create(ctx._h, self.arch.code, self.arch.C, self.tc, self.F, ptrs, shapes, n,
                                             byref(h)))
        self._h = h
        self.S = int(ctx._lib.dcs_model_num_sources(h))
        self.out_channels = int(ctx._lib.dcs_model_out_channels(h))

    def final_kernel(self, n_frames, n_clips=1, eps_mode=None):
        """Which kernel the fused path runs for the last decoder stage on a launch of this size: ``'f32x64'``,
        ``'f32x128'``, ``'bf16x3'`` or ``'one_batch'`` (the kernel of csrc/dsd_lat.hip a single short clip takes) -- ``dcs_model_final_kernel``; None for graphs
        without a fused decoder."""
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        code = int(self.ctx._lib.dcs_model_final_kernel(self._h, int(n_frames), int(n_clips), int(eps)))
        return {0: 'f32x64', 1: 'f32x128', 2: 'bf16x3', 3: 'one_batch'}.get(code)

    def set_latency_stages(self, stages):
        """Stages of the fused path that run on the one-batch kernels (``dcs_model_set_latency_stages``): -1 automatic,
        0 none, else bits 1 STFT, 2 conv1, 4 conv2, 8 bottleneck, 16 per-source dense, 32 transposed conv2, 64 final,
        128 iSTFT."""
        _lib.check(self.ctx._lib.dcs_model_set_latency_stages(self._h, int(stages)))

    def set_score_semantics(self, normalise='max', mixture='ch0'):
        """Score-informed graphs: ``normalise`` ``'max'`` (the separate script: every instrument's harmonic mask divided by
        its own maximum, separate_bach10.py:195) or ``'sum'`` (the trainers' dataset class: by the sum over the instruments,
        dataset.py:862); ``mixture`` ``'ch0'`` (script: soft masks x input channel 0, :485) or ``'sum'`` (trainers: x the sum
        of the input channels, trainCNNrwc.py:258-263).  ``dcs_model_set_score_semantics``."""
        try:
            n, m = {'max': 0, 'sum': 1}[normalise], {'ch0': 0, 'sum': 1}[mixture]
        except KeyError:
            raise ValueError("normalise must be 'max' or 'sum', mixture 'ch0' or 'sum'")
        _lib.check(self.ctx._lib.dcs_model_set_score_semantics(self._h, n, m))
        self.score_normalise, self.score_mixture = normalise, mixture

    def set_conv_precision(self, dtype):
        """``'f16'``: conv2 and its transpose use f16-input / f32-accumulate MFMA (BASELINE config 3);
        ``'f32'`` (default): exact f32."""
        if dtype not in ('f16', 'f32'):
            raise ValueError("conv precision must be 'f16' or 'f32'")
        _lib.check(self.ctx._lib.dcs_model_set_conv_precision(self._h, 1 if dtype == 'f16' else 0))

    @_on_ctx_stream
    def forward_masked(self, tiles_t, eps_mode=None, tie_mode=TIE_ALL):
        """tiles_t ``[n, C, tc, F]`` float32 device tensor -> ``[S, n, tc, F]``."""
        torch = _torch()
        n = int(tiles_t.shape[0])
        if tuple(tiles_t.shape[1:]) != (self.arch.C, self.tc, self.F):
            raise ValueError("input tiles %r do not match network input (n, %d, %d, %d)"
                             % (tuple(tiles_t.shape), self.arch.C, self.tc, self.F))
        tiles_t = tiles_t.contiguous()
        out = torch.empty((self.S, n, self.tc, self.F), dtype=torch.float32, device=tiles_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        _lib.check(self.ctx._lib.dcs_model_forward_masked(self._h, _ptr(tiles_t), n, int(eps), int(tie_mode), _ptr(out)))
        return out

    @_on_ctx_stream
    def forward_raw(self, tiles_t, tie_mode=TIE_ALL, channel_major=False):
        """Network output before masking, ``[n, out_channels, tc, F]`` (testing aid).  For the DSD
        graph the kernel emits channel-major ``[out_channels, n, tc, F]``; it is permuted here.
        ``channel_major=True``: the buffer as ``dcs_model_forward`` wrote it, ``[out_channels, n, tc, F]``, no copy
        (what :func:`mask_fold_apply` reads)."""
        torch = _torch()
        n = int(tiles_t.shape[0])
        tiles_t = tiles_t.contiguous()
        out = torch.empty((self.out_channels, n, self.tc, self.F), dtype=torch.float32, device=tiles_t.device)
        _lib.check(self.ctx._lib.dcs_model_forward(self._h, _ptr(tiles_t), n, int(tie_mode), _ptr(out)))
        return out if channel_major else out.permute(1, 0, 2, 3).contiguous()

    @_on_ctx_stream
    def forward_stereo_tiles(self, tiles_t):
        """The stereo (ILD) graph on tiles (``dcs_model_forward_stereo``): ``tiles_t`` ``[n, tc, C, ld]`` float32 in the row layout
        -- the ``C = 2`` channels of a frame side by side, ``ld`` = F rounded up to 4, columns ``F .. ld-1`` zero
        (``streaming.stereo_rows_from_tiles`` makes it from ``[n, C, tc, F]``) -> the rectified network output ``[S, n, tc, C, ld]``, the
        buffer as the kernel wrote it (columns ``F .. ld-1`` unspecified).  ``ValueError`` for another graph or shape."""
        torch = _torch()
        ld = stereo_ld(self.F)
        if self.arch.name != 'dsd_ild':
            raise ValueError("forward_stereo_tiles runs the stereo (ILD) graph, not '%s'" % self.arch.name)
        if tiles_t.dim() != 4 or tuple(tiles_t.shape[1:]) != (self.tc, self.arch.C, ld) or tiles_t.dtype != torch.float32:
            raise ValueError("input tiles %r do not match the row layout (n, %d, %d, %d) float32"
                             % (tuple(tiles_t.shape), self.tc, self.arch.C, ld))
        n = int(tiles_t.shape[0])
        tiles_t = tiles_t.contiguous()
        out = torch.empty((self.S, n, self.tc, self.arch.C, ld), dtype=torch.float32, device=tiles_t.device)
        if n:
            _lib.check(self.ctx._lib.dcs_model_forward_stereo(self._h, _ptr(tiles_t), n, _ptr(out)))
        return out

    @_on_ctx_stream
    def separate(self, plan, audio_t, overlap, tiler=TILER_SCRIPT, scale=0.3, eps_mode=None, tie_mode=TIE_ALL,
                 out=None):
        """Fused file-level path: 1-D float32 device tensor -> ``[S, L]`` float32 PCM."""
        torch = _torch()
        L = int(audio_t.numel())
        if out is None:
            out = torch.empty((self.S, L), dtype=torch.float32, device=audio_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_separate(self._h, plan._h, _ptr(audio_t), L, int(overlap), int(tiler),
                                              float(scale), int(eps), int(tie_mode), _ptr(out), byref(nt), byref(nf)))
        self.last_tiles, self.last_frames = nt.value, nf.value
        return out

    @_on_ctx_stream
    def separate_scoreinformed(self, plan, audio_t, notes, overlap, scale=0.3, eps_mode=None, tie_mode=TIE_ALL, out=None):
        """``dcs_separate_scoreinformed``: 1-D float32 device tensor + the note table ``[C, P, W]`` of
        :func:`deepconvsep_amd.score` (``expandMidi``'s layout) -> ``[S, L]`` float32 PCM, one call."""
        torch = _torch()
        notes = np.ascontiguousarray(notes, dtype=np.float64)
        if notes.ndim != 3:
            raise ValueError("notes must be [instruments, notes, 2*nharmonics+3]")
        L = int(audio_t.numel())
        if out is None:
            out = torch.empty((self.S, L), dtype=torch.float32, device=audio_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_separate_scoreinformed(
            self._h, plan._h, _ptr(audio_t), L, notes.ctypes.data_as(POINTER(c_double)), int(notes.shape[0]),
            int(notes.shape[1]), int(notes.shape[2]), int(overlap), float(scale), int(eps), int(tie_mode), _ptr(out),
            byref(nt), byref(nf)))
        self.last_tiles, self.last_frames = nt.value, nf.value
        return out

    @_on_ctx_stream
    def separate_batch(self, plan, audio_t, overlap, tiler=TILER_SCRIPT, scale=0.3, eps_mode=None, tie_mode=TIE_ALL,
                       out=None):
        """Fused path for equal-length clips sharing one set of launches: ``[B, L]`` float32 device tensor
        (rows contiguous) -> ``[B, S, L]`` float32 PCM; every clip gets the tiles and cross-fade :meth:`separate`
        would give it alone (DSD / hiphop graph)."""
        torch = _torch()
        if audio_t.dim() != 2 or audio_t.stride(1) != 1:
            raise ValueError("separate_batch expects a [clips, samples] tensor with contiguous rows")
        B, L = int(audio_t.shape[0]), int(audio_t.shape[1])
        if out is None:
            out = torch.empty((B, self.S, L), dtype=torch.float32, device=audio_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_separate_batch(self._h, plan._h, _ptr(audio_t), L, B, int(audio_t.stride(0)),
                                                    int(overlap), int(tiler), float(scale), int(eps), int(tie_mode),
                                                    _ptr(out), byref(nt), byref(nf)))
        self.last_tiles, self.last_frames = nt.value, nf.value
        return out

    @_on_ctx_stream
    def separate_ragged(self, plan, audio_t, lengths, overlap, tiler=TILER_SCRIPT, scale=0.3, eps_mode=None,
                        tie_mode=TIE_ALL, out=None):
        """Clips of different lengths sharing one set of launches: ``audio_t [B, Lmax]`` float32 device tensor (row c
        holds ``lengths[c]`` samples), returns ``[B, S, Lmax]`` float32 PCM of which ``[c, :, :lengths[c]]`` is valid.
        Every clip gets the frames, tiles and cross-fade :meth:`separate` would give it alone (every single-channel
        graph; frameSize 1024 / 2048 / 4096)."""
        torch = _torch()
        if audio_t.dim() != 2 or audio_t.stride(1) != 1:
            raise ValueError("separate_ragged expects a [clips, samples] tensor with contiguous rows")
        B, Lmax = int(audio_t.shape[0]), int(audio_t.shape[1])
        lens = (c_int64 * B)(*[int(x) for x in lengths])
        if len(lengths) != B or max(lens) > Lmax:
            raise ValueError("separate_ragged: %d lengths for %d clips of at most %d samples" % (len(lengths), B, Lmax))
        if out is None:
            out = torch.zeros((B, self.S, Lmax), dtype=torch.float32, device=audio_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        nt, nf = (c_int64 * B)(), (c_int64 * B)()
        _lib.check(self.ctx._lib.dcs_separate_ragged(self._h, plan._h, _ptr(audio_t), lens, B, int(audio_t.stride(0)),
                                                     int(overlap), int(tiler), float(scale), int(eps), int(tie_mode),
                                                     _ptr(out), int(out.stride(1)), nt, nf))
        self.last_tiles, self.last_frames = list(nt), list(nf)
        return out

    @_on_ctx_stream
    def separate_stereo(self, plan, audio_t, overlap, tiler=TILER_LIBRARY, scale=0.3, want_spectra=False, want_pcm=True):
        """Stereo (ILD) graph: ``[2, L]`` float32 device tensor (rows contiguous) -> PCM ``[2, S, L]`` (and, with
        ``want_spectra``, the cross-faded scaled magnitudes ``[2, S, T, F]``; ``want_pcm=False``: the spectra alone, no
        iSTFT runs)."""
        torch = _torch()
        if audio_t.dim() != 2 or audio_t.shape[0] != 2 or audio_t.stride(1) != 1:
            raise ValueError("separate_stereo expects a [2, samples] tensor with contiguous rows")
        L = int(audio_t.shape[1])
        T = _lib.frame_count(L, plan.hop)
        if not want_pcm and not want_spectra:
            raise ValueError("separate_stereo: neither PCM nor spectra requested")
        out = torch.empty((2, self.S, L), dtype=torch.float32, device=audio_t.device) if want_pcm else None
        sep = torch.empty((2, self.S, T, self.F), dtype=torch.float32, device=audio_t.device) if want_spectra else None
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_separate_stereo(self._h, plan._h, _ptr(audio_t), L, int(audio_t.stride(0)),
                                                     int(overlap), int(tiler), float(scale), _ptr(out),
                                                     _ptr(sep) if sep is not None else None, self.F, byref(nt), byref(nf)))
        self.last_tiles, self.last_frames = nt.value, nf.value
        if not want_pcm:
            return sep
        return (out, sep) if want_spectra else out

    @_on_ctx_stream
    def separate_spectra(self, plan, audio_t, overlap, tiler=TILER_SCRIPT, scale=0.3, eps_mode=None,
                         tie_mode=TIE_ALL):
        """Fused path stopped before the iSTFT: (sep ``[S,T,F]``, mag ``[T,F]``, phase ``[T,F]``)."""
        torch = _torch()
        L = int(audio_t.numel())
        T = _lib.frame_count(L, plan.hop)
        F = self.F
        sep = torch.empty((self.S, T, F), dtype=torch.float32, device=audio_t.device)
        mag = torch.empty((T, F), dtype=torch.float32, device=audio_t.device)
        ph = torch.empty((T, F), dtype=torch.float32, device=audio_t.device)
        eps = self.arch.eps_mode if eps_mode is None else eps_mode
        _lib.check(self.ctx._lib.dcs_separate_spectra(self._h, plan._h, _ptr(audio_t), L, int(overlap), int(tiler),
                                                      float(scale), int(eps), int(tie_mode), _ptr(sep), _ptr(mag),
                                                      _ptr(ph), F))
        return sep, mag, ph

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream(object):
    """``dcs_stream``: the device state of a streaming separation on one STFT plan -- sample, frame, ``p`` and time-frame rings
    whose size depends on ``(frameSize, hop, time_context, overlap, S, max_push)`` alone.  ``push`` and ``pull`` alternate
    strictly; the counts of every call are host integers (:class:`deepconvsep_amd.streaming.StreamCounts`), so the outputs are
    allocated at their exact size before the call and nothing waits for the device."""

    tile_channels = 1                # input channels of the tiles a push returns

    def __init__(self, plan, S, time_context, overlap, tiler=TILER_SCRIPT, eps_mode=EPS_A, scale=1.0, max_push=65536):
        from .streaming import StreamCounts
        self.ctx, self.plan = plan.ctx, plan
        self.S, self.tc, self.F = int(S), int(time_context), plan.bins
        self.max_push = int(max_push)
        rise = np.ascontiguousarray(np.linspace(0., 1.0, num=max(int(overlap), 1)), dtype=np.float64)
        h = c_void_p()
        _lib.check(self._create(int(overlap), int(tiler), int(eps_mode), float(scale), rise.ctypes.data_as(POINTER(c_double)), h))
        self._h = h
        self.counts = StreamCounts(plan.frame, plan.hop, time_context, overlap, tiler)
        self.max_tiles = int(self.ctx._lib.dcs_stream_max_tiles(h))
        self.pushed, self.ended = 0, False
        self._tiles = self._frames = self._folded = self._emitted = 0

    def _create(self, overlap, tiler, eps_mode, scale, rise_p, h):
        return self.ctx._lib.dcs_stream_create(self.plan._h, self.S, self.tc, overlap, tiler, eps_mode, scale, rise_p,
                                               self.max_push, byref(h))

    @property
    def bytes(self):
        return int(self.ctx._lib.dcs_stream_bytes(self._h))

    @_on_ctx_stream
    def push(self, audio_t=None, last=False, want_frames=False):
        """Appends ``audio_t`` (float32 device tensor ``[n]``, ``n <= max_push``; None: no samples), ``last=True`` ends the
        signal.  Returns the tiles that became ready, ``[n_new, 1, tc, F]`` -- with ``want_frames`` also the magnitude and phase
        rows of the frames that became complete, ``[n_frames, F]`` each."""
        torch = _torch()
        n = 0 if audio_t is None else int(audio_t.numel())
        if audio_t is not None and (audio_t.dim() != 1 or audio_t.dtype != torch.float32 or not audio_t.is_contiguous()):
            raise ValueError("Stream.push takes a contiguous float32 [n] tensor")
        c, P = self.counts, self.pushed + n
        want_t = max(0, min(c.tiles(P, bool(last)) - self._tiles, self.max_tiles))
        want_f = max(0, c.frames(P, bool(last)) - self._frames) if want_frames else 0
        tiles = torch.empty((want_t, self.tile_channels, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
        mag = torch.empty((want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        ph = torch.empty((want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_stream_push(self._h, _ptr(audio_t) if n else None, n, 1 if last else 0,
                                                 _ptr(tiles) if want_t else None, want_t, byref(nt),
                                                 _ptr(mag) if want_f else None, _ptr(ph) if want_f else None, self.F, byref(nf)))
        self.pushed, self.ended = P, bool(last)
        self._tiles += nt.value
        self._frames += nf.value
        self.last_tiles, self.last_frames = nt.value, nf.value
        if nt.value != want_t or (want_frames and nf.value != want_f):
            raise _lib.DcsError("dcs_stream_push returned %d tiles and %d frames, the host counts say %d and %d"
                                % (nt.value, nf.value, want_t, want_f))
        return (tiles, mag, ph) if want_frames else tiles

    @_on_ctx_stream
    def pull(self, p=None, want_est=False):
        """``p``: the first ``S`` channels of ``Network.forward_raw(tiles, ..., channel_major=True)`` for exactly the tiles of
        the preceding push (``[S, n, tc, F]`` float32, a view with a larger source stride is fine; None when the push returned
        none).  Returns the samples that became final, ``[S, n_out]`` float32 -- with ``want_est`` also the estimates of the
        frames that were folded, ``[S, rows, F]``."""
        torch = _torch()
        n = 0 if p is None else int(p.shape[1])
        if p is not None:
            if p.dim() != 4 or tuple(p.shape[2:]) != (self.tc, self.F) or int(p.shape[0]) != self.S or p.dtype != torch.float32:
                raise ValueError("Stream.pull expects p [%d, n, %d, %d] float32, got %r" % (self.S, self.tc, self.F, tuple(p.shape)))
            if n and not p[0].is_contiguous():
                p = p.contiguous()
        c = self.counts
        n_pcm = c.emitted(self.pushed, self.ended) - self._emitted
        n_fold = c.folded(self.pushed, self.ended) - self._folded
        pcm = torch.empty((self.S, n_pcm), dtype=torch.float32, device=self.ctx.device)
        est = torch.empty((self.S, n_fold, self.F), dtype=torch.float32, device=self.ctx.device) if want_est else None
        got = c_int64()
        _lib.check(self.ctx._lib.dcs_stream_pull(self._h, _ptr(p) if n else None, int(p.stride(0)) if n else 0, n,
                                                 _ptr(pcm) if n_pcm else None, n_pcm, n_pcm, byref(got),
                                                 _ptr(est) if want_est and n_fold else None, n_fold * self.F, self.F))
        self._emitted += got.value
        self._folded += n_fold
        self.last_samples = got.value
        if got.value != n_pcm:
            raise _lib.DcsError("dcs_stream_pull returned %d samples, the host counts say %d" % (got.value, n_pcm))
        return (pcm, est) if want_est else pcm

    def reset(self):
        _lib.check(self.ctx._lib.dcs_stream_reset(self._h))
        self.pushed, self.ended = 0, False
        self.last_folded = 0
        self._tiles = self._frames = self._folded = self._emitted = 0

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StreamMwf(object):
    """``dcs_stream_set_mwf`` / ``dcs_stream_mwf_last`` for the two-channel streams."""

    def set_mwf(self, niter, forget=1.0, loading=1e-3, eps=1e-10):
        """Arms the online multichannel Wiener filter (:class:`MwfOnline`, ``J = S``) for the pulls of this stream: before the
        first push, or after ``reset``; ``niter = 0`` turns it off.  Two channels only.  The filtered stems replace the masked
        ones in what ``pull`` returns; ``want_est`` still gives the unfiltered estimates.  The first frames of a signal are
        filtered on little evidence: this is not the whole-file filter."""
        _lib.check(self.ctx._lib.dcs_stream_set_mwf(self._h, int(niter), float(forget), float(loading), float(eps)))
        self.mwf_iters = int(niter)

    @_on_ctx_stream
    def last_mwf(self):
        """The filtered magnitudes and phases of the frames the last pull folded, ``[C, S, rows, F]`` each."""
        torch = _torch()
        rows = int(getattr(self, "last_folded", 0))
        mag = torch.empty((self.C, self.S, rows, self.F), dtype=torch.float32, device=self.ctx.device)
        ph = torch.empty((self.C, self.S, rows, self.F), dtype=torch.float32, device=self.ctx.device)
        _lib.check(self.ctx._lib.dcs_stream_mwf_last(self._h, _ptr(mag) if rows else None, _ptr(ph) if rows else None,
                                                     self.S * rows * self.F, rows * self.F, self.F))
        return mag, ph


class ChannelStream(_StreamMwf, Stream):
    """``dcs_stream_create_channels``: a :class:`Stream` that carries ``channels`` signal channels next to the down-mix the
    network sees -- one ring of ``p``, one fold per (frame, bin), an inverse per (channel, source).  The counts, the alternation
    and ``reset`` / ``close`` / ``bytes`` / ``max_tiles`` are the mono stream's."""

    def __init__(self, plan, S, channels, time_context, overlap, tiler=TILER_SCRIPT, eps_mode=EPS_A, scale=1.0, max_push=65536):
        self.C = int(channels)
        Stream.__init__(self, plan, S, time_context, overlap, tiler, eps_mode, scale, max_push)

    def _create(self, overlap, tiler, eps_mode, scale, rise_p, h):
        return self.ctx._lib.dcs_stream_create_channels(self.plan._h, self.S, self.C, self.tc, overlap, tiler, eps_mode, scale,
                                                        rise_p, self.max_push, byref(h))

    @_on_ctx_stream
    def push(self, audio_t=None, last=False, want_frames=False):
        """Appends ``audio_t`` (float32 device tensor ``[C + 1, n]``: the channels, then the down-mix; rows contiguous, a view
        with a larger row stride is fine; ``n <= max_push``; None: no samples), ``last=True`` ends the signal.  Returns the
        tiles of the down-mix that became ready, ``[n_new, 1, tc, F]`` -- with ``want_frames`` also the channels' magnitude and
        phase rows of the frames that became complete, ``[C, n_frames, F]`` each."""
        torch = _torch()
        n = 0 if audio_t is None else int(audio_t.shape[-1])
        if audio_t is not None and (audio_t.dim() != 2 or int(audio_t.shape[0]) != self.C + 1 or audio_t.dtype != torch.float32
                                    or (n and (audio_t.stride(1) != 1 or audio_t.stride(0) < n))):
            raise ValueError("ChannelStream.push takes a float32 [%d, n] tensor with contiguous rows" % (self.C + 1))
        c, P = self.counts, self.pushed + n
        want_t = max(0, min(c.tiles(P, bool(last)) - self._tiles, self.max_tiles))
        want_f = max(0, c.frames(P, bool(last)) - self._frames) if want_frames else 0
        tiles = torch.empty((want_t, 1, self.tc, self.F), dtype=torch.float32, device=self.ctx.device)
        mag = torch.empty((self.C, want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        ph = torch.empty((self.C, want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_stream_push_channels(self._h, _ptr(audio_t) if n else None, int(audio_t.stride(0)) if n else 0,
                                                          n, 1 if last else 0, _ptr(tiles) if want_t else None, want_t, byref(nt),
                                                          _ptr(mag) if want_f else None, _ptr(ph) if want_f else None,
                                                          want_f * self.F, self.F, byref(nf)))
        self.pushed, self.ended = P, bool(last)
        self._tiles += nt.value
        self._frames += nf.value
        self.last_tiles, self.last_frames = nt.value, nf.value
        if nt.value != want_t or (want_frames and nf.value != want_f):
            raise _lib.DcsError("dcs_stream_push_channels returned %d tiles and %d frames, the host counts say %d and %d"
                                % (nt.value, nf.value, want_t, want_f))
        return (tiles, mag, ph) if want_frames else tiles

    @_on_ctx_stream
    def pull(self, p=None, want_est=False):
        """``p`` as for :meth:`Stream.pull`.  Returns the samples that became final, ``[C, S, n_out]`` float32 -- with
        ``want_est`` also the estimates of the frames that were folded, ``[C, S, rows, F]``."""
        torch = _torch()
        n = 0 if p is None else int(p.shape[1])
        if p is not None:
            if p.dim() != 4 or tuple(p.shape[2:]) != (self.tc, self.F) or int(p.shape[0]) != self.S or p.dtype != torch.float32:
                raise ValueError("ChannelStream.pull expects p [%d, n, %d, %d] float32, got %r"
                                 % (self.S, self.tc, self.F, tuple(p.shape)))
            if n and not p[0].is_contiguous():
                p = p.contiguous()
        c = self.counts
        n_pcm = c.emitted(self.pushed, self.ended) - self._emitted
        n_fold = c.folded(self.pushed, self.ended) - self._folded
        pcm = torch.empty((self.C, self.S, n_pcm), dtype=torch.float32, device=self.ctx.device)
        est = torch.empty((self.C, self.S, n_fold, self.F), dtype=torch.float32, device=self.ctx.device) if want_est else None
        got = c_int64()
        _lib.check(self.ctx._lib.dcs_stream_pull_channels(self._h, _ptr(p) if n else None, int(p.stride(0)) if n else 0, n,
                                                          _ptr(pcm) if n_pcm else None, self.S * n_pcm, n_pcm, n_pcm, byref(got),
                                                          _ptr(est) if want_est and n_fold else None,
                                                          self.S * n_fold * self.F, n_fold * self.F, self.F))
        self._emitted += got.value
        self._folded += n_fold
        self.last_samples, self.last_folded = got.value, n_fold
        if got.value != n_pcm:
            raise _lib.DcsError("dcs_stream_pull_channels returned %d samples, the host counts say %d" % (got.value, n_pcm))
        return (pcm, est) if want_est else pcm


class StereoStream(_StreamMwf, Stream):
    """``dcs_stream_create_stereo``: a :class:`Stream` for the stereo (ILD) graph -- ``channels`` rows of samples, magnitudes and
    phases and no down-mix; ``push`` returns tiles in the row layout ``[n_new, tc, C, ld]`` that
    :meth:`Network.forward_stereo_tiles` takes, ``pull`` takes ``p`` per (source, channel) and folds the stereo trainer's
    per-channel mask.  The counts, the alternation and ``reset`` / ``close`` / ``bytes`` / ``max_tiles`` are the mono stream's."""

    def __init__(self, plan, S, channels, time_context, overlap, tiler=TILER_LIBRARY, scale=1.0, max_push=65536):
        self.C = int(channels)
        self.ld = stereo_ld(plan.bins)
        Stream.__init__(self, plan, S, time_context, overlap, tiler, EPS_B, scale, max_push)

    def _create(self, overlap, tiler, eps_mode, scale, rise_p, h):
        return self.ctx._lib.dcs_stream_create_stereo(self.plan._h, self.S, self.C, self.tc, overlap, tiler, scale, rise_p,
                                                      self.max_push, byref(h))

    @_on_ctx_stream
    def push(self, audio_t=None, last=False, want_frames=False):
        """Appends ``audio_t`` (float32 device tensor ``[C, n]``, rows contiguous, a view with a larger row stride is fine;
        ``n <= max_push``; None: no samples), ``last=True`` ends the signal.  Returns the tiles that became ready, ``[n_new, tc,
        C, ld]`` -- with ``want_frames`` also the channels' magnitude and phase rows of the frames that became complete, ``[C,
        n_frames, F]`` each."""
        torch = _torch()
        n = 0 if audio_t is None else int(audio_t.shape[-1])
        if audio_t is not None and (audio_t.dim() != 2 or int(audio_t.shape[0]) != self.C or audio_t.dtype != torch.float32
                                    or (n and (audio_t.stride(1) != 1 or audio_t.stride(0) < n))):
            raise ValueError("StereoStream.push takes a float32 [%d, n] tensor with contiguous rows" % self.C)
        c, P = self.counts, self.pushed + n
        want_t = max(0, min(c.tiles(P, bool(last)) - self._tiles, self.max_tiles))
        want_f = max(0, c.frames(P, bool(last)) - self._frames) if want_frames else 0
        tiles = torch.empty((want_t, self.tc, self.C, self.ld), dtype=torch.float32, device=self.ctx.device)
        mag = torch.empty((self.C, want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        ph = torch.empty((self.C, want_f, self.F), dtype=torch.float32, device=self.ctx.device) if want_frames else None
        nt, nf = c_int64(), c_int64()
        _lib.check(self.ctx._lib.dcs_stream_push_stereo(self._h, _ptr(audio_t) if n else None, int(audio_t.stride(0)) if n else 0,
                                                        n, 1 if last else 0, _ptr(tiles) if want_t else None, want_t, byref(nt),
                                                        _ptr(mag) if want_f else None, _ptr(ph) if want_f else None,
                                                        want_f * self.F, self.F, byref(nf)))
        self.pushed, self.ended = P, bool(last)
        self._tiles += nt.value
        self._frames += nf.value
        self.last_tiles, self.last_frames = nt.value, nf.value
        if nt.value != want_t or (want_frames and nf.value != want_f):
            raise _lib.DcsError("dcs_stream_push_stereo returned %d tiles and %d frames, the host counts say %d and %d"
                                % (nt.value, nf.value, want_t, want_f))
        return (tiles, mag, ph) if want_frames else tiles

    @_on_ctx_stream
    def pull(self, p=None, want_est=False):
        """``p`` for exactly the tiles of the preceding push (None when it returned none), float32: what
        :meth:`Network.forward_stereo_tiles` returned, ``[S, n, tc, C, ld]``, or the Lasagne layout ``[S * C, n, tc, F]`` (output
        channel ``s C + c``).  Returns the samples that became final, ``[C, S, n_out]`` float32 -- with ``want_est`` also the
        estimates of the frames that were folded, ``[C, S, rows, F]``."""
        torch = _torch()
        n = 0 if p is None else int(p.shape[1])
        if p is not None:
            rows = p.dim() == 5 and tuple(p.shape) == (self.S, n, self.tc, self.C, self.ld)
            planes = p.dim() == 4 and tuple(p.shape) == (self.S * self.C, n, self.tc, self.F)
            if not (rows or planes) or p.dtype != torch.float32:
                raise ValueError("StereoStream.pull expects p [%d, n, %d, %d, %d] or [%d, n, %d, %d] float32, got %r"
                                 % (self.S, self.tc, self.C, self.ld, self.S * self.C, self.tc, self.F, tuple(p.shape)))
            p = p.contiguous()
            strides = ((n * self.tc * self.C * self.ld, self.ld, self.C * self.ld) if rows else
                       (self.C * n * self.tc * self.F, n * self.tc * self.F, self.F))
        c = self.counts
        n_pcm = c.emitted(self.pushed, self.ended) - self._emitted
        n_fold = c.folded(self.pushed, self.ended) - self._folded
        pcm = torch.empty((self.C, self.S, n_pcm), dtype=torch.float32, device=self.ctx.device)
        est = torch.empty((self.C, self.S, n_fold, self.F), dtype=torch.float32, device=self.ctx.device) if want_est else None
        got = c_int64()
        ss, cs, pl = strides if n else (0, 0, 0)
        _lib.check(self.ctx._lib.dcs_stream_pull_stereo(self._h, _ptr(p) if n else None, ss, cs, pl, n,
                                                        _ptr(pcm) if n_pcm else None, self.S * n_pcm, n_pcm, n_pcm, byref(got),
                                                        _ptr(est) if want_est and n_fold else None,
                                                        self.S * n_fold * self.F, n_fold * self.F, self.F))
        self._emitted += got.value
        self._folded += n_fold
        self.last_samples, self.last_folded = got.value, n_fold
        if got.value != n_pcm:
            raise _lib.DcsError("dcs_stream_pull_stereo returned %d samples, the host counts say %d" % (got.value, n_pcm))
        return (pcm, est) if want_est else pcm


class ScoreStream(Stream):
    """``dcs_stream_create_score``: a :class:`Stream` for the score-informed graphs.  ``melody`` is the note table
    ``[instruments, notes, 2*nharmonics+3]`` of ``score.melody_table``, read once, here; ``normalise`` ``'max'`` | ``'sum'`` and
    ``mixture`` ``'ch0'`` | ``'sum'`` as in :meth:`Network.set_score_semantics`.  ``push`` returns tiles ``[n_new, instruments,
    tc, F]`` -- channel ``j`` is the harmonic mask of instrument ``j`` times the scaled magnitudes -- and the fold of ``pull``
    multiplies with the score-informed mixture; everything else (``pull``, ``reset``, which keeps the score, ``close``,
    ``bytes``, ``max_tiles``, the counts) is the mono stream's.

    ``follow``: an :class:`deepconvsep_amd.align.ScoreFollower` on the same context, with ``classes`` the int8 table of
    ``align.bin_classes`` for this plan's bins (``dcs_stream_set_follow``).  ``melody`` is then the table in SCORE time
    (``melody_table`` at nominal tempo with ``nframes`` = the follower's ``U``): a push computes the chroma of its new frames,
    asks the follower where in the score they are and paints audio frame ``t`` from score frame ``pos[t]``;
    :meth:`positions` returns the last push's.  The follower stays the caller's and must outlive the stream; ``reset`` resets
    it too."""

    def __init__(self, plan, S, melody, time_context, overlap, tiler=TILER_LIBRARY, eps_mode=EPS_A, scale=1.0, max_push=65536,
                 normalise='max', mixture='ch0', follow=None, classes=None, floor=1e-6):
        melody = np.ascontiguousarray(melody, dtype=np.float64)
        if melody.ndim != 3:
            raise ValueError("melody must be [instruments, notes, 2*nharmonics+3]")
        try:
            self._codes = ({'max': 0, 'sum': 1}[normalise], {'ch0': 0, 'sum': 1}[mixture])
        except KeyError:
            raise ValueError("normalise must be 'max' or 'sum', mixture 'ch0' or 'sum'")
        self._melody = melody
        self.ninst = self.tile_channels = int(melody.shape[0])
        Stream.__init__(self, plan, S, time_context, overlap, tiler, eps_mode, scale, max_push)
        del self._melody                 # the library keeps its own converted copy
        self.follow = None
        if follow is not None:
            if classes is None:
                raise ValueError("a followed ScoreStream needs the pitch classes of its bins (align.bin_classes)")
            cls = np.ascontiguousarray(classes, dtype=np.int8)
            if cls.shape != (self.F,):
                raise ValueError("classes must have one entry per bin (%d), got %r" % (self.F, cls.shape))
            try:
                _lib.check(self.ctx._lib.dcs_stream_set_follow(self._h, follow._h, c_void_p(cls.ctypes.data), float(floor)))
            except Exception:
                self.close()
                raise
            self.follow = follow         # kept alive as long as the stream

    def _create(self, overlap, tiler, eps_mode, scale, rise_p, h):
        m = self._melody
        return self.ctx._lib.dcs_stream_create_score(self.plan._h, self.S, self.tc, overlap, tiler, eps_mode, scale, rise_p,
                                                     self.max_push, m.ctypes.data_as(POINTER(c_double)), int(m.shape[0]),
                                                     int(m.shape[1]), int(m.shape[2]), self._codes[0], self._codes[1], byref(h))

    @_on_ctx_stream
    def positions(self):
        """int32 device tensor: the score frame of every audio frame the last push completed (``dcs_stream_follow_last``)."""
        torch = _torch()
        if self.follow is None:
            raise ValueError("this ScoreStream follows no score (follow=...)")
        cap = self.counts.max_frames(self.max_push)
        pos = torch.empty((cap,), dtype=torch.int32, device=self.ctx.device)
        n = c_int64()
        _lib.check(self.ctx._lib.dcs_stream_follow_last(self._h, _ptr(pos), cap, byref(n)))
        return pos[:n.value]


class MwfOnline(object):
    """``dcs_mwf_online``: the multichannel Wiener filter on a stream -- a causal form of :meth:`Context.mwf` whose state is
    one Hermitian 2x2 matrix per (source, bin), whatever the length of the signal.  ``push`` filters the next frames; the
    result does not depend on how the frames are cut into pushes.  ``forget`` in (0, 1] weighs the past down per frame,
    ``loading`` adds that fraction of an isotropic covariance to every spatial covariance (without it the first frame's are of
    rank one).  It is not the batch filter and is not expected to match it: the first frames of a signal are filtered on
    little evidence."""

    def __init__(self, ctx, F, J, niter, forget=1.0, loading=1e-3, eps=1e-10):
        self.ctx, self.F, self.J, self.niter = ctx, int(F), int(J), int(niter)
        h = c_void_p()
        _lib.check(ctx._lib.dcs_mwf_online_create(ctx._h, self.F, self.J, self.niter, float(forget), float(loading), float(eps),
                                                  byref(h)))
        self._h = h

    @property
    def bytes(self):
        return int(self.ctx._lib.dcs_mwf_online_bytes(self._h))

    @property
    def frames(self):
        """Frames pushed since the filter was made or reset."""
        return int(self.ctx._lib.dcs_mwf_online_frames(self._h))

    @_on_ctx_stream
    def push(self, mag, phase, src, pre_div=1.0):
        """``mag``, ``phase`` ``[2, n, F]`` (the mixture), ``src`` ``[2, J, n, F]`` (per-channel source magnitudes, divided by
        ``pre_div`` before use), float32 device tensors -> (magnitudes, phases) of the filtered images, both ``[2, J, n, F]``."""
        torch = _torch()
        if mag.dim() != 3 or src.dim() != 4 or tuple(phase.shape) != tuple(mag.shape) or int(mag.shape[0]) != 2 \
                or tuple(src.shape) != (2, self.J, int(mag.shape[1]), self.F) or int(mag.shape[2]) != self.F:
            raise ValueError("MwfOnline.push expects mag, phase [2, n, %d] and src [2, %d, n, %d], got %r, %r, %r"
                             % (self.F, self.J, self.F, tuple(mag.shape), tuple(phase.shape), tuple(src.shape)))
        if any(t.dtype != torch.float32 or t.device != self.ctx.device for t in (mag, phase, src)):
            raise ValueError("MwfOnline.push expects float32 tensors on %s" % (self.ctx.device,))
        mag, phase, src = mag.contiguous(), phase.contiguous(), src.contiguous()
        J, T, F = self.J, int(mag.shape[1]), self.F
        out_mag = torch.empty((2, J, T, F), dtype=torch.float32, device=src.device)
        out_phase = torch.empty((2, J, T, F), dtype=torch.float32, device=src.device)
        _lib.check(self.ctx._lib.dcs_mwf_online_push_f32(self._h, _ptr(mag), _ptr(phase), T * F, _ptr(src), J * T * F, T * F, F, T,
                                                         float(pre_div), _ptr(out_mag), _ptr(out_phase)))
        return out_mag, out_phase

    def reset(self):
        _lib.check(self.ctx._lib.dcs_mwf_online_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_mwf_online_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tile(ctx, mag_t, time_context, overlap, tiler, scale=1.0):
    """``generate_overlapadd`` on the device: mag_t ``[T,F]`` or ``[C,T,F]`` float32 -> (tiles
    ``[n,C,tc,F]``, n)."""
    torch = _torch()
    if mag_t.dim() == 2:
        mag_t = mag_t.unsqueeze(0)
    with ctx.stream_scope():
        mag_t = mag_t.contiguous()
    C, T, F = (int(x) for x in mag_t.shape)
    n = _lib.tile_count(T, time_context, overlap, tiler)
    with ctx.stream_scope():
        tiles = torch.empty((n, C, time_context, F), dtype=torch.float32, device=mag_t.device)
        if n:
            _lib.check(ctx._lib.dcs_tile(ctx._h, _ptr(mag_t), T * F, F, C, T, F, int(time_context), int(overlap),
                                         int(tiler), float(scale), _ptr(tiles), n))
    return tiles, n


def mwf(ctx, mag_t, phase_t, src_t, niter, pre_div=1.0, eps=1e-10):
    """:meth:`Context.mwf`: the multichannel Wiener filter the reference left unfinished (util.py:633-719) on the device."""
    return ctx.mwf(mag_t, phase_t, src_t, niter, pre_div, eps)


def mask_fold_apply(ctx, p, mag, time_context, overlap, eps_mode, n_frames=None, want_mask=False):
    """``dcs_mask_fold_apply``: the soft masks of the rectified network output ``p`` ``[S, n, tc, F]`` (the first ``S``
    channels of ``Network.forward_raw(..., channel_major=True)``; a view whose source stride is larger is fine), cross-faded
    over the tiles like ``overlapadd_multi``, times the magnitudes ``mag`` ``[C, T, F]`` of every channel -> ``est``
    ``[C, S, n_frames, F]`` (``n_frames`` defaults to ``T``; rows past the last tile are zero) and, with ``want_mask``, the
    cross-faded masks ``[S, n_frames, F]`` as well.  float32 device tensors; ``eps_mode`` ``EPS_A`` or ``EPS_B``."""
    torch = _torch()
    if p.dim() != 4 or mag.dim() != 3 or int(p.shape[2]) != int(time_context) or int(p.shape[3]) != int(mag.shape[2]):
        raise ValueError("mask_fold_apply expects p [S, n, %d, F] and mag [C, T, F], got %r and %r"
                         % (int(time_context), tuple(p.shape), tuple(mag.shape)))
    if any(t.dtype != torch.float32 or t.device != ctx.device for t in (p, mag)):
        raise ValueError("mask_fold_apply expects float32 tensors on %s" % (ctx.device,))
    S, n, tc, F = (int(x) for x in p.shape)
    C, T = int(mag.shape[0]), int(mag.shape[1])
    rows = T if n_frames is None else int(n_frames)
    if rows < 0 or rows > T:
        raise ValueError("mask_fold_apply: n_frames %d outside 0 .. %d, the rows of mag" % (rows, T))
    rise = np.ascontiguousarray(np.linspace(0., 1.0, num=int(overlap)), dtype=np.float64)
    with ctx.stream_scope():
        if n == 0:
            p = torch.empty((S, 1), dtype=torch.float32, device=mag.device)   # never read; an empty tensor has no address
        elif (S > 1 and p.stride(0) < n * tc * F) or not p[0].is_contiguous():
            p = p.contiguous()
        mag = mag.contiguous()
        est = torch.empty((C, S, rows, F), dtype=torch.float32, device=mag.device)
        mask = torch.empty((S, rows, F), dtype=torch.float32, device=mag.device) if want_mask else None
        _lib.check(ctx._lib.dcs_mask_fold_apply(ctx._h, _ptr(p), int(p.stride(0)), n, S, tc, int(overlap), F, int(eps_mode),
                                                rise.ctypes.data_as(POINTER(c_double)), _ptr(mag), T * F, C, rows, F,
                                                _ptr(est), S * rows * F, rows * F, _ptr(mask), rows * F))
    return (est, mask) if want_mask else est


def pcm_to_int16(ctx, pcm_t, out=None):
    """``(audio_out * 32767).astype('int16')`` on the device (separate_dsd.py:307-309): float32 tensor of any shape
    (contiguous) -> int16 tensor of the same shape."""
    torch = _torch()
    with ctx.stream_scope():
        pcm_t = pcm_t.contiguous()
        if out is None:
            out = torch.empty(pcm_t.shape, dtype=torch.int16, device=pcm_t.device)
        _lib.check(ctx._lib.dcs_pcm_to_int16(ctx._h, _ptr(pcm_t), int(pcm_t.numel()), _ptr(out)))
    return out


def pcm16_to_float(ctx, pcm16_t, channels, mode=0, out=None):
    """``dcs_pcm16_to_float``: int16 wav frames on the device -> the mono float32 signal the scripts separate.  ``pcm16_t``
    ``[B, stride]`` int16 (row c = clip c's interleaved frames, zero padded), ``channels`` per frame; returns ``[B, stride //
    channels]`` float32.  ``mode`` 0: (L + R) / 2 for two or more channels, the channel itself for mono (separate_dsd.py:
    285-287); 1: L + R (separate_ikala.py:229)."""
    torch = _torch()
    if pcm16_t.dim() != 2 or pcm16_t.stride(1) != 1 or pcm16_t.dtype != torch.int16:
        raise ValueError("pcm16_to_float expects a [clips, interleaved samples] int16 tensor with contiguous rows")
    B, n = int(pcm16_t.shape[0]), int(pcm16_t.shape[1]) // int(channels)
    with ctx.stream_scope():
        if out is None:
            out = torch.empty((B, n), dtype=torch.float32, device=pcm16_t.device)
        _lib.check(ctx._lib.dcs_pcm16_to_float(ctx._h, _ptr(pcm16_t), n, int(channels), int(mode), B, int(pcm16_t.stride(0)),
                                               _ptr(out), int(out.stride(0))))
    return out


def overlap_add(ctx, out_t, overlap):
    """``overlapadd_multi`` on the device: out_t ``[S, n, tc, F]`` float32 -> ``[S, n*(tc-ov)+tc, F]``."""
    torch = _torch()
    S, n, tc, F = (int(x) for x in out_t.shape)
    rows = n * (tc - overlap) + tc
    rise = np.ascontiguousarray(np.linspace(0., 1.0, num=overlap), dtype=np.float64)
    with ctx.stream_scope():
        out_t = out_t.contiguous()
        sep = torch.empty((S, rows, F), dtype=torch.float32, device=out_t.device)
        _lib.check(ctx._lib.dcs_overlap_add(ctx._h, _ptr(out_t), n, S, tc, int(overlap), F,
                                            rise.ctypes.data_as(POINTER(c_double)), _ptr(sep), rows * F, F))
    return sep
