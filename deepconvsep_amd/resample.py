"""Sample-rate conversion in front of and behind the separators (``dcs_resample_f32``, csrc/resample.hip).

The reference's models take 44 100 Hz features and its scripts refuse every other file (separate_dsd.py:283).  Here such a
file is converted to 44 100 Hz on the device, separated, and the sources converted back to the file's own rate.

For rates ``fi -> fo``: ``up / down = fo / fi`` in lowest terms, ``R = max(up, down) / rolloff``, ``H = ceil(Z R)`` and, on
the integer grid ``t = -H .. H`` at rate ``up fi``::

    h[t] = (up / R) sinc(t / R) I0(beta sqrt(1 - (t / (Z R))^2)) / I0(beta)       |t| <= Z R, else 0
    y[m] = sum_n x[n] h[m down - n up],   0 <= n < L,  |m down - n up| <= H,   m = 0 .. ceil(L up / down) - 1

which is ``scipy.signal.resample_poly(x, up, down, window=h / up)``: zero outside ``[0, L)``, centred, no delay.  The design
(this module, float64 NumPy) is handed to the library like the STFT's window; the sum runs in float32 on the device.
``rolloff = 0.95`` with ``Z = 32`` zero crossings keeps a tone at 0.40 min(fi, fo) to 122 dB and puts one 6 % above the new
Nyquist at -97.6 dB; the price is the transition band -- a tone at 0.45 min(fi, fo) is already attenuated (24 dB SNR).
"""
import ctypes
from ctypes import POINTER, byref, c_double, c_void_p
from math import gcd

import numpy as np

from . import _lib

TARGET_RATE = 44100      # what every model of the reference was trained on


def ratio(fi, fo):
    """``(up, down)``: ``fo / fi`` in lowest terms."""
    fi, fo = int(fi), int(fo)
    if fi < 1 or fo < 1:
        raise ValueError("sample rates must be positive integers, got %r -> %r" % (fi, fo))
    g = gcd(fi, fo)
    return fo // g, fi // g


def design(fi, fo, zero_crossings=32, beta=12.0, rolloff=0.95):
    """``(up, down, taps float64 [2 H + 1], H)`` of the Kaiser-windowed sinc above."""
    up, down = ratio(fi, fo)
    if not (zero_crossings >= 1 and 0.0 < rolloff <= 1.0 and beta >= 0.0):
        raise ValueError("design needs zero_crossings >= 1, 0 < rolloff <= 1 and beta >= 0")
    R = max(up, down) / rolloff
    width = zero_crossings * R
    H = int(np.ceil(width))
    t = np.arange(-H, H + 1, dtype=np.float64)
    inside = np.abs(t) <= width
    arg = np.where(inside, 1.0 - (t / width) ** 2, 0.0)
    taps = (up / R) * np.sinc(t / R) * np.i0(beta * np.sqrt(arg)) / np.i0(beta)
    taps = np.where(inside, taps, 0.0)
    return up, down, taps, H


def out_length(L, up, down):
    """``ceil(L up / down)``: samples ``L`` input samples give."""
    L, up, down = int(L), int(up), int(down)
    if L < 0 or up < 1 or down < 1:
        raise ValueError("out_length needs L >= 0 and up, down >= 1")
    return (L * up + down - 1) // down


class Resampler(object):
    """``dcs_resampler``: the polyphase table of one ``(fi, fo, design)`` on the device.  Calling it converts a float32
    device tensor ``[L]`` or ``[n_clips, L]`` (rows contiguous) in one launch and returns a device tensor."""

    def __init__(self, ctx, fi, fo, **kw):
        self.ctx = ctx
        self.fi, self.fo = int(fi), int(fo)
        self.up, self.down, taps, self.half = design(fi, fo, **kw)
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        h = c_void_p()
        _lib.check(ctx._lib.dcs_resample_plan(ctx._h, self.up, self.down, taps.ctypes.data_as(POINTER(c_double)), self.half,
                                              byref(h)))
        self._h = h

    def out_length(self, L):
        return out_length(L, self.up, self.down)

    def __call__(self, x, out=None):
        import torch
        if x.dim() not in (1, 2) or x.dtype != torch.float32 or x.device != self.ctx.device or (x.numel() and x.stride(-1) != 1):
            raise ValueError("Resampler takes a float32 tensor [L] or [n_clips, L] with contiguous rows on %s" % (self.ctx.device,))
        squeeze = x.dim() == 1
        n, L = (1, int(x.shape[0])) if squeeze else (int(x.shape[0]), int(x.shape[1]))
        M = self.out_length(L)
        with self.ctx.stream_scope():
            if out is None:
                out = torch.empty((n, M), dtype=torch.float32, device=x.device)
            elif tuple(out.shape) != (n, M) or out.dtype != torch.float32 or out.stride(1) != 1:
                raise ValueError("out must be a float32 %r tensor with contiguous rows" % ((n, M),))
            in_stride = L if squeeze else int(x.stride(0))
            _lib.check(self.ctx._lib.dcs_resample_f32(self._h, c_void_p(x.data_ptr()), L, n, in_stride,
                                                      c_void_p(out.data_ptr()), int(out.stride(0))))
        return out[0] if squeeze else out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_resample_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResampleCounts(object):
    """How far a streaming conversion has come after ``P`` input samples -- integers only (the formulas of
    ``dcs_resample_stream`` in include/dcs.h).  Output ``m`` touches inputs ``ceil((m down - half) / up) ..
    floor((m down + half) / up)``; mid-stream it is final once all of them are below ``P``."""

    def __init__(self, up, down, half):
        self.up, self.down, self.half = int(up), int(down), int(half)
        if self.up < 1 or self.down < 1 or self.half < 0:
            raise ValueError("ResampleCounts needs up, down >= 1 and half >= 0")

    def emitted(self, P, ended=False):
        P = int(P)
        if ended:
            return out_length(P, self.up, self.down)
        top = P * self.up - 1 - self.half
        return 0 if top < 0 else top // self.down + 1

    def history(self):
        """samples before ``P`` an output not yet emitted can reach: strictly fewer than this"""
        return 2 * self.half // self.up + 2

    def delay_samples(self):
        """input samples the outputs trail the input by (``half / up``)"""
        return self.half / float(self.up)


class StreamResampler(object):
    """``dcs_resample_stream``: ``rows`` signals converted ``fi -> fo`` in lock-step as they arrive.  ``push(x)`` takes the
    next samples (float32 device tensor ``[rows, n]`` with contiguous rows, ``n <= max_block``) and returns the outputs that
    became final, ``[rows, n_i]`` on the device; ``push(x, last=True)`` ends the signal and returns the rest.  The outputs,
    concatenated, are those of :class:`Resampler` on the whole signal bit for bit; the state is one ring of
    ``max_block + counts.history()`` samples per row."""

    def __init__(self, ctx, fi, fo, rows, max_block=65536, **design_kw):
        self.ctx, self.rows, self.max_block = ctx, int(rows), int(max_block)
        self.plan = ctx.resampler(fi, fo, **design_kw)
        self.counts = ResampleCounts(self.plan.up, self.plan.down, self.plan.half)
        h = c_void_p()
        _lib.check(ctx._lib.dcs_resample_stream_create(self.plan._h, self.rows, self.max_block, byref(h)))
        self._h = h
        self.pushed, self.emitted, self.ended = 0, 0, False

    def push(self, x=None, last=False):
        import torch
        n = 0 if x is None else int(x.shape[-1])
        if x is not None and (x.dim() != 2 or int(x.shape[0]) != self.rows or x.dtype != torch.float32
                              or x.device != self.ctx.device or (n and (x.stride(1) != 1 or x.stride(0) < n))):
            raise ValueError("StreamResampler.push takes a float32 [%d, n] tensor with contiguous rows on %s"
                             % (self.rows, self.ctx.device))
        want = max(0, self.counts.emitted(self.pushed + n, bool(last)) - self.emitted)
        got = ctypes.c_int64()
        with self.ctx.stream_scope():
            out = torch.empty((self.rows, want), dtype=torch.float32, device=self.ctx.device)
            _lib.check(self.ctx._lib.dcs_resample_stream_push(self._h, c_void_p(x.data_ptr()) if n else None,
                                                              int(x.stride(0)) if n else 0, n, 1 if last else 0,
                                                              c_void_p(out.data_ptr()) if want else None, want, want, byref(got)))
        self.pushed += n
        self.emitted += got.value
        self.ended = bool(last)
        if got.value != want:
            raise _lib.DcsError("dcs_resample_stream_push returned %d samples, the host counts say %d" % (got.value, want))
        return out

    def reset(self):
        _lib.check(self.ctx._lib.dcs_resample_stream_reset(self._h))
        self.pushed, self.emitted, self.ended = 0, 0, False

    @property
    def device_bytes(self):
        return int(self.ctx._lib.dcs_resample_stream_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_resample_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resample(audio, fi, fo, ctx=None, **kw):
    """Host array ``[L]`` or ``[n, L]`` at ``fi`` Hz -> float64 at ``fo`` Hz with the same leading shape (float32 on the
    device).  ``fi == fo`` returns an unchanged copy."""
    a = np.asarray(audio)
    if a.ndim not in (1, 2):
        raise ValueError("resample takes [L] or [n, L] arrays, got shape %r" % (a.shape,))
    if int(fi) == int(fo):
        return np.array(a, dtype=np.float64)
    if ctx is None:
        from .runtime import default_context
        ctx = default_context()
    rs = ctx.resampler(fi, fo, **kw)
    return ctx.to_host(rs(ctx.to_device(a, np.float32))).astype(np.float64)
