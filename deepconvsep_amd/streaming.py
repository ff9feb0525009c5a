"""Streaming separation: push blocks of audio, pull finished stems, constant memory (``dcs_stream``, csrc/stream.hip).

``Separator.separate`` and its siblings need the whole signal; :class:`StreamSeparator` takes it as it comes and returns, block
by block, the samples of the same computation (``stft_norm`` -> tiler -> network -> the cross-faded masks of
``dcs_mask_fold_apply`` on the unscaled magnitudes -> ``istft_norm``) as soon as no later input can change them: a fixed
``time_context * hop + frameSize`` samples behind the input at the most, in device memory that depends on the block size and
not on the length of the signal.

:class:`StreamCounts` is the host arithmetic of the schedule (the table in include/dcs.h); it needs neither the library nor a
GPU.
"""
import numpy as np

from .arch import TILER_LIBRARY, TILER_SCRIPT

_TILER_CODES = {'script': TILER_SCRIPT, 'library': TILER_LIBRARY, TILER_SCRIPT: TILER_SCRIPT, TILER_LIBRARY: TILER_LIBRARY}


class StreamCounts(object):
    """How far each stage of a stream has come after ``P`` pushed samples -- integers only.

    ``N`` frameSize, ``h`` hop, ``H = N / 2``, ``st = tc - ov``.  Mid-stream a frame counts once all its ``N`` samples are in, a
    tile once its ``tc`` frames are, a frame is folded once no later tile can reach it (``t < K st``) and a sample emitted once
    no later frame can (``q + H < Tf h``).  ``ended=True``: ``P`` is the signal's length ``L`` and the counts are the
    whole-file ones (``dcs_frame_count``, ``dcs_tile_count``, every frame, every sample)."""

    def __init__(self, frame, hop, time_context, overlap, tiler='script'):
        self.N, self.h, self.tc, self.ov = int(frame), int(hop), int(time_context), int(overlap)
        self.H, self.st = self.N // 2, self.tc - self.ov
        self.tiler = _TILER_CODES[tiler]
        if self.N < 2 or self.N & (self.N - 1):
            raise ValueError("frameSize %d is not a power of two" % self.N)
        if self.h < 1 or self.h > self.H or self.N % self.h:
            raise ValueError("hopSize %d must divide frameSize %d and be at most half of it" % (self.h, self.N))
        if not 1 <= self.ov < self.tc:
            raise ValueError("overlap %d not in [1, %d)" % (self.ov, self.tc))

    def frames(self, P, ended=False):
        P = int(P)
        if ended:
            return -(-P // self.h) + 2                                   # int(ceil(L / hop) + 2), transform.py:309
        return 0 if P < self.H else (P - self.H) // self.h + 1

    def tiles(self, P, ended=False):
        A = self.frames(P, ended)
        if not ended:
            return 0 if A < self.tc else (A - self.tc) // self.st + 1
        guard = self.tc if self.tiler == TILER_SCRIPT else self.ov       # tiles while start + guard < T
        return 0 if A <= guard else (A - guard - 1) // self.st + 1

    def folded(self, P, ended=False):
        return self.frames(P, True) if ended else self.tiles(P) * self.st

    def emitted(self, P, ended=False):
        return int(P) if ended else max(0, self.folded(P) * self.h - self.H)

    def latency_samples(self):
        """Mid-stream ``P - emitted(P) < latency_samples()`` once the first tile is ready."""
        return self.tc * self.h + self.N

    # what one push of at most max_push samples can produce, the end included (the ring sizes of csrc/stream.hip)
    def max_frames(self, max_push):
        return (int(max_push) + self.H + self.h - 1) // self.h + 3

    def max_tiles(self, max_push):
        return (self.max_frames(max_push) + self.st - 1) // self.st + 2


class StreamSeparator(object):
    """``Separator.stream()``: the separator's model and STFT plan behind a stream.

    ``push(block)`` takes the next samples of a mono signal at 44 100 Hz (any length; blocks longer than ``max_block`` are cut)
    and returns the float64 samples ``[S, n_i]`` that became final, ``finish()`` ends the signal and returns the rest: the
    lengths add up to the signal's.  Between the two halves of the stream (``dcs_stream_push`` / ``dcs_stream_pull``) the tiles
    that became ready go through ``net.forward_raw(tiles, tie_mode, channel_major=True)[:S]``, the composition
    ``Separator.channel_spectra`` uses.  ``push_device`` / ``finish_device`` do the same on float32 device tensors.
    ``reset()`` starts another signal.  Single-input-channel graphs only."""

    def __init__(self, separator, max_block=65536, sample_rate=44100):
        separator._require_mono_graph("stream")
        if int(sample_rate) != 44100:
            raise ValueError("a stream takes 44 100 Hz audio, not %d Hz (convert the blocks first)" % int(sample_rate))
        if int(max_block) < 1:
            raise ValueError("max_block must be at least 1 sample")
        self.sep, self.ctx = separator, separator.ctx
        self.max_block = int(max_block)
        self.counts = StreamCounts(separator.frameSize, separator.hopSize, separator.tc, separator.overlap, separator.tiler)
        self._engine = None              # the device state: made by the first block
        self._pushed, self._ended = 0, False

    @property
    def S(self):
        return self.sep.net.S

    def _stream(self):
        if self._engine is None:
            from .runtime import Stream
            s = self.sep
            self._engine = Stream(s.plan, s.net.S, s.tc, s.overlap, s.tiler, s.net.arch.eps_mode, s.scale_factor,
                                  self.max_block)
        return self._engine

    def _step(self, piece, last):
        """one push -> network -> pull; ``piece`` float32 device tensor ``[n]`` or None"""
        eng = self._stream()
        tiles = eng.push(piece, last=last)
        p = None
        if int(tiles.shape[0]):
            p = self.sep.net.forward_raw(tiles, self.sep.tie_mode, channel_major=True)[:self.S]
        return eng.pull(p)

    def push_device(self, block_t):
        """``block_t`` float32 device tensor ``[n]`` -> float32 ``[S, n_i]`` on the device"""
        torch = _runtime()._torch()
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        if block_t.dim() != 1:
            raise ValueError("a stream takes mono blocks ([n] tensors), got shape %r" % (tuple(block_t.shape),))
        with self.ctx.stream_scope():
            block_t = block_t.contiguous()
            outs = [self._step(block_t[i:i + self.max_block], False) for i in range(0, int(block_t.numel()), self.max_block)]
            self._pushed += int(block_t.numel())
            if len(outs) == 1:
                return outs[0]
            if not outs:
                return torch.empty((self.S, 0), dtype=torch.float32, device=self.ctx.device)
            return torch.cat(outs, dim=1)

    def finish_device(self):
        """ends the signal -> the remaining float32 samples ``[S, rest]`` on the device.  A signal too short for one tile raises
        what ``Separator.separate_channels`` raises for it."""
        if self._ended:
            raise ValueError("the stream has ended: finish() was already called (reset() starts another signal)")
        self._ended = True
        if self.counts.tiles(self._pushed, True) == 0:
            raise IndexError("tuple index out of range")  # what overlapadd_multi hits on an empty output array
        with self.ctx.stream_scope():
            return self._step(None, True)

    def push(self, block):
        block = np.asarray(block)
        if block.ndim != 1:
            raise ValueError("a stream takes mono blocks ([n] arrays), got shape %r" % (block.shape,))
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        return self.ctx.to_host(self.push_device(self.ctx.to_device(block, np.float32))).astype(np.float64)

    def finish(self):
        pcm = self.finish_device()
        return self.ctx.to_host(pcm).astype(np.float64)

    def reset(self):
        if self._engine is not None:
            self._engine.reset()
        self._pushed, self._ended = 0, False

    @property
    def device_bytes(self):
        """device bytes the stream holds (``dcs_stream_bytes``): a function of the shapes and ``max_block`` alone"""
        return self._stream().bytes


def _runtime():
    from . import runtime
    return runtime
