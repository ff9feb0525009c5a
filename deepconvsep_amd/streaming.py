"""Streaming separation: push blocks of audio, pull finished stems, constant memory (``dcs_stream``, csrc/stream.hip).

``Separator.separate`` and its siblings need the whole signal; :class:`StreamSeparator` takes it as it comes and returns, block
by block, the samples of the same computation (``stft_norm`` -> tiler -> network -> the cross-faded masks of
``dcs_mask_fold_apply`` on the unscaled magnitudes -> ``istft_norm``) as soon as no later input can change them: a fixed
``time_context * hop + frameSize`` samples behind the input at the most, in device memory that depends on the block size and
not on the length of the signal.

:class:`ScoreStreamSeparator` does it for the score-informed graphs: the score is known before the audio, so the harmonic masks
of every frame are formed as the frame arrives (``dcs_stream_create_score``).  With ``follow_scores`` the score is at nominal
tempo and the stream follows it as the audio arrives (``dcs_stream_set_follow``, ``align.ScoreFollower``).

:class:`ChannelStreamSeparator` does the same for a stereo signal -- the stems of ``Separator.separate_channels`` on one engine
-- :class:`StereoStreamSeparator` streams the one graph that is stereo by construction (``dsd_ild``: the network sees both
channels and answers per source and channel, ``dcs_stream_create_stereo``), and :class:`RateStream` puts any of them between two
streaming sample-rate converters (``dcs_resample_stream``) for audio at another rate than 44 100 Hz.

:class:`StreamCounts` is the host arithmetic of the schedule (the table in include/dcs.h); it needs neither the library nor a
GPU.
"""
import math

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


def stereo_ld(F):
    """floats per channel in a row of the stereo (ILD) graph's row layout: the bins rounded up to a multiple of 4"""
    return (int(F) + 3) // 4 * 4


def stereo_rows_from_tiles(tiles):
    """Lasagne tiles ``[n, C, tc, F]`` (NumPy) -> the row layout ``[n, tc, C, ld]`` ``dcs_model_forward_stereo`` reads: the
    channels of a frame side by side, columns ``F .. ld-1`` zero"""
    tiles = np.asarray(tiles)
    n, C, tc, F = tiles.shape
    rows = np.zeros((n, tc, C, stereo_ld(F)), dtype=tiles.dtype)
    rows[..., :F] = tiles.transpose(0, 2, 1, 3)
    return rows


def stereo_tiles_from_rows(rows, F):
    """the inverse, on any number of leading axes: ``[..., n, tc, C, ld]`` (NumPy, e.g. the ``[S, n, tc, C, ld]`` of
    ``Network.forward_stereo_tiles``) -> ``[..., n, C, tc, F]``"""
    rows = np.asarray(rows)
    if rows.ndim < 4 or rows.shape[-1] != stereo_ld(F):
        raise ValueError("rows %r are not [..., n, tc, C, %d]" % (rows.shape, stereo_ld(F)))
    return np.ascontiguousarray(np.swapaxes(rows[..., :int(F)], -2, -3))


class StreamSeparator(object):
    """``Separator.stream()``: the separator's model and STFT plan behind a stream.

    ``push(block)`` takes the next samples of a mono signal at 44 100 Hz (any length; blocks longer than ``max_block`` are cut)
    and returns the float64 samples ``[S, n_i]`` that became final, ``finish()`` ends the signal and returns the rest: the
    lengths add up to the signal's.  Between the two halves of the stream (``dcs_stream_push`` / ``dcs_stream_pull``) the tiles
    that became ready go through ``net.forward_raw(tiles, tie_mode, channel_major=True)[:S]``, the composition
    ``Separator.channel_spectra`` uses.  ``push_device`` / ``finish_device`` do the same on float32 device tensors.
    ``reset()`` starts another signal.  Single-input-channel graphs only."""

    def __init__(self, separator, max_block=65536, sample_rate=44100):
        self._check_graph(separator)
        if int(sample_rate) != 44100:
            raise ValueError("a stream takes 44 100 Hz audio, not %d Hz (convert the blocks first)" % int(sample_rate))
        if int(max_block) < 1:
            raise ValueError("max_block must be at least 1 sample")
        self.sep, self.ctx = separator, separator.ctx
        self.max_block = int(max_block)
        self.counts = StreamCounts(separator.frameSize, separator.hopSize, separator.tc, separator.overlap, separator.tiler)
        self._engine = None              # the device state: made by the first block
        self._pushed, self._ended = 0, False

    @staticmethod
    def _check_graph(separator):
        if separator.net.arch.C != 1 and separator.arch_name != 'dsd_ild':
            raise ValueError("stream feeds a single-input-channel graph; '%s' takes %d input channels, one per instrument of a "
                             "score: use stream_scoreinformed(melody)" % (separator.arch_name, separator.net.arch.C))
        separator._require_mono_graph("stream")

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


class ScoreStreamSeparator(StreamSeparator):
    """``Separator.stream_scoreinformed(melody)``: score-informed separation on a stream, with :class:`StreamSeparator`'s
    interface (so :class:`RateStream` wraps it as it wraps that one).

    ``melody`` is the note table ``[instruments, notes, 2*nharmonics+3]`` of ``score.melody_table`` for the WHOLE signal at
    44 100 Hz -- it is known before the audio arrives and read once.  A push forms the harmonic masks of the frames it
    completed (``filterSpec`` per absolute frame, the separator's ``score_normalise``), the tiles carry one channel per
    instrument, mask times scaled magnitudes, and the fold multiplies the cross-faded soft masks with the score-informed
    mixture on the unscaled magnitudes (the separator's ``score_mixture``).  The masks agree with the whole-file
    ``dcs_score_masks`` whenever no note row ends past the signal's frame count, which a table built with ``nframes`` = that
    count guarantees.

    ``follow_scores``: the score at NOMINAL tempo, one ``(on, off, names)`` per instrument as ``score.read_score`` returns it
    -- the case nobody can have aligned beforehand.  ``melody`` must then be the table in SCORE time, ``melody_table`` on the
    same files with ``nframes = score_frames(follow_scores)``.  The constructor builds the score's chroma at the separator's
    hop (``align.score_chroma``) and an ``align.ScoreFollower`` (``follower_args``: its ``window``, ``max_step``, ``back``,
    ``penalty``; ``fmin``, ``fmax``, ``tuning_freq``, ``floor`` of the audio's chroma; ``nharmonics``, ``decay`` of the
    score's); every push asks it where in the score its new frames are and paints their masks from there.  ``positions()``
    returns the score frames of the audio frames the last ``push`` / ``finish`` completed."""

    def __init__(self, separator, melody, max_block=65536, follow_scores=None, **follower_args):
        if separator.net.arch.C == 1:
            raise ValueError("stream_scoreinformed feeds one input channel per instrument of the score; '%s' takes one input "
                             "channel: use stream()" % separator.arch_name)
        if separator.arch_name == 'dsd_ild':
            raise ValueError("stream_scoreinformed: '%s' is no score-informed graph" % separator.arch_name)
        melody = np.ascontiguousarray(melody, dtype=np.float64)
        if melody.ndim != 3 or separator.net.arch.C != melody.shape[0]:
            raise ValueError("the network takes %d score channels, the note table has %d"
                             % (separator.net.arch.C, melody.shape[0] if melody.ndim else 0))
        if int(max_block) < 1:
            raise ValueError("max_block must be at least 1 sample")
        self.sep, self.ctx = separator, separator.ctx
        self.melody = melody
        self.max_block = int(max_block)
        self.counts = StreamCounts(separator.frameSize, separator.hopSize, separator.tc, separator.overlap, separator.tiler)
        self._engine = None              # the device state: made by the first block
        self._pushed, self._ended = 0, False
        self._follow = None
        if follow_scores is None:
            if follower_args:
                raise TypeError("unexpected arguments without follow_scores: %s" % ", ".join(sorted(follower_args)))
            return
        from . import align
        known = set(align.FOLLOWER_ARGS) | {"fmin", "fmax", "tuning_freq", "floor", "nharmonics", "decay"}
        if set(follower_args) - known:
            raise TypeError("unexpected arguments: %s" % ", ".join(sorted(set(follower_args) - known)))
        follow_scores = list(follow_scores)
        if len(follow_scores) != melody.shape[0]:
            raise ValueError("the note table has %d instruments, follow_scores %d" % (melody.shape[0], len(follow_scores)))
        U = score_frames(follow_scores, separator.hopSize)
        table_end = float(melody[:, :, 1].max()) if melody.shape[1] else 0.0
        if table_end > U:
            raise ValueError("with follow_scores the note table is in score time: its last note ends at frame %d, the score has %d "
                             "frames (build it with nframes = score_frames(follow_scores, hopSize))" % (int(table_end), U))
        self._score_S = align.score_chroma(follow_scores, U, separator.hopSize, 44100,
                                           **{k: follower_args[k] for k in ("nharmonics", "decay") if k in follower_args})
        self._classes = align.bin_classes(separator.frameSize, 44100,
                                          **{k: follower_args[k] for k in ("fmin", "fmax", "tuning_freq") if k in follower_args})
        self._floor = float(follower_args.get("floor", 1e-6))
        self._follow_args = {k: follower_args[k] for k in align.FOLLOWER_ARGS if k in follower_args}
        # one launch of the follower takes all the frames one push of the stream can complete
        self._follow_args["max_frames"] = max(int(self._follow_args.get("max_frames", 4096)), self.counts.max_frames(self.max_block))
        self._follow = align.ScoreFollower(self.ctx, self._score_S, **self._follow_args)
        self._positions = []

    def _stream(self):
        if self._engine is None:
            from .runtime import ScoreStream
            s = self.sep
            follow = dict(follow=self._follow, classes=self._classes, floor=self._floor) if self._follow is not None else {}
            self._engine = ScoreStream(s.plan, s.net.S, self.melody, s.tc, s.overlap, s.tiler, s.net.arch.eps_mode,
                                       s.scale_factor, self.max_block, s.score_normalise, s.score_mixture, **follow)
        return self._engine

    def _step(self, piece, last):
        pcm = StreamSeparator._step(self, piece, last)
        if self._follow is not None:
            self._positions.append(self._engine.positions())
        return pcm

    def push_device(self, block_t):
        if self._follow is not None:
            self._positions = []
        return StreamSeparator.push_device(self, block_t)

    def finish_device(self):
        if self._follow is not None:
            self._positions = []
        return StreamSeparator.finish_device(self)

    def reset(self):
        StreamSeparator.reset(self)      # the engine's reset resets the follower too
        if self._follow is not None:
            self._positions = []

    def close(self):
        """frees the device state: the stream first, then the follower it reads (which must outlive the stream's pushes)"""
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
            self._engine = None
        if getattr(self, "_follow", None) is not None:
            self._follow.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def positions(self):
        """int32 NumPy: the score frame of every audio frame the last ``push`` / ``finish`` completed (it waits for the device)"""
        if self._follow is None:
            raise ValueError("this stream follows no score (stream_scoreinformed(melody, follow_scores=...))")
        torch = _runtime()._torch()
        if not self._positions:
            return np.zeros(0, dtype=np.int32)
        with self.ctx.stream_scope():
            return torch.cat(self._positions).cpu().numpy()

    @property
    def device_bytes(self):
        """``dcs_stream_bytes`` plus, on a followed stream, the follower's ``dcs_follow_bytes``"""
        return self._stream().bytes + (self._follow.device_bytes if self._follow is not None else 0)


def score_frames(scores, hop, sample_rate=44100):
    """frames of a score at nominal tempo, ``ceil(end * fps) + 1`` -- the ``U`` of ``align.align_scores`` and of a followed
    stream, and the ``nframes`` its note table is built with"""
    end = max([float(np.max(off)) for _, off, _ in scores if len(off)] or [0.0])
    return int(math.ceil(end * float(sample_rate) / float(hop))) + 1


class ChannelStreamSeparator(object):
    """``Separator.stream_channels()``: stereo stems from a mono model on a stream -- what ``Separator.separate_channels``
    computes on a whole file (the cross-faded masks of the down-mix on each channel's own magnitudes, inverted with that
    channel's phase), block by block on ONE engine (``dcs_stream_create_channels``): one ring of ``p``, one fold.
    ``mwf_iters > 0``: every pull sends the frames it folded through that many iterations of the ONLINE multichannel Wiener
    filter (``runtime.MwfOnline``; ``mwf_forget``, ``mwf_loading`` its parameters) before the inverse, each (channel, source)
    then with its own phase.  That filter is causal -- it is not ``separate_channels(mwf_iters=...)`` and does not match it: the
    first frames of a signal are filtered on little evidence.

    ``push(block)`` takes the next samples ``[n, 2]`` of a 44 100 Hz signal and returns the float64 samples ``[n_i, S, 2]`` that
    became final, ``finish()`` ends the signal and returns the rest.  The down-mix the network sees is formed on the host in
    float64 (``to_mono``), so its input is bit for bit that of ``StreamSeparator`` on ``to_mono(block)``.  ``push_device`` /
    ``finish_device`` take float32 device tensors ``[3, n]`` (L, R, down-mix) and return ``[2, S, n_i]``.  Single-input-channel
    graphs only."""

    channels = 2
    rows_in = 3                      # signal rows a device block carries: L, R, down-mix

    def __init__(self, separator, max_block=65536, mwf_iters=0, mwf_forget=1.0, mwf_loading=1e-3):
        separator._require_mono_graph("stream_channels")
        if int(max_block) < 1:
            raise ValueError("max_block must be at least 1 sample")
        self._set_mwf(mwf_iters, mwf_forget, mwf_loading)
        self.sep, self.ctx = separator, separator.ctx
        self.max_block = int(max_block)
        self.counts = StreamCounts(separator.frameSize, separator.hopSize, separator.tc, separator.overlap, separator.tiler)
        self._engine = None              # the device state: made by the first block
        self._pushed, self._ended = 0, False

    @property
    def S(self):
        return self.sep.net.S

    def _set_mwf(self, iters, forget, loading):
        self.mwf = (int(iters), float(forget), float(loading))
        if not 0 <= self.mwf[0] <= 100:
            raise ValueError("mwf_iters %d not in 0 .. 100" % self.mwf[0])

    def _arm(self, engine):
        if self.mwf[0]:
            engine.set_mwf(self.mwf[0], forget=self.mwf[1], loading=self.mwf[2])
        return engine

    def _stream(self):
        if self._engine is None:
            from .runtime import ChannelStream
            s = self.sep
            self._engine = self._arm(ChannelStream(s.plan, s.net.S, self.channels, s.tc, s.overlap, s.tiler, s.net.arch.eps_mode,
                                                   s.scale_factor, self.max_block))
        return self._engine

    def _step(self, piece, last):
        """one push -> network -> pull; ``piece`` float32 device tensor ``[3, n]`` or None"""
        eng = self._stream()
        tiles = eng.push(piece, last=last)
        p = None
        if int(tiles.shape[0]):
            p = self.sep.net.forward_raw(tiles, self.sep.tie_mode, channel_major=True)[:self.S]
        return eng.pull(p)

    def push_device(self, a3):
        """``a3`` float32 device tensor ``[3, n]`` (L, R, down-mix; ``[2, n]``, L and R, for a :class:`StereoStreamSeparator`) ->
        float32 ``[2, S, n_i]`` on the device"""
        torch = _runtime()._torch()
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        if a3.dim() != 2 or int(a3.shape[0]) != self.rows_in:
            raise ValueError("this stream takes [%d, n] tensors (L, R%s), got shape %r"
                             % (self.rows_in, ", down-mix" if self.rows_in == 3 else "", tuple(a3.shape)))
        with self.ctx.stream_scope():
            n = int(a3.shape[1])
            outs = [self._step(a3[:, i:i + self.max_block], False) for i in range(0, n, self.max_block)]
            self._pushed += n
            if len(outs) == 1:
                return outs[0]
            if not outs:
                return torch.empty((self.channels, self.S, 0), dtype=torch.float32, device=self.ctx.device)
            return torch.cat(outs, dim=2)

    def finish_device(self):
        """ends the signal -> the remaining float32 samples ``[2, S, rest]`` on the device.  A signal too short for one tile
        raises what ``Separator.separate_channels`` raises for it."""
        if self._ended:
            raise ValueError("the stream has ended: finish() was already called (reset() starts another signal)")
        self._ended = True
        if self.counts.tiles(self._pushed, True) == 0:
            raise IndexError("tuple index out of range")  # what overlapadd_multi hits on an empty output array
        with self.ctx.stream_scope():
            return self._step(None, True)

    def _to_host(self, pcm):
        return np.ascontiguousarray(self.ctx.to_host(pcm).astype(np.float64).transpose(2, 1, 0))      # [n_i, S, 2]

    def push(self, block):
        from .separation import to_mono
        block = np.asarray(block)
        if block.ndim != 2 or block.shape[1] != self.channels:
            raise ValueError("a channel stream takes stereo blocks ([n, 2] arrays), got shape %r" % (block.shape,))
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        a3 = np.stack([block[:, 0], block[:, 1], to_mono(block, self.sep.arch_name)])
        return self._to_host(self.push_device(self.ctx.to_device(a3, np.float32)))

    def finish(self):
        return self._to_host(self.finish_device())

    def reset(self):
        if self._engine is not None:
            self._engine.reset()
        self._pushed, self._ended = 0, False

    @property
    def device_bytes(self):
        """device bytes the stream holds (``dcs_stream_bytes``): a function of the shapes and ``max_block`` alone"""
        return self._stream().bytes


class StereoStreamSeparator(ChannelStreamSeparator):
    """``Separator.stream_stereo()``: the stereo (ILD) DSD100 graph on a stream -- what ``Separator.separate_stereo`` computes
    on a whole file (two-channel tiles from the library tiler, one network pass per tile, the stereo trainer's mask per channel,
    cross-faded, on that channel's own magnitudes and phase), block by block (``dcs_stream_create_stereo``).

    ``push(block)`` takes the next samples ``[n, 2]`` of a 44 100 Hz signal and returns the float64 samples ``[n_i, S, 2]`` that
    became final, ``finish()`` ends the signal and returns the rest; ``push_device`` / ``finish_device`` take float32 device
    tensors ``[2, n]`` and return ``[2, S, n_i]``.  Between the two halves of the stream the tiles that became ready go through
    ``net.forward_stereo_tiles``.  ``reset``, ``device_bytes`` and ``counts`` as in the other classes.  The ``dsd_ild`` graph
    only (``ValueError`` otherwise).  ``mwf_iters > 0`` arms the ONLINE multichannel Wiener filter as in
    :class:`ChannelStreamSeparator`: causal, not ``separate_stereo(mwf_iters=...)``, whose statistics run over the whole
    signal, and not expected to match it -- the first frames of a signal are filtered on little evidence."""

    rows_in = 2                      # signal rows a device block carries: no down-mix

    def __init__(self, separator, max_block=65536, mwf_iters=0, mwf_forget=1.0, mwf_loading=1e-3):
        if separator.arch_name != 'dsd_ild':
            raise ValueError("stream_stereo runs the stereo (ILD) graph; '%s' takes %d input channel(s): use stream() or "
                             "stream_channels()" % (separator.arch_name, separator.net.arch.C))
        if int(max_block) < 1:
            raise ValueError("max_block must be at least 1 sample")
        self._set_mwf(mwf_iters, mwf_forget, mwf_loading)
        self.sep, self.ctx = separator, separator.ctx
        self.max_block = int(max_block)
        # the library tiler whatever the separator's: the stereo trainer calls util.generate_overlapadd (separate_stereo)
        self.counts = StreamCounts(separator.frameSize, separator.hopSize, separator.tc, separator.overlap, TILER_LIBRARY)
        self._engine = None              # the device state: made by the first block
        self._pushed, self._ended = 0, False

    def _stream(self):
        if self._engine is None:
            from .runtime import StereoStream
            s = self.sep
            self._engine = self._arm(StereoStream(s.plan, s.net.S, self.channels, s.tc, s.overlap, TILER_LIBRARY, s.scale_factor,
                                                  self.max_block))
        return self._engine

    def _step(self, piece, last):
        """one push -> network -> pull; ``piece`` float32 device tensor ``[2, n]`` or None"""
        eng = self._stream()
        tiles = eng.push(piece, last=last)
        p = self.sep.net.forward_stereo_tiles(tiles) if int(tiles.shape[0]) else None
        return eng.pull(p)

    def push(self, block):
        block = np.asarray(block)
        if block.ndim != 2 or block.shape[1] != self.channels:
            raise ValueError("a stereo stream takes stereo blocks ([n, 2] arrays), got shape %r" % (block.shape,))
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        return self._to_host(self.push_device(self.ctx.to_device(np.ascontiguousarray(block.T), np.float32)))


class RateStream(object):
    """A stream at any sample rate: ``inner`` (a :class:`StreamSeparator`, a :class:`ChannelStreamSeparator` or a
    :class:`StereoStreamSeparator`) between two streaming converters (``dcs_resample_stream``) -- ``sample_rate -> 44 100`` on
    the 1, 3 or 2 signal rows in front, ``44 100 -> sample_rate`` on the ``S`` or ``2 S`` stems behind.  ``push`` takes blocks at ``sample_rate`` in the layout ``inner`` takes
    and returns the finished stems at ``sample_rate`` in the layout ``inner`` returns; ``finish()`` flushes the three stages and
    crops, as the whole-file paths do (``Separator._at_model_rate``), so that the lengths add up to the samples pushed.  Each
    stage's outputs are those of the whole-file conversion bit for bit, so the result is the whole-file ``Resampler`` in front,
    ``inner`` on the 44 100 Hz signal cut where the converter's counts cut it, and the whole-file ``Resampler`` behind.  All
    device state is sized by ``inner.max_block`` and the filter design; ``sample_rate == 44100`` passes straight through."""

    def __init__(self, inner, sample_rate):
        from .resample import TARGET_RATE
        if not isinstance(inner, (StreamSeparator, ChannelStreamSeparator)):
            raise TypeError("RateStream wraps a StreamSeparator, a ChannelStreamSeparator or a StereoStreamSeparator, got %r"
                            % (type(inner).__name__,))
        if int(sample_rate) != sample_rate or int(sample_rate) < 1:
            raise ValueError("sample_rate must be a positive integer, got %r" % (sample_rate,))
        self.inner, self.ctx = inner, inner.ctx
        self.sample_rate, self.model_rate = int(sample_rate), TARGET_RATE
        self.stereo = isinstance(inner, ChannelStreamSeparator)
        self.max_block = inner.max_block
        self.passthrough = self.sample_rate == self.model_rate
        self._down = self._up = None     # the converters: made by the first block
        self._pushed = self._emitted = 0
        self._ended = False

    @property
    def S(self):
        return self.inner.S

    def _stages(self):
        if self._down is None:
            from .resample import StreamResampler
            rows_in, rows_out = (self.inner.rows_in, 2 * self.S) if self.stereo else (1, self.S)
            self._down = StreamResampler(self.ctx, self.sample_rate, self.model_rate, rows_in, self.max_block)
            self._up = StreamResampler(self.ctx, self.model_rate, self.sample_rate, rows_out, self.max_block)
        return self._down, self._up

    def latency_samples(self):
        """Mid-stream ``pushed - emitted < latency_samples()`` (input samples at ``sample_rate``) once output has started: with
        ``r = sample_rate / 44100``, the front filter's ``(half + 1) / up`` input samples, plus ``r`` times the inner stream's
        look-ahead (``StreamCounts.latency_samples``) and the back filter's ``(half + 1) / up`` samples at 44 100 Hz."""
        if self.passthrough:
            return self.inner.counts.latency_samples()
        from .resample import design
        up_d, _, _, half_d = design(self.sample_rate, self.model_rate)
        up_u, down_u, _, half_u = design(self.model_rate, self.sample_rate)
        bound = (half_d + 1) / float(up_d) + (self.inner.counts.latency_samples() * up_u + half_u + 1) / float(down_u)
        return int(np.ceil(bound))

    def _back(self, pcm, last):
        """the stems at 44 100 Hz (``[S, n]`` or ``[2, S, n]``; None: none) through the back converter, in pieces of at most
        ``max_block``"""
        torch = _runtime()._torch()
        _, up = self._stages()
        rows = pcm.reshape(up.rows, int(pcm.shape[-1])) if pcm is not None else None
        n = 0 if rows is None else int(rows.shape[1])
        cuts = list(range(0, n, self.max_block)) or [0]
        outs = []
        for i in cuts:
            piece = rows[:, i:i + self.max_block] if n else None
            outs.append(up.push(piece, last=last and i == cuts[-1]))
        out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        if last:                                                    # ceil(ceil(L u / d) d / u) >= L: crop, as _at_model_rate
            out = out[:, :max(0, self._pushed - self._emitted)]
        self._emitted += int(out.shape[1])
        return out.reshape(2, self.S, int(out.shape[1])) if self.stereo else out

    def push_device(self, x):
        """``x`` float32 device tensor at ``sample_rate``: ``[n]`` (mono inner), ``[3, n]`` (L, R, down-mix) or ``[2, n]`` (a
        :class:`StereoStreamSeparator`) -> the finished
        stems at ``sample_rate``, ``[S, n_i]`` or ``[2, S, n_i]``"""
        if self.passthrough:
            return self.inner.push_device(x)
        torch = _runtime()._torch()
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        if x.dim() != (2 if self.stereo else 1) or (self.stereo and int(x.shape[0]) != self.inner.rows_in):
            raise ValueError("this stream takes %s tensors, got shape %r"
                             % ("[%d, n]" % self.inner.rows_in if self.stereo else "[n]", tuple(x.shape)))
        down, _ = self._stages()
        with self.ctx.stream_scope():
            rows = x if self.stereo else x.reshape(1, int(x.shape[0]))
            n = int(rows.shape[1])
            outs = []
            for i in range(0, n, self.max_block):
                y = down.push(rows[:, i:i + self.max_block].contiguous())
                self._pushed += int(min(self.max_block, n - i))
                outs.append(self._back(self.inner.push_device(y if self.stereo else y[0]), False))
            if len(outs) == 1:
                return outs[0]
            if not outs:
                shape = (2, self.S, 0) if self.stereo else (self.S, 0)
                return torch.empty(shape, dtype=torch.float32, device=self.ctx.device)
            return torch.cat(outs, dim=-1)

    def finish_device(self):
        """ends the signal: flushes the front converter, the inner stream and the back converter -> the remaining stems,
        cropped so that the lengths add up to the samples pushed"""
        if self.passthrough:
            return self.inner.finish_device()
        torch = _runtime()._torch()
        if self._ended:
            raise ValueError("the stream has ended: finish() was already called (reset() starts another signal)")
        self._ended = True
        down, _ = self._stages()
        with self.ctx.stream_scope():
            y = down.push(None, last=True)
            first = self.inner.push_device(y if self.stereo else y[0])
            rest = self.inner.finish_device()
            return torch.cat([self._back(first, False), self._back(rest, True)], dim=-1)

    def push(self, block):
        if self.passthrough:
            return self.inner.push(block)
        from .separation import to_mono
        block = np.asarray(block)
        if self._ended:
            raise ValueError("the stream has ended: reset() starts another signal")
        if self.stereo:
            if block.ndim != 2 or block.shape[1] != 2:
                raise ValueError("this stream takes stereo blocks ([n, 2] arrays), got shape %r" % (block.shape,))
            rows = [block[:, 0], block[:, 1]]
            if self.inner.rows_in == 3:
                rows.append(to_mono(block, self.inner.sep.arch_name))
            block = np.stack(rows)
        elif block.ndim != 1:
            raise ValueError("this stream takes mono blocks ([n] arrays), got shape %r" % (block.shape,))
        return self._to_host(self.push_device(self.ctx.to_device(block, np.float32)))

    def finish(self):
        if self.passthrough:
            return self.inner.finish()
        return self._to_host(self.finish_device())

    def _to_host(self, pcm):
        return self.inner._to_host(pcm) if self.stereo else self.ctx.to_host(pcm).astype(np.float64)

    def reset(self):
        self.inner.reset()
        for st in (self._down, self._up):
            if st is not None:
                st.reset()
        self._pushed = self._emitted = 0
        self._ended = False

    @property
    def device_bytes(self):
        """the inner stream's bytes plus the two converters' rings"""
        if self.passthrough:
            return self.inner.device_bytes
        down, up = self._stages()
        return self.inner.device_bytes + down.device_bytes + up.device_bytes


def _runtime():
    from . import runtime
    return runtime
