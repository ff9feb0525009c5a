"""Score-to-audio alignment: put a score at nominal tempo onto the recording before the harmonic masks are painted.

Every score-informed entry point assumes that the ``<inst>_b.txt`` files are already in the recording's time.  Bach10 ships
hand-aligned scores; a MIDI or notation export does not.  This module aligns one:

  audio -> magnitudes (the STFT plan) -> chroma per frame (``dcs_chroma``)   |
  score  -> chroma per frame of the score's own time (host, a few hundred notes) |-> DTW (``dcs_dtw``) -> path
  path -> time map (score frame -> audio frame) -> warped onsets and offsets

The two hot steps run on the GPU (csrc/align.hip); there is no CPU path for them.  The reference has no counterpart.

That needs the whole recording.  :class:`ScoreFollower` (csrc/follow.hip) is the causal form with constant memory -- one DTW row
over a window of score frames per audio frame that arrives -- which a score stream uses (``runtime.ScoreStream(follow=...)``);
:func:`follow_scores` runs it over a file so that the two alignments can be compared.
"""
import math
import os
from ctypes import c_void_p

import numpy as np

from . import _lib
from .score import read_score, str2midi, write_score

AUTO_BAND_CELLS = 1 << 26          # band='auto': no band up to this many cells, ceil(max(T, U) / 8) beyond


def bin_classes(frameSize, sampleRate=44100, fmin=100., fmax=5000., tuning_freq=440.):
    """int8 ``[frameSize/2+1]``: the pitch class (0 = C ... 9 = A ... 11 = B) of every FFT bin whose centre frequency lies in
    ``[fmin, fmax]``, -1 for the others (bin 0 included) -- ``int(floor(12 log2(f / tuning) + 69 + 0.5)) mod 12`` in float64."""
    F = int(frameSize) // 2 + 1
    f = np.arange(F, dtype=np.float64) * (float(sampleRate) / float(frameSize))
    cls = np.full(F, -1, dtype=np.int8)
    use = (f >= float(fmin)) & (f <= float(fmax)) & (f > 0)
    midi = np.floor(12.0 * np.log2(f[use] / float(tuning_freq)) + 69.0 + 0.5).astype(np.int64)
    cls[use] = (midi % 12).astype(np.int8)
    return cls


def score_chroma(scores, U, hop, sampleRate, nharmonics=6, decay=0.7):
    """Chroma ``[U, 12]`` float32 of a score in its own time.  ``scores``: one ``(on, off, names)`` per instrument, as
    :func:`deepconvsep_amd.score.read_score` returns it.  Frame ``u`` stands for time ``u * hop / sampleRate`` (the STFT's frame
    ``n`` is centred on sample ``n * hop``); a note covers the frames ``ceil(on * fps) <= u < ceil(off * fps)`` with ``fps =
    sampleRate / hop`` exactly; harmonic ``k = 1 .. nharmonics`` adds ``decay ** (k - 1)`` to the class ``(midi + int(floor(12
    log2 k + 0.5))) mod 12``; the instruments are summed, rows L2-normalised (float64, rounded once), an empty row is
    ``1 / sqrt(12)`` in every class."""
    U = int(U)
    fps = float(sampleRate) / float(hop)
    acc = np.zeros((U, 12), dtype=np.float64)
    shift = [int(math.floor(12.0 * math.log2(k) + 0.5)) for k in range(1, int(nharmonics) + 1)]
    weight = [float(decay) ** k for k in range(int(nharmonics))]
    for on, off, names in scores:
        for a, b, name in zip(np.asarray(on, dtype=np.float64), np.asarray(off, dtype=np.float64), names):
            midi = str2midi(name)
            if not midi > 0:
                continue
            u0, u1 = max(0, int(math.ceil(a * fps))), min(U, int(math.ceil(b * fps)))
            if u1 <= u0:
                continue
            for s, w in zip(shift, weight):
                acc[u0:u1, (int(midi) + s) % 12] += w
    norm = np.sqrt((acc * acc).sum(axis=1))
    out = np.full((U, 12), 1.0 / math.sqrt(12.0), dtype=np.float64)
    live = norm > 0
    out[live] = acc[live] / norm[live, None]
    return out.astype(np.float32)


def chroma(ctx, mag_t, classes, floor=1e-6):
    """``dcs_chroma``: ``mag_t`` ``[T, F]`` float32 device tensor (rows contiguous, any row pitch), ``classes`` the int8 table
    of :func:`bin_classes` -> ``[T, 12]`` float32 device tensor of unit-norm rows (uniform where the norm is not above
    ``floor``)."""
    from .runtime import _ptr, _torch
    torch = _torch()
    if mag_t.dim() != 2 or mag_t.stride(1) != 1 or mag_t.dtype != torch.float32:
        raise ValueError("chroma expects a float32 [frames, bins] tensor with contiguous rows")
    cls = np.ascontiguousarray(classes, dtype=np.int8)
    T, F = int(mag_t.shape[0]), int(mag_t.shape[1])
    if cls.shape != (F,):
        raise ValueError("classes must have one entry per bin (%d), got %r" % (F, cls.shape))
    with ctx.stream_scope():
        out = torch.empty((T, 12), dtype=torch.float32, device=mag_t.device)
        _lib.check(ctx._lib.dcs_chroma(ctx._h, _ptr(mag_t), int(mag_t.stride(0)) if T > 1 else F, T, F,
                                       c_void_p(cls.ctypes.data), float(floor), _ptr(out)))
    return out


def dtw_bytes(T, U, band=None):
    """Device scratch ``dtw`` takes for this shape (``dcs_dtw_bytes``)."""
    n = int(_lib.load().dcs_dtw_bytes(int(T), int(U), -1 if band is None else int(band)))
    if n < 0:
        raise ValueError(_lib.load().dcs_last_error().decode("utf-8", "replace"))
    return n


def dtw(ctx, A_t, S_t, band=None):
    """``dcs_dtw``: ``A_t`` ``[T, 12]``, ``S_t`` ``[U, 12]`` float32 device tensors -> ``(path [n, 2] int32 NumPy, cost)``, the
    cells ``(t, u)`` of the cheapest monotone path from ``(0, 0)`` to ``(T-1, U-1)`` under ``c = 1 - <a, s>`` and its cost.
    ``band``: cells further than ``band`` score frames from the straight line are excluded (None: no band).  Only the path
    and two scalars come back to the host.  ``ValueError`` when the band leaves no path."""
    from .runtime import _ptr, _torch
    torch = _torch()
    for x in (A_t, S_t):
        if x.dim() != 2 or int(x.shape[1]) != 12 or x.dtype != torch.float32:
            raise ValueError("dtw expects float32 [frames, 12] tensors")
    T, U = int(A_t.shape[0]), int(S_t.shape[0])
    with ctx.stream_scope():
        A_t, S_t = A_t.contiguous(), S_t.contiguous()
        path = torch.empty((max(T + U - 1, 1), 2), dtype=torch.int32, device=A_t.device)
        n = torch.zeros((1,), dtype=torch.int64, device=A_t.device)
        cost = torch.empty((1,), dtype=torch.float32, device=A_t.device)
        _lib.check(ctx._lib.dcs_dtw(ctx._h, _ptr(A_t), T, _ptr(S_t), U, -1 if band is None else int(band), _ptr(path), _ptr(n),
                                    _ptr(cost)))
        n_h = int(n.cpu().item())
        cost_h = float(cost.cpu().item())
        if n_h == 0:
            raise ValueError("dtw: band %r leaves no path from (0, 0) to (%d, %d)" % (band, T - 1, U - 1))
        return path[:n_h].cpu().numpy(), cost_h


def time_map(path, U):
    """For every score frame ``u`` the mean audio frame ``t`` of its path points: float64 ``[U]``, non-decreasing (a monotone
    path visits every ``u``, and the points of ``u + 1`` start where those of ``u`` end or one row later)."""
    path = np.asarray(path)
    U = int(U)
    count = np.bincount(path[:, 1], minlength=U).astype(np.float64)
    total = np.bincount(path[:, 1], weights=path[:, 0].astype(np.float64), minlength=U)
    if (count == 0).any():
        raise ValueError("path does not visit every score frame")
    return total / count


def warp_times(times, tmap, fps):
    """Score times (s) -> audio times (s): ``np.interp(times * fps, arange(U), tmap) / fps``."""
    tmap = np.asarray(tmap, dtype=np.float64)
    return np.interp(np.asarray(times, dtype=np.float64) * float(fps), np.arange(len(tmap), dtype=np.float64), tmap) / float(fps)


def auto_band(T, U):
    return None if int(T) * int(U) <= AUTO_BAND_CELLS else -(-max(int(T), int(U)) // 8)


def align_scores(transform, audio, scores, band='auto', sample_rate=44100, **chroma_args):
    """Align ``scores`` (one ``(on, off, names)`` per instrument, score time in seconds) to ``audio`` (float ``[L]`` at
    ``sample_rate`` Hz).  ``transform``: a :class:`deepconvsep_amd.transform.transformFFT` (its frame size, hop and window
    make the features) or a :class:`deepconvsep_amd.runtime.StftPlan`.  Returns ``(aligned, path, cost)``: the scores with
    warped onsets and offsets (names as given), the DTW path ``[n, 2]`` and its cost.  ``band``: ``'auto'`` -- none up to
    2^26 cells, ``ceil(max(T, U) / 8)`` beyond -- or None or a number of score frames.  ``chroma_args``: ``fmin``, ``fmax``,
    ``tuning_freq``, ``floor`` of the audio side, ``nharmonics``, ``decay`` of the score side."""
    plan = transform._get_plan() if hasattr(transform, "_get_plan") else transform
    ctx = plan.ctx
    fps = float(sample_rate) / float(plan.hop)
    audio_args = {k: chroma_args.pop(k) for k in ("fmin", "fmax", "tuning_freq") if k in chroma_args}
    floor = chroma_args.pop("floor", 1e-6)
    a = ctx.to_device(np.asarray(audio).reshape(-1), np.float32)
    mag, _ = plan.forward(a, phase=False)
    T = int(mag.shape[0])
    A = chroma(ctx, mag, bin_classes(plan.frame, sample_rate, **audio_args), floor=floor)
    end = max([float(np.max(off)) for _, off, _ in scores if len(off)] or [0.0])
    U = int(math.ceil(end * fps)) + 1
    S = ctx.to_device(score_chroma(scores, U, plan.hop, sample_rate, **chroma_args), np.float32)
    if band == 'auto':
        band = auto_band(T, U)
    path, cost = dtw(ctx, A, S, band=band)
    tmap = time_map(path, U)
    aligned = [(warp_times(on, tmap, fps), warp_times(off, tmap, fps), list(names)) for on, off, names in scores]
    return aligned, path, cost


class ScoreFollower(object):
    """``dcs_follow``: a score follower with constant memory -- online DTW, one row over a window of ``window`` score frames per
    audio frame (csrc/follow.hip; include/dcs.h has the recurrence).  ``S`` ``[U, 12]`` is the score's chroma
    (:func:`score_chroma`), uploaded once.  ``max_step``: the most score frames one audio frame may advance (1 .. 4);
    ``back``: the cells kept behind the position (None: ``window // 4``); ``penalty``: the cost of a step other than 1;
    ``max_frames``: the most frames one launch takes (``push`` cuts longer blocks).  The result does not depend on how the
    frames are cut into pushes.  It follows a performance forward from the score's first frame, at up to ``max_step`` times
    nominal tempo, and never corrects a position it has given."""

    def __init__(self, ctx, S, window=512, max_step=2, back=None, penalty=1.0 / 16, max_frames=4096):
        from ctypes import byref
        S = np.ascontiguousarray(S, dtype=np.float32)
        if S.ndim != 2 or S.shape[1] != 12 or S.shape[0] < 1:
            raise ValueError("ScoreFollower expects score chroma [frames >= 1, 12], got %r" % (S.shape,))
        window, max_step = int(window), int(max_step)
        back = window // 4 if back is None else int(back)
        if window % 64 or not 64 <= window <= 1024:
            raise ValueError("window must be a multiple of 64 in 64 .. 1024, got %d" % window)
        if not 1 <= max_step <= 4:
            raise ValueError("max_step must be 1 .. 4, got %d" % max_step)
        if not 0 <= back < window:
            raise ValueError("back must be in [0, window), got %d" % back)
        if not (math.isfinite(float(penalty)) and float(penalty) >= 0):
            raise ValueError("penalty must be finite and not negative, got %r" % (penalty,))
        if int(max_frames) < 1:
            raise ValueError("max_frames must be at least 1")
        self.ctx, self.U, self.window, self.max_step, self.back = ctx, int(S.shape[0]), window, max_step, back
        self.penalty, self.max_frames = float(penalty), int(max_frames)
        h = c_void_p()
        _lib.check(ctx._lib.dcs_follow_create(ctx._h, c_void_p(S.ctypes.data), self.U, window, max_step, back, self.penalty,
                                              self.max_frames, byref(h)))
        self._h = h

    @property
    def device_bytes(self):
        """device bytes the follower holds (``dcs_follow_bytes``): the score and one row, whatever has been pushed"""
        return int(self.ctx._lib.dcs_follow_bytes(self._h))

    @property
    def frames(self):
        """frames pushed since the follower was made or reset"""
        return int(self.ctx._lib.dcs_follow_frames(self._h))

    def push(self, chroma_t):
        """``chroma_t`` ``[n, 12]`` float32 device tensor (:func:`chroma`'s rows) -> int32 ``[n]`` device tensor: the score frame
        the performance has reached at each of these audio frames.  Nothing waits for the device."""
        from .runtime import _ptr, _torch
        torch = _torch()
        if chroma_t.dim() != 2 or int(chroma_t.shape[1]) != 12 or chroma_t.dtype != torch.float32:
            raise ValueError("ScoreFollower.push expects a float32 [frames, 12] tensor")
        with self.ctx.stream_scope():
            chroma_t = chroma_t.contiguous()
            n = int(chroma_t.shape[0])
            pos = torch.empty((n,), dtype=torch.int32, device=chroma_t.device)
            for i in range(0, n, self.max_frames):
                k = min(self.max_frames, n - i)
                _lib.check(self.ctx._lib.dcs_follow_push(self._h, _ptr(chroma_t[i:i + k]), k, _ptr(pos[i:i + k])))
        return pos

    def row(self):
        """``(row, w0, p)``: the window's row ``[window]`` float32 NumPy (cell ``w0 + i`` at ``i``, +inf past the score's end),
        the window start and the position (``dcs_follow_row``; this one waits for the device)."""
        from .runtime import _ptr, _torch
        torch = _torch()
        with self.ctx.stream_scope():
            row = torch.empty((self.window,), dtype=torch.float32, device=self.ctx.device)
            w0 = torch.empty((1,), dtype=torch.int64, device=self.ctx.device)
            p = torch.empty((1,), dtype=torch.int32, device=self.ctx.device)
            _lib.check(self.ctx._lib.dcs_follow_row(self._h, _ptr(row), _ptr(w0), _ptr(p)))
            return row.cpu().numpy(), int(w0.cpu().item()), int(p.cpu().item())

    def reset(self):
        """starts another signal; the score stays"""
        _lib.check(self.ctx._lib.dcs_follow_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.dcs_follow_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def follow_time_map(pos, U):
    """The time map of a position track: score frame ``u`` -> the first audio frame ``t`` with ``pos[t] >= u``; past the last
    position reached it continues at nominal tempo, ``t_last + (u - pos_last)``.  float64 ``[U]``, non-decreasing."""
    pos = np.asarray(pos, dtype=np.int64)
    if pos.ndim != 1 or pos.size < 1:
        raise ValueError("follow_time_map expects a position per audio frame, at least one")
    if (np.diff(pos) < 0).any():
        raise ValueError("positions must not decrease")
    u = np.arange(int(U), dtype=np.int64)
    first = np.searchsorted(pos, u, side='left').astype(np.float64)
    past = u > pos[-1]
    first[past] = (pos.size - 1) + (u[past] - pos[-1])
    return first


FOLLOWER_ARGS = ("window", "max_step", "back", "penalty", "max_frames")


def follow_scores(transform, audio, scores, sample_rate=44100, **args):
    """:func:`align_scores` done causally: the same magnitudes and chroma, pushed through a :class:`ScoreFollower` in blocks
    instead of one DTW over the whole recording, so every position depends on the audio up to its frame alone.  Returns
    ``(aligned, pos)``: the scores with warped onsets and offsets and the int32 position per audio frame.  ``args``: the
    follower's ``window``, ``max_step``, ``back``, ``penalty``, ``max_frames`` and the chroma arguments of ``align_scores``.
    It exists to be compared with the offline alignment; a stream follows with
    ``Separator.stream_scoreinformed(melody, follow_scores=...)``."""
    plan = transform._get_plan() if hasattr(transform, "_get_plan") else transform
    ctx = plan.ctx
    fps = float(sample_rate) / float(plan.hop)
    follower_args = {k: args.pop(k) for k in FOLLOWER_ARGS if k in args}
    audio_args = {k: args.pop(k) for k in ("fmin", "fmax", "tuning_freq") if k in args}
    floor = args.pop("floor", 1e-6)
    a = ctx.to_device(np.asarray(audio).reshape(-1), np.float32)
    mag, _ = plan.forward(a, phase=False)
    if int(mag.shape[0]) < 1:
        raise ValueError("follow_scores: %d samples of audio give no frame to follow" % int(a.numel()))
    A = chroma(ctx, mag, bin_classes(plan.frame, sample_rate, **audio_args), floor=floor)
    end = max([float(np.max(off)) for _, off, _ in scores if len(off)] or [0.0])
    U = int(math.ceil(end * fps)) + 1
    follower = ScoreFollower(ctx, score_chroma(scores, U, plan.hop, sample_rate, **args), **follower_args)
    try:
        pos = follower.push(A).cpu().numpy()
    finally:
        follower.close()
    tmap = follow_time_map(pos, U)
    aligned = [(warp_times(on, tmap, fps), warp_times(off, tmap, fps), list(names)) for on, off, names in scores]
    return aligned, pos


def align_score_files(wav, score_dir, out_dir, files, frameSize=2048, hopSize=512, band='auto', resample=False, online=False,
                      **chroma_args):
    """The command-line step: align the score files ``files`` of ``score_dir`` to the wav file and write them, under the same
    names, into ``out_dir``.  Frames of 2048 samples every 512 by default: the features' own analysis, finer in time than the
    separation's 4096.  A file at another rate than 44 100 Hz is aligned at its own rate with ``resample`` (scores are
    in seconds) and refused without, as the separation scripts do.  Returns ``(path, cost)`` -- with ``online`` (the causal
    alignment of :func:`follow_scores`; ``band`` is not used) ``(pos, None)``."""
    from .separation import read_wav, to_mono
    from .transform import transformFFT
    rate, audio = read_wav(wav)
    if rate != 44100 and not resample:
        raise ValueError("Sample rate is not 44100 (pass resample to align at the file's own rate)")
    audio = to_mono(audio, 'bach10_si')
    scores = [read_score(os.path.join(score_dir, f)) for f in files]
    tt = transformFFT(frameSize=frameSize, hopSize=hopSize, sampleRate=rate, precision='float32')
    if online:
        aligned, path = follow_scores(tt, audio, scores, sample_rate=rate, **chroma_args)
        cost = None
    else:
        aligned, path, cost = align_scores(tt, audio, scores, band=band, sample_rate=rate, **chroma_args)
    os.makedirs(out_dir, exist_ok=True)
    for f, (on, off, names) in zip(files, aligned):
        write_score(os.path.join(out_dir, f), on, off, names)
    return path, cost
