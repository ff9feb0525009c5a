"""Score-to-audio alignment: put a score at nominal tempo onto the recording before the harmonic masks are painted.

Every score-informed entry point assumes that the ``<inst>_b.txt`` files are already in the recording's time.  Bach10 ships
hand-aligned scores; a MIDI or notation export does not.  This module aligns one:

  audio -> magnitudes (the STFT plan) -> chroma per frame (``dcs_chroma``)   |
  score  -> chroma per frame of the score's own time (host, a few hundred notes) |-> DTW (``dcs_dtw``) -> path
  path -> time map (score frame -> audio frame) -> warped onsets and offsets

The two hot steps run on the GPU (csrc/align.hip); there is no CPU path for them.  The reference has no counterpart.
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


def align_score_files(wav, score_dir, out_dir, files, frameSize=2048, hopSize=512, band='auto', resample=False, **chroma_args):
    """The command-line step: align the score files ``files`` of ``score_dir`` to the wav file and write them, under the same
    names, into ``out_dir``.  Frames of 2048 samples every 512 by default: the features' own analysis, finer in time than the
    separation's 4096.  A file at another rate than 44 100 Hz is aligned at its own rate with ``resample`` (scores are
    in seconds) and refused without, as the separation scripts do.  Returns ``(path, cost)``."""
    from .separation import read_wav, to_mono
    from .transform import transformFFT
    rate, audio = read_wav(wav)
    if rate != 44100 and not resample:
        raise ValueError("Sample rate is not 44100 (pass resample to align at the file's own rate)")
    audio = to_mono(audio, 'bach10_si')
    scores = [read_score(os.path.join(score_dir, f)) for f in files]
    tt = transformFFT(frameSize=frameSize, hopSize=hopSize, sampleRate=rate, precision='float32')
    aligned, path, cost = align_scores(tt, audio, scores, band=band, sample_rate=rate, **chroma_args)
    os.makedirs(out_dir, exist_ok=True)
    for f, (on, off, names) in zip(files, aligned):
        write_score(os.path.join(out_dir, f), on, off, names)
    return path, cost
