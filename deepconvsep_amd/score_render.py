"""The RWC-sample and Sibelius training sets of the Bach10 trainers, rendered from scores on the MI355X instead of on disk.

The reference trains its Bach10 models on data it generates: ``examples/bach10/compute_features_bach10rwc.py`` re-synthesises
every score note by note from RWC instrument samples (rwc.py) in hundreds of combinations of onset shift, dynamics, style
and player, transforms each variant and writes it as a float64 ``.data`` file.  Here a variant of a score chunk is a
*virtual file*: per track a list of notes ``(b, bank segment, len)`` on top of a note bank that stays resident on the
device (:class:`deepconvsep_amd.rwc.NoteBank`), and the STFT's loader assembles it (csrc/fft_score_render.hip):

    track_s[n] = bank[off_m + (n - b_m)]  for the LARGEST m of track s with b_m <= n < b_m + len_m, else 0     0 <= n < size
    mix[n]     = ((track_0[n] + track_1[n]) + track_2[n]) + track_3[n]

-- each note is assigned into its track (compute_features_bach10rwc.py:131-134), so a later note overwrites an earlier one
where they overlap, and ``getMidi`` returns ``begin - shift`` / ``end + shift``: overlaps are the normal case.

The functions up to :func:`pack_tables` are pure host code.  :func:`render_score_features`
(``dcs_stft_forward_score_render_*``) writes the reference's files or returns their contents; :class:`ScoreRenderedWindows`
(``dcs_trainer_gather_score_render``) is ``FeatureWindows`` without files.  There is no CPU fallback.
:func:`score_informed_files` is the score-informed generator (``examples/bach10_scoreinformed/compute_features_bach10rwc.py``:
notes from ``expandMidi`` placed at frame x hop, two note tables per file); :func:`render_score_informed_features` writes its
files and :class:`ScoreInformedRenderedWindows` (``dcs_trainer_gather_score_informed_render``) is ``ScoreFeatureWindows``
without files, harmonic masks included.
:func:`sibelius_files` covers ``compute_features_bach10sibelius.py``, whose rule -- whole recordings shifted and scaled --
is the one :mod:`deepconvsep_amd.augment` already renders.
"""
import base64
import collections
import itertools
import os
from ctypes import POINTER, c_int64

import numpy as np

from . import _lib
from .augment import Track, VirtualFile, render_blocks, shift_samples
from .score import _score_path, _select, read_score, str2midi
from .runtime import _ptr
from .training import RenderedFeed, WindowFeed  # noqa: F401  (importable from here as before)

SOURCES = ('bassoon', 'clarinet', 'saxophone', 'violin')      # the score files <source>_g<style>.txt, in track order
INSTRUMENT_IDS = (30, 31, 27, 15)                             # their RWC instrument numbers (:215)
DYNAMICS, STYLES, CASES = ('F', 'M', 'P'), ('NO',), (1, 2, 3)  # :212-214

# name: the reference's file stem; size: rendered samples; tracks: per source a tuple of notes (b, offset, len) -- first
# sample in the track, offset of the segment in the bank, samples
ScoreFile = collections.namedtuple('ScoreFile', 'name size tracks')


def note_times(instrument, FilePath, beginTime, finishTime, samplerate, hop, timeSpan_on, timeSpan_off, nframes):
    """What the generator takes from ``util.getMidi`` (util.py:332-386, :416-418): the notes of ``<FilePath>/<instrument>
    .txt`` that touch [beginTime, finishTime], times relative to beginTime and clamped to the chunk, without the notes
    that end at 0, are empty, begin past ``nframes`` frames or are shorter than 10 ms; ``(begin - timeSpan_on clamped at 0,
    end + timeSpan_off clamped at the chunk's length, MIDI numbers)``.  None where getMidi takes its other branch (fewer
    than two notes selected), which the generator cannot unpack."""
    on, off, names = read_score(_score_path(instrument, FilePath))
    sel = _select(on, off, beginTime, finishTime)
    if sel is None:
        return None
    first, last, b, e = sel
    names = names[first:last + 1]
    tframes = float(nframes) * float(hop) / float(samplerate)
    keep = ~((e <= 0) | (e <= b) | (b >= tframes) | ((e - b) < 0.01))
    begin = [np.maximum(0, x - timeSpan_on) for x in b[keep].tolist()]
    end = [np.minimum(finishTime - beginTime, x + timeSpan_off) for x in e[keep].tolist()]
    return begin, end, [str2midi(n) for n, k in zip(names, keep.tolist()) if k]


def midi_length(instrument, FilePath):
    """util.getMidiLength (util.py:517-524): the largest note end of the score, in seconds."""
    _, off, _ = read_score(_score_path(instrument, FilePath))
    return max(off.tolist())


def _n_permutations(n, r):
    out = 1
    for k in range(n - r + 1, n + 1):
        out *= k
    return out


def unrank_permutation(index, n, r):
    """Element ``index`` of ``itertools.permutations(range(n), r)``."""
    pool, out = list(range(n)), []
    for i in range(r):
        q, index = divmod(index, _n_permutations(n - 1 - i, r - 1 - i))
        out.append(pool.pop(q))
    return tuple(out)


def rwc_combinations(time_shifts=(0., 0.1, 0.2), n_dynamics=3, n_styles=1, cases=CASES, nsources=4, sample_size=400, seed=0,
                     materialise=False):
    """``Engine.__init__`` (compute_features_bach10rwc.py:59-87): per source a tuple (time shift, index of the dynamics,
    index of the style, player), one float64 ``[nsources, 4]`` array per combination.  With fewer tuples than sources:
    every element of ``itertools.product`` whose time shifts are not all equal (one dynamics) or whose dynamics are not all
    equal (one time shift); otherwise the permutations of the tuples; if nothing is left, the first tuple for every source.
    Of more than ``sample_size`` combinations, ``RandomState(seed).choice(len(combo), size=sample_size, replace=False)``
    picks (the reference's draw is unseeded).  The default setting has 27 tuples, 421 200 permutations: the drawn indices
    are unranked instead of the list being built, unless ``materialise``; the selection is the same."""
    intensity_shifts, style_shifts = list(range(n_dynamics)), list(range(n_styles))
    cc = [(t, j, l, k) for t in time_shifts for j in intensity_shifts for l in style_shifts for k in cases]
    sample_size = int(sample_size)
    if len(cc) < nsources:
        combo = []
        for c in itertools.product(cc, repeat=nsources):
            c = np.array(c)
            if (len(intensity_shifts) == 1 and not all(x == c[0, 0] for x in c[:, 0])) \
                    or (len(time_shifts) == 1 and not all(x == c[0, 1] for x in c[:, 1])):
                combo.append(c)
        combo = np.array(combo)
    elif materialise:
        combo = np.array(list(itertools.permutations(cc, nsources)))
    else:
        total = _n_permutations(len(cc), nsources)
        idx = np.random.RandomState(seed).choice(total, size=sample_size, replace=False) if sample_size < total \
            else np.arange(total)
        return np.array([[cc[i] for i in unrank_permutation(int(j), len(cc), nsources)] for j in idx], dtype=np.float64)
    if len(combo) == 0:
        combo = np.array([[[time_shifts[0], intensity_shifts[0], style_shifts[0], cases[0]] for _ in range(nsources)]])
    if sample_size < len(combo):
        combo = combo[np.random.RandomState(seed).choice(len(combo), size=sample_size, replace=False)]
    return np.asarray(combo, dtype=np.float64)


def file_name(piece, c, chnk):
    """The stem of the reference's file (:141): ``<piece>_<str(c) in base64, as Python 2's 'base64' codec writes it -- 76
    characters a line, every line ended by a newline>_<chunk>``.  ``str(c)`` is NumPy's print of the float64 array and
    follows the installed NumPy."""
    return piece + '_' + base64.encodebytes(str(c).encode('ascii')).decode('ascii') + '_' + str(chnk)


def score_files(FilePath, piece, bank, combos, chunk_size=45, sr=44100, hop=512, style_midi='_original', sources=SOURCES,
                instrument_ids=INSTRUMENT_IDS, dynamics=DYNAMICS, styles=STYLES):
    """The virtual files of one piece (``Engine.__call__``, :92-141): for every combination ``c`` of ``combos`` and every
    chunk, one :class:`ScoreFile`.  The chunks (:99-109): ``chunk_size`` seconds, at most the longest score
    (``int(midi_length)``), ``int(floor(longest / chunk_size))`` of them; ``size = int(chunk_size * sr - int(max shift *
    sr))`` (:115).  Per source the notes of :func:`note_times` with the source's shift on both sides (:122), each the
    segment ``bank.segment((instrument, note, dynamics, style, case), end - begin)`` placed at ``b = int(floor(begin *
    sr))`` with ``len = min(segment length, size - b)`` (:130-134).

    No file where the reference writes none: a note missing from the bank (GetOutOfLoop, :127-128), a source without a
    usable selection in the chunk (getMidi's five-value return, :122), a note that begins at or past ``size`` (the slice
    assignment raises, :132)."""
    scores = [s + '_g' + style_midi for s in sources]
    max_length = 0
    for s in scores:
        max_length = max(max_length, int(midi_length(s, FilePath)))
    if chunk_size > max_length:
        chunk_size = max_length
    out = []
    if chunk_size <= 0:
        return out
    for c in combos:
        c = np.array(c)
        for chnk in range(int(np.floor(max_length / chunk_size))):
            chunk_start, chunk_end = chunk_size * chnk, (chnk + 1) * chunk_size
            nframes = int(np.ceil(chunk_size * sr / np.double(hop))) + 2
            size = int(chunk_size * sr - int(np.max(c[:, 0].astype(float)) * sr))
            tracks = []
            for i, s in enumerate(scores):
                nt = note_times(s, FilePath, chunk_start, chunk_end, sr, hop, c[i, 0], c[i, 0], nframes)
                notes = None
                if nt is not None:
                    notes = []
                    for begin, end, nr in zip(*nt):
                        seg = bank.segment((instrument_ids[i], nr, dynamics[int(c[i, 1])], styles[int(c[i, 2])], int(c[i, 3])),
                                           end - begin)
                        b = int(np.floor(begin * sr))
                        if seg is None or b >= size:
                            notes = None
                            break
                        notes.append((b, seg[0], min(seg[1], size - b)))
                if notes is None:
                    tracks = None
                    break
                tracks.append(tuple(notes))
            if tracks is not None:
                out.append(ScoreFile(file_name(piece, c, chnk), size, tuple(tracks)))
    return out


# a ScoreFile with the two note tables the score-informed generator writes next to it: float64 [S, nelem_g, 2 nharmonics + 3]
ScoreInformedFile = collections.namedtuple('ScoreInformedFile', 'name size tracks melody_g melody_e')

SI_NHARMONICS, SI_INTERVAL, SI_TUNING = 20, 50, 440          # bach10_scoreinformed/compute_features_bach10rwc.py:231-233


def si_file_name(c, chnk):
    """The stem of the score-informed generator's files below ``<feature_path>/<piece>/<style>/`` (bach10_scoreinformed/
    compute_features_bach10rwc.py:156): ``<str(c) in base64, as for file_name>_<chunk>``; the files are ``<stem>__m_``,
    ``<stem>__g_`` and ``<stem>__e_`` ``.data`` / ``.shape``."""
    return base64.encodebytes(str(c).encode('ascii')).decode('ascii') + '_' + str(chnk)


def score_informed_files(FilePath, bank, combos, chunk_size=45, sr=44100, hop=512, frame=4096, style_midi='_original',
                         sources=SOURCES, instrument_ids=INSTRUMENT_IDS, dynamics=DYNAMICS, styles=STYLES,
                         nharmonics=SI_NHARMONICS, interval=SI_INTERVAL, tuning_freq=SI_TUNING):
    """The virtual files of one piece as the score-informed generator makes them (``Engine.__call__``,
    bach10_scoreinformed/compute_features_bach10rwc.py:96-163): for every combination ``c`` and every chunk one
    :class:`ScoreInformedFile`.  Chunks and ``size`` as in :func:`score_files`, except that the longest score is not
    truncated to whole seconds (:105).  The notes come from ``score.expandMidi``, in frames: ``melody_g`` with the source's
    shift on both sides, ``melody_e`` with the shift + 0.2 s and ``fermata`` = the shift + 0.5 s (:133-137), both ``[S,
    nelem_g, 2 nharmonics + 3]`` with ``nelem_g`` the largest ``getMidiNum`` of the sources, at least 1 (:116-121).  Every
    row of ``melody_g`` with a MIDI number > 0 is the segment ``bank.segment(key, (end frame - first frame) * hop / sr)``
    placed by assignment at ``b = int(floor(first frame * hop))`` with ``len = min(segment length, size - b)`` (:140-150).
    ``expandMidi`` keeps score order and its first frames are a monotonic function of the onsets, so ``b`` is non-decreasing
    within a track and ``dcs_score_render_pack`` takes the notes as they are.

    No file where the reference writes none: a note missing from the bank (GetOutOfLoop, :143-144); a source with fewer
    than two notes selected in the chunk (``expandMidi`` returns None, :134 raises); a note at ``b > size`` of which more
    than one sample would be left after the cut ``segment[:size - b]`` (the assignment into the empty slice raises, :148).
    A note at ``b == size``, or past it with at most one sample left, is assigned into an empty slice and paints nothing:
    the file is written without it.  GetOutOfLoop is caught per chunk (:162); the other two leave ``__call__``, so the later
    chunks of that combination are not written either."""
    from .score import expandMidi, getMidiNum
    scores = [s + '_g' + style_midi for s in sources]
    max_length = 0
    for s in scores:
        max_length = max(max_length, midi_length(s, FilePath))
    if chunk_size > max_length:
        chunk_size = max_length
    out = []
    if chunk_size <= 0:
        return out
    for c in combos:
        c = np.array(c)
        for chnk in range(int(np.floor(max_length / chunk_size))):
            chunk_start, chunk_end = float(chunk_size * chnk), float((chnk + 1) * chunk_size)
            nelem_g = 1
            for s in scores:
                nelem_g = max(getMidiNum(s, FilePath, chunk_start, chunk_end), nelem_g)
            melody_g = np.zeros((len(scores), int(nelem_g), 2 * nharmonics + 3))
            melody_e = np.zeros((len(scores), int(nelem_g), 2 * nharmonics + 3))
            nframes = int(np.ceil(chunk_size * sr / np.double(hop))) + 2
            size = int(chunk_size * sr - int(np.max(c[:, 0].astype(float)) * sr))
            tracks, raised = [], False
            for i, s in enumerate(scores):
                g = expandMidi(s, FilePath, chunk_start, chunk_end, interval, tuning_freq, nharmonics, sr, hop, frame, c[i, 0],
                               c[i, 0], nframes)
                e = None if g is None else expandMidi(s, FilePath, chunk_start, chunk_end, interval, tuning_freq, nharmonics, sr,
                                                      hop, frame, c[i, 0] + 0.2, c[i, 0] + 0.2, nframes, fermata=c[i, 0] + 0.5)
                if g is None or e is None:
                    tracks, raised = None, True
                    break
                melody_g[i, :g.shape[0], :] = g
                melody_e[i, :e.shape[0], :] = e
                notes = []
                for m in range(int(nelem_g)):
                    if not melody_g[i, m, 2] > 0:
                        continue
                    seg = bank.segment((instrument_ids[i], int(melody_g[i, m, 2]), dynamics[int(c[i, 1])], styles[int(c[i, 2])],
                                        int(c[i, 3])), float(melody_g[i, m, 1] - melody_g[i, m, 0]) * hop / sr)
                    if seg is None:
                        notes = None
                        break
                    b, ln = int(np.floor(melody_g[i, m, 0] * hop)), max(seg[1], 0)
                    if b >= size:
                        if b > size and ln - (b - size) > 1:
                            notes, raised = None, True
                            break
                        continue
                    if min(ln, size - b) > 0:
                        notes.append((b, seg[0], min(ln, size - b)))
                if notes is None:
                    tracks = None
                    break
                tracks.append(tuple(notes))
            if tracks is not None:
                out.append(ScoreInformedFile(si_file_name(c, chnk), size, tuple(tracks), melody_g, melody_e))
            if raised:
                break
    return out


def sibelius_combinations(time_shifts=(0.,), intensity_shifts=(1.,), nsources=4):
    """compute_features_bach10sibelius.py:67-79: ``[nsources, 2]`` arrays of (time shift, gain); the rule of
    ``augment.cs_combinations``."""
    from .augment import cs_combinations
    return cs_combinations(time_shifts, intensity_shifts, nsources)


def sibelius_files(lengths, time_shifts=(0.,), intensity_shifts=(1.,), sr=44100, name='piece', signals=None):
    """compute_features_bach10sibelius.py:89-128 as ``augment.VirtualFile``s, one whole-file chunk each: per combination
    ``c`` source ``i`` (``lengths[i]`` samples) is shifted by ``c[i, 0]`` s with zero padding (either sign, :104-120),
    scaled by ``c[i, 1]`` and added into the mixture in source order (:122-123); ``size = lengths[0] - int(max shift * sr)``
    (:101).  Track ``i`` reads the signal ``signals[i]`` (default ``(name, i)``) and goes to channel ``1 + i``; the stem is
    ``<name>_<str(c) in base64>`` (:128).  Rendered by ``augment.render_features`` / ``augment.RenderedWindows``."""
    out = []
    for c in sibelius_combinations(time_shifts, intensity_shifts, len(lengths)):
        c = np.array(c)
        size = max(int(lengths[0] - int(np.max(np.array(c[:, 0])) * sr)), 0)
        tracks = tuple(Track((name, i) if signals is None else signals[i], shift_samples(c[i, 0], sr), float(c[i, 1]), 1 + i)
                       for i in range(len(lengths)))
        stem = name + '_' + base64.encodebytes(str(c).encode('ascii')).decode('ascii')
        out.append(VirtualFile(tracks, 1.0, size, ((0, size),), (stem,)))
    return out


def pack_notes(tracks, bank_len):
    """``dcs_score_render_pack`` on the host: ``tracks`` = per track a sequence of ``(b, offset, len)``; returns the int64
    table ``[notes, 4]`` = (b, offset, len, E), E the running maximum of ``b + len`` within the track, and the note count of
    every track.  ``ValueError`` for a note outside the bank, a negative ``b`` or ``len``, or a track whose ``b`` decrease."""
    counts = np.asarray([len(t) for t in tracks], dtype=np.int64)
    notes = np.asarray([n for t in tracks for n in t], dtype=np.int64).reshape(-1, 3)
    packed = np.zeros((len(notes), 4), dtype=np.int64)
    _lib.check(_lib.load().dcs_score_render_pack(notes.ctypes.data, counts.ctypes.data, len(counts), int(bank_len),
                                                 packed.ctypes.data))
    return packed, counts


def pack_tables(sfiles, bank_len, hop):
    """The device tables of ``dcs_trainer_gather_score_render``: the packed notes of all virtual files back to back and one
    row per file, ``(size, T, then (first note, note count) per track)``."""
    packed, counts = pack_notes([t for sf in sfiles for t in sf.tracks], bank_len)
    first = np.concatenate([[0], np.cumsum(counts)])
    rows, k = [], 0
    for sf in sfiles:
        r = [sf.size, int(np.ceil(sf.size / float(hop)) + 2)]
        for _ in sf.tracks:
            r += [first[k], counts[k]]
            k += 1
        rows.append(r)
    return packed, np.asarray(rows, dtype=np.int64)


def render_score_audio(bank, sf):
    """The rendered audio of ``sf`` on the host, float64 ``[size, 1 + S]`` -- the array the reference hands to
    compute_transform (:120-139): column ``1 + s`` = track s, notes assigned in list order; column 0 = ``np.sum`` over the
    tracks, which adds them in order.  ``bank``: a ``NoteBank`` or its flat data."""
    data = np.asarray(getattr(bank, 'data', bank), dtype=np.float64)
    audio = np.zeros((sf.size, len(sf.tracks) + 1))
    for s, notes in enumerate(sf.tracks):
        for b, off, ln in notes:
            ln = min(ln, sf.size - b)
            if ln > 0:
                audio[b:b + ln, s + 1] = data[off:off + ln]
    mix = audio[:, 1].copy()
    for s in range(1, len(sf.tracks)):
        mix = mix + audio[:, s + 1]
    audio[:, 0] = mix
    return audio


def render_score_features(tt, bank, sf, out_dir=None):
    """The feature block of the virtual file ``sf`` in one launch (``dcs_stft_forward_score_render_f64`` / ``_f32`` after
    ``tt.precision``): ``[1 + S, T, F]`` float64, or with ``out_dir`` the files ``<out_dir>/<name>__m_.data`` / ``.shape``
    through ``tt.saveTensor`` -- what ``tt.compute_transform(audio, path, phase=False)`` writes for the host-rendered
    audio -- and the path of the ``.data`` file.  ``tt``: a ``transformFFT``; ``bank``: a ``NoteBank``."""
    bank_t = bank.device(np.float64 if tt.precision == 'float64' else np.float32, tt._get_plan().ctx)
    S = len(sf.tracks)
    counts = np.asarray([len(t) for t in sf.tracks], dtype=np.int64)
    notes = np.asarray([n for t in sf.tracks for n in t], dtype=np.int64).reshape(-1, 3)
    T = _lib.frame_count(sf.size, tt.hopSize)
    got = c_int64(0)
    out = render_blocks(tt, 'dcs_stft_forward_score_render', S, [T], [sf.name], out_dir, lambda fn, plan, out, rows: fn(
        plan._h, _ptr(bank_t), bank.length, S, notes.ctypes.data, counts.ctypes.data, int(sf.size), _ptr(out), plan.bins, rows,
        POINTER(c_int64)(got)))
    assert got.value == T
    return out[0]


class ScoreRenderedWindows(RenderedFeed):
    """``FeatureWindows`` without feature files: the training windows of the virtual files ``sfiles`` are assembled and
    transformed per batch from the note bank (uploaded once as float32, with the note and file tables) by
    ``dcs_trainer_gather_score_render``.

    Every virtual file takes the place of one ``.data`` file: the same ``reference_slots`` / ``all_slots`` of its ``T =
    frame_count(size, hop)`` frames, the same ``RandomState(seed + epoch).permutation`` over the window table, the same
    ``F``, ``total``, ``iteration_size``, ``gather(rows)`` and ``batches(epoch)``."""

    def __init__(self, bank, sfiles, time_context=30, overlap=25, mult_factor=0.3, windows='reference', batch_size=32, seed=0,
                 ctx=None, frameSize=4096, hopSize=512, window=None):
        self.sfiles = list(sfiles)
        RenderedFeed.__init__(self, self.sfiles, mult_factor, frameSize, hopSize, window, windows, time_context, overlap,
                              batch_size, seed, ctx)
        self.bank = bank
        self.notes, self.rows = pack_tables(self.sfiles, bank.length, self.hop)
        self.names = [sf.name for sf in self.sfiles]
        self._set_table(r[1] for r in self.rows)
        self._bank_d = None

    def _upload(self):
        if self._bank_d is not None:
            return
        import torch
        self._open()
        self._bank_d = self.bank.device(np.float32, self.ctx)
        with self.ctx.stream_scope():
            self._notes_d = torch.from_numpy(self.notes if len(self.notes) else np.zeros((1, 4), np.int64)).to(self.ctx.device)
            self._rows_d = torch.from_numpy(self.rows).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, 1, tc, F]`` and targets ``[B, sources, tc, F]`` (device tensors) of the window-table rows ``rows``."""
        self._upload()
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, 1, self.sources)
            _lib.check(self.ctx._lib.dcs_trainer_gather_score_render(
                self.ctx._h, self._plan._h, _ptr(self._bank_d), self.bank.length, _ptr(self._notes_d), len(self.notes),
                _ptr(self._rows_d), len(self.rows), _ptr(win_d), B, self.tc, self.sources, self.mult, _ptr(x), _ptr(t)))
        return x, t


def render_score_informed_features(tt, bank, sf, out_dir=None):
    """What the score-informed generator writes for the virtual file ``sf`` (bach10_scoreinformed/
    compute_features_bach10rwc.py:156-158): the ``[1 + S, T, F]`` float64 block of :func:`render_score_features` and the two
    note tables.  Returns ``(block, melody_g, melody_e)``, or with ``out_dir`` writes ``<out_dir>/<name>__m_``, ``__g_`` and
    ``__e_`` ``.data`` / ``.shape`` through ``tt.saveTensor`` -- the files ``ScoreFeatureWindows`` loads -- and returns the
    path of the ``__m_.data`` file."""
    g, e = np.ascontiguousarray(sf.melody_g, dtype=np.float64), np.ascontiguousarray(sf.melody_e, dtype=np.float64)
    if out_dir is None:
        return render_score_features(tt, bank, sf), g, e
    path = render_score_features(tt, bank, sf, out_dir)
    tt.saveTensor(g, '_' + tt.suffix + '_g_')
    tt.saveTensor(e, '_' + tt.suffix + '_e_')
    return path


class ScoreInformedRenderedWindows(ScoreRenderedWindows):
    """``ScoreFeatureWindows`` without feature files: the windows of the :class:`ScoreInformedFile` s ``sfiles``, harmonic
    masks included, come per batch from the note bank in one launch (``dcs_trainer_gather_score_informed_render``).  The
    bank, the packed render notes, the file descriptors and the mask tables of ``pitch_code`` (``'g'``: ``melody_g``,
    ``'e'``: ``melody_e``, packed by ``dcs_trainer_pack_score``) stay on the device.  ``gather(rows)`` returns inputs and
    targets, both ``[B, S, tc, F]``; window table, ``batches(epoch)``, ``total`` and ``iteration_size`` are those of
    :class:`ScoreRenderedWindows`."""

    def __init__(self, bank, sfiles, pitch_code='e', **kw):
        if pitch_code not in ('g', 'e'):
            raise ValueError("pitch_code must be 'g' or 'e'")
        super(ScoreInformedRenderedWindows, self).__init__(bank, sfiles, **kw)
        self.pitch_code = pitch_code
        self.ninst = self.sources
        tables = [np.asarray(sf.melody_g if pitch_code == 'g' else sf.melody_e, dtype=np.float64) for sf in self.sfiles]
        widths = set(t.shape[2] for t in tables)
        if len(widths) > 1:
            raise ValueError("note tables disagree on their width")
        self.width = widths.pop() if widths else 0
        if tables and (self.width < 5 or self.width % 2 == 0):
            raise ValueError("note table width %d (odd, from 5)" % self.width)
        if any(t.shape[0] != self.sources for t in tables):
            raise ValueError("a note table per track is needed")
        self._tables = tables
        self._masks_d = None

    def _upload(self):
        if self._masks_d is not None:
            return
        super(ScoreInformedRenderedWindows, self)._upload()
        import torch
        from .score_training import pack_notes as pack_masks
        packed, mask_files, off = [], [], 0
        for t in self._tables:
            m = pack_masks(self.ctx._lib, t, self.F)
            packed.append(m.ravel())
            mask_files.append((off, t.shape[1]))
            off += m.size
        self.mask_len = off
        with self.ctx.stream_scope():
            self._mask_files_d = torch.from_numpy(np.asarray(mask_files, dtype=np.int64).reshape(-1, 2)).to(self.ctx.device)
            self._masks_d = torch.from_numpy(np.concatenate(packed + [np.zeros(1, np.int32)])).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, S, tc, F]`` = mask_j * (mult_factor * mixture) and targets ``[B, S, tc, F]`` (device tensors) of the
        window-table rows ``rows``."""
        self._upload()
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, self.sources, self.sources)
            _lib.check(self.ctx._lib.dcs_trainer_gather_score_informed_render(
                self.ctx._h, self._plan._h, _ptr(self._bank_d), self.bank.length, _ptr(self._notes_d), len(self.notes),
                _ptr(self._rows_d), len(self.rows), _ptr(self._masks_d), self.mask_len, _ptr(self._mask_files_d), self.width,
                _ptr(win_d), B, self.tc, self.sources, self.mult, _ptr(x), _ptr(t)))
        return x, t


def load_bank(rwc_path, instrument_ids=INSTRUMENT_IDS, styles=STYLES, cases=CASES, dynamics=DYNAMICS):
    """The note bank of the generator's four instruments (:217-219)."""
    from .rwc import Instrument, NoteBank
    return NoteBank.from_instruments([Instrument(rwc_path, i, list(styles), list(cases), list(dynamics)) for i in instrument_ids])


def _dataset_opening(db, original, sample_size, seed, pieces=None):
    """What the two generators' main programs open with: ``(style name, style_midi, [(piece, its combinations)])``.
    ``--original`` 1: the original scores, time shifts 0, 0.1, 0.2; 0: the ground-truth aligned scores, no shifts, at most 50
    combinations.  Every piece (a directory of ``db`` that begins with a digit) draws its combinations from ``seed`` + its
    position."""
    if original:
        style, style_midi, time_shifts = 'original', '_original', (0., 0.1, 0.2)
    else:
        style, style_midi, time_shifts = 'gt', '', (0.,)
        sample_size = min(50, sample_size)
    if pieces is None:
        pieces = [f for f in sorted(os.listdir(db)) if os.path.isdir(os.path.join(db, f)) and f[0].isdigit()]
    return style, style_midi, [(f, rwc_combinations(time_shifts, len(DYNAMICS), len(STYLES), CASES, len(SOURCES), sample_size,
                                                    seed + k)) for k, f in enumerate(pieces)]


def dataset_files(db, bank, chunk_size=45, sample_size=400, original=True, seed=0, sr=44100, hop=512):
    """The virtual files of a Bach10 Sibelius tree ``db`` (``<piece>/<source>_g<style>.txt``) as the generator's main
    program makes them (:202-231; ``original`` and ``sample_size``: :func:`_dataset_opening`).  Returns ``[(piece, style
    name, its ScoreFiles)]``."""
    style, style_midi, pieces = _dataset_opening(db, original, sample_size, seed)
    return [(f, style, score_files(os.path.join(db, f), f, bank, combos, chunk_size, sr, hop, style_midi)) for f, combos in pieces]


def si_dataset_files(db, bank, chunk_size=45., sample_size=400, original=True, seed=0, sr=44100, hop=512, frame=4096,
                     pieces=None):
    """The virtual files of a Bach10 Sibelius tree ``db`` as the score-informed generator's main program makes them
    (bach10_scoreinformed/compute_features_bach10rwc.py:216-249): the styles, shifts and ``sample_size`` rule of
    :func:`dataset_files`, the combinations of :func:`rwc_combinations` (one rule for both generators) drawn per piece from
    ``seed`` + its position, the files of :func:`score_informed_files`.  Returns ``[(piece, style name, its files)]``; the
    reference writes them below ``<feature_path>/<piece>/<style name>/``."""
    style, style_midi, pieces = _dataset_opening(db, original, sample_size, seed, pieces)
    return [(f, style, score_informed_files(os.path.join(db, f), bank, combos, chunk_size, sr, hop, frame, style_midi))
            for f, combos in pieces]
