"""The RWC instrument-sound notes the Bach10 RWC generator synthesises its training data from: host side of the reference's
rwc.py (Instrument :47-107, Note :131-188) and the note bank the score renderer reads (csrc/fft_score_render.hip).

The tree is ``<rwc>/mat/<name>.wav.mat`` (a MATLAB struct ``featureStruct`` with the note numbers, note starts and ends in
samples, dynamics, style, instrument id and sample rate of one recording) and ``<rwc>/wav/<instid><case>/<NAME>.WAV`` (the
recording: all notes of one instrument, player, style and dynamics one after the other).

Differences from the reference, on purpose:

* The directory listing is sorted.  The reference walks ``os.listdir`` in whatever order the file system gives and
  ``getNote`` returns the first match, so which of two recordings with the same (note, dynamics, style, case) is used
  depends on the file system; here it is the first by name.
* The RMS onset trim of ``getAudio`` (:154-188: hop 128, window 1024, threshold 0.01) is computed ONCE per note, on the
  whole note, and its effect on the note's start is stored (``noteStart``; ``rawStart`` keeps the annotation).  The
  reference adds the trim to ``noteStart`` on every call, inside pool workers: what a note sounds like there depends on
  which durations were asked for before and by which process.  That is not reproduced.
* Notes are mono; a recording with more than one channel is a ``ValueError`` (the reference would slice rows of a 2-D
  array and fail later).
"""
import collections
import os

import numpy as np

TRIM_HOP, TRIM_WINDOW, TRIM_THRESHOLD = 128, 1024, 0.01


def onset_frames(note):
    """rwc.py:167-179: the RMS of 1024-sample windows every 128 samples (the last ones shorter); the frame before the first
    one above 0.01, or 0."""
    n = int(np.ceil(len(note) / np.double(TRIM_HOP)))
    energy = np.zeros(n)
    for k in range(n):
        seg = note[k * TRIM_HOP:k * TRIM_HOP + TRIM_WINDOW]
        energy[k] = np.sqrt(np.sum(np.power(seg, 2)) / len(seg))
    if n == 0:
        return 0
    return int(np.maximum(0, np.argmax(energy > TRIM_THRESHOLD) - 1))


def parse_mat(mat):
    """The fields the reference reads from ``loadmat(...)['featureStruct']`` by position (rwc.py:84-99, :143-149)."""
    fs = mat['featureStruct'][0][0]
    return dict(sampleRate=fs[0][0][0][3][0][0], dynamics=str(fs[3][0]), instid=fs[4][0][0], instrumentName=str(fs[6][0]),
                instrumentSymbol=str(fs[7][0]), style=str(fs[9][0]), nr=np.asarray(fs[14][0]), start=np.asarray(fs[15][0]),
                end=np.asarray(fs[16][0]))


def _mono(audio, where):
    audio = np.asarray(audio)
    if audio.ndim != 1:
        raise ValueError("%s: a note recording must be mono, got an array of shape %r" % (where, audio.shape))
    return np.asarray(audio, dtype=np.float64)


def segment_length(n_whole, start, end, sr, max_duration):
    """Samples ``Note.getAudio(max_duration)`` returns (rwc.py:161-164, :184-187) for a note of ``n_whole`` samples whose
    (trimmed) start and end are ``start`` and ``end`` seconds: the whole note when ``max_duration`` is 0 or the note is
    shorter, else ``int((start + max_duration) * sr) - int(start * sr)``, cut where the recording ends."""
    if max_duration == 0 or (end - start) < max_duration:
        return int(n_whole)
    return int(min(int((start + max_duration) * sr) - int(start * sr), n_whole))


class Note(object):
    """One note of a recording (rwc.py:131-188).  ``audio``: the whole recording, mono float; ``info``: :func:`parse_mat`
    of its .mat file; ``fid``: index of the note in it; ``sr``: the recording's sample rate (default: the annotation's).
    ``noteStart`` is the annotated start plus the onset trim."""

    def __init__(self, audio, info, fid, case, wav_path=None, code=None, noteid=0, sr=None):
        self.wav_path, self.code, self.fid, self.noteid, self.case = wav_path, code, int(fid), noteid, case
        self.sampleRate = info['sampleRate']
        self.style, self.dynamics, self.instid = info['style'], info['dynamics'], info['instid']
        self.piece = self.style + '_' + self.dynamics + '_' + str(case)
        self.nr = info['nr'][fid]
        self.rawStart = float(info['start'][fid]) / float(self.sampleRate)
        self.noteEnd = float(info['end'][fid]) / float(self.sampleRate)
        # getAudio slices with the recording's own rate (:159-164); the annotation's rate converts the note's bounds (:147)
        self.sr = sr = self.sampleRate if sr is None else sr
        audio = _mono(audio, wav_path or code or 'note')
        whole = audio[int(self.rawStart * sr):int(self.noteEnd * sr)]
        self.onset = onset_frames(whole)
        self.noteStart = self.rawStart
        if self.onset > 0:
            self.noteStart = self.rawStart + self.onset * float(TRIM_HOP) / sr
            whole = audio[int(self.noteStart * sr):int(self.noteEnd * sr)]
        self.length = self.noteEnd - self.noteStart
        self.whole = np.array(whole, dtype=np.float64)

    def segment_length(self, max_duration=0):
        return segment_length(len(self.whole), self.noteStart, self.noteEnd, self.sr, max_duration)

    def getAudio(self, max_duration=0):
        return self.whole[:self.segment_length(max_duration)]


class Instrument(object):
    """All notes of one RWC instrument (rwc.py:47-107): the recordings ``<path>/wav/<instid><case>/*.WAV`` of the allowed
    players whose name holds one of the allowed styles and ends in one of the allowed dynamics, each with its
    ``<path>/mat/<name>.wav.mat``.  Sorted listing; see the module's notes."""

    def __init__(self, path, instid, allowed_styles=None, allowed_case=None, allowed_dynamics=None):
        from scipy import io
        from .separation import read_wav
        self.path, self.instid = path, instid
        self.allowed_styles = allowed_styles
        self.allowed_case = allowed_case if allowed_case is not None else [1, 2, 3]
        self.allowed_dynamics = allowed_dynamics if allowed_dynamics is not None else ['P', 'F', 'M']
        self.notes, self.wav_list, self.missing = [], [], []
        for case in self.allowed_case:
            d = os.path.join(path, 'wav', str(instid) + str(case))
            for f in sorted(os.listdir(d)):
                if not f.endswith(".WAV"):
                    continue
                if allowed_styles is not None and not any(s in f for s in allowed_styles):
                    continue
                if self.allowed_dynamics and not any(s + '.WAV' in f for s in self.allowed_dynamics):
                    continue
                matfile = os.path.join(path, 'mat', f.lower() + '.mat')
                if not os.path.isfile(matfile):
                    self.missing.append(matfile)
                    continue
                info = parse_mat(io.loadmat(matfile))
                wav = os.path.join(d, f)
                wav_sr, audio = read_wav(wav)
                self.wav_list.append(wav)
                for i in range(len(info['nr'])):
                    self.notes.append(Note(audio, info, i, case, wav, f.lower(), len(self.notes), wav_sr))
        self.total_notes = len(self.notes)

    def getNote(self, nr, dynamics='F', style='NO', case=1):
        for n in self.notes:
            if n.nr == nr and n.dynamics == dynamics and n.style == style and n.case == case:
                return n
        return None


Entry = collections.namedtuple('Entry', 'offset length start end sr')


class NoteBank(object):
    """All notes back to back: ``index[(instrument, note number, dynamics, style, case)] = Entry(offset, length, start, end,
    sr)`` -- ``offset`` and ``length`` of the whole (trimmed) note in ``data``, and what :func:`segment_length` needs.  The
    first note of a key wins, as in ``getNote``.  ``data`` is float64; :meth:`device` uploads it once per dtype (float32
    for the feed, float64 for files)."""

    def __init__(self, notes):
        """``notes``: iterable of ``(key, whole note, start s, end s, sample rate)``."""
        self.index, parts, off = {}, [], 0
        for key, whole, start, end, sr in notes:
            if key in self.index:
                continue
            whole = _mono(whole, str(key))
            self.index[key] = Entry(off, len(whole), float(start), float(end), sr)
            parts.append(whole)
            off += len(whole)
        self.length = off
        self.data = np.concatenate(parts) if parts else np.zeros(0)
        self._dev = {}

    @classmethod
    def from_instruments(cls, instruments):
        return cls(((int(ins.instid), int(n.nr), n.dynamics, n.style, int(n.case)), n.whole, n.noteStart, n.noteEnd, n.sr)
                   for ins in instruments for n in ins.notes)

    @classmethod
    def from_arrays(cls, arrays, sr=44100):
        """``arrays``: key -> mono array, each a whole note that begins at 0 s of its own recording."""
        return cls((k, x, 0.0, len(x) / float(sr), sr) for k, x in arrays.items())

    def segment(self, key, max_duration=0):
        """``(offset, length)`` in ``data`` of what ``getNote(...).getAudio(max_duration)`` returns; None without the note."""
        e = self.index.get(key)
        if e is None:
            return None
        return e.offset, segment_length(e.length, e.start, e.end, e.sr, max_duration)

    def device(self, dtype, ctx=None):
        from .runtime import default_context
        ctx = ctx if ctx is not None else default_context()
        k = (np.dtype(dtype).name, id(ctx))
        if k not in self._dev:
            self._dev[k] = ctx.to_device(self.data if self.length else np.zeros(1), dtype)
        return self._dev[k]
