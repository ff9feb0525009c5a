"""The data augmentations of the hiphop (HHDS) trainers, rendered on the MI355X instead of on disk.

The reference trains examples/hiphopss with augmented data: ``compute_features_cs_aug.py`` (circular shifts per source),
``compute_features_instr_aug.py`` (one source muted) and ``compute_features_mix_aug.py`` (sources of four different songs)
render every variant on the host, transform it and write it as a float64 ``.data`` file that ``LargeDataset`` reads back.
Here a variant is a *virtual file*: a few integers per track on top of source audio that stays resident on the device, and
the STFT's loader renders it (csrc/fft_render.hip):

    r_s[n] = g_s * x_s[n - k_s]  if 0 <= n - k_s < L_s  else 0,      0 <= n < size
    mix[n] = m * (((r_0 + r_1) + r_2) + r_3)                          tracks in the reference's order of addition

which is ``util.circular_shift(x, min_size=size, cs, sampleRate)`` (util.py:62-81) with ``k = shift_samples(cs, sr)``.
Chunks ``[a, a + Lc)`` of the rendered signals are what the reference hands to ``compute_transform``; one chunk of one
variant is one ``.data`` file of the reference, ``[5, T, F]`` = mixture, vocals, bass, drums, other.

The functions up to :func:`table_rows` are pure host code.  :func:`render_features` (``dcs_stft_forward_render_*``) writes
the reference's files or returns their contents; :class:`RenderedWindows` (``dcs_trainer_gather_render``) is
``FeatureWindows`` without files.  There is no CPU fallback.
"""
import collections
import itertools
import os
from ctypes import POINTER, c_double, c_int64

import numpy as np

from . import _lib
from .runtime import StftPlan, _ptr, default_context  # noqa: F401  (StftPlan, WindowFeed: importable from here as before)
from .training import RenderedFeed, WindowFeed  # noqa: F401

CHANNELS = ('vocals', 'bass', 'drums', 'other')       # channels 1 .. 4 of a feature file (0 is the mixture)
# the order in which each script adds the sources into its mixture (compute_features.py:85, compute_features_cs_aug.py:120,
# compute_features_instr_aug.py:109, compute_features_mix_aug.py:82, :190)
ADD_ORDER = {'none': ('bass', 'drums', 'other', 'vocals'), 'cs': ('vocals', 'bass', 'drums', 'other'),
             'instr': ('bass', 'drums', 'other', 'vocals'), 'mix': ('bass', 'drums', 'other', 'vocals')}
KINDS = ('none', 'cs', 'instr', 'mix')

# signal: key of the source signal, (song, source name); k: shift in samples; g: gain; c: output channel 1 .. S
Track = collections.namedtuple('Track', 'signal k g c')
# tracks in add order; m: mixture scale; size: rendered length; chunks: (a, Lc) pairs; names: one file stem per chunk
VirtualFile = collections.namedtuple('VirtualFile', 'tracks m size chunks names')


def shift_samples(cs, sr):
    """The shift ``util.circular_shift(audio, min_size, cs, sr)`` applies, in samples: ``int(cs * sr)`` zeros in front for
    cs > 0 (util.py:76), ``int(abs(cs * sr))`` samples dropped for cs < 0 (:70), none for cs == 0."""
    if cs > 0:
        return int(cs * sr)
    if cs < 0:
        return -int(abs(cs * sr))
    return 0


def cs_combinations(time_shifts=(0., 0.2), intensity_shifts=(1.,), nsources=4):
    """compute_features_cs_aug.py:52-67: the (time shift, intensity) pair of every source, one ``[nsources, 2]`` array per
    variant.  With fewer pairs than sources: every element of ``itertools.product`` whose time shifts are not all equal
    (one intensity) or whose intensities are not all equal (one time shift) -- 14 variants for the reference's
    ``[0, 0.2] x [1]``; otherwise the permutations of the pairs; if nothing is left, the first pair for every source."""
    cc = [(t, g) for t in time_shifts for g in intensity_shifts]
    if len(cc) < nsources:
        combo = []
        for c in itertools.product(cc, repeat=nsources):
            c = np.array(c)
            if (len(intensity_shifts) == 1 and not all(x == c[0, 0] for x in c[:, 0])) \
                    or (len(time_shifts) == 1 and not all(x == c[0, 1] for x in c[:, 1])):
                combo.append(c)
    else:
        combo = [np.array(c) for c in itertools.permutations(cc, nsources)]
    if len(combo) == 0:
        combo = [np.array([[time_shifts[0], intensity_shifts[0]] for _ in range(nsources)])]
    return combo


def instrument_activation():
    """compute_features_instr_aug.py:49-53: ``[5, 4]``, row ``ins`` mutes column ``ins`` (bass, drums, other, vocals); row 4
    is the full mix."""
    act = np.ones((5, 4))
    for i in range(4):
        act[i, i] = 0
    return act


def mix_selections(songs, seed=0):
    """compute_features_mix_aug.py:143-156: every tenth combination of four songs and, of each, every tenth permutation,
    starting at two draws from 0 .. 9 -- ``RandomState(seed)`` here, unseeded in the reference.  Returns ``(comb, songs of
    the combination, p)``: bass comes from ``songs[p[0]]``, drums ``p[1]``, other ``p[2]``, vocals ``p[3]``."""
    rs = np.random.RandomState(seed)
    batch = int(rs.randint(10, size=1)[0])
    out = []
    for comb, f in enumerate(itertools.combinations(songs, 4)):
        if comb % 10 != batch:
            continue
        n = int(rs.randint(10, size=1)[0])
        for perm, p in enumerate(itertools.permutations(range(4))):
            if perm % 10 == n:
                out.append((comb, tuple(f), tuple(p)))
    return out


def chunk_bounds(size, sr=44100, rest=True, chunk=None):
    """The ``(a, Lc)`` chunks the feature generators cut from a rendered signal of ``size`` samples: ``int(size / (30.0 *
    sr))`` blocks of ``chunk`` = 30 s and, with ``rest``, what follows the last block -- also when that is nothing, and for
    a song shorter than one block its only chunk (compute_features.py:93-132; mix_aug's second half takes whole blocks
    only, :208-219).  The blocks are counted from ``size``, the rendered length."""
    chunk = 30 * int(sr) if chunk is None else int(chunk)
    n = int(size / float(chunk))
    out = [(i * chunk, chunk) for i in range(n)]
    if rest:
        out.append((n * chunk, int(size) - n * chunk))
    return out


def _file(tracks, m, size, sr, chunk, rest, name):
    chunks = chunk_bounds(size, sr, rest, chunk)
    return VirtualFile(tuple(tracks), float(m), int(size), tuple(chunks), tuple(name(i) for i in range(len(chunks))))


def virtual_files(kind, lengths, sr=44100, chunk=None, song='song', time_shifts=(0., 0.2), intensity_shifts=(1.,),
                  seed=0, songs=None):
    """The virtual files of one song (``kind`` 'none', 'cs', 'instr': ``lengths`` maps source name -> samples) or of a data
    set (``'mix'``: ``lengths`` is one such mapping per song, ``songs`` their names).

    none   compute_features.py:55-132: bass + drums + other + vocals, m 1, size len(other); ``<song>_<i>``
    cs     compute_features_cs_aug.py: one file per element of :func:`cs_combinations`, vocals + bass + drums + other, shift
           ``shift_samples(cs, sr)`` and gain per source, size ``len(vocals) - int(max cs * sr)`` (:98); ``<song>_<i>_cs<index
           of each source's shift in time_shifts>``
    instr  compute_features_instr_aug.py: five files, gains = row ``ins`` of :func:`instrument_activation`, m 1/4 (the
           targets are not scaled), size len(bass); ``<song>_<i>_<ins + 1>``
    mix    compute_features_mix_aug.py: every song by the plain rule with m 1/4 (:47-135; a song without vocals: a vocals
           track of gain 0 over its ``other`` signal), then :func:`mix_selections` of ``--seed``: the four sources from four
           songs, m 1/4, size the shortest, whole blocks only; ``combination_<c>_perm_<p>_block_<i + 1>`` (:218)
    """
    ch = {s: 1 + i for i, s in enumerate(CHANNELS)}
    if kind == 'none':
        tr = [Track((song, s), 0, 1.0, ch[s]) for s in ADD_ORDER[kind]]
        return [_file(tr, 1.0, lengths['other'], sr, chunk, True, lambda i: "%s_%d" % (song, i))]
    if kind == 'cs':
        out = []
        for c in cs_combinations(time_shifts, intensity_shifts, len(CHANNELS)):
            size = int(lengths['vocals'] - int(np.max(c[:, 0]) * sr))
            tr = [Track((song, s), shift_samples(c[j, 0], sr), float(c[j, 1]), ch[s]) for j, s in enumerate(ADD_ORDER[kind])]
            tag = "".join(str(list(time_shifts).index(x)) for x in c[:, 0])
            out.append(_file(tr, 1.0, max(size, 0), sr, chunk, True, lambda i, tag=tag: "%s_%d_cs%s" % (song, i, tag)))
        return out
    if kind == 'instr':
        act = instrument_activation()
        out = []
        for ins in range(5):
            tr = [Track((song, s), 0, float(act[ins, j]), ch[s]) for j, s in enumerate(ADD_ORDER[kind])]
            out.append(_file(tr, 0.25, lengths['bass'], sr, chunk, True, lambda i, ins=ins: "%s_%d_%d" % (song, i, ins + 1)))
        return out
    if kind != 'mix':
        raise ValueError("kind must be one of %r" % (KINDS,))
    songs = list(range(len(lengths))) if songs is None else list(songs)
    out = []
    for name, ln in zip(songs, lengths):
        tr = []
        for s in ADD_ORDER[kind]:
            if s == 'vocals' and ln.get('vocals') is None:
                tr.append(Track((name, 'other'), 0, 0.0, ch[s]))      # instrumental: silent vocals (:71-78)
            else:
                tr.append(Track((name, s), 0, 1.0, ch[s]))
        out.append(_file(tr, 0.25, ln['other'], sr, chunk, True, lambda i, name=name: "%s_%d" % (name, i)))
    by_name = dict(zip(songs, lengths))
    for comb, f, p in mix_selections(songs, seed):
        tr = []
        for j, s in enumerate(ADD_ORDER[kind]):
            silent = by_name[f[p[j]]][s] is None         # vocals of an instrumental: silent here too (the reference raises)
            tr.append(Track((f[p[j]], 'other' if silent else s), 0, 0.0 if silent else 1.0, ch[s]))
        size = min(by_name[t.signal[0]][t.signal[1]] for t in tr)
        stem = "combination_%d_perm_%d_%d_%d_%d_block_" % ((comb,) + tuple(p))
        out.append(_file(tr, 0.25, size, sr, chunk, False, lambda i, stem=stem: stem + str(i + 1)))
    return out


def table_rows(vfiles, index, hop):
    """The device table of ``dcs_trainer_gather_render``: one row per (virtual file, chunk) -- ``(size, a, Lc, T, then
    (offset, L_s, k_s, c_s) per track)`` int64 -- and its gains ``(m, g_s)`` float64.  ``index`` maps a track's signal key to
    its ``(offset, length)`` in the bank."""
    rows, gains = [], []
    for vf in vfiles:
        for a, Lc in vf.chunks:
            T = int(np.ceil(Lc / float(hop)) + 2)
            r = [vf.size, a, Lc, T]
            for t in vf.tracks:
                off, L = index[t.signal]
                r += [off, L, t.k, t.c]
            rows.append(r)
            gains.append([vf.m] + [t.g for t in vf.tracks])
    return np.asarray(rows, dtype=np.int64), np.asarray(gains, dtype=np.float64)


def bank_index(signals):
    """Key -> ``(offset, length)`` of the signals laid back to back in the order of ``signals``, and the total length."""
    index, off = {}, 0
    for k, x in signals.items():
        index[k] = (off, len(x))
        off += len(x)
    return index, off


class Bank(object):
    """Mono source signals back to back on the device: ``signals`` maps a key (song, source name) to a 1-D array; ``index``
    maps the key to ``(offset, length)``.  Uploaded once, as ``dtype``."""

    def __init__(self, signals, dtype=np.float32, ctx=None):
        self.ctx = ctx if ctx is not None else default_context()
        self.index, self.length = bank_index(signals)
        flat = np.concatenate([np.asarray(x, dtype=dtype).ravel() for x in signals.values()]) if self.length \
            else np.zeros(1, dtype)
        self.tensor = self.ctx.to_device(flat, dtype)


def render_blocks(tt, entry, S, frames, names, out_dir, call):
    """What the feature renderers share.  ``call(fn, plan, out, rows)`` runs ``fn`` = the library's ``entry`` + ``_f64`` /
    ``_f32`` (after ``tt.precision``) into ``out``, a device tensor of ``rows`` = (1 + S) * sum(frames) rows of ``plan.bins``,
    and returns its code.  Returns the blocks ``[1 + S, T, F]`` float64 of ``frames``, or with ``out_dir`` writes block i as
    ``<out_dir>/<names[i]>__m_.data`` / ``.shape`` through ``tt.saveTensor`` and returns the paths of the ``.data`` files."""
    import torch
    plan = tt._get_plan()
    ctx = plan.ctx
    f64 = tt.precision == 'float64'
    rows = (1 + S) * sum(frames)
    with ctx.stream_scope():
        out = torch.empty((max(rows, 1), plan.bins), dtype=torch.float64 if f64 else torch.float32, device=ctx.device)
        _lib.check(call(getattr(ctx._lib, entry + ('_f64' if f64 else '_f32')), plan, out, rows))
        host = out.double().cpu().numpy()
    blocks, at = [], 0
    for T in frames:
        blocks.append(host[at:at + (1 + S) * T].reshape(1 + S, T, plan.bins))
        at += (1 + S) * T
    if out_dir is None:
        return blocks
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, b in zip(names, blocks):
        tt.out_path = os.path.join(out_dir, name + '.data')
        tt.saveTensor(np.ascontiguousarray(b), '_' + tt.suffix + '_m_')
        paths.append(tt.out_path.replace('.data', '_' + tt.suffix + '_m_.data'))
    return paths


def render_features(tt, bank, vf, out_dir=None):
    """The feature blocks of the virtual file ``vf``, all chunks in one launch (``dcs_stft_forward_render_f64`` / ``_f32``
    after ``tt.precision``, the bank's dtype): a list ``[chunk] -> [1 + S, T, F]`` float64, or with ``out_dir`` the files
    ``<out_dir>/<name>__m_.data`` / ``.shape`` through ``tt.saveTensor`` (what ``tt.compute_transform(audio, path,
    phase=False)`` writes for the host-rendered chunk) and the list of paths.  ``tt``: a ``transformFFT``."""
    import torch
    if bank.tensor.dtype != (torch.float64 if tt.precision == 'float64' else torch.float32):
        raise ValueError("the bank holds %s, the transform computes in %s" % (bank.tensor.dtype, tt.precision))
    S = len(vf.tracks)
    tracks = np.asarray([list(bank.index[t.signal]) + [t.k, t.c] for t in vf.tracks], dtype=np.int64)
    gains = np.asarray([vf.m] + [t.g for t in vf.tracks], dtype=np.float64)
    chunks = np.asarray(vf.chunks, dtype=np.int64).reshape(-1, 2)
    n = len(chunks)
    frames = [_lib.frame_count(int(Lc), tt.hopSize) for _, Lc in chunks]
    got = (c_int64 * max(n, 1))()
    out = render_blocks(tt, 'dcs_stft_forward_render', S, frames, vf.names, out_dir, lambda fn, plan, out, rows: fn(
        plan._h, _ptr(bank.tensor), bank.length, S, tracks.ctypes.data_as(POINTER(c_int64)),
        gains.ctypes.data_as(POINTER(c_double)), int(vf.size), chunks.ctypes.data_as(POINTER(c_int64)), n, _ptr(out), plan.bins,
        rows, got))
    assert list(got)[:n] == frames
    return out


def render_audio(signals, vf):
    """The rendered signals of ``vf`` on the host, float64 ``[1 + S, size]`` (mixture, then the channels): what the
    reference holds before it slices its chunks -- for the ``mixture*.wav`` files the generators write."""
    out = np.zeros((1 + len(vf.tracks), vf.size))
    mix = None
    for t in vf.tracks:
        x = np.asarray(signals[t.signal], dtype=np.float64)
        n0, n1 = max(0, t.k), min(vf.size, len(x) + t.k)
        if n1 > n0:
            out[t.c, n0:n1] = t.g * x[n0 - t.k:n1 - t.k]
        mix = out[t.c].copy() if mix is None else mix + out[t.c]
    out[0] = vf.m * mix
    return out


class RenderedWindows(RenderedFeed):
    """``FeatureWindows`` without feature files: the training windows of the virtual files ``vfiles`` are transformed per
    batch from ``signals`` (key -> mono signal, uploaded once as float32) by ``dcs_trainer_gather_render``.

    Every (virtual file, chunk) takes the place of one ``.data`` file: the same ``reference_slots`` / ``all_slots`` of its
    ``T = frame_count(Lc, hop)`` frames, the same ``RandomState(seed + epoch).permutation`` over the window table, the same
    ``F``, ``total``, ``iteration_size``, ``gather(rows)`` and ``batches(epoch)``."""

    def __init__(self, signals, vfiles, time_context=30, overlap=25, mult_factor=0.3, windows='reference', batch_size=32,
                 seed=0, ctx=None, frameSize=1024, hopSize=512, window=None):
        self.vfiles = list(vfiles)
        RenderedFeed.__init__(self, self.vfiles, mult_factor, frameSize, hopSize, window, windows, time_context, overlap,
                              batch_size, seed, ctx)
        self._signals = signals
        self.index = bank_index(signals)[0]
        self.rows, self.gains = table_rows(self.vfiles, self.index, self.hop)
        self.names = [n for vf in self.vfiles for n in vf.names]
        self._set_table(r[3] for r in self.rows)
        self._bank = None

    def _upload(self):
        if self._bank is not None:
            return
        import torch
        self._open()
        self._bank = Bank(self._signals, np.float32, self.ctx)
        self._signals = None
        with self.ctx.stream_scope():
            self._rows_d = torch.from_numpy(self.rows).to(self.ctx.device)
            self._gains_d = torch.from_numpy(self.gains).to(self.ctx.device)

    def gather(self, rows):
        """Inputs ``[B, 1, tc, F]`` and targets ``[B, sources, tc, F]`` (device tensors) of the window-table rows ``rows``."""
        self._upload()
        with self.ctx.stream_scope():
            win_d, B, x, t = self._batch(rows, 1, self.sources)
            _lib.check(self.ctx._lib.dcs_trainer_gather_render(
                self.ctx._h, self._plan._h, _ptr(self._bank.tensor), self._bank.length, _ptr(self._rows_d),
                _ptr(self._gains_d), len(self.rows), _ptr(win_d), B, self.tc, self.sources, self.mult, _ptr(x), _ptr(t)))
        return x, t


def _mono(path):
    from .separation import read_wav
    sr, a = read_wav(path)
    if a.ndim > 1 and a.shape[1] > 1:
        a = (a[:, 0] + a[:, 1]) / 2
    elif a.ndim > 1:
        a = a[:, 0]
    return sr, np.asarray(a, dtype=np.float64)


def dataset_signals(db, kind, sample_rate=44100, chunk=None, seed=0):
    """The source signals and virtual files of an HHDS tree ``db`` (``Mixtures/Dev/<song>/``, ``Sources/Dev/<song>/{vocals,
    bass,drums,other}.wav``) for one of the four generators: ``(signals, vfiles, songs)`` with ``signals[(song, source)]``
    mono float64 and ``songs`` = (name, split, its virtual files) in the reference's order.  The songs are those listed under
    Mixtures/Dev (the cs script adds Mixtures/Test, compute_features_cs_aug.py:70-71).  A song without vocals.wav is skipped
    by the plain script (compute_features.py:68-81) and has silent vocals for 'mix' (compute_features_mix_aug.py:71-78)."""
    if kind not in KINDS:
        raise ValueError("kind must be one of %r" % (KINDS,))
    splits = {}
    for split in (("Dev", "Test") if kind == 'cs' else ("Dev",)):
        d = os.path.join(db, "Mixtures", split)
        if split == "Dev" or os.path.isdir(d):
            for f in os.listdir(d):
                if not f.startswith('.'):
                    splits.setdefault(f, split)
    signals, lengths, names = {}, [], []
    for f in sorted(splits):
        src = os.path.join(db, "Sources", splits[f], f)
        if not os.path.isfile(os.path.join(src, "vocals.wav")) and kind == 'none':
            continue
        ln = {}
        for s in CHANNELS:
            path = os.path.join(src, s + ".wav")
            if s == 'vocals' and kind == 'mix' and not os.path.isfile(path):
                ln[s] = None
                continue
            sr, x = _mono(path)
            assert sr == sample_rate, "Sample rate needs to be %d" % sample_rate
            signals[(f, s)] = x
            ln[s] = len(x)
        names.append(f)
        lengths.append(ln)
    if kind == 'mix':
        vfiles = virtual_files(kind, lengths, sample_rate, chunk, seed=seed, songs=names)
        songs = [(f, splits[f], [vf]) for f, vf in zip(names, vfiles)] + [(None, "Dev", vfiles[len(names):])]
        return signals, vfiles, songs
    songs = [(f, splits[f], virtual_files(kind, ln, sample_rate, chunk, song=f)) for f, ln in zip(names, lengths)]
    return signals, [vf for _, _, v in songs for vf in v], songs
