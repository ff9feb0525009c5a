"""Host side of the score renderer (deepconvsep_amd/rwc.py, score_render.py) against the reference's own lines, recorded in
tests/golden/score_render.npz by tests/golden/make_golden_score_render.py on the seeded inputs of tests/score_render_ref.py.
No GPU: the packer ``dcs_score_render_pack`` is host code of libdcs."""
import os

import numpy as np
import pytest

import score_render_ref as R
from deepconvsep_amd import augment, rwc, score_render as sr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "score_render.npz"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return R.write_rwc_tree(str(tmp_path_factory.mktemp("rwc")))


@pytest.fixture(scope="module")
def piece(tmp_path_factory):
    return R.write_scores(str(tmp_path_factory.mktemp("db")))


@pytest.fixture(scope="module")
def instruments(tree):
    return [rwc.Instrument(tree, i, list(R.STYLES), list(R.CASES), list(R.DYNAMICS)) for i in R.INSTRUMENT_IDS]


@pytest.fixture(scope="module")
def bank(instruments):
    return rwc.NoteBank.from_instruments(instruments)


def _files(piece, bank):
    """The recorded (combination, chunk) pairs as ScoreFiles."""
    out = []
    for ci, chnk, _, _ in R.RENDERS:
        sfs = sr.score_files(piece, R.PIECE, bank, [R.COMBOS[ci]], R.CHUNK, R.SR, 64)
        assert len(sfs) == 3
        out.append(sfs[chnk])
    return out


# ------------------------------------------------------------------------------------------------ the RWC tree
def test_tree_reader_lists_what_the_reference_lists(g, instruments, tree):
    """The .mat files are written by scipy.io.savemat as a struct whose fields stand where rwc.py:84-99, :143-149 index
    them; the reference's Instrument read the same tree for the golden file."""
    for ins in instruments:
        got = np.asarray([[n.nr, R.DYNAMICS.index(n.dynamics), n.case, len(n.whole)] for n in ins.notes], dtype=np.int64)
        assert np.array_equal(got, g["inst_%d" % ins.instid])
        assert all(n.style == 'NO' for n in ins.notes)             # the staccato recording is filtered out
    assert [os.path.basename(m) for m in instruments[1].missing] == ['312qqnom.wav.mat']
    # two recordings hold (30, 57, F, NO, 1): the sorted listing takes 301XXNOF.WAV
    first = instruments[0].getNote(57, 'F', 'NO', 1)
    assert os.path.basename(first.wav_path) == '301XXNOF.WAV'
    dup = [n for n in instruments[0].notes if (n.nr, n.dynamics, n.case) == (57, 'F', 1)]
    assert len(dup) == 2 and not np.array_equal(dup[0].whole, dup[1].whole)
    b = rwc.NoteBank.from_instruments(instruments)
    e = b.index[(30, 57, 'F', 'NO', 1)]
    assert np.array_equal(b.data[e.offset:e.offset + e.length], first.whole)
    assert instruments[0].getNote(99, 'F', 'NO', 1) is None and b.segment((30, 99, 'F', 'NO', 1)) is None


def test_onset_trim_is_the_reference_s_first_call(g, tree):
    notes = rwc.Instrument(tree, R.TRIM_ID, list(R.STYLES), [1], ['F']).notes
    assert len(notes) == len(R.TRIM_LEADS)
    for k, n in enumerate(notes):
        assert np.array_equal(n.getAudio(0), g["trim_whole_%d" % k])
        assert np.array_equal(n.getAudio(R.TRIM_LONG), g["trim_long_%d" % k])
        assert n.noteStart == g["trim_start"][k]
        assert len(n.getAudio(R.TRIM_LONG)) < len(n.whole)
        assert np.array_equal(n.getAudio(0), n.whole)              # a second call changes nothing
    # 1024 samples of silence fit into the first window; longer ones are trimmed, to the hop before the first loud window
    assert [n.onset > 0 for n in notes] == [False, False, False, True, True]
    assert all(n.noteStart == n.rawStart + n.onset * 128.0 / R.SR for n in notes)


def test_notes_must_be_mono():
    info = dict(sampleRate=1000.0, dynamics='F', instid=1, style='NO', nr=np.array([60]), start=np.array([0.]),
                end=np.array([100.]))
    with pytest.raises(ValueError):
        rwc.Note(np.zeros((200, 2)), info, 0, 1)
    with pytest.raises(ValueError):
        rwc.NoteBank.from_arrays({(1, 60, 'F', 'NO', 1): np.zeros((10, 2))})


def test_bank_from_arrays_and_segment_lengths():
    b = rwc.NoteBank.from_arrays({'a': np.arange(10.), 'b': np.arange(2500.)}, sr=1000)
    assert b.length == 2510 and b.index['b'].offset == 10
    assert b.segment('b', 0) == (10, 2500) and b.segment('b', 3.0) == (10, 2500)       # shorter than max_duration: whole
    assert b.segment('b', 0.3) == (10, 300) and b.segment('b', 2.5) == (10, 2500)
    # the reference's float64 expressions, start not at 0
    assert rwc.segment_length(200000, 0.1234, 3.0, 44100, 0.5) == int((0.1234 + 0.5) * 44100) - int(0.1234 * 44100)
    assert rwc.segment_length(100, 0.1234, 3.0, 44100, 0.5) == 100                     # cut where the recording ends


# ------------------------------------------------------------------------------------------------ scores and combinations
def test_note_times_equal_getMidi(g, piece):
    nframes = int(np.ceil(R.CHUNK * R.SR / np.double(64))) + 2
    dropped = False
    for s in R.SOURCES:
        assert sr.midi_length(s + "_g_original", piece) == float(g["midi_length_" + s])
        for chnk in range(3):
            for j, sh in enumerate((0., 0.1, 0.2)):
                b, e, notes = sr.note_times(s + "_g_original", piece, R.CHUNK * chnk, R.CHUNK * (chnk + 1), R.SR, 64, sh, sh, nframes)
                want = g["midi_%s_%d_%d" % (s, chnk, j)]
                assert np.array_equal(np.asarray([b, e, notes], dtype=np.float64), want), (s, chnk, sh)
        if s == 'violin':
            b, _, _ = sr.note_times(s + "_g_original", piece, 0, R.CHUNK, R.SR, 64, 0., 0., nframes)
            dropped = 0.5 not in [round(x, 3) for x in b]
    assert dropped                                                 # the 5 ms note


def test_combinations_equal_the_engine_s(g):
    assert np.array_equal(sr.rwc_combinations((0., 0.1, 0.2), 3, 1, (1, 2, 3), 4, 400, seed=5), g["combos_default"])
    assert np.array_equal(sr.rwc_combinations((0., 0.2), 1, 1, (1,), 4, 400, seed=0), g["combos_few_shifts"])
    assert np.array_equal(sr.rwc_combinations((0.,), 2, 1, (1,), 4, 10, seed=3), g["combos_few_dynamics"])
    assert np.array_equal(sr.rwc_combinations((0.,), 1, 1, (2,), 4, 400, seed=0), g["combos_single"])
    assert g["combos_few_shifts"].shape == (14, 4, 4) and g["combos_few_dynamics"].shape == (10, 4, 4)
    assert g["combos_single"].shape == (1, 4, 4)


def test_the_unranked_draw_equals_the_materialised_one():
    a = sr.rwc_combinations(sample_size=400, seed=11)
    b = sr.rwc_combinations(sample_size=400, seed=11, materialise=True)
    assert a.shape == (400, 4, 4) and np.array_equal(a, b)
    import itertools
    assert [sr.unrank_permutation(i, 5, 3) for i in range(60)] == list(itertools.permutations(range(5), 3))


# ------------------------------------------------------------------------------------------------ the virtual files
def test_score_files_render_the_reference_s_audio(g, piece, bank):
    for k, ((ci, chnk, _, _), sf) in enumerate(zip(R.RENDERS, _files(piece, bank))):
        c = R.COMBOS[ci]
        want = g["audio_%d" % k]
        assert sf.size == len(want) == int(R.CHUNK * R.SR - int(c[:, 0].max() * R.SR))
        assert sf.name == sr.file_name(R.PIECE, c, chnk) and sf.name.startswith(R.PIECE + '_') and sf.name.endswith('_%d' % chnk)
        # the segment lengths getAudio returned, in the order of the calls
        seg = []
        for i, (b, lengths) in enumerate(_segments(piece, bank, c, chnk)):
            seg += lengths
            assert [n[0] for n in sf.tracks[i]] == [int(np.floor(x * R.SR)) for x in b]
            assert [n[2] for n in sf.tracks[i]] == [min(L, sf.size - n[0]) for L, n in zip(lengths, sf.tracks[i])]
        assert seg == list(g["seglen_%d" % k])
        got = sr.render_score_audio(bank, sf)
        assert got.shape == want.shape and np.array_equal(got, want), k
        # the mixture is the sequential sum
        assert np.array_equal(got[:, 0], ((got[:, 1] + got[:, 2]) + got[:, 3]) + got[:, 4])


def test_packed_tables(piece, bank):
    sfs = _files(piece, bank)
    notes, rows = sr.pack_tables(sfs, bank.length, 64)
    assert notes.dtype == np.int64 and rows.shape == (4, 2 + 2 * 4)
    at = 0
    for sf, r in zip(sfs, rows):
        assert r[0] == sf.size and r[1] == int(np.ceil(sf.size / 64.0) + 2)
        for s, tr in enumerate(sf.tracks):
            assert (r[2 + 2 * s], r[3 + 2 * s]) == (at, len(tr))
            p = notes[at:at + len(tr)]
            assert np.array_equal(p[:, :3], np.asarray(tr, dtype=np.int64))
            assert (np.diff(p[:, 0]) >= 0).all()
            assert np.array_equal(p[:, 3], np.maximum.accumulate(p[:, 0] + p[:, 2]))
            at += len(tr)
    assert at == len(notes)


def _segments(piece, bank, c, chnk):
    """Per source the begins of its notes and the lengths of the segments getAudio returns for them, before the cut."""
    nframes = int(np.ceil(R.CHUNK * R.SR / np.double(64))) + 2
    out = []
    for i, s in enumerate(R.SOURCES):
        b, e, notes = sr.note_times(s + "_g_original", piece, R.CHUNK * chnk, R.CHUNK * (chnk + 1), R.SR, 64, c[i, 0], c[i, 0], nframes)
        keys = [(R.INSTRUMENT_IDS[i], n, R.DYNAMICS[int(c[i, 1])], 'NO', int(c[i, 3])) for n in notes]
        out.append((b, [bank.segment(key, y - x)[1] for key, x, y in zip(keys, b, e)]))
    return out


def test_the_fixture_holds_every_case(piece, bank):
    """The shapes are only worth their time if the scores reach every case of the overwrite rule."""
    seen = dict.fromkeys(('overlap', 'inside', 'equal_b', 'cut', 'gap', 'three', 'first_in_frame_0', 'first_at_0'), False)
    frame, hop = 256, 64
    for (ci, chnk, _, _), sf in zip(R.RENDERS, _files(piece, bank)):
        uncut = _segments(piece, bank, R.COMBOS[ci], chnk)
        for s, tr in enumerate(sf.tracks):
            b = np.asarray([n[0] for n in tr])
            e = b + np.asarray([n[2] for n in tr])
            owner = np.full(sf.size + 1, -1)                       # the note heard at every sample: the latest that covers it
            for m in range(len(tr)):
                owner[b[m]:e[m]] = m
            for m in range(1, len(tr)):
                seen['overlap'] |= bool(b[m - 1] < b[m] < e[m - 1] < e[m])
                seen['equal_b'] |= bool(b[m] == b[m - 1] == 0 and e[m] > 0 and owner[0] == m)
                q = owner[b[m] - 1] if b[m] > 0 else -1
                seen['inside'] |= bool(0 <= q < m and owner[e[m]] == q and b[q] < b[m] and e[m] < e[q])
            seen['cut'] |= any(x + n == sf.size and n < L for x, n, L in zip(b, e - b, uncut[s][1]))
            silent = np.flatnonzero(owner[b.min():sf.size] >= 0)
            seen['gap'] |= bool(len(silent) > 1 and np.diff(silent).max() > frame + 1)
            for t in range(int(np.ceil(sf.size / float(hop))) + 2):
                f0, f1 = t * hop - frame // 2, t * hop + frame // 2
                seen['three'] |= int(((b < f1) & (e > f0)).sum()) >= 3
            seen['first_in_frame_0'] |= bool(0 < b[0] < frame // 2)
            seen['first_at_0'] |= bool(b[0] == 0)
    assert all(seen.values()), seen


def test_files_the_reference_does_not_write_are_not_produced(tmp_path, bank):
    c0 = R.COMBOS[0]
    full = sr.score_files(R.write_scores(str(tmp_path / "ok")), R.PIECE, bank, [c0], R.CHUNK, R.SR, 64)
    assert len(full) == 3
    # a note the bank does not hold (E4 = 64): GetOutOfLoop for the chunk it is in
    scores = dict(R.SCORES)
    scores['saxophone'] = [n if n[0] != 2.30 else (2.30, 3.00, 'E4') for n in R.SCORES['saxophone']]
    got = sr.score_files(R.write_scores(str(tmp_path / "missing"), scores=scores), R.PIECE, bank, [c0], R.CHUNK, R.SR, 64)
    assert [f.name for f in got] == [full[0].name, full[2].name]
    # a source with one note in the first chunk: getMidi returns five values into four names
    scores = dict(R.SCORES)
    scores['violin'] = [(0.10, 1.90, 'C4')] + [n for n in R.SCORES['violin'] if n[0] >= 2.2]
    got = sr.score_files(R.write_scores(str(tmp_path / "lonely"), scores=scores), R.PIECE, bank, [c0], R.CHUNK, R.SR, 64)
    assert [f.name for f in got] == [full[1].name, full[2].name]
    # a note that begins past size: 1.95 s with no shift of its own while another source's shift takes 0.2 s off the size
    scores = dict(R.SCORES)
    scores['clarinet'] = [n if n[0] != 1.70 else (1.95, 2.40, 'B3') for n in R.SCORES['clarinet']]
    late = R.write_scores(str(tmp_path / "late"), scores=scores)
    c1 = R.COMBOS[1]
    assert c1[1, 0] == 0 and c1[:, 0].max() == 0.2
    got = sr.score_files(late, R.PIECE, bank, [c1], R.CHUNK, R.SR, 64)
    assert [f.name for f in got] == [sr.file_name(R.PIECE, c1, 1), sr.file_name(R.PIECE, c1, 2)]
    assert len(sr.score_files(late, R.PIECE, bank, [c0], R.CHUNK, R.SR, 64)) == 3      # size 2000: the note fits


def test_unordered_and_out_of_bank_tables_are_rejected():
    ok = [[(0, 0, 10), (5, 10, 10), (5, 0, 3)], [(7, 2, 1)]]
    packed, counts = sr.pack_notes(ok, 20)
    assert list(counts) == [3, 1] and list(packed[:, 3]) == [10, 15, 15, 8]
    for bad, bank_len in (([[(5, 0, 10), (4, 0, 10)]], 20),            # b decreases within a track
                          ([[(0, 15, 10)]], 20),                       # reaches past the bank
                          ([[(0, -1, 10)]], 20), ([[(-1, 0, 10)]], 20), ([[(0, 0, -1)]], 20), ([[(0, 21, 0)]], 20)):
        with pytest.raises(ValueError):
            sr.pack_notes(bad, bank_len)
    sr.pack_notes([[(5, 0, 10)], [(4, 0, 10)]], 20)                    # the order holds per track, not across tracks


# ------------------------------------------------------------------------------------------------ Sibelius
def test_sibelius_files_render_the_reference_s_audio(g):
    combos = sr.sibelius_combinations(R.SIB_SHIFTS, R.SIB_GAINS, 4)
    assert np.array_equal(np.asarray(combos), g["sib_combos"]) and len(combos) == 78
    vfs = sr.sibelius_files(R.SIB_LENGTHS, R.SIB_SHIFTS, R.SIB_GAINS, R.SR, name='p')
    signals = {('p', i): x for i, x in enumerate(R.sibelius_sources())}
    for k, ci in enumerate(R.SIB_PICK):
        want = g["sib_audio_%d" % k]
        vf = vfs[ci]
        assert vf.size == len(want) and vf.chunks == ((0, vf.size),) and vf.m == 1.0
        got = augment.render_audio(signals, vf)
        assert np.array_equal(got.T, want), k
    gt = sr.sibelius_files(R.SIB_LENGTHS, (0.,), (1.,), R.SR)
    assert len(gt) == 1 and gt[0].size == R.SIB_LENGTHS[0] and all(t.k == 0 and t.g == 1.0 for t in gt[0].tracks)
