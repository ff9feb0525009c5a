"""Host rule of the score-informed RWC generator (deepconvsep_amd/score_render.py: ``score_informed_files``) against the
reference's own lines, recorded in tests/golden/score_render_si.npz by tests/golden/make_golden_score_render_si.py on the
seeded inputs of tests/score_render_si_ref.py.  No GPU: the packer ``dcs_score_render_pack`` is host code of libdcs."""
import os

import numpy as np
import pytest

import score_render_ref as R
import score_render_si_ref as SI
from deepconvsep_amd import rwc, score_render as sr

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sorted(('unequal', 'gt', 'overwrite', 'cut', 'past'))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "score_render_si.npz"))


@pytest.fixture(scope="module")
def g_bach10():
    return np.load(os.path.join(HERE, "golden", "score_render.npz"))


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    return SI.write_pieces(str(tmp_path_factory.mktemp("db")))


@pytest.fixture(scope="module")
def bank(tmp_path_factory):
    tree = R.write_rwc_tree(str(tmp_path_factory.mktemp("rwc")))
    return rwc.NoteBank.from_instruments([rwc.Instrument(tree, i, list(R.STYLES), list(R.CASES), list(R.DYNAMICS))
                                          for i in R.INSTRUMENT_IDS])


def files(db, bank, piece, style, combos):
    return sr.score_informed_files(SI.piece_dir(db, piece), bank, combos, SI.CHUNK, SI.SR, SI.HOP, SI.FRAME,
                                   SI.STYLE_MIDI[style], nharmonics=SI.NHARMONICS, interval=SI.INTERVAL, tuning_freq=SI.TUNING)


@pytest.fixture(scope="module")
def rendered(db, bank):
    """The recorded (piece, style, combination, chunk) as ScoreInformedFiles."""
    out = []
    for piece, style, ci, chnk in SI.RENDERS:
        sfs = files(db, bank, piece, style, [R.COMBOS[ci]])
        assert len(sfs) == 3
        out.append(sfs[chnk])
    return out


@pytest.mark.parametrize("k", range(len(SI.RENDERS)))
def test_virtual_files_equal_what_the_reference_hands_to_its_transform(g, bank, rendered, k):
    piece, style, ci, chnk = SI.RENDERS[k]
    sf = rendered[k]
    audio = g["audio_%d" % k]
    assert sf.size == audio.shape[0]
    np.testing.assert_array_equal(sr.render_score_audio(bank, sf), audio)
    np.testing.assert_array_equal(sf.melody_g, g["melody_g_%d" % k])
    np.testing.assert_array_equal(sf.melody_e, g["melody_e_%d" % k])
    assert sf.melody_g.dtype == np.float64 and sf.melody_g.shape[2] == 2 * SI.NHARMONICS + 3
    stem = bytes(g["stem_%d" % k]).decode('ascii')
    assert os.path.join(piece, style, sf.name) == stem
    assert stem.endswith('_%d' % chnk)


def test_the_recorded_pairs_hold_every_case(g, rendered):
    """What the generator asserted of the reference's output, asserted of the project's tables."""
    seen = {}
    for k, (piece, style, ci, chnk) in enumerate(SI.RENDERS):
        sf, c = rendered[k], R.COMBOS[ci]
        seglen = g["seglen_%d" % k].tolist()
        # the uncut segment lengths in the generator's order: every row of melody_g with a MIDI number
        rows = [(int(np.floor(sf.melody_g[i, m, 0] * SI.HOP)), seglen.pop(0)) for i in range(4)
                for m in range(sf.melody_g.shape[1]) if sf.melody_g[i, m, 2] > 0]
        assert not seglen
        has = dict(unequal=len(set(c[:, 0])) > 1, gt=style == 'gt', overwrite=SI.overwrites(sf.tracks),
                   cut=any(b < sf.size and ln > sf.size - b for b, ln in rows), past=any(b >= sf.size for b, _ in rows))
        assert [has[n] for n in CASES] == g["cases_%d" % k].tolist(), (k, has)
        for n, v in has.items():
            seen[n] = seen.get(n, False) or v
        if has['past']:    # the notes at and past size are in the table and not in the track
            assert sum(len(t) for t in sf.tracks) < len(rows)
    assert all(seen.values()), seen
    assert g["cases_0"][CASES.index('unequal')] and g["cases_0"][CASES.index('cut')]
    assert g["cases_1"][CASES.index('gt')] and g["cases_1"][CASES.index('overwrite')]


@pytest.mark.parametrize("piece", SI.WRITTEN)
def test_files_the_reference_does_not_write_are_not_produced(g, db, bank, piece):
    want = [tuple(r) for r in g["written_" + piece].tolist()]
    got = []
    for ci in SI.WRITTEN_COMBOS:
        c = R.COMBOS[ci]
        names = [sr.si_file_name(np.array(c), chnk) for chnk in range(3)]
        for sf in files(db, bank, piece, 'original', [c]):
            got.append((ci, names.index(sf.name)))
    assert got == want
    if piece != '05-Edge':
        assert len(want) < 3 * len(SI.WRITTEN_COMBOS)      # the fixture really holds a file that is not written


def test_combinations_are_the_bach10_generator_s_rule(g, g_bach10):
    """``Engine.__init__`` of the score-informed generator draws what ``rwc_combinations`` draws -- one rule, one copy."""
    for name in ("combos_default", "combos_few_shifts", "combos_few_dynamics", "combos_single"):
        np.testing.assert_array_equal(g[name], g_bach10[name])
    np.testing.assert_array_equal(sr.rwc_combinations(SI.SHIFTS, 3, 1, [1, 2, 3], 4, 400, 5), g["combos_default"])
    np.testing.assert_array_equal(sr.rwc_combinations([0., 0.2], 1, 1, [1], 4, 400, 0), g["combos_few_shifts"])
    np.testing.assert_array_equal(sr.rwc_combinations([0.], 2, 1, [1], 4, 10, 3), g["combos_few_dynamics"])
    np.testing.assert_array_equal(sr.rwc_combinations([0.], 1, 1, [2], 4, 400, 0), g["combos_single"])


def test_the_tables_go_through_the_packer_unchanged(g, bank, rendered):
    """``b`` is non-decreasing within every track, so ``dcs_score_render_pack`` accepts the notes in the generator's order;
    the golden tables say the same of the reference's own first frames."""
    for k, sf in enumerate(rendered):
        packed, counts = sr.pack_notes(sf.tracks, bank.length)
        flat = [n for t in sf.tracks for n in t]
        assert counts.tolist() == [len(t) for t in sf.tracks]
        np.testing.assert_array_equal(packed[:, :3], np.asarray(flat, dtype=np.int64).reshape(-1, 3))
        at = 0
        for t in sf.tracks:
            b = packed[at:at + len(t), 0]
            assert np.all(np.diff(b) >= 0)
            np.testing.assert_array_equal(packed[at:at + len(t), 3], np.maximum.accumulate(b + packed[at:at + len(t), 2]))
            at += len(t)
        mg = g["melody_g_%d" % k]
        for i in range(mg.shape[0]):
            first = mg[i, mg[i, :, 2] > 0, 0]
            assert np.all(np.diff(first) >= 0)
    packed, rows = sr.pack_tables(rendered, bank.length, SI.HOP)
    assert rows.shape == (len(rendered), 2 + 2 * 4)


def test_dataset_files_original_and_gt(db, bank):
    """``--original 0``: style gt, the scores <source>_g.txt, one shift, at most 50 combinations."""
    only = [R.PIECE]
    out = sr.si_dataset_files(db, bank, chunk_size=SI.CHUNK, sample_size=60, original=False, seed=1, sr=SI.SR, hop=SI.HOP,
                              frame=SI.FRAME, pieces=only)
    (piece, style, sfs), = out
    assert (piece, style) == (R.PIECE, 'gt') and len(sfs) == 50 * 3
    assert all(sf.size == 2000 for sf in sfs)
    out = sr.si_dataset_files(db, bank, chunk_size=SI.CHUNK, sample_size=3, original=True, seed=1, sr=SI.SR, hop=SI.HOP,
                              frame=SI.FRAME, pieces=only)
    (piece, style, sfs), = out
    assert (piece, style) == (R.PIECE, 'original') and len(sfs) == 3 * 3
    combos = sr.rwc_combinations(SI.SHIFTS, 3, 1, sr.CASES, 4, 3, 1)
    assert [sf.name for sf in sfs] == [sr.si_file_name(np.array(c), k) for c in combos for k in range(3)]
