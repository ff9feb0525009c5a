"""The host side of the augmented hiphop trainers (deepconvsep_amd/augment.py) without a GPU: the shift rule, the
enumerations and the chunking against the reference's own lines (tests/golden/augment_cs.npz, written by
tests/golden/make_golden_augment.py), the virtual-file tables of the four generators, the window table and the command
lines."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import augment_ref
from deepconvsep_amd import augment
from deepconvsep_amd.training import FeatureWindows
from deepconvsep_amd.transform import write_shape_file

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "augment_cs.npz"))


def test_shift_samples_and_closed_form_equal_circular_shift(golden):
    sr = int(golden["sr"])
    x = golden["shift_x"]
    shifts, sizes = list(golden["shift_cs"]), list(golden["shift_sizes"])
    assert sorted(shifts) == sorted([0., 0.2, -0.2, 0.07, -0.07, 100., -100.]) and min(sizes) < len(x) < max(sizes)
    assert [augment.shift_samples(cs, sr) for cs in (0., 0.2, -0.2, 0.07, -0.07, 100., -100.)] == [0, 5, -5, 1, -1, 2500, -2500]
    assert augment.shift_samples(0.2, 44100) == 8820 and augment.shift_samples(-0.07, 44100) == -3087
    for i, (cs, size) in enumerate(itertools.product(shifts, sizes)):
        want = golden["shift_%d" % i]
        got = augment_ref.shifted(x, int(size), augment.shift_samples(cs, sr))
        assert want.shape == (size,) and np.array_equal(got, want), (cs, size)
        sig = {('s', 'x'): x}
        vf = augment.VirtualFile((augment.Track(('s', 'x'), augment.shift_samples(cs, sr), 1.0, 1),), 1.0, int(size), (), ())
        assert np.array_equal(augment.render_audio(sig, vf)[1], want), (cs, size)
    assert not golden["shift_%d" % (2 * shifts.index(100.))].any()          # beyond the signal: silence of min_size samples


def test_combinations_and_activation_equal_the_reference(golden):
    combos = augment.cs_combinations([0., 0.2], [1.], 4)
    assert len(combos) == 14 and np.array_equal(np.asarray(combos), golden["combos"])
    # :66-67: one time shift and one intensity leave nothing, the first pair for every source is taken
    fb = augment.cs_combinations([0.], [1.], 4)
    assert np.array_equal(np.asarray(fb), golden["combos_fallback"]) and np.asarray(fb).shape == (1, 4, 2)
    # as many pairs as sources: the permutation branch (:65)
    assert len(augment.cs_combinations([0., 0.1, 0.2, 0.3], [1.], 4)) == 24
    assert np.array_equal(augment.instrument_activation(), golden["activation"])


@pytest.mark.parametrize("size,want", [
    (4095, [(0, 2048), (2048, 2047)]),                    # one sample below a multiple
    (4096, [(0, 2048), (2048, 2048), (4096, 0)]),         # a multiple: the rest is empty, and still a file
    (4097, [(0, 2048), (2048, 2048), (4096, 1)]),
    (700, [(0, 700)]),                                    # shorter than one chunk: the rest chunk only
])
def test_chunk_bounds(size, want):
    assert augment.chunk_bounds(size, 1000, chunk=2048) == want
    assert augment.chunk_bounds(size, 1000, rest=False, chunk=2048) == [w for w in want if w[1] == 2048]


def test_chunk_bounds_default_is_thirty_seconds_and_cs_counts_blocks_from_the_rendered_size(golden):
    assert augment.chunk_bounds(3 * 44100 * 30 + 5) == [(i * 1323000, 1323000) for i in range(3)] + [(3969000, 5)]
    # vocals of exactly two blocks: the 0.2 s shift shortens the rendered signal below the second block
    sr, chunk = 1000, 2048
    vf = augment.virtual_files('cs', dict(vocals=4096, bass=4096, drums=4096, other=4096), sr=sr, chunk=chunk)[0]
    assert vf.size == 4096 - 200 and vf.chunks == ((0, 2048), (2048, 1848))
    # the golden's own chunking (the reference's lines :92, :122-147 at 25 Hz)
    for tag in ("a", "b"):
        got = augment.chunk_bounds(int(golden[tag + "_size"]), int(golden["sr"]))
        assert [Lc for _, Lc in got] == list(golden[tag + "_chunk_lengths"])


def _lengths():
    return dict(vocals=7000, bass=6000, drums=5000, other=3000)


def test_virtual_files_of_the_three_single_song_generators():
    ln = _lengths()
    (vf,) = augment.virtual_files('none', ln, sr=1000, chunk=2048, song='s')
    assert [t.signal[1] for t in vf.tracks] == ['bass', 'drums', 'other', 'vocals'] and [t.c for t in vf.tracks] == [2, 3, 4, 1]
    assert vf.m == 1.0 and vf.size == ln['other'] and all(t.k == 0 and t.g == 1.0 for t in vf.tracks)
    assert vf.names == ('s_0', 's_1') and vf.chunks == ((0, 2048), (2048, 952))

    cs = augment.virtual_files('cs', ln, sr=1000, chunk=2048, song='s')
    assert len(cs) == 14
    for vf, c in zip(cs, augment.cs_combinations()):
        assert [t.signal[1] for t in vf.tracks] == ['vocals', 'bass', 'drums', 'other'] and [t.c for t in vf.tracks] == [1, 2, 3, 4]
        assert [t.k for t in vf.tracks] == [200 if x else 0 for x in c[:, 0]] and vf.m == 1.0
        assert vf.size == 7000 - 200 and len(vf.chunks) == 4
    assert cs[0].names[0] == 's_0_cs0001' and cs[-1].names[3] == 's_3_cs1110'
    assert len(set(n for vf in cs for n in vf.names)) == 14 * 4

    ins = augment.virtual_files('instr', ln, sr=1000, chunk=2048, song='s')
    assert len(ins) == 5
    for i, vf in enumerate(ins):
        assert [t.signal[1] for t in vf.tracks] == ['bass', 'drums', 'other', 'vocals'] and vf.m == 0.25 and vf.size == 6000
        assert [t.g for t in vf.tracks] == [0.0 if j == i else 1.0 for j in range(4)]      # the targets keep gain 1
        assert vf.names[0] == 's_0_%d' % (i + 1)


def test_virtual_files_of_mix_aug_are_reproducible_from_the_seed():
    songs = ['s%d' % i for i in range(7)]
    lengths = [dict(vocals=5000 + 100 * i, bass=5100 + 90 * i, drums=5300 - 50 * i, other=5200 + 10 * i) for i in range(7)]
    lengths[2]['vocals'] = None                      # an instrumental
    a = augment.virtual_files('mix', lengths, sr=1000, chunk=2048, seed=3, songs=songs)
    b = augment.virtual_files('mix', lengths, sr=1000, chunk=2048, seed=3, songs=songs)
    c = augment.virtual_files('mix', lengths, sr=1000, chunk=2048, seed=4, songs=songs)
    assert a == b and a != c
    first, second = a[:7], a[7:]
    for name, ln, vf in zip(songs, lengths, first):
        assert vf.m == 0.25 and vf.size == ln['other'] and [t.c for t in vf.tracks] == [2, 3, 4, 1]
        assert len(vf.chunks) == 3 and vf.names[0] == name + '_0'
    assert first[2].tracks[3] == augment.Track(('s2', 'other'), 0, 0.0, 1)               # silent vocals
    sel = augment.mix_selections(songs, 3)
    assert len(second) == len(sel) > 0
    for (comb, f, p), vf in zip(sel, second):
        assert comb % 10 == sel[0][0] % 10 and len(set(f)) == 4
        assert [t.signal for t in vf.tracks] == [(f[p[0]], 'bass'), (f[p[1]], 'drums'), (f[p[2]], 'other'), (f[p[3]], 'vocals')]
        assert [t.c for t in vf.tracks] == [2, 3, 4, 1] and vf.m == 0.25
        assert vf.size == min(dict(zip(songs, lengths))[t.signal[0]][t.signal[1]] for t in vf.tracks)
        assert all(Lc == 2048 for _, Lc in vf.chunks) and len(vf.chunks) == vf.size // 2048       # whole blocks only
        assert vf.names[0] == "combination_%d_perm_%d_%d_%d_%d_block_1" % ((comb,) + p)


def test_rendered_rule_equals_the_reference_render(golden):
    """augment.render_audio and tests/augment_ref.render on the golden's sources equal what the reference's lines rendered."""
    sr = int(golden["sr"])
    src = {('song', s): golden["src_" + s] for s in augment.CHANNELS}
    for tag in ("a", "b"):
        c, size = golden[tag + "_c"], int(golden[tag + "_size"])
        tracks = tuple(augment.Track(('song', s), augment.shift_samples(c[j, 0], sr), float(c[j, 1]), 1 + j)
                       for j, s in enumerate(augment.ADD_ORDER['cs']))
        vf = augment.VirtualFile(tracks, 1.0, size, tuple(augment.chunk_bounds(size, sr)), ())
        assert np.array_equal(augment.render_audio(src, vf), golden[tag + "_rendered"])
        ref = augment_ref.render([(src[t.signal], t.k, t.g, t.c) for t in tracks], 1.0, size)
        assert np.array_equal(ref, golden[tag + "_rendered"])
    assert not golden["b_rendered"][4].any() and golden["b_rendered"][1].any()
    # variant 5 of the 14 is what virtual_files builds
    vf5 = augment.virtual_files('cs', {s: len(golden["src_" + s]) for s in augment.CHANNELS}, sr=sr)[5]
    assert vf5.size == int(golden["a_size"]) and [t.k for t in vf5.tracks] == [augment.shift_samples(x, sr) for x in golden["a_c"][:, 0]]


def test_table_rows_layout():
    ln = _lengths()
    vfs = augment.virtual_files('cs', ln, sr=1000, chunk=2048, song='s')[:2]
    index = {('s', 'vocals'): (0, 7000), ('s', 'bass'): (7000, 6000), ('s', 'drums'): (13000, 5000), ('s', 'other'): (18000, 3000)}
    rows, gains = augment.table_rows(vfs, index, 512)
    assert rows.shape == (8, 4 + 4 * 4) and rows.dtype == np.int64 and gains.shape == (8, 5) and gains.dtype == np.float64
    assert list(rows[3]) == [6800, 6144, 656, 4, 0, 7000, 0, 1, 7000, 6000, 0, 2, 13000, 5000, 0, 3, 18000, 3000, 200, 4]
    assert list(gains[3]) == [1.0, 1.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("windows", ["reference", "all"])
def test_rendered_windows_slot_table_equals_feature_windows(tmp_path, windows):
    """Same frame counts, same table: every (virtual file, chunk) stands for one .data file."""
    rs = np.random.RandomState(0)
    ln = _lengths()
    signals = {('s', s): rs.uniform(-0.1, 0.1, n) for s, n in ln.items()}
    vfs = augment.virtual_files('cs', ln, sr=1000, chunk=2048, song='s')[:3] + \
        augment.virtual_files('instr', dict(ln, bass=150), sr=1000, chunk=2048, song='s')[:1]       # a file shorter than tc
    rw = augment.RenderedWindows(signals, vfs, time_context=8, overlap=5, mult_factor=0.3, windows=windows, batch_size=4,
                                 seed=7, frameSize=256, hopSize=64)
    paths = []
    for i, r in enumerate(rw.rows):
        p = str(tmp_path / ("%03d.data" % i))
        write_shape_file(p.replace('.data', '.shape'), (5, int(r[3]), 129))
        paths.append(p)
    fw = FeatureWindows(paths, 8, 5, 0.3, windows, 4, 7)
    assert np.array_equal(rw.table, fw.table) and rw.table.dtype == fw.table.dtype
    assert (rw.F, rw.total, rw.iteration_size) == (fw.F, fw.total, fw.iteration_size) and rw.F == 129
    assert int(rw.rows[-1][3]) < 8 and len(rw.names) == len(rw.rows)


def test_package_exports():
    import deepconvsep_amd as dcs
    assert dcs.RenderedWindows is augment.RenderedWindows and dcs.render_features is augment.render_features


@pytest.mark.parametrize("script,words", [
    ("examples/hiphopss/compute_features.py", ("--augment", "none,cs,instr,mix", "--feature_path", "--seed")),
    ("examples/hiphopss/train_hhds.py", ("--augment", "none,cs,instr,mix", "--render", "--skip_sep", "--nepochs")),
])
def test_command_lines_parse_and_print_help(script, words):
    exe = os.path.join(ROOT, script)
    r = subprocess.run([sys.executable, exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in words), r.stdout + r.stderr
    r = subprocess.run([sys.executable, exe, "--db", "x", "--augment", "nonsense"], capture_output=True, text=True)
    assert r.returncode == 2


def test_trainer_selections_per_augmentation():
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_hhds", os.path.join(ROOT, "examples", "hiphopss", "train_hhds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MODELS == {'none': 'hh_fft_1024', 'cs': 'hh_cs_aug_fft_1024', 'instr': 'hh_instr_aug_fft_1024',
                          'mix': 'hh_mix_aug_fft_1024'}
    assert mod.FEATURE_DIRS == {'none': 't1', 'cs': 't1_cs_aug', 'instr': 't1_instr_aug', 'mix': 't1_mix_aug'}
    assert mod.loss_weights('mix') == (0.000001, 0.00001, 0.00003) and mod.loss_weights('cs') == (0.001, 0.01, 0.03)
    assert mod.dev_mixture('instr') == 'mixture_5.wav' and mod.dev_mixture('cs') == 'mixture.wav'
