"""The stereo (ILD) DSD100 trainer, CPU side: the float64 restatement tests/train_ild_ref.py against the reference's own
loss code (tests/golden/train_ild_loss.npz, written by tests/golden/make_golden_train_ild.py), parameter shapes and
initialisation, the window tables of StereoFeatureWindows, and the feature script's file naming."""
import importlib.util
import math
import os

import numpy as np
import pytest

import train_ild_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_ild_loss.npz")


@pytest.mark.parametrize("case", ["plain", "zeros"])
def test_restatement_matches_the_reference_loss(case):
    """Both are float64 and only the summation order differs: rtol 1e-10 on the ten values (the stage-2 loss, the eight
    errors_insts, the ILD term) and on the stage-1 loss."""
    g = np.load(GOLDEN)
    p, x, tgt, r = (g["%s_%s" % (case, k)] for k in ("p", "x", "tgt", "r"))
    if case == "zeros":
        assert (p[:, 0::2].sum(axis=1) == 0).any() and (p.sum(axis=1) == 0).any()      # all outputs zero
        assert ((tgt[:, 0::2] == 0) & (tgt[:, 1::2] == 0)).any()                       # a silent target pair
    got = train_ild_ref.components_np(p, x, tgt, r, stage=2)
    want = g["%s_values" % case]
    assert got.shape == (10,) and np.isfinite(want).all()
    print(case, "got", got, "want", want)
    np.testing.assert_allclose(got, want, rtol=1e-10)
    got1 = train_ild_ref.components_np(p, x, tgt, r, stage=1)
    np.testing.assert_allclose(got1[0], float(g["%s_loss1" % case]), rtol=1e-10)
    np.testing.assert_allclose(got1[1:9], want[1:9], rtol=1e-10)
    assert got1[9] == 0.0
    # the ILD term is what stage 2 adds, with the weight of :228
    np.testing.assert_allclose(got[0] - got1[0], want[9], rtol=1e-9)
    heavy = train_ild_ref.components_np(p, x, tgt, r, stage=2, ild_weight=1.0)
    np.testing.assert_allclose(heavy[9], 500 * want[9], rtol=1e-10)


def test_ild_term_depends_on_the_draw_in_silent_bins():
    g = np.load(GOLDEN)
    p, x, tgt, r = (g["zeros_%s" % k] for k in ("p", "x", "tgt", "r"))
    r2 = r.copy()
    r2[1] = 0.1 * np.random.RandomState(9).randn(*r[1].shape)
    a = train_ild_ref.components_np(p, x, tgt, r, stage=2)
    b = train_ild_ref.components_np(p, x, tgt, r2, stage=2)
    assert abs(a[9] - b[9]) > 1e-3 * a[9]
    np.testing.assert_allclose(a[1:9], b[1:9], rtol=1e-9)       # the squared errors do not


def test_parameter_shapes_and_glorot_bounds():
    from deepconvsep_amd import stereo_training as st
    from deepconvsep_amd.arch import ARCHS
    tc, F = 30, 513
    shapes = st.param_shapes(tc, F)
    assert shapes == [tuple(s) for s in ARCHS['dsd_ild'].param_shapes(tc, F)]
    flat = 50 * 16
    assert len(shapes) == 17
    assert shapes[0] == (50, 2, 1, 513) and shapes[3] == (50, 50, 15, 1) and shapes[6] == (flat, 256)
    assert shapes[8:16:2] == [(256, flat)] * 4 and shapes[9:16:2] == [(flat,)] * 4 and shapes[16] == (8,)
    params = st.glorot_init(tc, F, seed=3)
    for p, s in zip(params, shapes):
        assert p.shape == s and p.dtype == np.float32
        if len(s) == 1:
            assert not p.any()
            continue
        rf = int(np.prod(s[2:])) if len(s) > 2 else 1
        a = math.sqrt(3.0) * math.sqrt(2.0 / ((s[0] + s[1]) * rf))
        assert np.abs(p).max() <= a and np.abs(p).max() > 0.9 * a
    again = st.glorot_init(tc, F, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(params, again))
    assert st.ILD_EPS == 1e-12 and st.ILD_WEIGHT == 1.0 / 500.0 and st.RAND_STD == 0.1


def test_trainable_is_unchanged():
    from deepconvsep_amd import training
    assert training.TRAINABLE == ("dsd", "ikala_nopool", "bach10")
    with pytest.raises(NotImplementedError):
        training.param_shapes("dsd_ild", 30, 513)


def _loadfile_slots(T, tc, overlap):
    """NumPy restatement of LargeDatasetMulti.loadFile's slot rule (dataset.py:931-1007 with getNum :596-602): slot i of
    the getNum(T) slots holds the window at start_i, or stays zero."""
    n = int(np.maximum(1, int(np.floor((T + (np.floor(float(T) / tc) * overlap)) / tc))))
    filled = [None] * n
    if tc > T:
        filled[0] = 0
        return filled
    i, start = 0, 0
    while (start + tc) < T:
        if i >= 0 and i < n:
            filled[i] = start
        i += 1
        start = start - overlap + tc
    return filled


def _write_pair(d, name, T, F, cin=2, cout=8, seed=0):
    from deepconvsep_amd.transform import write_shape_file
    rs = np.random.RandomState(seed)
    out = []
    for kind, c in (("in", cin), ("out", cout)):
        a = rs.uniform(size=(c, T, F))
        path = os.path.join(str(d), "%s_%s_m_.data" % (name, kind))
        a.tofile(path)
        write_shape_file(path.replace(".data", ".shape"), a.shape)
        out.append(a)
    return out


def test_window_tables_follow_loadfile(tmp_path):
    from deepconvsep_amd.stereo_training import StereoFeatureWindows
    Ts = (100, 7, 30, 31, 64, 12)
    for i, T in enumerate(Ts):
        _write_pair(tmp_path, "song%d_0" % i, T, 5, seed=i)
    (tmp_path / "orphan_0_in_m_.data").write_bytes(b"")          # no _out_ next to it: not a pair
    (tmp_path / "note.txt").write_text("x")
    for tc, ov in ((30, 25), (12, 3), (10, 0)):
        w = StereoFeatureWindows([str(tmp_path)], time_context=tc, overlap=ov, batch_size=4)
        assert [os.path.basename(p[0]) for p in w.pairs] == ["song%d_0_in_m_.data" % i for i in range(len(Ts))]
        assert all(p[1].endswith("_out_m_.data") for p in w.pairs)
        assert (w.channels_in, w.channels_out, w.F) == (2, 8, 5)
        want = []
        for i, T in enumerate(Ts):
            want += [(i, s) if s is not None else (-1, 0) for s in _loadfile_slots(T, tc, ov)]
        assert w.table.tolist() == [list(v) for v in want]
        assert w.total == len(want) and w.iteration_size == len(want) // 4
        every = StereoFeatureWindows([str(tmp_path)], time_context=tc, overlap=ov, windows='all', batch_size=4)
        want_all = []
        for i, T in enumerate(Ts):
            want_all += [(i, 0)] if tc > T else [(i, s) for s in range(0, T - tc + 1, tc - ov)]
        assert every.table.tolist() == [list(v) for v in want_all]
    with pytest.raises(ValueError):
        StereoFeatureWindows([str(tmp_path)], windows='some')


def test_mismatched_pairs_are_refused(tmp_path):
    from deepconvsep_amd.stereo_training import StereoFeatureWindows
    from deepconvsep_amd.transform import write_shape_file
    _write_pair(tmp_path, "a_0", 40, 5)
    _write_pair(tmp_path, "b_0", 40, 5, cout=7)                   # 7 outputs for 2 inputs, and not the 8 of a_0
    with pytest.raises(ValueError):
        StereoFeatureWindows([str(tmp_path)])
    os.remove(str(tmp_path / "b_0_in_m_.data"))
    write_shape_file(str(tmp_path / "a_0_out_m_.shape"), (8, 41, 5))   # T differs between in and out
    with pytest.raises(ValueError):
        StereoFeatureWindows([str(tmp_path)])


def _script(name):
    path = os.path.join(ROOT, "examples", "dsd100_2ch_ILD", name)
    spec = importlib.util.spec_from_file_location("ild_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_feature_script_names_chunks_and_channels(tmp_path, monkeypatch):
    """compute_features.py with the transform replaced by a recorder: per song the _in_ files (two channels) then the _out_
    files (eight channels: vocals L, R, bass L, R, drums L, R, other L, R), 30 s chunks plus the rest, a song shorter than
    30 s its rest alone."""
    from deepconvsep_amd.separation import write_wav
    cf = _script("compute_features.py")
    sr = 44100
    lengths = {"051 - Long": 30 * sr + 5000, "052 - Short": 2 * sr}
    for song, n in lengths.items():
        (tmp_path / "Mixtures" / "Dev" / song).mkdir(parents=True)
        (tmp_path / "Sources" / "Dev" / song).mkdir(parents=True)
        t = np.arange(n) / float(sr)
        stems = []
        for k, s in enumerate(cf.SOURCES):
            st = np.stack([0.1 * (k + 1) * np.sin(2 * np.pi * 110 * (k + 1) * t), 0.05 * (k + 1) * np.ones(n)], axis=1)
            write_wav(str(tmp_path / "Sources" / "Dev" / song / (s + ".wav")), st, sr)
            stems.append(st)
        write_wav(str(tmp_path / "Mixtures" / "Dev" / song / "mixture.wav"), sum(stems), sr)
    (tmp_path / "Mixtures" / "Dev" / ".hidden").mkdir()
    calls = []

    class Recorder(object):
        suffix = ''

        def __init__(self, **kw):
            self.kw = kw

        def compute_transform(self, audio, out_path=None, phase=False, save=True):
            calls.append((self.suffix, os.path.basename(out_path), audio.shape, phase, audio.mean(axis=0)))

    monkeypatch.setattr(cf, "transformFFT", Recorder)
    cf.main(["--db", str(tmp_path)])
    names = [(c[0], c[1], c[2]) for c in calls]
    assert names == [("in", "051 - Long_0.data", (30 * sr, 2)), ("in", "051 - Long_1.data", (5000, 2)),
                     ("out", "051 - Long_0.data", (30 * sr, 8)), ("out", "051 - Long_1.data", (5000, 8)),
                     ("in", "052 - Short_0.data", (2 * sr, 2)), ("out", "052 - Short_0.data", (2 * sr, 8))]
    assert not any(c[3] for c in calls)
    # channel order of the eight: the right channel of source k is the constant 0.05 (k + 1)
    out = calls[-1][4]
    np.testing.assert_allclose(out[1::2], [0.05, 0.10, 0.15, 0.20], atol=1e-4)
    assert (tmp_path / "transforms" / "feature_folder").is_dir()
    # the file names the transform derives from the suffix are the ones the feed pairs up
    from deepconvsep_amd.transform import TransformFFT
    assert "suffix" in TransformFFT._PARAMS
    assert cf.chunk_bounds(2 * sr, sr) == [(0, 2 * sr)]
    assert cf.chunk_bounds(60 * sr, sr) == [(0, 30 * sr), (30 * sr, 60 * sr), (60 * sr, 60 * sr)]
