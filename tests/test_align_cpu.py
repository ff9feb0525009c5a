"""Host side of the score-to-audio alignment (deepconvsep_amd/align.py) and the float64 oracle of tests/align_ref.py that
tests/test_gpu_align.py holds the device to.  No GPU."""
import inspect
import itertools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import align_ref  # noqa: E402
from deepconvsep_amd import _lib, align  # noqa: E402
from deepconvsep_amd.score import read_score, str2midi, write_score  # noqa: E402
from deepconvsep_amd.separation import train_auto, train_auto_scores  # noqa: E402

SYMBOLS = ("dcs_chroma", "dcs_dtw", "dcs_dtw_bytes", "dcs_dtw_tile")


def test_oracle_dtw_equals_brute_force_enumeration():
    """every T, U <= 5, without a band and with bands 0 .. 2: D at every cell, the end cost and the path the tie rule picks.
    Costs are small multiples of 1/4 (exact sums, many ties)."""
    rs = np.random.RandomState(0)
    checked = refused = 0
    for T, U in itertools.product(range(1, 6), repeat=2):
        for band in (None, 0, 1, 2):
            for _ in range(3):
                # features whose products are the costs wanted: a = e_i rows scaled, s likewise, so that c = 1 - a . s takes
                # few distinct values
                A = np.zeros((T, 12))
                S = np.zeros((U, 12))
                A[np.arange(T), rs.randint(0, 3, T)] = rs.randint(1, 4, T) * 0.5
                S[np.arange(U), rs.randint(0, 3, U)] = rs.randint(1, 4, U) * 0.5
                cost = 1.0 - A @ S.T
                ok = align_ref.in_band(T, U, band)
                want_path, Dmin = align_ref.brute_force(cost, ok)
                path, end, D = align_ref.dtw(A, S, band=band)
                assert np.array_equal(D, Dmin), (T, U, band)
                if want_path is None:
                    assert path is None and end == np.inf
                    refused += 1
                else:
                    assert np.array_equal(path, want_path), (T, U, band, path, want_path)
                    assert end == Dmin[-1, -1] == align_ref.path_cost(A, S, path)
                    checked += 1
    assert checked > 250 and refused > 0


def test_oracle_dtw_float32_and_float64_agree_on_dyadic_features():
    A, S = align_ref.dyadic_features(70, 91, seed=4)
    p64, c64, _ = align_ref.dtw(A, S)
    p32, c32, _ = align_ref.dtw(A, S, dtype=np.float32)
    assert np.array_equal(p64, p32) and c64 == c32
    diag = np.sum((np.diff(p64, axis=0) == 1).all(axis=1))
    assert 0 < diag < len(p64) - 1                                    # all three steps occur


def test_bin_classes():
    cls = align.bin_classes(2048)
    assert cls.dtype == np.int8 and cls.shape == (1025,)
    f = np.arange(1025) * 44100.0 / 2048
    assert cls[int(round(440.0 * 2048 / 44100))] == 9                 # A4
    assert cls[int(round(261.63 * 2048 / 44100))] == 0                # C4
    assert cls[0] == -1
    assert (cls[(f < 100.0) | (f > 5000.0)] == -1).all() and (cls[(f >= 100.0) & (f <= 5000.0)] >= 0).all()
    assert set(np.unique(cls)) == set(range(-1, 12))
    # another tuning moves the classes with it; a table that starts at 0 Hz still leaves bin 0 out
    assert align.bin_classes(2048, tuning_freq=466.16)[int(round(466.16 * 2048 / 44100))] == 9
    assert align.bin_classes(64, fmin=0.0, fmax=1e9)[0] == -1


def test_score_chroma():
    scores, _ = align_ref.piece()
    U = align_ref.score_frames(scores)
    got = align.score_chroma(scores, U, align_ref.HOP, align_ref.RATE)
    assert got.dtype == np.float32 and got.shape == (U, 12)
    assert np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() <= 4 * 2.0 ** -24
    assert np.abs(got - align_ref.score_chroma(scores, U)).max() <= 2.0 ** -24
    for name in ("C4", "Bb3", "F#5"):
        assert align_ref.name_to_midi(name) == str2midi(name)
    empty = align.score_chroma([(np.zeros(0), np.zeros(0), [])], 7, 512, 44100)
    assert np.array_equal(empty, np.full((7, 12), np.float32(1 / math.sqrt(12))))
    # one A4 from frame 2 to frame 4: the fundamental, the octave and the double octave on A, the twelfth and its octave on E, the
    # major third on C#
    fps = 44100 / 512
    one = align.score_chroma([(np.array([2 / fps]), np.array([4 / fps]), ["A4"])], 6, 512, 44100).astype(np.float64)
    w = np.zeros(12)
    w[9], w[4], w[1] = 1 + 0.7 + 0.7 ** 3, 0.7 ** 2 + 0.7 ** 5, 0.7 ** 4
    assert np.abs(one[2:4] - w / np.sqrt((w * w).sum())).max() <= 2.0 ** -24
    assert np.array_equal(one[[0, 1, 4, 5]], np.full((4, 12), float(np.float32(1 / math.sqrt(12)))))


def test_time_map_and_warp_times():
    path = np.array([(0, 0), (1, 0), (2, 1), (2, 2), (3, 3), (4, 3), (5, 3), (6, 4)], dtype=np.int32)
    tmap = align.time_map(path, 5)
    assert tmap.dtype == np.float64 and np.array_equal(tmap, [0.5, 2.0, 2.0, 4.0, 6.0])
    assert (np.diff(tmap) >= 0).all()
    with pytest.raises(ValueError):
        align.time_map(path[path[:, 1] != 1], 5)
    oracle = align_ref.oracle_run()
    assert (np.diff(align.time_map(oracle["path"], oracle["U"])) >= 0).all()
    diag = np.stack([np.arange(50), np.arange(50)], axis=1)
    times = np.array([0.0, 0.1234, 0.3, 49 / 86.1328125])
    assert np.abs(align.warp_times(times, align.time_map(diag, 50), 86.1328125) - times).max() <= 1e-15
    assert align.auto_band(8192, 8192) is None and align.auto_band(8193, 8192) == 1025


def test_write_score_round_trips(tmp_path):
    scores, _ = align_ref.piece()
    on, off, names = scores[1]
    on = on + 1.0 / 3.0                                               # not float32 values: read_score delivers float32
    path = str(tmp_path / "clarinet_b.txt")
    write_score(path, on, off, names)
    on2, off2, names2 = read_score(path)
    assert np.array_equal(on2, on.astype(np.float32).astype(np.float64)) and np.array_equal(off2, off) and names2 == list(names)
    write_score(path, on2, off2, names2)
    on3, off3, names3 = read_score(path)
    assert np.array_equal(on3, on2) and np.array_equal(off3, off2) and names3 == names2


def test_oracle_aligns_the_synthetic_piece():
    """The yardstick of the GPU test: float64 throughout.  Measured: T = 795, U = 688, 61 notes; onset error median 0.512, p90
    2.347, max 14.2 frames after alignment against a median of 61.6 (max 102) before; the path strays 37.5 score frames from
    the straight line."""
    r = align_ref.oracle_run()
    med, p90 = float(np.median(r["errors"])), float(np.percentile(r["errors"], 90))
    un = float(np.median(r["unaligned"]))
    print("T %d U %d: onset error median %.3f p90 %.3f max %.3f frames; unaligned median %.2f max %.1f; stray %.1f"
          % (r["T"], r["U"], med, p90, r["errors"].max(), un, r["unaligned"].max(), r["stray"]))
    assert med <= un / 10.0                                           # the condition on the input
    assert abs(med - align_ref.ORACLE_MEDIAN) <= 2e-3 and abs(p90 - align_ref.ORACLE_P90) <= 2e-3
    assert abs(un - align_ref.ORACLE_UNALIGNED_MEDIAN) <= 0.1
    assert r["stray"] <= align_ref.ORACLE_MAX_STRAY < 64
    banded = align_ref.oracle_run(64)
    assert np.array_equal(banded["path"], r["path"]) and banded["cost"] == r["cost"]
    assert abs(align_ref.path_cost(r["A"], r["S"], r["path"]) - r["cost"]) <= 1e-9


def test_header_declares_and_library_exports_the_alignment():
    assert set(SYMBOLS) <= set(_lib.header_symbols())
    lib = _lib.load()
    for n in SYMBOLS:
        assert getattr(lib, n).argtypes is not None, n
    B = lib.dcs_dtw_tile()
    assert B >= 1
    # scratch follows the band, not T x U
    assert 0 < lib.dcs_dtw_bytes(20000, 20000, 200) * 5 <= lib.dcs_dtw_bytes(20000, 20000, -1)
    assert align.dtw_bytes(20000, 20000, 200) == lib.dcs_dtw_bytes(20000, 20000, 200)
    for T, U, band in ((10, 100, 2), (0, 5, -1), (5, 0, -1), (5, 5, -2), ((1 << 20) + 1, 5, -1), (5, (1 << 20) + 1, -1),
                       (1 << 20, 1 << 20, -1)):
        assert lib.dcs_dtw_bytes(T, U, band) == -1, (T, U, band)
    with pytest.raises(ValueError):
        align.dtw_bytes(10, 100, 2)
    assert lib.dcs_dtw_bytes(10, 100, 5) > 0 and lib.dcs_dtw_bytes(1, 8, 3) > 0 and lib.dcs_dtw_bytes(1 << 20, 1 << 20, 100) > 0
    # a null context is refused before anything else is looked at
    assert lib.dcs_dtw(None, None, 5, None, 5, -1, None, None, None) == _lib.DCS_EINVAL
    assert lib.dcs_chroma(None, None, 5, 5, 5, None, 1e-6, None) == _lib.DCS_EINVAL


def test_scripts_take_the_new_options():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("align_scores.py", "separate_bach10.py"):
        spec = importlib.util.spec_from_file_location("si_" + name[:-3], os.path.join(root, "examples", "bach10_scoreinformed", name))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert ("--band" in mod.USAGE) == (name == "align_scores.py") and ("--align" in mod.USAGE) == (name != "align_scores.py")
        with pytest.raises(SystemExit):
            mod.main(["--no-such-option"])
        if name == "separate_bach10.py":
            # the flag reaches train_auto; without it the call is the one the script made before
            calls = []
            mod.train_auto = lambda *a, **kw: calls.append((a, kw))
            mod.main(["-i", "mix.wav", "-o", "out", "-m", "model.pkl"])
            mod.main(["-i", "mix.wav", "-o", "out", "-m", "model.pkl", "--align"])
            assert [kw["align"] for _, kw in calls] == [False, True]
            assert calls[0][0] == calls[1][0] == ("mix.wav", "out", "model.pkl", 0.3, 30, 25, 32, 2049, 4096, 512)
            # the library's train_auto keeps its signature; the variant that takes the score directory has it in front
            assert ["score_dir"] + list(inspect.signature(train_auto).parameters) == list(inspect.signature(train_auto_scores).parameters)
