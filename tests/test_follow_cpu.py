"""CPU-only checks around the score follower (csrc/follow.hip): the NumPy restatement of tests/follow_ref.py against a brute-force
enumeration, the window rule, the time map of ``align.follow_scores``, what the Python classes refuse before they reach the
device, the header and the command lines.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from deepconvsep_amd import _lib, align  # noqa: E402

import align_ref  # noqa: E402
import follow_ref  # noqa: E402

LAM = 1.0 / 16


def test_restatement_equals_brute_force_enumeration():
    """all T, U <= 6, K in {1, 2, 3}, W >= U, dyadic features (every sum exact): row + the sum of the minima taken off it is the
    minimum over every step sequence in {0 .. K}^(T-1) from u = 0, a step other than 1 costing 1/16"""
    n = 0
    for T in range(1, 7):
        for U in range(1, 7):
            A, S = align_ref.dyadic_features(T, U, seed=10 * T + U)
            for K in (1, 2, 3):
                for dtype in (np.float64, np.float32):
                    r = follow_ref.follow(A, S, 64, K, 16, LAM, dtype=dtype)
                    got = r["rows"][-1].astype(np.float64) + r["msum"][-1]
                    want = follow_ref.brute_force(A, S, K, LAM)
                    assert np.array_equal(got, want), (T, U, K, dtype.__name__, got, want)
                    # the position is the running maximum of the rows' lowest minima
                    assert np.array_equal(r["pos"], np.maximum.accumulate(r["q"]))
                n += 1
    assert n == 108


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("shape", [(150, 200), (200, 131), (90, 260), (70, 50)])
def test_window_rule(shape, K):
    """w0 never decreases, the cell of q is inside the window the frame was computed on and the one it leaves behind, cells
    outside the window are +inf, and the window ends clamped at U - W"""
    T, U = shape
    W, back = 64, 16
    A, S = align_ref.unit_features(T, U, seed=T + K)
    r = follow_ref.follow(A, S, W, K, back, LAM)
    w0, q = r["w0"], r["q"]
    assert (np.diff(w0) >= 0).all() and w0[0] == 0 and w0.max() <= max(0, U - W)
    before = np.concatenate(([0], w0[:-1]))
    assert (q >= before).all() and (q < before + W).all() and (q >= w0).all() and (q < w0 + W).all()
    u = np.arange(U)[None, :]
    outside = (u < w0[:, None]) | (u >= w0[:, None] + W)
    assert np.isposinf(r["rows"][outside]).all()
    assert (r["rows"][np.arange(T), q] == 0).all() and np.isfinite(r["msum"]).all()
    assert (w0 == np.maximum.accumulate(np.clip(np.minimum(q - back, U - W), 0, None))).all()


def test_time_map_of_a_position_track():
    pos = np.array([0, 0, 1, 1, 1, 3, 3, 4], dtype=np.int32)
    tmap = align.follow_time_map(pos, 8)
    # frames 0 .. 4 were reached at 0, 2, 5 (2 was stepped over: the first frame at or past it), 5, 7; then nominal tempo
    assert tmap.dtype == np.float64 and tmap.tolist() == [0, 2, 5, 5, 7, 8, 9, 10]
    assert np.array_equal(tmap, follow_ref.time_map(pos, 8))
    assert align.follow_time_map([5], 3).tolist() == [0, 0, 0]
    assert align.follow_time_map([0], 3).tolist() == [0, 1, 2]
    rs = np.random.RandomState(3)
    for _ in range(20):
        pos = np.cumsum(rs.randint(0, 3, rs.randint(1, 40)))
        U = int(rs.randint(1, 2 * pos[-1] + 3))
        tmap = align.follow_time_map(pos, U)
        assert np.array_equal(tmap, follow_ref.time_map(pos, U)) and (np.diff(tmap) >= 0).all()
    # onsets and offsets go through warp_times: linear between the frames on either side
    fps = 10.0
    tmap = align.follow_time_map(np.array([0, 0, 1, 1, 1, 3, 3, 4]), 8)
    assert np.allclose(align.warp_times([0.0, 0.1, 0.15, 0.4, 0.6], tmap, fps), [0.0, 0.2, 0.35, 0.7, 0.9])
    with pytest.raises(ValueError):
        align.follow_time_map([3, 2], 4)
    with pytest.raises(ValueError):
        align.follow_time_map([], 4)


def test_onset_error_helper():
    """a track that reaches every score frame when the piece's tempo map says it is due: the onset is rounded up to a score
    frame (up to 1.4 audio frames at the slowest tempo) and the frame it is reached at up to an audio frame"""
    scores, _ = align_ref.piece()
    U = align_ref.score_frames(scores)
    T = int(np.ceil(float(align_ref.audio_time(align_ref.SCORE_SECONDS)) * align_ref.FPS)) + 8
    due = align_ref.audio_time(np.arange(U) / align_ref.FPS) * align_ref.FPS      # the audio frame score frame u is due at
    pos = np.searchsorted(due, np.arange(T), side='right') - 1
    pos = np.maximum.accumulate(np.clip(pos, 0, U - 1))
    err = follow_ref.onset_errors(pos, scores, U)
    assert err.shape == (sum(len(on) for on, _, _ in scores),) and err.max() < max(align_ref.RATES) + 1.0
    late = follow_ref.onset_errors(np.maximum(pos - 20, 0), scores, U)
    assert np.median(late) > 10


def test_python_classes_refuse_before_the_device():
    S = np.zeros((5, 12), np.float32)
    for kw in (dict(window=32), dict(window=96), dict(window=2048), dict(max_step=0), dict(max_step=5), dict(back=-1),
               dict(back=512), dict(penalty=-0.5), dict(penalty=float("inf")), dict(penalty=float("nan")), dict(max_frames=0)):
        with pytest.raises(ValueError):
            align.ScoreFollower(None, S, **kw)
    for bad in (np.zeros((5, 11)), np.zeros((0, 12)), np.zeros(12)):
        with pytest.raises(ValueError):
            align.ScoreFollower(None, bad)


def test_header_declares_and_library_exports_the_follower():
    names = ("dcs_follow_create", "dcs_follow_destroy", "dcs_follow_reset", "dcs_follow_bytes", "dcs_follow_frames",
             "dcs_follow_push", "dcs_follow_row", "dcs_stream_set_follow", "dcs_stream_follow_last")
    declared = set(_lib.header_symbols())
    lib = _lib.load()
    for name in names:
        assert name in declared and hasattr(lib, name), name
    src = open(os.path.join(ROOT, "deepconvsep_amd", "csrc", "build.sh")).read()
    assert re.search(r"\bfollow\.hip\b", src)


def test_scripts_take_the_new_options(monkeypatch, tmp_path):
    import importlib.util

    def load(*parts):
        spec = importlib.util.spec_from_file_location("cli_" + parts[-1][:-3], os.path.join(ROOT, "examples", *parts))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cli = load("bach10_scoreinformed", "align_scores.py")
    seen = []

    def fake(wav, score_dir, out_dir, files, **kw):
        seen.append(kw)
        return (np.arange(3), None) if kw.get("online") else (np.zeros((4, 2), np.int32), 1.5)
    monkeypatch.setattr(cli, "align_score_files", fake)
    cli.main(["-i", "a.wav", "-s", "scores", "-o", "out", "--online"])
    cli.main(["-i", "a.wav", "-s", "scores", "-o", "out"])
    assert seen[0].get("online") is True and "online" not in seen[1] and seen[1] == dict(band='auto', resample=False)
    stream = load("separate_stream.py")
    with pytest.raises(SystemExit):
        stream.main(["-a", "dsd", "-i", "a.wav", "-o", str(tmp_path), "-m", "m.pkl", "--follow"])
