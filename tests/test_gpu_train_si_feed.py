"""The score-informed trainer's feed on the MI355X: ``ScoreFeatureWindows.gather`` and the raw ``dcs_trainer_gather_score``
(train::gather_score_kernel, csrc/train_core.hip) against the NumPy restatement tests/score_feed_ref.py, bit for bit; that
restatement equals the reference's loadFile + filterSpec + products on the same cases (tests/test_train_si_cpu.py)."""
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest

import score_feed_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(path, files, notes, code="e"):
    """Feature files and note tables as examples/bach10_scoreinformed/compute_features.py leaves them."""
    from deepconvsep_amd.transform import write_shape_file
    for k, (a, n) in enumerate(zip(files, notes)):
        for arr, name in ((a, "_m_"), (n, "_%s_" % code)):
            stem = os.path.join(str(path), "%02d-piece_%s" % (k, name))
            np.asarray(arr, dtype=np.float64).tofile(stem + ".data")
            write_shape_file(stem + ".shape", arr.shape)


def _feed(path, files, notes, tc, ov, mult, **kw):
    from deepconvsep_amd.score_training import ScoreFeatureWindows
    _write(path, files, notes)
    return ScoreFeatureWindows([str(path)], 'e', tc, ov, mult, kw.pop("windows", "reference"), kw.pop("batch_size", 4), **kw)


def _check(fw, files, notes, rows, what=""):
    x, t = fw.gather(rows)
    got_x, got_t = x.cpu().numpy(), t.cpu().numpy()
    want_x, want_t = S.gather_np(files, notes, fw.table[np.asarray(rows)], fw.tc, fw.F, fw.mult)
    assert got_x.dtype == np.float32 and got_x.shape == want_x.shape, what
    assert np.array_equal(got_x, want_x), (what, np.argwhere(got_x != want_x)[:4])
    assert np.array_equal(got_t, want_t), (what, np.argwhere(got_t != want_t)[:4])
    return got_x, got_t


def test_fixture_cases_equal_the_restatement_and_the_reference(golden, tmp_path):
    g = golden("train_si_feed")
    files, notes = S.fixture_files(), S.fixture_notes()
    for k, (T, _, mult) in enumerate(S.FILES):
        sub = tmp_path / str(k)
        sub.mkdir()
        fw = _feed(sub, [files[k]], [notes[k]], S.TC, S.OVERLAP, mult)
        assert fw.F == S.F and fw.ninst == 4 and fw.width == 9
        x, t = _check(fw, [files[k]], [notes[k]], np.arange(fw.total), "file %d" % k)
        assert np.array_equal(x, g["inputs_%d" % k]) and np.array_equal(t, g["targets_%d" % k]), k


def _random_notes(rs, T, F, P=6, width=9):
    n = np.zeros((4, P, width))
    for j in range(4):
        for p in range(P):
            if rs.uniform() < 0.25:
                continue
            t0 = rs.randint(0, T)
            n[j, p, 0], n[j, p, 1], n[j, p, 2] = t0, t0 + rs.randint(1, 12), rs.randint(40, 80)
            for k in range((width - 3) // 2):
                f0 = rs.randint(0, F)
                n[j, p, 3 + 2 * k], n[j, p, 4 + 2 * k] = f0, min(F, f0 + rs.randint(0, 4))
    return n


@pytest.mark.parametrize("windows", ["reference", "all"])
@pytest.mark.parametrize("F", [1, 6, 7, 13, 64])
def test_rows_across_files_in_one_batch(tmp_path, windows, F):
    """Files of different T in one table (shorter than tc, T == tc, T == tc + 1, zero slots, many windows), every row once in
    one batch in a shuffled order, then a second batch with repeats, then a batch of one row."""
    tc, ov = 8, 5
    rs = np.random.RandomState(F)
    Ts = (5, 8, 9, 40, 16, 23)
    files = [S.data_pattern(4, T, F, 3 * i) for i, T in enumerate(Ts)]
    notes = [_random_notes(rs, T, F, P=3 + i) for i, T in enumerate(Ts)]
    fw = _feed(tmp_path, files, notes, tc, ov, 0.3, windows=windows)
    assert fw.total > 8
    _check(fw, files, notes, rs.permutation(fw.total), "all rows")
    _check(fw, files, notes, rs.randint(0, fw.total, size=7), "repeats")
    for row in (0, fw.total - 1):
        _check(fw, files, notes, [row], "one row")


def test_real_size_batch_and_two_epochs(tmp_path):
    """F 2049, tc 30, forty harmonics' worth of table width (43), a batch of 32; then two epochs of batches() in the seeded
    order."""
    tc, ov, F = 30, 25, 2049
    rs = np.random.RandomState(5)
    files = [S.data_pattern(4, T, F, i) for i, T in enumerate((70, 45))]
    notes = [_random_notes(rs, T, F, P=20, width=43) for T in (70, 45)]
    fw = _feed(tmp_path, files, notes, tc, ov, 0.25, windows="all", batch_size=5, seed=3)
    assert fw.total == 9 + 4
    _check(fw, files, notes, np.arange(fw.total), "real size")
    _check(fw, files, notes, rs.randint(0, fw.total, size=32), "batch of 32")
    for epoch in (0, 1):
        perm = np.random.RandomState(3 + epoch).permutation(fw.total)
        got = list(fw.batches(epoch))
        assert len(got) == fw.iteration_size == 2
        for b, (x, t) in enumerate(got):
            wx, wt = S.gather_np(files, notes, fw.table[perm[5 * b:5 * b + 5]], tc, F, 0.25)
            assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(t.cpu().numpy(), wt), (epoch, b)
    assert not np.array_equal(np.random.RandomState(3).permutation(13), np.random.RandomState(4).permutation(13))


def _raw(ctx, data, files_tab, packed, note_tab, win, tc, F, ninst, width, scale, pad=64):
    """The raw entry point with sentinel words around both outputs."""
    import torch
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import _ptr
    B = len(win)
    n = B * ninst * tc * F
    with ctx.stream_scope():
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)  # noqa: E731
        d, ft, pk, nt, w = dev(data), dev(files_tab), dev(packed), dev(note_tab), dev(win)
        bufs = [torch.full((n + 2 * pad,), -77.0, dtype=torch.float32, device=ctx.device) for _ in range(2)]
        rc = ctx._lib.dcs_trainer_gather_score(ctx._h, _ptr(d), _ptr(ft), _ptr(pk), _ptr(nt), _ptr(w), B, tc, F, ninst, width,
                                               scale, c_void_p(bufs[0].data_ptr() + 4 * pad), c_void_p(bufs[1].data_ptr() + 4 * pad))
        _lib.check(rc)
        out = [b.cpu().numpy() for b in bufs]
    for o in out:
        assert (o[:pad] == -77.0).all() and (o[n + pad:] == -77.0).all()
    return [o[pad:n + pad].reshape(B, ninst, tc, F) for o in out]


def test_raw_entry_point_sentinels_and_argument_checks():
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import default_context
    from deepconvsep_amd.score_training import pack_notes
    ctx = default_context()
    files, notes = S.fixture_files(), S.fixture_notes()
    tc, F = S.TC, S.F
    data = np.concatenate([a.astype(np.float32).ravel() for a in files])
    offs = np.cumsum([0] + [a.size for a in files])
    files_tab = np.asarray([(offs[i], files[i].shape[1]) for i in range(3)], dtype=np.int64)
    packed = [pack_notes(ctx._lib, n, F) for n in notes]
    assert packed[0].shape == (4, 3, 8) and packed[0].dtype == np.int32
    noffs = np.cumsum([0] + [p.size for p in packed])
    note_tab = np.asarray([(noffs[i], packed[i].shape[1]) for i in range(3)], dtype=np.int64)
    flat = np.concatenate([p.ravel() for p in packed])
    win = np.asarray([(0, 5), (-1, 0), (1, 0), (0, 15), (2, 0), (0, 0), (0, 19)], dtype=np.int32)
    x, t = _raw(ctx, data, files_tab, flat, note_tab, win, tc, F, 4, 9, 0.5)
    wx, wt = S.gather_np(files, notes, win, tc, F, 0.5)
    assert np.array_equal(x, wx) and np.array_equal(t, wt)
    assert not x[1].any() and not x[6][:, 5:].any() and x[6][:, 4].all()       # a zero slot; frames past T
    # the table width, the instrument count and the bin ranges are checked
    for ninst, width in ((33, 9), (0, 9), (4, 8), (4, 3)):
        with pytest.raises(ValueError):
            _raw(ctx, data, files_tab, flat, note_tab, win, tc, F, ninst, width, 0.5)
    with pytest.raises(ValueError):
        pack_notes(ctx._lib, np.zeros((33, 1, 9)), F)
    with pytest.raises(ValueError):
        pack_notes(ctx._lib, np.zeros((4, 1, 8)), F)
    bad = notes[0].copy()
    bad[1, 0, 4] = F + 1                                                       # a band that ends past the last bin
    with pytest.raises(ValueError) as e:
        pack_notes(ctx._lib, bad, F)
    assert "outside" in str(e.value)
    out = np.zeros((4, 3, 8), dtype=np.int32)
    rc = ctx._lib.dcs_trainer_pack_score(np.ascontiguousarray(bad).ctypes.data_as(c_void_p), 4, 3, 9, F,
                                         out.ctypes.data_as(c_void_p))
    assert rc == _lib.DCS_ESHAPE
    bad = notes[0].copy()
    bad[1, 0, 3] = -1
    with pytest.raises(ValueError):
        pack_notes(ctx._lib, bad, F)


def test_feed_equals_the_one_window_entry_point(tmp_path):
    """What the launch replaces: per window one dcs_score_masks_norm(.., start, start + tc, DCS_SCORE_NORM_SUM, ..) on the
    scaled mixture rows, which tests/test_gpu_score.py pins to the reference's method body."""
    from deepconvsep_amd.runtime import default_context
    from deepconvsep_amd.score import score_masks
    ctx = default_context()
    tc, ov, F = 8, 5, 37
    rs = np.random.RandomState(2)
    files = [S.data_pattern(4, 40, F, 0)]
    notes = [_random_notes(rs, 40, F, P=8)]
    fw = _feed(tmp_path, files, notes, tc, ov, 0.5, windows="all")
    x, _ = fw.gather(np.arange(fw.total))
    x = x.cpu().numpy()
    for b, (_, start) in enumerate(fw.table):
        mag = ctx.to_device((np.float32(0.5) * files[0][0, start:start + tc].astype(np.float32)), np.float32)
        inp, _ = score_masks(ctx, mag, notes[0], int(start), int(start) + tc, normalise='sum')
        assert np.array_equal(ctx.to_host(inp), x[b]), b


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_si_feed as T
import score_feed_ref as S
from deepconvsep_amd.runtime import default_context
files, notes = S.fixture_files(), S.fixture_notes()
fw = T._feed(sys.argv[3], files, notes, S.TC, S.OVERLAP, 0.5)
x, t = T._check(fw, files, notes, np.arange(fw.total), "guarded")
default_context().check_guards()
np.save(sys.argv[2], np.concatenate([x.ravel(), t.ravel()]))
"""


def test_guard_harness_red_zones_and_poisons(tmp_path):
    outs = []
    for poison in ("255", "127"):
        env = dict(os.environ, DCS_WS_GUARD="4096", DCS_WS_POISON=poison)
        dst = str(tmp_path / ("out_%s.npy" % poison))
        sub = tmp_path / poison
        sub.mkdir()
        rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst, str(sub)], env=env, timeout=300,
                            capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-3000:]
        outs.append(np.load(dst))
    assert np.array_equal(outs[0], outs[1])
