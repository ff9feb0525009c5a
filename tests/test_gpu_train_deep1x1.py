"""The deep score-informed trainer (build_ca_1x1, csrc/train_deep1x1.hip) on the MI355X against the float64 restatement
tests/train_deep1x1_ref.py.

The gradient of this graph jumps wherever one of its ~4e5 pre-activations crosses zero, so the comparison has two parts
(INTEGRATION.md): (1) the device's loss and gradients against the float64 restatement evaluated at the device's own rectifier
codes (``ScoreTrainer.rectify_codes()``), with the project's tolerances -- loss and errors rtol 1e-5, per-array relative norm
<= 1e-4; (2) the device's codes against the restatement's own sign pattern: at most a 1e-4 share of a layer's units may differ,
and only where |pre64| <= 1e-5 max |pre64| of the layer (train_deep1x1_ref.check_codes)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import train_deep1x1_ref as R
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(params, r, B, tc, F, **kw):
    from deepconvsep_amd.score_training import ScoreTrainer
    return ScoreTrainer(params=params, branches=params[18].shape[0] // 200, batch_size=B, time_context=tc, feat_size=F, rand=r,
                        function='build_ca_1x1', **kw)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def _two_part(params, x, r, tgt, out, g, codes, label):
    """Both parts of the criterion; returns the float64 gradients at the device's codes."""
    want, g64, info = R.loss_and_grads(params, x, tgt, r, codes=codes)
    q = np.abs(info['q'])
    assert q.min() >= 1e-3 * q.max(), "the output rectify is not out of the comparison"
    with_own = R.loss_and_grads(params, x, tgt, r)[2]
    R.check_codes(codes, with_own['pres'], label)
    rels = [_rel(a, b) for a, b in zip(g, g64)]
    print(label, "out7", out, "want", want)
    print(label, "gradient errors", ["%.2e" % v for v in rels])
    assert not out[5:].any()
    np.testing.assert_allclose(out[:5], want, rtol=1e-5)
    for i in range(22):
        assert g[i].shape == g64[i].shape
        assert np.linalg.norm(g64[i][:200] if 18 <= i <= 20 else g64[i]) > 0, i
        assert rels[i] <= 1e-4, (i, rels[i])
    return g64


SHAPES = [(2, 19, 253), (2, 20, 257), (3, 28, 261), (1, 30, 513), (1, 30, 2049)]


@pytest.mark.parametrize("B,tc,F", SHAPES)
def test_gradients_and_loss_by_the_two_part_criterion(B, tc, F):
    params, x, r, tgt = R.setup(B, tc, F, seed=B + tc)
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    codes = t.rectify_codes()
    assert t.losses(x, tgt) == pytest.approx(list(out[1:5]), rel=1e-12)
    t.close()
    assert [c.shape[1] for c in codes] == [30, 50, 70, 100, 200, 200, 200]
    g64 = _two_part(params, x, r, tgt, out, g, codes, "deep1x1 %r" % ((B, tc, F),))
    # b_l and bb_l sit on opposite sides of a rectify: their gradients differ, and each matches (above)
    for k in range(7):
        assert not np.array_equal(g[3 * k + 1], g[3 * k + 2]), k
        assert _rel(g64[3 * k + 1], g64[3 * k + 2]) > 1e-3, k
    # the dead rows and final-bias entries
    for i in (18, 19, 20):
        assert not g[i][200:].any() and not g64[i][200:].any()
    assert not g[21][4:].any() and not g64[21][4:].any()


def test_one_update_matches_float64():
    """The bounds of test_gpu_train_si.py::test_one_update_matches_float64, float64 Adadelta on the float64 gradients at the
    device's codes."""
    B, tc, F = 2, 20, 257
    params, x, r, tgt = R.setup(B, tc, F, seed=4)
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    codes = t.rectify_codes()
    P, G = t.params(), t.gradients()
    A, D = t.adadelta_state()
    t.close()
    _, g64, _ = R.loss_and_grads(params, x, tgt, r, codes=codes)
    zeros = [np.zeros(p.shape) for p in params]
    P64, A64, D64 = train_ref.adadelta(params, g64, zeros, zeros)
    for i in range(22):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i
    for i in (18, 19, 20):
        assert np.array_equal(P[i][200:], params[i][200:]) and not np.array_equal(P[i][:200], params[i][:200])
        assert not G[i][200:].any() and not A[i][200:].any() and not D[i][200:].any()
    assert np.array_equal(P[21][4:], params[21][4:]) and (P[21][:4] != params[21][:4]).all()


def test_dead_arrays_stay_bit_identical_and_the_live_only_layout_trains_the_same_bits():
    B, tc, F = 2, 19, 253
    params, x, r, tgt = R.setup(B, tc, F, seed=8)
    res = []
    for p in (params, R.live(params)):
        t = _trainer(p, r, B, tc, F)
        outs = [t.step(x, tgt) for _ in range(5)]
        A, D = t.adadelta_state()
        res.append((outs, t.params(), t.gradients(), A, D))
        t.close()
    outs, P, G, A, D = res[0]
    for i in (18, 19, 20, 21):
        n = 4 if i == 21 else 200
        assert np.linalg.norm(params[i][n:]) > 0
        assert np.array_equal(P[i][n:], params[i][n:]), i
        assert not G[i][n:].any() and not A[i][n:].any() and not D[i][n:].any(), i
    for i in range(22):
        assert not np.array_equal(P[i], params[i]), i
    assert outs == res[1][0]
    for a, b in zip(R.live(P), res[1][1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("site", ["conv2", "conv1x1"])
def test_exact_ties_use_half(site):
    """A zeroed filter with a zero bias: its pre-activations are exactly 0, the device says 0.5, and its gradients are the
    float64 restatement's with 0.5 there -- not with 0, not with 1."""
    B, tc, F = 2, 19, 253
    params, x, r, tgt = R.setup(B, tc, F, seed=12)
    w, layer = (3, 1) if site == "conv2" else (18, 6)
    params[w][7] = 0
    params[w + 1][7] = 0
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    codes = t.rectify_codes()
    t.close()
    assert (codes[layer][:, 7] == 0.5).all()
    assert ((codes[layer] == 0.5).sum(axis=(0, 2, 3)) > 0).sum() == 1
    _two_part(params, x, r, tgt, out, g, codes, "tie " + site)
    for tie in (0.0, 1.0):
        wrong = [c.copy() for c in codes]
        wrong[layer][wrong[layer] == 0.5] = tie
        _, gw, _ = R.loss_and_grads(params, x, tgt, r, codes=wrong)
        assert max(_rel(g[i], gw[i]) for i in (w, w + 1)) > 1e-2, (site, tie)


def test_two_trainers_are_bit_identical():
    B, tc, F = 2, 20, 257
    params, x, r, tgt = R.setup(B, tc, F, seed=9)
    res = []
    for _ in range(2):
        t = _trainer(params, r, B, tc, F)
        for _ in range(3):
            t.step(x, tgt)
        res.append(t.params() + t.gradients())
        t.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_twenty_steps_follow_float64_and_learn():
    """The loss curve (not the weights) against float64 Adadelta on the restatement's own codes, the project's rtol 1e-3.
    The learning rate is 0.005: computed on the CPU with tests/train_deep1x1_ref.py, the float64 curve then falls
    monotonically (12.068 -> 11.963), the float32 restatement follows it within 2.7e-7 relative and a 1e-6 relative change of
    the start moves it by 5.6e-8 -- at 0.05, the shallow graphs' value, the same curve oscillates from step 12 on and the
    float32 restatement itself leaves it by 86 % (units change sign along the way), which would test nothing."""
    B, tc, F, lr = 2, 19, 253, 0.005
    params, x, r, _ = R.setup(B, tc, F, seed=5)
    m = x[:, 0:1] + x[:, 1:2] + x[:, 2:3] + x[:, 3:4]
    tgt = np.concatenate([0.4 * m, 0.3 * m, 0.2 * m, 0.1 * m], axis=1).astype(np.float32)
    t = _trainer(params, r, B, tc, F, learning_rate=lr)
    got = [t.step(x, tgt) for _ in range(20)]
    t.close()
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g, _ = R.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, A, D = train_ref.adadelta(P, g, A, D, lr=lr)
    print("got", got, "want", want)
    np.testing.assert_allclose(got, want, rtol=1e-3)
    assert all(b < a for a, b in zip(got, got[1:])), got


def test_forward_equals_the_separator_and_a_saved_model_separates(tmp_path):
    import deepconvsep_amd as dcs
    from deepconvsep_amd.arch import ARCHS, resolve
    from deepconvsep_amd.runtime import Network, default_context
    from deepconvsep_amd.score import melody_table
    from deepconvsep_amd.separation import SI_SCORE_FILES, SI_SCORE_PARAMS, blackmanharris
    from deepconvsep_amd.synth import synth_audio
    from test_gpu_train_si import _score_dir
    B, tc, F, frame = 2, 30, 513, 1024
    params, x, r, tgt = R.setup(B, tc, F, seed=11)
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    path = str(tmp_path / "model.pkl")
    t.save_model(path)
    ctx = default_context()
    got = ctx.to_host(t.forward(x))
    t.close()
    loaded = dcs.load_model(path)
    assert len(loaded) == 22 and resolve("bach10_si", loaded, tc, F) is ARCHS["bach10_si_1x1"]
    net = Network(ctx, "bach10_si", loaded, tc, F)
    ref = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
    assert got.shape == (B, 4, tc, F)
    assert np.array_equal(got, ref.reshape(got.shape))
    audio = synth_audio(2 * 44100, seed=1)
    _score_dir(tmp_path, len(audio) / 44100.0)
    nframes = int(np.ceil(len(audio) / 512.0)) + 2
    melody = melody_table(SI_SCORE_FILES, str(tmp_path), nframes, 44100, 512, frame, **SI_SCORE_PARAMS)
    sep = dcs.Separator("bach10_si", loaded, 0.2, tc, 25, 32, F, frame, 512, blackmanharris, tiler='library',
                        score_normalise='sum', score_mixture='sum')
    pcm = sep.separate_scoreinformed(audio, melody)
    assert pcm.shape[0] == 4 and np.isfinite(pcm).all() and np.abs(pcm).max() > 0


def test_all_zero_batch_and_kept_nan():
    B, tc, F = 2, 19, 253
    params, x, r, tgt = R.setup(B, tc, F, seed=13)
    for i in range(21):
        if params[i].ndim == 1:
            params[i][:] = 0          # with every inner bias zero an all-zero batch gives q = fb, the same in all four sources
    t = _trainer(params, r, B, tc, F)
    z = np.zeros_like(x)
    out, g = t.loss_and_gradients(z, np.zeros_like(tgt))
    assert out[0] == 0 and not out[1:].any()
    assert all(not a.any() for a in g)
    t.close()
    params[21][:] = 0
    t = _trainer(params, np.zeros_like(r), B, tc, F)
    out, _ = t.loss_and_gradients(z, tgt)
    t.close()
    want = R.loss_and_grads(params, z, tgt, np.zeros_like(r))[0]
    assert np.isnan(want[0]) and np.isnan(out[0])


def test_bad_arguments():
    from deepconvsep_amd import score_training
    from deepconvsep_amd.score_training import ScoreTrainer
    mk = lambda p, B, tc, F, **kw: ScoreTrainer(params=p, batch_size=B, time_context=tc, feat_size=F,  # noqa: E731
                                                rand=np.zeros((B, 1, tc, F)), function='build_ca_1x1', **kw)
    good = score_training.glorot_init(19, 253, function='build_ca_1x1')
    assert len(good) == 22
    for tc, F in ((18, 253), (19, 252), (19, 2050), (1025, 253)):
        with pytest.raises(ValueError):
            mk(good, 1, tc, F)
    for B in (0, 1025):
        with pytest.raises(ValueError):
            mk(good, B, 19, 253)
    with pytest.raises(ValueError):   # the array count
        mk(good[:-1], 1, 19, 253)
    with pytest.raises(ValueError):   # the 17-array graph's parameters
        mk(score_training.glorot_init(19, 253), 1, 19, 253)
    bad = list(good)
    bad[3] = np.zeros((50, 30, 1, 3), np.float32)
    with pytest.raises(ValueError):
        mk(bad, 1, 19, 253)
    t = mk(good, 1, 19, 253)
    io = np.zeros((1, 4, 19, 253), np.float32)
    with pytest.raises(ValueError):   # mode + 4 belongs to the two-stage graph
        t.run(io, io, 4)
    t.close()
    from test_gpu_train_si import _setup, _trainer as si_trainer
    p, x, r, tgt = _setup(2, 12, 93, seed=1)
    t = si_trainer(p, r, 2, 12, 93)
    with pytest.raises(NotImplementedError):
        t.rectify_codes()
    t.close()


def test_dsd_and_score_trainers_unchanged_next_to_a_deep_trainer():
    import test_gpu_train as TD
    import test_gpu_train_si as TS
    for T, shape, seed in ((TD, (7, 20, 65), 3), (TS, (3, 12, 131), 3)):
        res = []
        for with_deep in (False, True):
            other = None
            if with_deep:
                p, x2, r2, tgt2 = R.setup(2, 19, 253, seed=1)
                other = _trainer(p, r2, 2, 19, 253)
            params, x, r, tgt = T._setup(*shape, seed=seed)
            t = T._trainer(params, r, *shape)
            outs = []
            for _ in range(3):
                outs.append(t.step(x, tgt))
                if other is not None:
                    other.step(x2, tgt2)
            res.append((outs, t.params()))
            t.close()
            if other is not None:
                other.close()
        assert res[0][0] == res[1][0]
        for a, b in zip(res[0][1], res[1][1]):
            assert np.array_equal(a, b)


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_deep1x1 as T
from deepconvsep_amd.runtime import default_context
res = []
for branches in (4, 1):
    params, x, r, tgt = T.R.setup(3, 28, 261, seed=3, branches=branches)
    t = T._trainer(params, r, 3, 28, 261)
    for _ in range(2):
        t.step(x, tgt)
    out, g = t.loss_and_gradients(x, tgt)
    p = t.params()
    a, d = t.adadelta_state()
    c = t.rectify_codes()
    assert np.isfinite(out).all() and all(np.isfinite(v).all() for v in p + g + a + d + c)
    res += [out.astype(np.float32)] + [v.ravel() for v in p + g]
default_context().check_guards()
np.save(sys.argv[2], np.concatenate(res))
"""


def test_guard_harness_red_zones_and_poisons(tmp_path):
    outs = []
    for poison in ("255", "127"):
        env = dict(os.environ, DCS_WS_GUARD="4096", DCS_WS_POISON=poison)
        dst = str(tmp_path / ("out_%s.npy" % poison))
        rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst], env=env, timeout=300, capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-3000:]
        outs.append(np.load(dst))
    assert np.array_equal(outs[0], outs[1])


def test_command_line_trains_resumes_and_separates(tmp_path):
    from deepconvsep_amd.separation import load_model, write_wav
    from test_gpu_train_si import _score_dir, _tone
    db = tmp_path / "Bach10" / "Sources"
    out = tmp_path / "out"
    out.mkdir()
    n = 3 * 44100
    sources = ("bassoon", "clarinet", "saxphone", "violin")
    piece = "01-AchGott"
    (db / piece).mkdir(parents=True)
    for k, s in enumerate(sources):
        write_wav(str(db / piece / ("%s-%s.wav" % (piece, s))), _tone(n, 110.0 * (k + 1), k), 44100)
    for code in ("_g", "_b"):
        _score_dir(db / piece, n / 44100.0, code)
    ex = os.path.join(ROOT, "examples", "bach10_scoreinformed")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=300, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db), "--frame_size", "1024")
    assert rc.returncode == 0, rc.stderr[-3000:]
    common = ["--db", str(db), "--output", str(out), "--model", "m", "--batch_size", "2", "--frame_size", "1024",
              "--function", "build_ca_1x1"]
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch 2 of 2" in rc.stdout and "training loss for violin" in rc.stdout
    name = "model_m_x_gt.pkl"
    assert (out / "models" / name).is_file() and len(load_model(str(out / "models" / name))) == 22
    with open(str(out / "models" / "loss_m_x_gt.data"), "rb") as fh:
        assert len(pickle.load(fh)) == 2
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    for s in sources:
        assert (out / "output" / "m_x_gt" / ("%s-%s.wav" % (piece, s))).is_file()
