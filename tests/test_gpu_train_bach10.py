"""Bach10 trainer on the MI355X (csrc/train_bach10.hip on csrc/train_ca.hip and csrc/train_core.hip) against the float64
autograd restatement tests/train_bach10_ref.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_edges
import train_bach10_ref
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = "bach10"


def _setup(B, tc, F, seed, bias=0.05):
    """The inputs of test_gpu_train_ikala.py::_setup on four channels.  Output biases 0.1 + |.| keep the sum of the four
    outputs away from zero (>= 0.26 on the shapes below), where the masks are well conditioned: plain float32 autograd is
    within 1.2e-6 relative of float64 on every gradient for all eight shapes of the gradient test."""
    from deepconvsep_amd import training
    rs = np.random.RandomState(seed)
    params = training.glorot_init(ARCH, tc, F, seed)
    for i in (1, 2, 4, 5, 7, 9, 11, 13, 15, 16):
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    params[16] = np.float32(0.1) + np.abs(params[16])
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 4, tc, F))).astype(np.float32)
    return params, x, r, tgt


def _trainer(params, r, B, tc, F, **kw):
    from deepconvsep_amd.training import Trainer
    return Trainer(arch=ARCH, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, **kw)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("B,tc,F", [(1, 30, 129), (5, 12, 131), (3, 9, 65), (2, 3, 30), (2, 30, 33), (64, 12, 93),
                                    (32, 30, 513), (2, 30, 2049)])
def test_gradients_and_loss_match_float64(B, tc, F):
    params, x, r, tgt = _setup(B, tc, F, seed=B + tc)
    want, g64 = train_bach10_ref.loss_and_grads(params, x, tgt, r)
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    print("out7", out, "want", want)
    rels = [_rel(a, b) for a, b in zip(g, g64)]
    print("gradient errors", ["%.2e" % v for v in rels])
    assert not out[5:].any()
    np.testing.assert_allclose(out[:5], want, rtol=1e-5)
    assert len(g) == 17
    for i, (a, b) in enumerate(zip(g, g64)):
        assert a.shape == b.shape
        assert np.linalg.norm(b) > 0, i
        assert rels[i] <= 1e-4, (i, rels[i])
    # elementwise, against the float32 restatement's own error at the same inputs (train_edges.check_gradients)
    _, g32 = train_bach10_ref.loss_and_grads(params, x, tgt, r, dtype=torch.float32)
    train_edges.check_gradients(g, g64, g32, B, "bach10 %r" % ((B, tc, F),))
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(g[1], g[2]) and np.array_equal(g[4], g[5])
    assert t.losses(x, tgt) == pytest.approx(list(want[1:]), rel=1e-5)
    t.close()


def test_one_update_matches_float64():
    """After one train_fn: params, accu and delta_accu against float64 Adadelta on the float64 gradients (the bounds of
    test_gpu_train_ikala.py::test_one_update_matches_float64)."""
    B, tc, F = 4, 12, 93
    params, x, r, tgt = _setup(B, tc, F, seed=4)
    _, g64 = train_bach10_ref.loss_and_grads(params, x, tgt, r)
    P64, A64, D64 = train_ref.adadelta(params, g64, [np.zeros(p.shape) for p in params],
                                       [np.zeros(p.shape) for p in params])
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    P = t.params()
    A, D = t.adadelta_state()
    for i in range(17):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i


def test_twenty_steps_follow_float64_and_learn():
    """As for DSD and iKala: a small learning rate (0.05) and output biases of 0.1 (all outputs positive everywhere) keep
    the trajectory well conditioned -- in float64 it goes 3.447 -> 0.989 and a 1e-6 relative change of the start moves it by
    9.4e-7 relative at most -- and the targets split the mixture 0.4 / 0.3 / 0.2 / 0.1, which the masks can reach."""
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    B, tc, F = 4, 9, 65
    params = training.glorot_init(ARCH, tc, F, seed=5)
    params[16] = params[16] + np.float32(0.1)
    r = np.random.RandomState(6).uniform(size=(B, 1, tc, F)).astype(np.float32)
    rs = np.random.RandomState(7)
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    tgt = np.concatenate([0.4 * x, 0.3 * x, 0.2 * x, 0.1 * x], axis=1).astype(np.float32)
    t = Trainer(arch=ARCH, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, learning_rate=0.05)
    got = [t.step(x, tgt) for _ in range(20)]
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g = train_bach10_ref.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, A, D = train_ref.adadelta(P, g, A, D, lr=0.05)
    print("got", got, "want", want)
    np.testing.assert_allclose(got, want, rtol=1e-3)
    assert got[-1] < 0.5 * got[0], got


def test_two_trainers_are_bit_identical():
    B, tc, F = 32, 30, 129
    params, x, r, tgt = _setup(B, tc, F, seed=9)
    res = []
    for _ in range(2):
        t = _trainer(params, r, B, tc, F)
        for _ in range(10):
            t.step(x, tgt)
        res.append(t.params())
        t.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_saved_model_loads_in_network_and_separates(tmp_path):
    """The reference's working size: frame size 4096, 2049 bins, 166 650 x 256 dense matrices, an 856 MB model."""
    import deepconvsep_amd as dcs
    from deepconvsep_amd.runtime import Network, default_context
    from deepconvsep_amd.separation import blackmanharris
    from deepconvsep_amd.synth import synth_audio
    B, tc, F = 2, 30, 2049
    params, x, r, tgt = _setup(B, tc, F, seed=11)
    t = _trainer(params, r, B, tc, F)
    for _ in range(3):
        t.step(x, tgt)
    path = str(tmp_path / "model.pkl")
    t.save_model(path)
    loaded = dcs.load_model(path)
    assert len(loaded) == 17 and loaded[6].shape == (166650, 256)
    ctx = default_context()
    net = Network(ctx, "bach10", loaded, tc, F)
    ref = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
    got = ctx.to_host(t.forward(x))
    t.close()
    assert got.shape == (B, 4, tc, F)
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    sep = dcs.Separator("bach10", loaded, 0.2, 30, 25, 32, 2049, 4096, 512, blackmanharris, ctx=ctx)
    pcm = sep.separate(synth_audio(44100, seed=1))
    assert pcm.shape == (4, 44100) and np.isfinite(pcm).all()


def test_dsd_and_ikala_trainers_unchanged_next_to_a_bach10_trainer():
    import test_gpu_train as TD
    import test_gpu_train_ikala as TI
    for T, shape, seed in ((TD, (7, 20, 65), 3), (TI, (3, 12, 131), 3)):
        res = []
        for with_bach10 in (False, True):
            other = None
            if with_bach10:
                p, x2, r2, tgt2 = _setup(2, 12, 93, seed=1)
                other = _trainer(p, r2, 2, 12, 93)
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


def test_bad_arguments():
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    good = training.glorot_init(ARCH, 12, 93)
    # tc 2 .. 47 (from 48 on the bach10 graph's inference kernels refuse, so there is nothing to train for), F 30 .. 2049
    for tc, F in ((1, 93), (48, 93), (65, 93), (12, 29), (12, 2050)):
        with pytest.raises(ValueError):
            Trainer(arch=ARCH, params=good, batch_size=1, time_context=tc, feat_size=F, rand=np.zeros((1, 1, tc, F)))
    with pytest.raises(ValueError):   # batch 1 .. 1024
        Trainer(arch=ARCH, params=good, batch_size=1025, time_context=12, feat_size=93, rand=np.zeros((1025, 1, 12, 93)))
    with pytest.raises(ValueError):   # parameter count
        Trainer(arch=ARCH, params=good[:16], batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    bad = list(good)
    bad[3] = np.zeros((30, 30, 7, 1), np.float32)
    with pytest.raises(ValueError):   # parameter shape: conv2 is 8 x 1 at tc 12
        Trainer(arch=ARCH, params=bad, batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    for arch in ("ikala", "bach10_si"):
        with pytest.raises(NotImplementedError):
            Trainer(arch=arch, batch_size=1, time_context=30, feat_size=513, rand=np.zeros((1, 1, 30, 513)))
    t = Trainer(arch=ARCH, params=good, batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    with pytest.raises(ValueError):   # two-channel (iKala) targets
        t.step(np.zeros((1, 1, 12, 93), np.float32), np.zeros((1, 2, 12, 93), np.float32))
    t.close()
    # the ends of the ranges train: kh = 1 at tc 2, w1 = 1 at F 30, tc 47
    for tc, F in ((2, 34), (3, 30), (47, 33)):
        params, x, r, tgt = _setup(1, tc, F, seed=2)
        t = _trainer(params, r, 1, tc, F)
        assert np.isfinite(t.step(x, tgt))
        t.close()


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_bach10 as T
from deepconvsep_amd.runtime import default_context
params, x, r, tgt = T._setup(3, 12, 131, seed=3)
t = T._trainer(params, r, 3, 12, 131)
for _ in range(3):
    t.step(x, tgt)
out, g = t.loss_and_gradients(x, tgt)
p = t.params()
assert np.isfinite(out).all() and all(np.isfinite(a).all() for a in p + g)
default_context().check_guards()
np.save(sys.argv[2], np.concatenate([out.astype(np.float32)] + [a.ravel() for a in p + g]))
"""


def test_guard_harness_red_zones_and_poisons(tmp_path):
    outs = []
    for poison in ("255", "127"):
        env = dict(os.environ, DCS_WS_GUARD="4096", DCS_WS_POISON=poison)
        dst = str(tmp_path / ("out_%s.npy" % poison))
        rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst], env=env, timeout=300,
                            capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-3000:]
        outs.append(np.load(dst))
    assert np.array_equal(outs[0], outs[1])


def _tone(n, f, seed):
    t = np.arange(n) / 44100.0
    return 0.2 * np.sin(2 * np.pi * f * t) * (1 + 0.1 * np.random.RandomState(seed).randn(n))


def test_command_lines_features_train_resume_separate(tmp_path):
    from deepconvsep_amd.separation import write_wav
    from deepconvsep_amd.transform import read_shape_file
    db = tmp_path / "Bach10" / "Sources"
    out = tmp_path / "out"
    out.mkdir()
    n = 2 * 44100
    pieces = ("01-AchGott", "02-AchLieben")
    sources = ("bassoon", "clarinet", "saxphone", "violin")
    for i, piece in enumerate(pieces):
        (db / piece).mkdir(parents=True)
        for k, s in enumerate(sources):
            write_wav(str(db / piece / ("%s-%s.wav" % (piece, s))), _tone(n, 110.0 * (k + 1) * (i + 1), 10 * i + k), 44100)
    (db / "notes").mkdir()                                          # no digit first: not a piece
    ex = os.path.join(ROOT, "examples", "bach10")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=300, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db), "--frame_size", "1024")
    assert rc.returncode == 0, rc.stderr[-3000:]
    feats = sorted(f for f in os.listdir(db / "transforms" / "t3") if f.endswith(".data"))
    assert len(feats) == 2 and feats[0].startswith("01-AchGott") and feats[1].startswith("02-AchLieben")
    for f in feats:
        shp = read_shape_file(str(db / "transforms" / "t3" / f.replace(".data", ".shape")))
        assert shp[0] == 5 and shp[2] == 513
    common = ["--db", str(db), "--output", str(out), "--model", "m", "--batch_size", "4", "--frame_size", "1024"]
    rc = run(os.path.join(ex, "train_bach10.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch 2 of 2" in rc.stdout and "training loss:" in rc.stdout and "training loss for violin" in rc.stdout
    assert "training loss for bassoon" in rc.stdout
    assert (out / "models" / "model_m.pkl").is_file()
    with open(str(out / "models" / "loss_m.data"), "rb") as fh:
        assert len(pickle.load(fh)) == 2
    assert not (out / "output").exists()
    rc = run(os.path.join(ex, "train_bach10.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    for piece in pieces:
        for s in sources:
            assert (out / "output" / "m" / ("%s-%s.wav" % (piece, s))).is_file()
    assert not (out / "output" / "m_original").exists()              # the Sibelius loop runs only with --dbs
    # --skip --load --dbs: no training, both separation loops; the renditions spell saxophone right
    dbs = tmp_path / "Bach10" / "Sibelius"
    midi = ("bassoon", "clarinet", "saxophone", "violin")
    for i, piece in enumerate(pieces):
        (dbs / piece).mkdir(parents=True)
        for style in ("fast", "slow", "original"):
            for k, s in enumerate(midi):
                write_wav(str(dbs / piece / ("%s_%s_%s.wav" % (piece, style, s))), _tone(44100, 220.0 * (k + 1), k), 44100)
    before = (out / "models" / "model_m.pkl").stat().st_mtime_ns
    rc = run(os.path.join(ex, "train_bach10.py"), *(common + ["--skip", "--load", "--dbs", str(dbs)]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch" not in rc.stdout and (out / "models" / "model_m.pkl").stat().st_mtime_ns == before
    for piece in pieces:
        for style in ("fast", "slow", "original"):
            for s in midi:
                assert (out / "output" / "m_original" / ("%s_%s_%s.wav" % (piece, style, s))).is_file()
