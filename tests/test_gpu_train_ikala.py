"""iKala trainer on the MI355X (csrc/train_ikala.hip on csrc/train_ca.hip and csrc/train_core.hip) against the float64
autograd restatement tests/train_ikala_ref.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_edges
import train_ikala_ref
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = "ikala_nopool"


def _setup(B, tc, F, seed, neg=False, bias=0.05):
    from deepconvsep_amd import training
    rs = np.random.RandomState(seed)
    params = training.glorot_init(ARCH, tc, F, seed)
    for i in (1, 2, 4, 5, 7, 9, 11, 12):
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    # output biases 0.1 + |.|: with biases near 0.05 both outputs sit close to 0 in places, where the masks divide by a
    # small sum, and a 1e-7 relative change of the parameters moves the float64 dense gradients by 3.5e-5 (3e-7 here)
    params[12] = np.float32(0.1) + np.abs(params[12])
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 2, tc, F))).astype(np.float32)
    if neg:   # targets = the masked sources: vocals_error and acc_error vanish and E = -negative_error_voc < 0
        p = train_ikala_ref.forward_np(params, x)
        s = p + 1e-8 * r.astype(np.float64)
        tgt = (s / s.sum(axis=1, keepdims=True) * x).astype(np.float32)
    return params, x, r, tgt


def _trainer(params, r, B, tc, F, **kw):
    from deepconvsep_amd.training import Trainer
    return Trainer(arch=ARCH, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, **kw)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("B,tc,F,neg", [(1, 30, 93, False), (5, 12, 131, False), (32, 30, 513, False),
                                        (64, 12, 93, False), (3, 12, 131, True)])
def test_gradients_and_loss_match_float64(B, tc, F, neg):
    params, x, r, tgt = _setup(B, tc, F, seed=B + tc, neg=neg)
    want, g64 = train_ikala_ref.loss_and_grads(params, x, tgt, r)
    E = want[1] + want[2] - want[3]
    assert (E < 0) == neg
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    assert not out[5:].any()
    # neg: vocals_error and acc_error vanish by construction (float32 noise of the masks); held to 1e-5 of the loss
    np.testing.assert_allclose(out[:5], want, rtol=1e-5, atol=1e-5 * want[0] if neg else 0)
    assert len(g) == 13
    for i, (a, b) in enumerate(zip(g, g64)):
        assert a.shape == b.shape
        assert _rel(a, b) <= 1e-4, (i, _rel(a, b))
    # elementwise, against the float32 restatement's own error at the same inputs (train_edges.check_gradients)
    _, g32 = train_ikala_ref.loss_and_grads(params, x, tgt, r, dtype=torch.float32)
    train_edges.check_gradients(g, g64, g32, B, "ikala %r" % ((B, tc, F, neg),))
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(g[1], g[2]) and np.array_equal(g[4], g[5])
    assert t.losses(x, tgt) == pytest.approx(list(want[1:]), rel=1e-5, abs=1e-5 * want[0] if neg else 0)


def test_one_update_matches_float64():
    """After one train_fn: params, accu and delta_accu against float64 Adadelta on the float64 gradients (the bound of
    test_gpu_train.py::test_one_update_matches_float64)."""
    B, tc, F = 4, 12, 93
    params, x, r, tgt = _setup(B, tc, F, seed=4)
    _, g64 = train_ikala_ref.loss_and_grads(params, x, tgt, r)
    P64, A64, D64 = train_ref.adadelta(params, g64, [np.zeros(p.shape) for p in params],
                                       [np.zeros(p.shape) for p in params])
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    P = t.params()
    A, D = t.adadelta_state()
    for i in range(13):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i


def test_twenty_steps_follow_float64_and_learn():
    """As for DSD: a small learning rate (0.05) and output biases of 0.1 (both outputs positive everywhere) keep the
    trajectory well conditioned -- a 1e-6 relative change of the float64 start moves the 20-step loss by 4e-4 -- and the
    targets split the mixture 0.7 / 0.3, which the masks can reach (the loss falls from 7.8 to 0.31)."""
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    B, tc, F = 4, 10, 87
    params = training.glorot_init(ARCH, tc, F, seed=5)
    params[12] = params[12] + np.float32(0.1)
    r = np.random.RandomState(6).uniform(size=(B, 1, tc, F)).astype(np.float32)
    rs = np.random.RandomState(7)
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    tgt = np.concatenate([0.7 * x, 0.3 * x], axis=1).astype(np.float32)
    t = Trainer(arch=ARCH, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, learning_rate=0.05)
    got = [t.step(x, tgt) for _ in range(20)]
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g = train_ikala_ref.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, A, D = train_ref.adadelta(P, g, A, D, lr=0.05)
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
    import deepconvsep_amd as dcs
    from deepconvsep_amd.runtime import Network, default_context
    from deepconvsep_amd.synth import synth_audio
    B, tc, F = 8, 30, 513
    params, x, r, tgt = _setup(B, tc, F, seed=11)
    t = _trainer(params, r, B, tc, F)
    for _ in range(3):
        t.step(x, tgt)
    path = str(tmp_path / "model.pkl")
    t.save_model(path)
    loaded = dcs.load_model(path)
    assert len(loaded) == 13 and loaded[6].shape == (90090, 256)
    ctx = default_context()
    net = Network(ctx, "ikala", loaded, tc, F)
    assert net.arch.name == ARCH
    ref = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
    got = ctx.to_host(t.forward(x))
    assert got.shape == (B, 2, tc, F)
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    sep = dcs.Separator("ikala", loaded, 0.3, 30, 20, 32, 513, 1024, 512, np.hanning, ctx=ctx)
    assert sep.net.arch.name == ARCH
    pcm = sep.separate(synth_audio(44100, seed=1))
    assert pcm.shape == (2, 44100) and np.isfinite(pcm).all()


def test_dsd_trainer_unchanged_next_to_an_ikala_trainer():
    import test_gpu_train as T
    res = []
    for with_ikala in (False, True):
        other = None
        if with_ikala:
            p, _, r2, _ = _setup(2, 12, 93, seed=1)
            other = _trainer(p, r2, 2, 12, 93)
        params, x, r, tgt = T._setup(7, 20, 65, seed=3)
        t = T._trainer(params, r, 7, 20, 65)
        outs = []
        for _ in range(3):
            outs.append(t.step(x, tgt))
            if other is not None:
                other.step(*_setup(2, 12, 93, seed=1)[1::2])
        res.append((outs, t.params()))
        t.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)


def test_bad_arguments():
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    with pytest.raises(NotImplementedError):
        Trainer(arch="ikala", params=training.glorot_init(ARCH, 30, 513)[:1] * 13, batch_size=1, time_context=30,
                feat_size=513, rand=np.zeros((1, 1, 30, 513)))
    for tc, F in ((9, 93), (65, 93)):
        with pytest.raises(ValueError):
            Trainer(arch=ARCH, params=training.glorot_init(ARCH, 12, 93), batch_size=1, time_context=tc, feat_size=F,
                    rand=np.zeros((1, 1, tc, F)))
    with pytest.raises(ValueError):   # F < 87: conv2 leaves no column
        Trainer(arch=ARCH, params=training.glorot_init(ARCH, 12, 93), batch_size=1, time_context=12, feat_size=86,
                rand=np.zeros((1, 1, 12, 86)))
    good = training.glorot_init(ARCH, 12, 93)
    with pytest.raises(ValueError):   # parameter count
        Trainer(arch=ARCH, params=good[:12], batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    bad = list(good)
    bad[3] = np.zeros((30, 30, 10, 19), np.float32)
    with pytest.raises(ValueError):   # parameter shape
        Trainer(arch=ARCH, params=bad, batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    t = Trainer(arch=ARCH, params=good, batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 12, 93)))
    with pytest.raises(ValueError):   # four-channel (DSD) targets
        t.step(np.zeros((1, 1, 12, 93), np.float32), np.zeros((1, 4, 12, 93), np.float32))


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_ikala as T
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
    db = tmp_path / "iKala"
    (db / "Wavfile").mkdir(parents=True)
    n = 2 * 44100
    for i, name in enumerate(("10161_chorus", "10164_verse")):
        music, voice = _tone(n, 110.0 * (i + 1), i), _tone(n, 440.0 * (i + 1), 10 + i)
        write_wav(str(db / "Wavfile" / (name + ".wav")), np.stack([music, voice], axis=1), 44100)
    ex = os.path.join(ROOT, "examples", "ikala")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=300, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db))
    assert rc.returncode == 0, rc.stderr[-3000:]
    feats = sorted(f for f in os.listdir(db / "transforms" / "t1") if f.endswith(".data"))
    assert [f.split("_")[0] for f in feats] == ["10161", "10164"]     # compute_transform's <name>__m_.data
    for f in feats:
        assert read_shape_file(str(db / "transforms" / "t1" / f.replace(".data", ".shape")))[0] == 3
    common = ["--db", str(db), "--model", "m", "--batch_size", "4"]
    rc = run(os.path.join(ex, "train_ikala.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch 2 of 2" in rc.stdout and "training loss" in rc.stdout and "Beta component for acc" in rc.stdout
    assert (db / "models" / "model_m.pkl").is_file()
    with open(str(db / "models" / "loss_m.data"), "rb") as fh:
        assert len(pickle.load(fh)) == 2
    rc = run(os.path.join(ex, "train_ikala.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    for name in ("10161_chorus", "10164_verse"):
        for suffix in ("-voice.wav", "-music.wav"):
            assert (db / "output" / "m" / (name + suffix)).is_file()
