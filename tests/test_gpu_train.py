"""DSD trainer on the MI355X (csrc/train_dsd.hip on csrc/train_dsd_graph.hip and csrc/train_core.hip) against the float64
autograd restatement tests/train_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_edges
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(B, tc, F, seed, neg=False, bias=0.05):
    from deepconvsep_amd import training
    rs = np.random.RandomState(seed)
    params = training.glorot_init("dsd", tc, F, seed)
    for i in (1, 2, 4, 5, 7, 9, 11, 13, 14):
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    params[14] = np.abs(params[14])
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 4, tc, F))).astype(np.float32)
    if neg:   # targets 0..2 = the masked sources: the own-source terms vanish and E < 0
        p = train_ref.forward_np(params, x)
        s = p + 1e-8 * r.astype(np.float64)
        tgt[:, 0:3] = (s[:, 0:3] / s.sum(axis=1, keepdims=True) * x).astype(np.float32)
    return params, x, r, tgt


def _trainer(params, r, B, tc, F):
    from deepconvsep_amd.training import Trainer
    return Trainer(params=params, batch_size=B, time_context=tc, feat_size=F, rand=r)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("B,tc,F,neg", [(1, 30, 65, False), (7, 20, 65, False), (32, 30, 513, False),
                                        (256, 20, 65, False), (7, 30, 65, True)])
def test_gradients_and_loss_match_float64(B, tc, F, neg):
    params, x, r, tgt = _setup(B, tc, F, seed=B + tc, neg=neg)
    want, g64 = train_ref.loss_and_grads(params, x, tgt, r)
    E = want[1] + want[3] + want[2] - want[4] - want[5] - want[6]
    assert (E < 0) == neg
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    # neg: the own-source components vanish by construction (~1e-13 of the loss); they are held to 1e-5 of the loss
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-5 * want[0] if neg else 0)
    for i, (a, b) in enumerate(zip(g, g64)):
        assert a.shape == b.shape
        assert _rel(a, b) <= 1e-4, (i, _rel(a, b))
    # elementwise, against the float32 restatement's own error at the same inputs (train_edges.check_gradients)
    _, g32 = train_ref.loss_and_grads(params, x, tgt, r, dtype=torch.float32)
    train_edges.check_gradients(g, g64, g32, B, "dsd %r" % ((B, tc, F, neg),))
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(g[1], g[2]) and np.array_equal(g[4], g[5])


def test_one_update_matches_float64():
    """After one train_fn: params, accu and delta_accu against float64 Adadelta on the float64 gradients.  Bound: the
    update u = g sqrt(eps) / sqrt((1 - rho) g^2 + eps) has |du/dg| <= 1, so |u - u64| <= |g - g64| elementwise, and the
    gradients agree to 1e-4 in norm: ||p - p64|| <= 1e-4 ||g64|| + float32 rounding of p (6e-8 ||p||); accu = 0.05 g^2 and
    delta = 0.05 u^2 then agree to ~2e-4 relative in norm."""
    B, tc, F = 8, 30, 65
    params, x, r, tgt = _setup(B, tc, F, seed=4)
    _, g64 = train_ref.loss_and_grads(params, x, tgt, r)
    P64, A64, D64 = train_ref.adadelta(params, g64, [np.zeros(p.shape) for p in params],
                                       [np.zeros(p.shape) for p in params])
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    P = t.params()
    A, D = t.adadelta_state()
    for i in range(15):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i


def _learnable(B, tc, F, seed):
    rs = np.random.RandomState(seed)
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    tgt = np.concatenate([c * x for c in (0.5, 0.2, 0.2, 0.1)], axis=1).astype(np.float32)
    return x, tgt


def test_twenty_steps_follow_float64_and_learn():
    """With Lasagne's lr = 1 and zero output biases the trajectory is chaotic in any arithmetic: where all four outputs are
    rectified to 0 the masks divide by 4e-8 r, and a 1e-6 relative change of the float64 start moves the loss by 2 % after
    two steps.  So the tracking run uses lr = 0.1 and output biases of 0.1 (every output positive), where the same
    perturbation moves the 20-step float64 trajectory by 2e-4."""
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    B, tc, F = 4, 10, 33
    params = training.glorot_init("dsd", tc, F, seed=5)
    params[14] = params[14] + np.float32(0.1)
    r = np.random.RandomState(6).uniform(size=(B, 1, tc, F)).astype(np.float32)
    x, tgt = _learnable(B, tc, F, 7)
    t = Trainer(params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, learning_rate=0.1)
    got = [t.step(x, tgt) for _ in range(20)]
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g = train_ref.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, A, D = train_ref.adadelta(P, g, A, D, lr=0.1)
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
    ctx = default_context()
    net = Network(ctx, "dsd", loaded, tc, F)
    ref = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
    got = ctx.to_host(t.forward(x))
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    sep = dcs.Separator("dsd", loaded, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, ctx=ctx)
    pcm = sep.separate(synth_audio(44100, seed=1))
    assert pcm.shape[0] == 4 and np.isfinite(pcm).all()


def test_bad_arguments():
    from deepconvsep_amd.training import Trainer
    with pytest.raises(NotImplementedError):
        Trainer(arch="ikala", params=[np.zeros(1)] * 15, batch_size=1, time_context=4, feat_size=5,
                rand=np.zeros((1, 1, 4, 5)))
    for tc, F, B in ((5, 65, 1), (66, 65, 1), (30, 2050, 1), (30, 65, 1025)):
        with pytest.raises(ValueError):
            from deepconvsep_amd import training
            Trainer(params=training.glorot_init("dsd", tc, F), batch_size=B, time_context=tc, feat_size=F,
                    rand=np.zeros((B, 1, tc, F)))


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train as T
from deepconvsep_amd.runtime import default_context
params, x, r, tgt = T._setup(7, 20, 65, seed=3)
t = T._trainer(params, r, 7, 20, 65)
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
    db = tmp_path / "DSD100"
    n = 2 * 44100
    for split, songs in (("Dev", ("a", "b")), ("Test", ("c",))):
        for song in songs:
            srcs = [_tone(n, f, i) for i, f in enumerate((440.0, 55.0, 110.0, 880.0))]
            md, sd = db / "Mixtures" / split / song, db / "Sources" / split / song
            md.mkdir(parents=True)
            sd.mkdir(parents=True)
            write_wav(str(md / "mixture.wav"), np.stack([sum(srcs) / 4] * 2, axis=1), 44100)
            for name, a in zip(("vocals", "bass", "drums", "other"), srcs):
                write_wav(str(sd / (name + ".wav")), np.stack([a / 4] * 2, axis=1), 44100)
    ex = os.path.join(ROOT, "examples", "dsd100")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=600, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db))
    assert rc.returncode == 0, rc.stderr[-3000:]
    common = ["--db", str(db), "--model", "m", "--batch_size", "4"]
    rc = run(os.path.join(ex, "train_dsd.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch 2 of 2" in rc.stdout and "training loss" in rc.stdout
    assert (db / "models" / "model_m.pkl").is_file() and (db / "models" / "loss_m.data").is_file()
    rc = run(os.path.join(ex, "train_dsd.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    for split, song in (("Dev", "a"), ("Test", "c")):
        assert (db / "output" / "m" / split / song / "vocals.wav").is_file()
