"""Score-informed Bach10 trainer on the MI355X (csrc/train_bach10si.hip on csrc/train_ca.hip and csrc/train_core.hip) against
the float64 autograd restatement tests/train_si_ref.py.  The tolerances are those of tests/test_gpu_train_bach10.py: the same
arithmetic with one decoder slot."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_edges
import train_ref
import train_si_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = train_si_ref.DEAD


def _setup(B, tc, F, seed, bias=0.05, branches=4):
    """The recipe of test_gpu_train_bach10.py::_setup with four non-negative input channels (their sum is that test's
    mixture range): Glorot weights, biases 0.05 N(0, 1), output biases 0.1 + |.| (the sum of the four live outputs stays away
    from zero, where the masks are well conditioned)."""
    from deepconvsep_amd import score_training
    rs = np.random.RandomState(seed)
    params = score_training.glorot_init(tc, F, seed, branches)
    last = len(params) - 1
    for i in [1, 2, 4, 5, 7] + list(range(9, last, 2)) + [last]:
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    params[last] = np.float32(0.1) + np.abs(params[last])
    x = (0.3 * rs.uniform(0, 0.25, size=(B, 4, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 4, tc, F))).astype(np.float32)
    return params, x, r, tgt


def _trainer(params, r, B, tc, F, **kw):
    from deepconvsep_amd.score_training import ScoreTrainer
    return ScoreTrainer(params=params, branches=4 if len(params) == 17 else 1, batch_size=B, time_context=tc, feat_size=F,
                        rand=r, **kw)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def _live(n):
    return [i for i in range(n) if i not in DEAD] if n == 17 else list(range(n))


SHAPES = [(1, 30, 129), (5, 12, 131), (3, 9, 65), (2, 3, 30), (2, 30, 33), (64, 12, 93), (32, 30, 513), (2, 30, 2049),
          (32, 30, 2049)]


@pytest.mark.parametrize("branches", [4, 1])
@pytest.mark.parametrize("B,tc,F", SHAPES)
def test_gradients_and_loss_match_float64(B, tc, F, branches):
    params, x, r, tgt = _setup(B, tc, F, seed=B + tc, branches=branches)
    want, g64 = train_si_ref.loss_and_grads(params, x, tgt, r)
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    print("out7", out, "want", want)
    rels = [_rel(a, b) for a, b in zip(g, g64)]
    print("gradient errors", ["%.2e" % v for v in rels])
    assert not out[5:].any()
    np.testing.assert_allclose(out[:5], want, rtol=1e-5)
    assert len(g) == len(params)
    for i in _live(len(g)):
        assert g[i].shape == g64[i].shape
        assert np.linalg.norm(g64[i]) > 0, i
        assert rels[i] <= 1e-4, (i, rels[i])
    if branches == 4:
        for i in DEAD:
            assert not g[i].any() and not g64[i].any(), i
        assert not g[16][4:].any() and not g64[16][4:].any()
    if F < 2049:
        # elementwise, against the float32 restatement's own error at the same inputs (train_edges.check_gradients)
        _, g32 = train_si_ref.loss_and_grads(params, x, tgt, r, dtype=torch.float32)
        train_edges.check_gradients(g, g64, g32, B, "bach10_si %r" % ((B, tc, F, branches),))
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(g[1], g[2]) and np.array_equal(g[4], g[5])
    assert t.losses(x, tgt) == pytest.approx(list(want[1:]), rel=1e-5)
    t.close()


@pytest.mark.parametrize("branches", [4, 1])
def test_one_update_matches_float64(branches):
    """After one train_fn: params, accu and delta_accu against float64 Adadelta on the float64 gradients (the bounds of
    test_gpu_train_bach10.py::test_one_update_matches_float64); the dead arrays come back as they were given."""
    B, tc, F = 4, 12, 93
    params, x, r, tgt = _setup(B, tc, F, seed=4, branches=branches)
    _, g64 = train_si_ref.loss_and_grads(params, x, tgt, r)
    P64, A64, D64 = train_ref.adadelta(params, g64, [np.zeros(p.shape) for p in params],
                                       [np.zeros(p.shape) for p in params])
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    P = t.params()
    G = t.gradients()
    A, D = t.adadelta_state()
    t.close()
    for i in range(len(params)):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i
    if branches == 4:
        for i in DEAD:
            assert np.linalg.norm(params[i]) > 0
            assert np.array_equal(P[i], params[i]), i
            assert not G[i].any() and not A[i].any() and not D[i].any(), i
        assert np.array_equal(P[16][4:], params[16][4:]) and (P[16][:4] != params[16][:4]).all()
        assert not G[16][4:].any() and not A[16][4:].any() and not D[16][4:].any()


def test_dead_arrays_stay_bit_identical_over_steps():
    B, tc, F = 3, 12, 131
    params, x, r, tgt = _setup(B, tc, F, seed=8)
    t = _trainer(params, r, B, tc, F)
    for _ in range(5):
        t.step(x, tgt)
    P, G = t.params(), t.gradients()
    A, D = t.adadelta_state()
    t.close()
    for i in DEAD:
        assert np.array_equal(P[i], params[i]) and not G[i].any() and not A[i].any() and not D[i].any(), i
    assert np.array_equal(P[16][4:], params[16][4:]) and not G[16][4:].any() and not A[16][4:].any() and not D[16][4:].any()
    for i in _live(17):
        assert not np.array_equal(P[i], params[i]), i


def _zero_site(params, site):
    p = [a.copy() for a in params]
    last = len(p) - 1
    if site == "branch":          # the pre-activation of the rectified branch layer is exactly 0
        p[8][:] = 0
        p[9][:] = 0
    elif site == "hidden":        # that of the 256-unit layer
        p[6][:] = 0
        p[7][:] = 0
    elif site == "output":        # that of the output layer: q = bo = 0 on the columns conv1^T leaves without a tap
        p[last][:] = 0
    return p


@pytest.mark.parametrize("branches", [4, 1])
@pytest.mark.parametrize("site", ["branch", "hidden", "output"])
def test_exact_ties_use_half(site, branches):
    """Pre-activations that are exactly zero: Theano's rectify'(0) = 0.5.  F 33 leaves three edge columns without a conv1^T
    tap, so with bo = 0 their q is exactly 0 (D > 0 there through eps r)."""
    B, tc, F = 2, 9, 33
    params, x, r, tgt = _setup(B, tc, F, seed=12, branches=branches)
    params = _zero_site(params, site)
    want, g64 = train_si_ref.loss_and_grads(params, x, tgt, r)
    _, g0 = train_si_ref.loss_and_grads(params, x, tgt, r, tie=0.0)
    assert any(np.linalg.norm(a - b) > 1e-6 * max(np.linalg.norm(a), 1e-30) for a, b in zip(g64, g0)), "the tie is not exercised"
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(x, tgt)
    t.close()
    np.testing.assert_allclose(out[:5], want, rtol=1e-5)
    for i in _live(len(g)):
        nb = np.linalg.norm(g64[i])
        if nb > 0:
            assert _rel(g[i], g64[i]) <= 1e-4, (site, i, _rel(g[i], g64[i]))
        else:
            assert not g[i].any(), (site, i)


def test_all_zero_batch_and_kept_nan():
    """An all-zero batch with positive output biases: loss 0, gradients 0, nothing moves.  With bo = 0 and r = 0 on the
    columns conv1^T leaves without a tap, D = 0 there: 0 / 0, and the NaN is kept, as in the reference."""
    B, tc, F = 2, 9, 33
    params, x, r, tgt = _setup(B, tc, F, seed=13)
    z4 = np.zeros_like(x)
    t = _trainer(params, r, B, tc, F)
    out, g = t.loss_and_gradients(z4, np.zeros_like(tgt))
    assert out[0] == 0 and not out[1:].any()
    assert all(not a.any() for a in g)
    assert t.step(z4, np.zeros_like(tgt)) == 0
    P = t.params()
    t.close()
    for a, b in zip(P, params):
        assert np.array_equal(a, b)
    p0 = [a.copy() for a in params]
    p0[16][:] = 0
    t = _trainer(p0, np.zeros_like(r), B, tc, F)
    out, _ = t.loss_and_gradients(x, tgt)
    t.close()
    want, _ = train_si_ref.loss_and_grads(p0, x, tgt, np.zeros_like(r))
    assert np.isnan(want[0]) and np.isnan(out[0])


def test_twenty_steps_follow_float64_and_learn():
    """As for Bach10: a small learning rate (0.05) and output biases of 0.1 (all outputs positive everywhere) keep the
    trajectory well conditioned -- in float64 it goes 3.403 -> 0.933 and a 1e-6 relative change of the start moves it by
    7.5e-7 relative at most (computed on the CPU with tests/train_si_ref.py) -- and the targets split the mixture 0.4 / 0.3 /
    0.2 / 0.1, which the masks can reach."""
    from deepconvsep_amd import score_training
    B, tc, F = 4, 9, 65
    params = score_training.glorot_init(tc, F, seed=5, branches=4)
    params[16] = params[16] + np.float32(0.1)
    r = np.random.RandomState(6).uniform(size=(B, 1, tc, F)).astype(np.float32)
    rs = np.random.RandomState(7)
    mix = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    w = rs.uniform(0.1, 1, size=(B, 4, tc, F))
    w /= w.sum(axis=1, keepdims=True)
    x = (w * mix).astype(np.float32)
    m = x[:, 0:1] + x[:, 1:2] + x[:, 2:3] + x[:, 3:4]
    tgt = np.concatenate([0.4 * m, 0.3 * m, 0.2 * m, 0.1 * m], axis=1).astype(np.float32)
    t = _trainer(params, r, B, tc, F, learning_rate=0.05)
    got = [t.step(x, tgt) for _ in range(20)]
    t.close()
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g = train_si_ref.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, A, D = train_ref.adadelta(P, g, A, D, lr=0.05)
    print("got", got, "want", want)
    np.testing.assert_allclose(got, want, rtol=1e-3)
    assert got[-1] < 0.5 * got[0], got


@pytest.mark.parametrize("branches", [4, 1])
def test_two_trainers_are_bit_identical(branches):
    B, tc, F = 32, 30, 129
    params, x, r, tgt = _setup(B, tc, F, seed=9, branches=branches)
    res = []
    for _ in range(2):
        t = _trainer(params, r, B, tc, F)
        for _ in range(10):
            t.step(x, tgt)
        res.append(t.params() + t.gradients())
        t.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_the_two_layouts_train_the_same_weights():
    """The 17-array trainer's live arrays and the 11-array trainer's are the same computation: bit-identical."""
    B, tc, F = 5, 12, 131
    params, x, r, tgt = _setup(B, tc, F, seed=10)
    res = []
    for p in (params, train_si_ref.live(params)):
        t = _trainer(p, r, B, tc, F)
        outs = [t.step(x, tgt) for _ in range(4)]
        res.append((outs, t.params()))
        t.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(train_si_ref.live(res[0][1]), res[1][1]):
        assert np.array_equal(a, b)


def test_dsd_and_bach10_trainers_unchanged_next_to_a_score_trainer():
    import test_gpu_train as TD
    import test_gpu_train_bach10 as TB
    for T, shape, seed in ((TD, (7, 20, 65), 3), (TB, (3, 12, 131), 3)):
        res = []
        for with_si in (False, True):
            other = None
            if with_si:
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


def _score_dir(path, seconds, code="_b"):
    """Four score files (bach10_scoreinformed/separate_bach10.py:455), seeded and monophonic."""
    from deepconvsep_amd.synth import synth_score_text
    for k, ins in enumerate(("bassoon", "clarinet", "saxophone", "violin")):
        with open(os.path.join(str(path), ins + code + ".txt"), "w") as fh:
            fh.write(synth_score_text(60 + k, seconds + 0.5, 40 + 5 * k, 58 + 4 * k))


def test_saved_17_array_model_loads_in_separator_and_separates(tmp_path):
    """A model the trainer wrote goes through Separator('bach10_si', ..., 'sum', 'sum') and separates as the oracle pipeline
    with the same semantics does."""
    import deepconvsep_amd as dcs
    from deepconvsep_amd.runtime import default_context
    from deepconvsep_amd.score import melody_table
    from deepconvsep_amd.separation import SI_SCORE_FILES, SI_SCORE_PARAMS, blackmanharris
    from deepconvsep_amd.synth import synth_audio
    from oracle import pipeline
    B, tc, F, frame = 2, 30, 513, 1024
    params, x, r, tgt = _setup(B, tc, F, seed=11)
    t = _trainer(params, r, B, tc, F)
    for _ in range(3):
        t.step(x, tgt)
    path = str(tmp_path / "model.pkl")
    t.save_model(path)
    got = default_context().to_host(t.forward(x))
    want = train_si_ref.forward_np(t.params(), x)[:, 0:4]
    t.close()
    assert got.shape == (B, 4, tc, F)
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    loaded = dcs.load_model(path)
    assert len(loaded) == 17 and loaded[0].shape == (30, 4, 1, 30)
    for i in DEAD:
        assert np.array_equal(loaded[i], params[i])
    audio = synth_audio(44100, seed=1)
    _score_dir(tmp_path, len(audio) / 44100.0)
    nframes = int(np.ceil(len(audio) / 512.0)) + 2
    melody = melody_table(SI_SCORE_FILES, str(tmp_path), nframes, 44100, 512, frame, **SI_SCORE_PARAMS)
    sep = dcs.Separator("bach10_si", loaded, 0.2, tc, 25, 32, F, frame, 512, blackmanharris, tiler='library',
                        score_normalise='sum', score_mixture='sum')
    pcm = sep.separate_scoreinformed(audio, melody)
    ref = pipeline.separate_scoreinformed(loaded, audio, melody, 0.2, tc, 25, 32, frame, 512, blackmanharris,
                                          normalise='sum', mixture='sum')
    ref = np.asarray(ref)
    assert pcm.shape == ref.shape and np.isfinite(pcm).all()
    assert np.abs(pcm - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_saved_11_array_model_resolves_to_the_single_branch_graph(tmp_path):
    import deepconvsep_amd as dcs
    from deepconvsep_amd.arch import ARCHS, resolve
    from deepconvsep_amd.runtime import Network, default_context
    B, tc, F = 2, 12, 93
    params, x, r, tgt = _setup(B, tc, F, seed=14, branches=1)
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt)
    path = str(tmp_path / "model11.pkl")
    t.save_model(path)
    ctx = default_context()
    got = ctx.to_host(t.forward(x))
    t.close()
    loaded = dcs.load_model(path)
    assert len(loaded) == 11 and resolve("bach10_si", loaded, tc, F) is ARCHS["bach10_si1"]
    net = Network(ctx, "bach10_si", loaded, tc, F)
    ref = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
    assert ref.shape == got.shape == (B, 4, tc, F)
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())


def test_bad_arguments():
    from deepconvsep_amd import score_training
    from deepconvsep_amd.score_training import ScoreTrainer
    from deepconvsep_amd.training import Trainer
    for branches in (4, 1):
        good = score_training.glorot_init(12, 93, branches=branches)
        mk = lambda p, B, tc, F: ScoreTrainer(params=p, branches=branches, batch_size=B, time_context=tc,  # noqa: E731
                                              feat_size=F, rand=np.zeros((B, 1, tc, F)))
        # tc 2 .. 47 (the largest time context the inference path of this graph runs), F 30 .. 2049
        for tc, F in ((1, 93), (48, 93), (65, 93), (12, 29), (12, 2050)):
            with pytest.raises(ValueError):
                mk(good, 1, tc, F)
        for B in (0, 1025):   # batch 1 .. 1024
            with pytest.raises(ValueError):
                mk(good, B, 12, 93)
        with pytest.raises(ValueError):   # parameter count
            mk(good[:-1], 1, 12, 93)
        bad = list(good)
        bad[3] = np.zeros((30, 30, 7, 1), np.float32)
        with pytest.raises(ValueError):   # parameter shape: conv2 is 8 x 1 at tc 12
            mk(bad, 1, 12, 93)
        bad = list(good)
        bad[0] = np.zeros((30, 1, 1, 30), np.float32)
        with pytest.raises(ValueError):   # the Bach10 graph's one-channel conv1
            mk(bad, 1, 12, 93)
        t = mk(good, 1, 12, 93)
        with pytest.raises(ValueError):   # three-channel inputs
            t.step(np.zeros((1, 3, 12, 93), np.float32), np.zeros((1, 4, 12, 93), np.float32))
        with pytest.raises(ValueError):   # mode + 4 belongs to the two-stage graph
            t.run(np.zeros((1, 4, 12, 93), np.float32), np.zeros((1, 4, 12, 93), np.float32), 4)
        with pytest.raises(ValueError):
            t.set_rand(np.zeros((1, 4, 12, 93), np.float32))
        t.close()
    # the layouts do not cross: 11 arrays into the 17-array graph and back
    with pytest.raises(ValueError):
        ScoreTrainer(params=score_training.glorot_init(12, 93, branches=1), branches=4, batch_size=1, time_context=12,
                     feat_size=93)
    with pytest.raises(ValueError):
        ScoreTrainer(branches=2)
    # the mono trainer still refuses this graph
    with pytest.raises(NotImplementedError):
        Trainer(arch="bach10_si", batch_size=1, time_context=30, feat_size=513, rand=np.zeros((1, 1, 30, 513)))
    # the ends of the ranges train: kh = 1 at tc 2, w1 = 1 at F 30, tc 47, F 2049, batch 1024
    for B, tc, F in ((1, 2, 34), (1, 3, 30), (1, 47, 33), (1, 2, 2049), (1024, 2, 30)):
        params, x, r, tgt = _setup(B, tc, F, seed=2, branches=1)
        t = _trainer(params, r, B, tc, F)
        assert np.isfinite(t.step(x, tgt))
        t.close()


def test_the_largest_time_context_loads_in_the_inference_path():
    """A model nothing can load is no use: tc 47 runs in dcs_model_create's score-informed graph, 48 does not."""
    from deepconvsep_amd import score_training
    from deepconvsep_amd.runtime import Network, default_context
    ctx = default_context()
    F = 33
    for tc, ok in ((47, True), (48, False)):
        params = score_training.glorot_init(tc, F, seed=1, branches=1)
        x = np.random.RandomState(0).uniform(0, 1, size=(1, 4, tc, F)).astype(np.float32)
        try:
            net = Network(ctx, "bach10_si", params, tc, F)
            p = ctx.to_host(net.forward_raw(ctx.to_device(x, np.float32)))
            ran = bool(np.isfinite(p).all())
        except (NotImplementedError, ValueError):
            ran = False
        assert ran == ok, tc


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_si as T
from deepconvsep_amd.runtime import default_context
res = []
for branches in (4, 1):
    params, x, r, tgt = T._setup(3, 12, 131, seed=3, branches=branches)
    t = T._trainer(params, r, 3, 12, 131)
    for _ in range(3):
        t.step(x, tgt)
    out, g = t.loss_and_gradients(x, tgt)
    p = t.params()
    a, d = t.adadelta_state()
    assert np.isfinite(out).all() and all(np.isfinite(v).all() for v in p + g + a + d)
    res += [out.astype(np.float32)] + [v.ravel() for v in p + g]
default_context().check_guards()
np.save(sys.argv[2], np.concatenate(res))
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
    from deepconvsep_amd.separation import load_model, write_wav
    from deepconvsep_amd.transform import read_shape_file
    db = tmp_path / "Bach10" / "Sources"
    out = tmp_path / "out"
    out.mkdir()
    n = 3 * 44100
    pieces = ("01-AchGott", "02-AchLieben")
    sources = ("bassoon", "clarinet", "saxphone", "violin")
    midi = ("bassoon", "clarinet", "saxophone", "violin")
    for i, piece in enumerate(pieces):
        (db / piece).mkdir(parents=True)
        for k, s in enumerate(sources):
            write_wav(str(db / piece / ("%s-%s.wav" % (piece, s))), _tone(n, 110.0 * (k + 1) * (i + 1), 10 * i + k), 44100)
        for code in ("_g", "_b"):
            _score_dir(db / piece, n / 44100.0, code)
    (db / "notes").mkdir()                                          # no digit first: not a piece
    ex = os.path.join(ROOT, "examples", "bach10_scoreinformed")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=300, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db), "--frame_size", "1024")
    assert rc.returncode == 0, rc.stderr[-3000:]
    t3 = db / "transforms" / "t3"
    feats = sorted(f for f in os.listdir(t3) if f.endswith("_m_.data"))
    assert len(feats) == 2 and feats[0].startswith("01-AchGott") and feats[1].startswith("02-AchLieben")
    for f in feats:
        shp = read_shape_file(str(t3 / f.replace(".data", ".shape")))
        assert shp[0] == 5 and shp[2] == 513
        for code in "gbe":
            nshp = read_shape_file(str(t3 / f.replace("_m_.data", "_%s_.shape" % code)))
            assert nshp[0] == 4 and nshp[2] == 43
    common = ["--db", str(db), "--output", str(out), "--model", "m", "--batch_size", "4", "--frame_size", "1024"]
    name = "model_m_gt.pkl"
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch 2 of 2" in rc.stdout and "training loss:" in rc.stdout and "training loss for violin" in rc.stdout
    assert "training loss for bassoon" in rc.stdout
    assert (out / "models" / name).is_file()
    assert len(load_model(str(out / "models" / name))) == 17
    with open(str(out / "models" / "loss_m_gt.data"), "rb") as fh:
        assert len(pickle.load(fh)) == 2
    assert not (out / "output").exists()
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    for piece in pieces:
        for s in sources:
            assert (out / "output" / "m_gt" / ("%s-%s.wav" % (piece, s))).is_file()
    # --skip --load: no training, the separation alone; the 11-array layout under its own name
    before = (out / "models" / name).stat().st_mtime_ns
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common + ["--skip", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch" not in rc.stdout and (out / "models" / name).stat().st_mtime_ns == before
    rc = run(os.path.join(ex, "train_bach10_si.py"), *(common[:4] + ["--model", "m1"] + common[6:] +
                                                      ["--nepochs", "1", "--branches", "1", "--skip_sep", "--pitch_code", "b",
                                                       "--windows", "all"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert len(load_model(str(out / "models" / "model_m1_gt.pkl"))) == 11
    # the separate script loads what the trainer wrote
    piece = pieces[0]
    from deepconvsep_amd.separation import read_wav
    audio = sum(read_wav(str(db / piece / ("%s-%s.wav" % (piece, s))))[1] for s in sources)
    work = tmp_path / "sep"
    work.mkdir()
    write_wav(str(work / "mix.wav"), audio, 44100)
    for s in midi:
        with open(str(db / piece / (s + "_b.txt"))) as src, open(str(work / (s + "_b.txt")), "w") as dst:
            dst.write(src.read())
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import separate_bach10 as S; "
            "S.train_auto(%r, %r, %r, 0.2, 30, 25, 4, 513, 1024, 512, trainer_semantics=True)"
            % (ROOT, ex, str(work / "mix.wav"), str(work), str(out / "models" / name)))
    rc = run("-c", code)
    assert rc.returncode == 0, rc.stderr[-3000:]
    for s in sources:
        assert (work / ("mix_%s.wav" % s)).is_file()
