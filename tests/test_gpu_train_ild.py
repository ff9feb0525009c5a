"""Stereo (ILD) DSD100 trainer on the MI355X (csrc/train_dsdild.hip on csrc/train_dsd_graph.hip and csrc/train_core.hip, StereoTrainer and
StereoFeatureWindows) against the float64 autograd restatement tests/train_ild_ref.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import feed_ref
import train_edges
import train_ild_ref
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIASES = (1, 2, 4, 5, 7, 9, 11, 13, 15, 16)
# (stage, keywords of train_ild_ref.components / StereoTrainer): stage 1, stage 2 at the reference's 1 / 500, and stage 2 with
# the ILD term dominant (at 1 / 500 it is under 0.5 % of the loss, and its gradient would go untested)
MODES = {"mse": (1, {}), "ild": (2, {}), "ild100": (2, {"ild_weight": 100.0})}


def _setup(B, tc, F, seed, bias=0.05):
    """The inputs of test_gpu_train_bach10.py::_setup on two input and eight output channels: Glorot weights, biases 0.05
    N(0, 1), output biases 0.1 + |.| (the sums of a channel's four outputs stay away from zero, where the masks are well
    conditioned), x = 0.3 U(0, 1), the two draws 0.1 N(0, 1), targets 0.3 U(0, 0.5)."""
    from deepconvsep_amd import stereo_training as st
    rs = np.random.RandomState(seed)
    params = st.glorot_init(tc, F, seed)
    for i in BIASES:
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    params[16] = np.float32(0.1) + np.abs(params[16])
    x = (0.3 * rs.uniform(0, 1, size=(B, 2, tc, F))).astype(np.float32)
    r = (0.1 * rs.randn(2, B, 4, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 8, tc, F))).astype(np.float32)
    return params, x, r, tgt


def _trainer(params, r, B, tc, F, **kw):
    from deepconvsep_amd.stereo_training import StereoTrainer
    return StereoTrainer(params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, **kw)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def _check_outputs(out, want, label=""):
    """The 16 outputs against the restatement's ten.  The eight errors are sums of squares of (source - target) over the
    device's float32 outputs, held to rtol 1e-5 like the components of the other trainers.  The ILD term is w sum_f d_f^2
    with d_f a difference of two means of levels 20 log10 (s_0 / s_1): a relative error delta of the float32 network
    outputs (1e-6) moves a level by 8.7 x 2 delta = 2e-5 dB and d_f, of the order of 1 dB, by 2e-5 relative, its square by
    4e-5: rtol 1e-4.  The loss is their sum."""
    print(label, "out", out[:10], "float64", want)
    assert out.shape == (16,) and not out[10:].any()
    np.testing.assert_allclose(out[1:9], want[1:9], rtol=1e-5)
    np.testing.assert_allclose(out[9], want[9], rtol=1e-4)
    assert abs(out[0] - want[0]) <= 1e-5 * (want[0] - want[9]) + 1e-4 * want[9]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("B,tc,F", [(2, 30, 33), (5, 12, 131), (1, 4, 1), (64, 12, 93), (32, 30, 513), (2, 30, 2049)])
def test_gradients_and_outputs_match_float64(B, tc, F, mode):
    stage, kw = MODES[mode]
    params, x, r, tgt = _setup(B, tc, F, seed=B + tc)
    want, g64 = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=stage, **kw)
    t = _trainer(params, r, B, tc, F, **kw)
    out, g = t.loss_and_gradients(x, tgt, ild=stage == 2)
    _check_outputs(out, want, "%s %r" % (mode, (B, tc, F)))
    if stage == 2:
        assert want[9] > 0
        print("ILD share of the loss: %.3g" % (want[9] / want[0]))
    else:
        assert out[9] == 0.0
    assert len(g) == 17
    for i, b in enumerate(g64):
        assert np.linalg.norm(b) > 0, i
    # relative norm <= 1e-4 and elementwise <= 8 e32, e32 the float32 restatement's own error at the same inputs (printed)
    _, g32 = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=stage, dtype=torch.float32, **kw)
    train_edges.check_gradients(g, g64, g32, B, "dsd_ild %s %r" % (mode, (B, tc, F)))
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(g[1], g[2]) and np.array_equal(g[4], g[5])
    losses = t.losses(x, tgt)
    assert losses.shape == (2, 4)
    np.testing.assert_allclose(losses.ravel(), want[1:9], rtol=1e-5)
    t.close()


def _zero_case(B=3, tc=10, F=33, seed=3):
    """tie_case 'q0' for this graph: the branch layers and the output bias zeroed, so every output pre-activation is exactly
    0 (all four outputs of both channels zero in every row: masks 0 / (eps r1), sources eps r1, r'(0) = 0.5 in dE/dq), and
    silent target bins.  eps = 1e-6 and draws of at least 0.01 in size keep dE/dq (of the order x t / (eps r)) finite in
    float32, as train_edges.tie_case does for Bach10; r1 and r2 share their sign per element, so that neither
    source_1 + eps r2 nor the level ratio is zero."""
    params, x, r, tgt = _setup(B, tc, F, seed)
    for i in range(8, 17):
        params[i] = np.zeros_like(params[i])
    sign = np.where(r[0] < 0, -1.0, 1.0)
    r = (sign[None] * (0.01 + np.abs(r))).astype(np.float32)
    tgt[:, 0:2, :, 5] = 0.0          # vocals silent in both mics in one bin
    tgt[1, 4:6] = 0.0                # drums silent in a whole window
    tgt[0, 2, 3, :] = 0.0            # bass silent in mic 0 only, one frame
    return params, x, r, tgt, dict(eps=1e-6)


def test_exact_zero_outputs_and_silent_targets():
    params, x, r, tgt, hyper = _zero_case()
    assert not train_ild_ref.forward_np(params, x).any()
    want, g64 = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=2, **hyper)
    assert np.isfinite(want).all() and all(np.isfinite(a).all() for a in g64)
    t = _trainer(params, r, *x.shape[:1], x.shape[2], x.shape[3], **hyper)
    assert not t.ctx.to_host(t.forward(x)).any()
    out, g = t.loss_and_gradients(x, tgt, ild=True)
    _check_outputs(out, want, "zero outputs")
    assert np.isfinite(out).all() and all(np.isfinite(a).all() for a in g)
    _, g32 = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=2, dtype=torch.float32, **hyper)
    train_edges.check_gradients(g, g64, g32, x.shape[0], "dsd_ild zero outputs")
    t.close()


def test_zero_over_zero_stays_nan():
    """All four outputs of a channel zero at an element whose draw r1 is exactly 0: the reference's 0 / 0.  The NaN is kept,
    in float64 and on the device; nothing else is compared."""
    params, x, r, tgt, hyper = _zero_case()
    r[0, 0, 0, 0, 0] = 0.0
    for stage in (1, 2):
        want, _ = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=stage, **hyper)
        assert np.isnan(want[0])
    t = _trainer(params, r, x.shape[0], x.shape[2], x.shape[3], **hyper)
    for ild in (False, True):
        out = t.ctx.to_host(t.run(x, tgt, 0, ild)).copy()
        assert np.isnan(out[0]), out
    t.close()


def test_one_update_matches_float64():
    """After one train_fn_ILD: params, accu and delta_accu against float64 Adadelta on the float64 gradients (the bounds of
    test_gpu_train_bach10.py::test_one_update_matches_float64)."""
    B, tc, F = 4, 12, 93
    params, x, r, tgt = _setup(B, tc, F, seed=4)
    _, g64 = train_ild_ref.loss_and_grads(params, x, tgt, r, stage=2)
    P64, A64, D64 = train_ref.adadelta(params, g64, [np.zeros(p.shape) for p in params],
                                       [np.zeros(p.shape) for p in params])
    t = _trainer(params, r, B, tc, F)
    t.step(x, tgt, ild=True)
    P = t.params()
    A, D = t.adadelta_state()
    for i in range(17):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert _rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert _rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i
    t.close()


def _reachable(B, tc, F):
    """Targets the masks can reach, as in the Bach10 test: source s is 0.4 / 0.3 / 0.2 / 0.1 of each input channel (so the
    true level differences are the mixture's own).  A small learning rate (0.05) and output biases of 0.3 (all outputs
    positive along the way) keep the trajectory well conditioned: in float64 it falls monotonically 8.579 -> 3.179, and a
    1e-6 relative change of the start moves it by 2.0e-7 relative at most.  With biases of 0.1 outputs reach zero from step
    13 on and the level differences jump."""
    from deepconvsep_amd import stereo_training as st
    params = st.glorot_init(tc, F, seed=5)
    params[16] = params[16] + np.float32(0.3)
    r = (0.1 * np.random.RandomState(6).randn(2, B, 4, tc, F)).astype(np.float32)
    x = (0.3 * np.random.RandomState(7).uniform(0.1, 1, size=(B, 2, tc, F))).astype(np.float32)
    tgt = np.stack([w * x[:, c] for w in (0.4, 0.3, 0.2, 0.1) for c in (0, 1)], axis=1).astype(np.float32)
    return params, x, r, tgt


def test_twenty_stage2_steps_follow_float64_and_learn():
    B, tc, F = 4, 10, 65
    params, x, r, tgt = _reachable(B, tc, F)
    t = _trainer(params, r, B, tc, F, learning_rate=0.05)
    got = [t.step(x, tgt, ild=True) for _ in range(20)]
    t.close()
    P = [np.asarray(p, np.float64) for p in params]
    A = [np.zeros(p.shape) for p in P]
    D = [np.zeros(p.shape) for p in P]
    want = []
    for _ in range(20):
        out, g = train_ild_ref.loss_and_grads(P, x, tgt, r, stage=2)
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
        outs = [t.step(x, tgt, ild=k >= 5) for k in range(10)]
        res.append((outs, t.params()))
        t.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_set_rand():
    """On inputs with silent target bins a new draw changes the stage-2 loss and reproduces the float64 value for that
    draw; a trainer created with draw A and set to B equals one created with B, bit for bit.  set_rand takes an ndarray or
    a device tensor."""
    B, tc, F = 3, 10, 33
    params, x, rA, tgt = _setup(B, tc, F, seed=8)
    tgt[:, 0:2, 2:5, :] = 0.0                    # vocals silent in both mics for three frames
    tgt[1, 6:8] = 0.0
    rB = (0.1 * np.random.RandomState(77).randn(*rA.shape)).astype(np.float32)
    wantA, _ = train_ild_ref.loss_and_grads(params, x, tgt, rA, stage=2)
    wantB, _ = train_ild_ref.loss_and_grads(params, x, tgt, rB, stage=2)
    assert abs(wantA[9] - wantB[9]) > 1e-3 * wantA[9]
    t = _trainer(params, rA, B, tc, F)
    outA = t.ctx.to_host(t.run(x, tgt, 0, True)).copy()
    t.set_rand(rB)
    outB = t.ctx.to_host(t.run(x, tgt, 0, True)).copy()
    _check_outputs(outA, wantA, "draw A")
    _check_outputs(outB, wantB, "draw B")
    assert outA[0] != outB[0] and outA[9] != outB[9]
    with pytest.raises(ValueError):
        t.set_rand(rB[:1])
    fresh = _trainer(params, rB, B, tc, F)
    t.set_rand(t.ctx.to_device(rB, np.float32))  # a device tensor this time
    res = []
    for tr in (t, fresh):
        outs = [tr.step(x, tgt, ild=True) for _ in range(3)]
        res.append((outs, tr.params()))
        tr.close()
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_set_rand_on_a_mono_graph():
    """dcs_trainer_set_rand works for every graph and takes the size given at create."""
    import test_gpu_train as TD
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import _ptr
    shape = (3, 10, 33)
    params, x, rA, tgt = TD._setup(*shape, seed=3)
    rB = np.random.RandomState(5).uniform(size=rA.shape).astype(np.float32)
    t = TD._trainer(params, rA, *shape)
    rB_d = t.ctx.to_device(rB, np.float32)
    with t.ctx.stream_scope():
        _lib.check(t.ctx._lib.dcs_trainer_set_rand(t._h, _ptr(rB_d)))
    fresh = TD._trainer(params, rB, *shape)
    a = [t.step(x, tgt) for _ in range(2)]
    b = [fresh.step(x, tgt) for _ in range(2)]
    assert a == b
    for p, q in zip(t.params(), fresh.params()):
        assert np.array_equal(p, q)
    t.close()
    fresh.close()


def test_saved_model_loads_in_network_and_separates(tmp_path):
    """The saved .pkl is a model of the inference library.  ``Network.forward_raw`` refuses the stereo graph by design (it
    runs through dcs_separate_stereo alone; tests/test_gpu_parity.py pins that), so the trainer's forward pass is held to
    the inference oracle's network (oracle.net_ref.forward, what the golden network case of this graph is made with) within
    1e-4 max, and the fused stereo separation of the loaded model to oracle.pipeline.separate_stereo within the 1e-4 of
    test_gpu_parity.py::test_stereo_ild_separation_matches_oracle."""
    import deepconvsep_amd as dcs
    from deepconvsep_amd.runtime import Network, default_context
    from oracle import net_ref, pipeline
    B, tc, F = 2, 30, 513
    params, x, r, tgt = _setup(B, tc, F, seed=11)
    t = _trainer(params, r, B, tc, F)
    for k in range(3):
        t.step(x, tgt, ild=k > 0)
    path = str(tmp_path / "model.pkl")
    t.save_model(path)
    loaded = dcs.load_model(path)
    assert len(loaded) == 17 and loaded[0].shape == (50, 2, 1, 513) and loaded[6].shape == (800, 256)
    assert loaded[16].shape == (8,)
    assert any(not np.array_equal(a, b) for a, b in zip(loaded, params))
    ctx = default_context()
    net = Network(ctx, "dsd_ild", loaded, tc, F)
    with pytest.raises(NotImplementedError):
        net.forward_raw(ctx.to_device(x, np.float32))
    ref = np.asarray(net_ref.forward("dsd_ild", loaded, x), dtype=np.float64)
    got = ctx.to_host(t.forward(x))
    t.close()
    assert got.shape == ref.shape == (B, 8, tc, F)
    print("forward: max |got - ref| %.3g, max |ref| %.3g" % (np.abs(got - ref).max(), np.abs(ref).max()))
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    sep = dcs.Separator("dsd_ild", loaded, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, ctx=ctx)
    n = 44100
    audio = np.stack([_tone(n, 220.0, 1), 0.5 * _tone(n, 220.0, 1) + 0.5 * _tone(n, 330.0, 2)], axis=1)
    out = sep.separate_stereo(audio)
    want = pipeline.separate_stereo(loaded, audio, 0.3, 30, 25, 32, 1024, 512, np.hanning)
    assert out.shape == want.shape == (n, 4, 2) and np.isfinite(out).all()
    print("separation: max |got - want| %.3g, max |want| %.3g" % (np.abs(out - want).max(), np.abs(want).max()))
    assert np.abs(out - want).max() < 1e-4 and np.abs(want).max() > 1e-3


def test_mono_trainers_unchanged_next_to_a_stereo_trainer():
    import test_gpu_train as TD
    import test_gpu_train_bach10 as TB
    import test_gpu_train_ikala as TI
    for T, shape, seed in ((TD, (7, 20, 65), 3), (TI, (3, 12, 131), 3), (TB, (3, 12, 93), 3)):
        res = []
        for with_stereo in (False, True):
            other = None
            if with_stereo:
                p, x2, r2, tgt2 = _setup(2, 12, 93, seed=1)
                other = _trainer(p, r2, 2, 12, 93)
            params, x, r, tgt = T._setup(*shape, seed=seed)
            t = T._trainer(params, r, *shape)
            outs = []
            for k in range(3):
                outs.append(t.ctx.to_host(t.run(x, tgt, 2)).copy())
                if other is not None:
                    other.step(x2, tgt2, ild=k % 2 == 1)
            assert all(o.shape == (7,) for o in outs)
            res.append((outs, t.params()))
            t.close()
            if other is not None:
                other.close()
        for a, b in zip(res[0][0], res[1][0]):
            assert np.array_equal(a, b)
        for a, b in zip(res[0][1], res[1][1]):
            assert np.array_equal(a, b)


def test_bad_arguments_and_range_ends():
    import test_gpu_train as TD
    from deepconvsep_amd import _lib
    from deepconvsep_amd import stereo_training as st
    from deepconvsep_amd.runtime import _ptr
    from deepconvsep_amd.stereo_training import StereoTrainer
    good = st.glorot_init(12, 93)
    rz = lambda B, tc, F: np.zeros((2, B, 4, tc, F))  # noqa: E731
    # time_context even 4 .. 64, F 1 .. 2049, batch 1 .. 1024
    for B, tc, F in ((1, 2, 93), (1, 13, 93), (1, 66, 93), (1, 12, 0), (1, 12, 2050), (0, 12, 93), (1025, 12, 93)):
        with pytest.raises(ValueError):
            StereoTrainer(params=good, batch_size=B, time_context=tc, feat_size=F, rand=rz(B, tc, F))
    with pytest.raises(ValueError):   # parameter count
        StereoTrainer(params=good[:15], batch_size=1, time_context=12, feat_size=93, rand=rz(1, 12, 93))
    bad = list(good)
    bad[0] = np.zeros((50, 1, 1, 93), np.float32)
    with pytest.raises(ValueError):   # the mono graph's conv1
        StereoTrainer(params=bad, batch_size=1, time_context=12, feat_size=93, rand=rz(1, 12, 93))
    with pytest.raises(ValueError):   # one draw instead of two
        StereoTrainer(params=good, batch_size=1, time_context=12, feat_size=93, rand=np.zeros((1, 1, 4, 12, 93)))
    t = StereoTrainer(params=good, batch_size=1, time_context=12, feat_size=93, rand=0.1 + rz(1, 12, 93))
    x, tgt = np.zeros((1, 2, 12, 93), np.float32), np.zeros((1, 8, 12, 93), np.float32)
    with pytest.raises(ValueError):   # mono inputs
        t.step(x[:, :1], tgt)
    with pytest.raises(ValueError):   # four target channels
        t.step(x, tgt[:, :4])
    with pytest.raises(ValueError):   # modes 3 and 7 do not exist
        t.run(x, tgt, 3)
    with pytest.raises(ValueError):
        t.run(x, tgt, 3, ild=True)
    t.close()
    # mode + 4 on a mono graph
    params, xm, rm, tm = TD._setup(2, 10, 33, seed=1)
    mono = TD._trainer(params, rm, 2, 10, 33)
    for mode in (4, 5, 6):
        with pytest.raises(ValueError):
            mono.run(xm, tm, mode)
    assert np.isfinite(mono.step(xm, tm))
    mono.close()
    # the ends of the ranges train, in both stages: kh = 2 at tc 4, tc 64, F 1
    for B, tc, F in ((1, 4, 7), (2, 64, 33), (3, 4, 1), (2, 6, 1)):
        params, x, r, tgt = _setup(B, tc, F, seed=2)
        t = _trainer(params, r, B, tc, F)
        assert np.isfinite(t.step(x, tgt)) and np.isfinite(t.step(x, tgt, ild=True))
        assert all(np.isfinite(p).all() for p in t.params())
        t.close()


_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_ild as T
from deepconvsep_amd.runtime import default_context
params, x, r, tgt = T._setup(3, 12, 131, seed=3)
t = T._trainer(params, r, 3, 12, 131)
for k in range(4):
    t.step(x, tgt, ild=k >= 2)
t.set_rand(r[::-1].copy())
out, g = t.loss_and_gradients(x, tgt, ild=True)
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


# ---------------------------------------------------------------------------------------------- the feed
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gather_channels_np(files, rows, tc, F, cin, cout, scale_in, scale_out):
    """What dcs_trainer_gather_channels must write: ``files[i]`` is ``[cin + cout, T_i, F]``; one float32 product per
    element, zero for file -1 and for frames past T_i."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    x = np.zeros((len(rows), cin, tc, F), dtype=np.float32)
    t = np.zeros((len(rows), cout, tc, F), dtype=np.float32)
    for b, (fi, start) in enumerate(rows):
        if fi < 0:
            continue
        a = np.asarray(files[fi], dtype=np.float32)
        n = max(0, min(tc, a.shape[1] - int(start)))
        x[b, :, :n] = np.float32(scale_in) * a[:cin, start:start + n]
        t[b, :, :n] = np.float32(scale_out) * a[cin:, start:start + n]
    return x, t


def _raw_gather_channels(ctx, files, rows, tc, F, cin, cout, scale_in, scale_out):
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import _ptr
    table, off = [], 0
    for a in files:
        table.append((off, a.shape[1]))
        off += a.size
    data_d = ctx.to_device(np.concatenate([a.ravel() for a in files]), np.float32)
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    with ctx.stream_scope():
        files_d = torch.from_numpy(np.asarray(table, dtype=np.int64)).to(ctx.device)
        win_d = torch.from_numpy(rows).to(ctx.device)
        x = torch.full((len(rows), cin, tc, F), 7.0, dtype=torch.float32, device=ctx.device)
        t = torch.full((len(rows), cout, tc, F), 7.0, dtype=torch.float32, device=ctx.device)
        _lib.check(ctx._lib.dcs_trainer_gather_channels(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(win_d), len(rows), tc, F,
                                                        cin, cout, scale_in, scale_out, _ptr(x), _ptr(t)))
    return ctx.to_host(x), ctx.to_host(t)


@pytest.mark.parametrize("cin,cout,F", [(2, 8, 5), (1, 4, 7), (3, 6, 4), (4, 16, 3), (1, 1, 1)])
def test_gather_channels_bit_for_bit(cin, cout, F):
    """Zero slots, a file shorter than tc, windows that run past the end of their file, scale_in != scale_out."""
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    tc = 6
    files = [feed_ref.data_pattern(cin + cout - 1, T, F, offset=100000 * i).astype(np.float32) / np.float32(7)
             for i, T in enumerate((20, 4, 6, 9))]
    rows = [(0, 0), (-1, 0), (1, 0), (0, 14), (0, 17), (2, 0), (3, 5), (-1, 0), (3, 3), (0, 5)]
    for scale_in, scale_out in ((0.3, 0.7), (1.0, 0.3), (0.3, 0.3)):
        x, t = _raw_gather_channels(ctx, files, rows, tc, F, cin, cout, scale_in, scale_out)
        wx, wt = _gather_channels_np(files, rows, tc, F, cin, cout, scale_in, scale_out)
        assert np.array_equal(_bits(x), _bits(wx)) and np.array_equal(_bits(t), _bits(wt))
    assert not x[1].any() and not t[7].any() and not x[2, :, 4:].any() and x[2, :, :4].all()


def test_gather_channels_next_to_the_mono_gathers(tmp_path):
    """One input channel, four outputs and equal factors is dcs_trainer_gather's layout: the three entry points agree, and
    each equals tests/feed_ref.py (the two existing gathers are unchanged)."""
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import _ptr, default_context
    ctx = default_context()
    tc, F = 6, 5
    files = [feed_ref.data_pattern(4, T, F, offset=1000 * i).astype(np.float32) for i, T in enumerate((15, 3, 8))]
    rows = [(0, 0), (1, 0), (-1, 0), (2, 2), (0, 9), (2, 5)]
    wx, wt = feed_ref.gather_np(files, rows, tc, F, 4, 0.3)
    x, t = _raw_gather_channels(ctx, files, rows, tc, F, 1, 4, 0.3, 0.3)
    assert np.array_equal(_bits(x), _bits(wx)) and np.array_equal(_bits(t), _bits(wt))
    table, off = [], 0
    for a in files:
        table.append((off, a.shape[1]))
        off += a.size
    data_d = ctx.to_device(np.concatenate([a.ravel() for a in files]), np.float32)
    for entry in ("gather", "sources"):
        with ctx.stream_scope():
            files_d = torch.from_numpy(np.asarray(table, dtype=np.int64)).to(ctx.device)
            win_d = torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(ctx.device)
            xo = torch.empty((len(rows), 1, tc, F), dtype=torch.float32, device=ctx.device)
            to = torch.empty((len(rows), 4, tc, F), dtype=torch.float32, device=ctx.device)
            if entry == "gather":
                _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(win_d), len(rows), tc, F,
                                                       0.3, _ptr(xo), _ptr(to)))
            else:
                _lib.check(ctx._lib.dcs_trainer_gather_sources(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(win_d), len(rows),
                                                               tc, F, 4, 0.3, _ptr(xo), _ptr(to)))
        assert np.array_equal(_bits(ctx.to_host(xo)), _bits(wx)) and np.array_equal(_bits(ctx.to_host(to)), _bits(wt))
    for cin, cout in ((0, 8), (5, 8), (2, 0), (2, 17)):
        with pytest.raises(ValueError):
            _raw_gather_channels(ctx, files, rows, tc, F, cin, cout, 1.0, 1.0)


def test_stereo_feature_windows_gather_and_batches(tmp_path):
    from test_train_ild_cpu import _write_pair
    from deepconvsep_amd.stereo_training import StereoFeatureWindows
    Ts = (40, 5, 6, 23)               # T < tc: one padded window; T == tc: a slot loadFile never fills (all zero)
    files = []
    for i, T in enumerate(Ts):
        a, b = _write_pair(tmp_path, "s%d_0" % i, T, 4, seed=i)
        files.append(np.concatenate([a, b]).astype(np.float32))
    w = StereoFeatureWindows([str(tmp_path)], time_context=6, overlap=2, mult_factor_in=0.3, mult_factor_out=0.5,
                             batch_size=4, seed=2)
    assert (w.table[:, 0] < 0).any()
    rows = list(range(w.total))
    x, t = w.gather(rows)
    wx, wt = _gather_channels_np(files, w.table, 6, 4, 2, 8, 0.3, 0.5)
    assert np.array_equal(_bits(w.ctx.to_host(x)), _bits(wx)) and np.array_equal(_bits(w.ctx.to_host(t)), _bits(wt))
    perm = np.random.RandomState(2 + 1).permutation(w.total)
    got = list(w.batches(1))
    assert len(got) == w.total // 4
    for b, (xb, tb) in enumerate(got):
        wxb, wtb = _gather_channels_np(files, w.table[perm[4 * b:4 * b + 4]], 6, 4, 2, 8, 0.3, 0.5)
        assert np.array_equal(w.ctx.to_host(xb), wxb) and np.array_equal(w.ctx.to_host(tb), wtb)


# ---------------------------------------------------------------------------------------------- the command lines
def _tone(n, f, seed):
    t = np.arange(n) / 44100.0
    return 0.2 * np.sin(2 * np.pi * f * t) * (1 + 0.1 * np.random.RandomState(seed).randn(n))


def test_command_lines_features_train_resume_separate(tmp_path):
    import scipy.io.wavfile
    from deepconvsep_amd.separation import write_wav
    from deepconvsep_amd.transform import read_shape_file
    db = tmp_path / "DSD100"
    out = tmp_path / "out"
    out.mkdir()
    n = 2 * 44100
    sources = ("vocals", "bass", "drums", "other")
    songs = {"Dev": ("051 - A", "052 - B"), "Test": ("001 - C",)}
    for sub, names in songs.items():
        for i, song in enumerate(names):
            (db / "Mixtures" / sub / song).mkdir(parents=True)
            (db / "Sources" / sub / song).mkdir(parents=True)
            stems = []
            for k, s in enumerate(sources):
                st = np.stack([_tone(n, 110.0 * (k + 1) * (i + 1), 10 * i + k) * (0.3 + 0.2 * k),
                               _tone(n, 110.0 * (k + 1) * (i + 1), 10 * i + k) * (0.9 - 0.2 * k)], axis=1) / 4
                write_wav(str(db / "Sources" / sub / song / (s + ".wav")), st, 44100)
                stems.append(st)
            write_wav(str(db / "Mixtures" / sub / song / "mixture.wav"), sum(stems), 44100)
    ex = os.path.join(ROOT, "examples", "dsd100_2ch_ILD")
    run = lambda *a: subprocess.run([sys.executable] + list(a), timeout=600, capture_output=True, text=True)  # noqa: E731
    rc = run(os.path.join(ex, "compute_features.py"), "--db", str(db))
    assert rc.returncode == 0, rc.stderr[-3000:]
    fdir = db / "transforms" / "feature_folder"
    feats = sorted(f for f in os.listdir(fdir) if f.endswith(".data"))
    assert feats == ["051 - A_0_in_m_.data", "051 - A_0_out_m_.data", "052 - B_0_in_m_.data", "052 - B_0_out_m_.data"]
    for f in feats:
        shp = read_shape_file(str(fdir / f.replace(".data", ".shape")))
        assert shp[0] == (2 if "_in_" in f else 8) and shp[2] == 513
    common = ["--db", str(db), "--output", str(out), "--model", "m", "--batch_size", "4", "--windows", "all"]
    rc = run(os.path.join(ex, "train_dsd_ild.py"), *(common + ["--nepochs", "2", "--skip_sep"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    so = rc.stdout
    assert "Training stage 1 (mse)..." in so and "Training stage 2 (ILD)..." in so
    assert so.index("Training stage 1") < so.index("Epoch 2 of 2") < so.index("Training stage 2")
    assert so.count("Epoch 1 of 2") == 2 and so.count("Epoch 2 of 2") == 1
    assert so.count("  training loss:") == 3
    for j in (0, 1):
        for s in sources:
            assert so.count("training loss for %s in mic %d:" % (s, j)) == 2
    assert "nchannels:  2" in so and "nsources:  4" in so
    assert (out / "models" / "model_m_noILD.pkl").is_file() and (out / "models" / "model_m.pkl").is_file()
    with open(str(out / "models" / "loss_m.data"), "rb") as fh:
        losses = pickle.load(fh)
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert not (out / "output").exists()
    rc = run(os.path.join(ex, "train_dsd_ild.py"), *(common + ["--nepochs", "1", "--load"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Separating" in rc.stdout
    for sub, names in songs.items():
        for song in names:
            for s in sources:
                path = out / "output" / "m" / "Sources" / sub / song / (s + ".wav")
                assert path.is_file(), path
                sr, wav = scipy.io.wavfile.read(str(path))
                assert sr == 44100 and wav.shape == (n, 2)
    # --skip: no training, the saved model separates
    before = (out / "models" / "model_m.pkl").stat().st_mtime_ns
    rc = run(os.path.join(ex, "train_dsd_ild.py"), *(common + ["--skip"]))
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert "Epoch" not in rc.stdout and (out / "models" / "model_m.pkl").stat().st_mtime_ns == before
