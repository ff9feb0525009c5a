"""The optimiser side of the training core on the MI355X (csrc/train_core.hip: adam_kernel, dcs_trainer_set_optimizer,
dcs_trainer_set, dcs_trainer_set_steps) through ``TrainerHandle``, on every graph family -- the DSD trainer, the
score-informed trainer in its 17-array and 11-array layouts, the deep 1x1 trainer and the stereo trainer -- against the
float64 restatements tests/adam_ref.py and tests/train_ref.py::adadelta, and the two schedules built on it
(examples/bach10_scoreinformed/train_bach10_si.py --second_pass, examples/dsd100_2ch_ILD/train_dsd_ild_3stages.py).

The update tests apply the float64 restatement to the DEVICE's own float32 gradients (two runs of the gradients are
bit-identical by the core's contract), so nothing but the update's own float32 arithmetic is compared."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import adam_ref
import train_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLES = ("dsd", "si17", "si11", "deep1x1", "stereo")
# the smallest shapes the existing suites use at the kernels' edges
SHAPES = {"dsd": (4, 10, 33), "si17": (2, 9, 33), "si11": (2, 9, 33), "deep1x1": (2, 19, 253), "stereo": (3, 10, 33)}
TINY = 1e-37     # below the smallest normal float32 (1.18e-38) a float32 has no relative precision left


def _case(handle, seed=3):
    """(params, x, r, tgt, make) of one handle with the well-conditioned inputs of its own test file; ``make(params)``
    creates a trainer on the draw r."""
    B, tc, F = SHAPES[handle]
    if handle == "dsd":
        import test_gpu_train as T
        params, x, r, tgt = T._setup(B, tc, F, seed)
    elif handle in ("si17", "si11"):
        import test_gpu_train_si as T
        params, x, r, tgt = T._setup(B, tc, F, seed, branches=4 if handle == "si17" else 1)
    elif handle == "deep1x1":
        import test_gpu_train_deep1x1 as T
        import train_deep1x1_ref as R
        params, x, r, tgt = R.setup(B, tc, F, seed)
    else:
        import test_gpu_train_ild as T
        params, x, r, tgt = T._setup(B, tc, F, seed)
    return params, x, r, tgt, lambda p: T._trainer(p, r, B, tc, F)


def _dead(handle, arrays):
    """The parts of a .pkl-ordered list that no gradient reaches and the trainer holds outside its stepped state."""
    if handle == "si17":
        return [arrays[i] for i in (10, 11, 12, 13, 14, 15)] + [arrays[16][4:]]
    if handle == "deep1x1":
        return [arrays[18][200:], arrays[19][200:], arrays[20][200:], arrays[21][4:]]
    return []


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _zeros(params):
    return [np.zeros(p.shape) for p in params]


def _check_adam_step(label, k, a_t, P, M, V, P64, M64, V64, mabs, pbound):
    """Device state after an Adam step of size ``a_t`` against the float64 state, elementwise.  ``k``: how many float32
    steps separate the two states.  ``mabs``: the same recursion as m on |g|, mabs' = beta1 mabs + (1 - beta1) |g| >=
    |m64| (started at the device's |m| where the float64 state starts from the device's): a rounding of m' is relative to
    its two terms, not to their sum, and from the second step on the terms can cancel; an error e of m_prev arrives as
    beta1 e, so with d the error of one step, e' <= beta1 (k - 1) d mabs + d mabs' <= k d mabs'.  On the first step mabs =
    |m64|, and the bounds are the plain relative ones.  ``pbound``: the parameter bound accumulated over the earlier steps.

    m, v: 1e-6 k relative -- the constants beta and 1 - beta rounded to float32 and the products and the sum are at most
    five roundings of 2^-24 (3e-7) a step.  p: 2^-23 |p64| for the subtraction, and 1e-6 k of the step a_t mabs / (sqrt(v) +
    eps): a_t, m' (as above), sqrt(v') (half v's error and its own rounding), the sum with eps, the product and the
    quotient are about eight roundings (5e-7).  Returns the parameter bound for the next step.  Prints, then asserts."""
    worst = [0.0, 0.0, 0.0]
    out = []
    for i in range(len(P64)):
        bm = 1e-6 * k * mabs[i] + TINY
        bv = 1e-6 * k * V64[i] + TINY
        stepabs = a_t * mabs[i] / (np.sqrt(V64[i]) + adam_ref.EPSILON)
        bp = pbound[i] + 2.0 ** -23 * np.abs(P64[i]) + 1e-6 * k * stepabs + TINY
        em, ev, ep = np.abs(M[i] - M64[i]), np.abs(V[i] - V64[i]), np.abs(P[i] - P64[i])
        if em.size:
            worst = [max(worst[0], float((em / bm).max())), max(worst[1], float((ev / bv).max())),
                     max(worst[2], float((ep / bp).max()))]
        out.append((em, bm, ev, bv, ep, bp))
    print("%s step %d: worst error / bound: m %.3f, v %.3f, p %.3f" % (label, k, worst[0], worst[1], worst[2]))
    for i, (em, bm, ev, bv, ep, bp) in enumerate(out):
        assert (em <= bm).all(), (label, k, "m", i, float((em / bm).max()))
        assert (ev <= bv).all(), (label, k, "v", i, float((ev / bv).max()))
        assert (ep <= bp).all(), (label, k, "p", i, float((ep / bp).max()))
    return [o[5] for o in out]


def _adam_steps(handle, nsteps):
    params, x, r, tgt, make = _case(handle)
    t = make(params)
    t.set_optimizer('adam')
    st = t.optimizer_state()
    assert st['kind'] == 'adam' and st['steps'] == 0
    assert st['hyper'] == {'learning_rate': 1e-3, 'beta1': 0.9, 'beta2': 0.999, 'epsilon': 1e-8}
    P64 = [np.asarray(p, np.float64) for p in params]
    M64, V64 = _zeros(params), _zeros(params)
    pbound, mabs = _zeros(params), _zeros(params)
    never = [np.ones(p.shape, bool) for p in params]     # elements whose gradient has been exactly zero at every step
    for k in range(1, nsteps + 1):
        _, g = t.loss_and_gradients(x, tgt)
        t.step(x, tgt)
        assert _same(g, t.gradients())     # the step used the gradients that mode 1 returned, bit for bit
        st = t.optimizer_state()
        assert st['steps'] == k
        P, (M, V) = t.params(), st['slots']
        mabs = [0.9 * a + 0.1 * np.abs(gi) for a, gi in zip(mabs, g)]
        P64, M64, V64, _ = adam_ref.adam(P64, g, M64, V64, k - 1)
        pbound = _check_adam_step(handle, k, adam_ref.a_t(k), P, M, V, P64, M64, V64, mabs, pbound)
        # exactly zero gradient so far: bit-unchanged parameters, zero m and v
        for i, gi in enumerate(g):
            never[i] &= gi == 0
            z = never[i]
            assert np.array_equal(P[i][z], params[i][z]) and not M[i][z].any() and not V[i][z].any(), i
        for a, b in zip(_dead(handle, P), _dead(handle, params)):
            assert a.size and np.abs(b).max() > 0 and np.array_equal(a, b)
        for a, z in zip(_dead(handle, g) + _dead(handle, M) + _dead(handle, V), 3 * _dead(handle, never)):
            assert not a.any() and z.all()
    t.close()


@pytest.mark.parametrize("handle", HANDLES)
def test_one_adam_update_against_the_kernels_own_gradients(handle):
    """Bounds (see _check_adam_step; k = 1, where they are the plain ones): m and v to 1e-6 relative, |p - p64| <= 2^-23
    |p64| + 1e-6 |step64|; parameters with exactly zero gradient, the dead arrays among them, are bit-unchanged."""
    _adam_steps(handle, 1)


@pytest.mark.parametrize("handle", HANDLES)
def test_three_adam_updates_against_the_kernels_own_gradients(handle):
    """The float64 state evolves from each step's device gradients; the bounds grow with the step index.  a_1 = 0.316 lr,
    a_2 = 0.235 lr and a_3 = 0.202 lr differ by far more than the bound: a stuck or off-by-one t fails here."""
    _adam_steps(handle, 3)


def test_twenty_adam_steps_follow_float64_and_learn():
    """DSD, the tame setup of test_gpu_train.py::test_twenty_steps_follow_float64_and_learn (output biases of 0.1), lr =
    1e-3 (Lasagne's default): the float64 reference's loss falls from 2.590 to 0.0183 over the 20 steps, far more than the
    10 % asked for.  Tolerance: on the CPU the loss trajectory of float64 autograd driving adam_ref and the same trajectory
    driven by float32 autograd (train_ref.loss_and_grads(..., dtype=torch.float32)) deviate by at most 5.74e-6 relative
    (at step 20; below 3e-7 for the first 14 steps); ten times that, 5.74e-5, is allowed here, since the device's
    summation order differs from torch's."""
    import test_gpu_train as T
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    B, tc, F = 4, 10, 33
    params = training.glorot_init("dsd", tc, F, seed=5)
    params[14] = params[14] + np.float32(0.1)
    r = np.random.RandomState(6).uniform(size=(B, 1, tc, F)).astype(np.float32)
    x, tgt = T._learnable(B, tc, F, 7)
    t = Trainer(params=params, batch_size=B, time_context=tc, feat_size=F, rand=r)
    t.set_optimizer('adam', learning_rate=1e-3)
    got = [t.step(x, tgt) for _ in range(20)]
    t.close()
    P = [np.asarray(p, np.float64) for p in params]
    M, V = _zeros(P), _zeros(P)
    want = []
    for k in range(20):
        out, g = train_ref.loss_and_grads(P, x, tgt, r)
        want.append(out[0])
        P, M, V, _ = adam_ref.adam(P, g, M, V, k, lr=1e-3)
    print("device", got)
    print("float64", want)
    print("relative deviation", np.abs(np.array(got) / np.array(want) - 1))
    assert want[-1] <= 0.9 * want[0]
    np.testing.assert_allclose(got, want, rtol=5.74e-5)
    assert got[-1] < got[0], got


def _run(t, x, tgt, n):
    return [t.step(x, tgt) for _ in range(n)]


def _full_state(t):
    st = t.optimizer_state()
    return t.params(), st['slots'][0], st['slots'][1], st


@pytest.mark.parametrize("kind", ("adadelta", "adam"))
@pytest.mark.parametrize("handle", HANDLES)
def test_set_optimizer_is_a_fresh_optimizer(handle, kind):
    """After 3 Adadelta steps, set_optimizer(kind) and 3 steps are bit-identical -- parameters and both slots -- to a new
    trainer created from params() with the same draw, set_optimizer(kind) and 3 steps."""
    params, x, r, tgt, make = _case(handle)
    t = make(params)
    _run(t, x, tgt, 3)
    mid = t.params()
    assert any(a.any() for a in t.optimizer_state()['slots'][0])
    t.set_optimizer(kind)
    st = t.optimizer_state()
    assert st['kind'] == kind and st['steps'] == 0 and not any(a.any() for s in st['slots'] for a in s)
    assert _same(t.params(), mid)
    la = _run(t, x, tgt, 3)
    a = _full_state(t)
    t.close()
    u = make(mid)
    if kind == 'adam':
        u.set_optimizer('adam')
    lb = _run(u, x, tgt, 3)
    b = _full_state(u)
    u.close()
    assert la == lb and a[3]['steps'] == b[3]['steps'] == 3
    assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])
    assert not _same(a[0], mid)


@pytest.mark.parametrize("kind", ("adadelta", "adam"))
@pytest.mark.parametrize("handle", HANDLES)
def test_exact_resume_from_a_checkpoint(handle, kind, tmp_path):
    """Six steps straight are bit-identical to 3 steps, save_checkpoint, a NEW trainer (other parameters, other optimiser),
    load_checkpoint and 3 steps.  Under Adam this needs the step count: a_4 is not a_1."""
    params, x, r, tgt, make = _case(handle)
    other = _case(handle, seed=11)[0]
    t = make(params)
    if kind == 'adam':
        t.set_optimizer('adam', learning_rate=2e-3, beta1=0.8)
    straight = _run(t, x, tgt, 6)
    a = _full_state(t)
    t.close()
    t = make(params)
    if kind == 'adam':
        t.set_optimizer('adam', learning_rate=2e-3, beta1=0.8)
    first = _run(t, x, tgt, 3)
    path = str(tmp_path / "ck.pkl")
    t.save_checkpoint(path)
    t.close()
    with open(path, "rb") as fh:
        assert fh.read(2) == b"\x80\x02"       # pickle protocol 2
    u = make(other)
    u.set_optimizer('adam' if kind == 'adadelta' else 'adadelta')
    _run(u, x, tgt, 1)
    u.load_checkpoint(path)
    st = u.optimizer_state()
    assert st['kind'] == kind and st['steps'] == 3
    if kind == 'adam':
        assert st['hyper'] == {'learning_rate': 2e-3, 'beta1': 0.8, 'beta2': 0.999, 'epsilon': 1e-8}
    rest = _run(u, x, tgt, 3)
    b = _full_state(u)
    u.close()
    assert first + rest == straight
    assert b[3]['steps'] == 6 and _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


@pytest.mark.parametrize("handle", ("si17", "deep1x1"))
def test_setting_an_optimizer_slot_leaves_the_dead_parameters_alone(handle):
    """A graph with nstate < nparams keeps its dead parameters outside the stepped state; dcs_trainer_set of slot 2 or 3 must
    not write there, whatever the caller's arrays hold at those places."""
    params, x, r, tgt, make = _case(handle)
    t = make(params)
    _run(t, x, tgt, 2)
    st = t.optimizer_state()
    P = t.params()
    for s in st['slots']:
        for a in _dead(handle, s):
            assert a.size and not a.any()
            a[...] = 7.0
    t.load_optimizer_state(st)
    assert _same(t.params(), P)
    for a, b in zip(_dead(handle, t.params()), _dead(handle, params)):
        assert np.array_equal(a, b)
    back = t.optimizer_state()
    assert back['steps'] == 2
    for s, s0 in zip(back['slots'], st['slots']):
        for a in _dead(handle, s):
            assert not a.any()
        for a in _dead(handle, s0):
            a[...] = 0.0
        assert _same(s, s0)
    t.close()


@pytest.mark.parametrize("kind", ("adadelta", "adam"))
@pytest.mark.parametrize("handle", HANDLES)
def test_set_params_on_a_live_trainer_keeps_the_optimizer(handle, kind):
    """set_params keeps both slots and the step count, and the next step is the float64 update from that state on the
    device's gradients.  Adam: the bounds of _check_adam_step at k = 1 (the float64 step starts from the device's float32
    state).  Adadelta (float64: train_ref.adadelta): accu' = rho accu + (1 - rho) g^2 is a sum of non-negative terms with
    the constants' float32 rounding (1 - 0.95f is 2.4e-7 off 0.05) and four more roundings: 1e-6 relative; u = g sqrt(delta
    + eps) / sqrt(accu' + eps) adds two sums, two roots (each halving its argument's error), a product and a quotient: 1e-6
    |u| on the parameter next to 2^-23 |p64| for the subtraction; delta' = rho delta + (1 - rho) u^2 carries twice u's error
    and the constants': 3e-6 relative."""
    params, x, r, tgt, make = _case(handle)
    other = _case(handle, seed=11)[0]
    t = make(params)
    if kind == 'adam':
        t.set_optimizer('adam')
    _run(t, x, tgt, 2)
    st = t.optimizer_state()
    t.set_params(other)
    assert _same(t.params(), other)
    now = t.optimizer_state()
    assert now['kind'] == kind and now['steps'] == 2 and now['hyper'] == st['hyper']
    assert _same(now['slots'][0], st['slots'][0]) and _same(now['slots'][1], st['slots'][1])
    _, g = t.loss_and_gradients(x, tgt)
    t.step(x, tgt)
    P, S2, S3, after = _full_state(t)
    t.close()
    assert after['steps'] == 3
    A0, B0 = st['slots']
    if kind == 'adam':
        mabs = [0.9 * np.abs(m) + 0.1 * np.abs(gi) for m, gi in zip(A0, g)]
        P64, M64, V64, _ = adam_ref.adam(other, g, A0, B0, 2)
        _check_adam_step(handle + " after set_params", 1, adam_ref.a_t(3), P, S2, S3, P64, M64, V64, mabs, _zeros(params))
    else:
        P64, A64, D64 = train_ref.adadelta(other, g, A0, B0)
        for i in range(len(P64)):
            u = np.abs(P64[i] - np.asarray(other[i], np.float64))
            assert (np.abs(S2[i] - A64[i]) <= 1e-6 * A64[i] + TINY).all(), i
            assert (np.abs(S3[i] - D64[i]) <= 3e-6 * D64[i] + TINY).all(), i
            assert (np.abs(P[i] - P64[i]) <= 2.0 ** -23 * np.abs(P64[i]) + 1e-6 * u + TINY).all(), i
    for a, b in zip(_dead(handle, P), _dead(handle, other)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("handle", HANDLES)
def test_bad_arguments_raise_and_leave_the_trainer_as_it_was(handle):
    from deepconvsep_amd import _lib
    params, x, r, tgt, make = _case(handle)
    t = make(params)
    _run(t, x, tgt, 1)
    with pytest.raises(ValueError, match="optimizer 'sgd'"):
        t.set_optimizer('sgd')
    with pytest.raises(TypeError, match="rho"):
        t.set_optimizer('adam', rho=0.5)
    with pytest.raises(ValueError, match=r"dcs_trainer_set_optimizer: kind 7 \(0 adadelta, 1 adam\)"):
        t._set_optimizer(7, [1.0, 0.5, 0.5, 1e-8])
    with pytest.raises(ValueError, match=r"adam beta1 1, beta2 0\.999 \(each in \[0, 1\)\)"):
        t.set_optimizer('adam', beta1=1.0)
    with pytest.raises(ValueError, match=r"adam beta1 0\.9, beta2 -0\.1"):
        t.set_optimizer('adam', beta2=-0.1)
    with pytest.raises(ValueError, match=r"adam epsilon 0 \(finite, above 0\)"):
        t.set_optimizer('adam', epsilon=0.0)
    with pytest.raises(ValueError, match=r"adadelta rho 1 \(in \[0, 1\)\)"):
        t.set_optimizer('adadelta', rho=1.0)
    with pytest.raises(ValueError, match=r"adadelta epsilon -1e-06"):
        t.set_optimizer('adadelta', epsilon=-1e-6)
    for lr in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match="learning rate"):
            t.set_optimizer('adam', learning_rate=lr)
    with pytest.raises(ValueError, match=r"dcs_trainer_set: which 1 "):
        t._set(1, params)
    with pytest.raises(ValueError, match=r"mismatch: got %d values to set %d parameters" % (len(params) - 1, len(params))):
        t.set_params(params[:-1])
    bad = list(params)
    bad[0] = np.zeros(tuple(params[0].shape[:-1]) + (params[0].shape[-1] + 1,), np.float32)
    with pytest.raises(ValueError, match="mismatch: parameter 0 has shape"):
        t.set_params(bad)
    with pytest.raises(ValueError, match="dcs_trainer_set_steps: -1 steps"):
        _lib.check(t.ctx._lib.dcs_trainer_set_steps(t._h, -1))
    with pytest.raises(ValueError, match="-1 steps"):
        t.load_optimizer_state(dict(t.optimizer_state(), steps=-1))       # refused before anything is written
    st = t.optimizer_state()
    assert st['kind'] == 'adadelta' and st['steps'] == 1 and any(a.any() for a in st['slots'][0])
    la = _run(t, x, tgt, 2)
    a = _full_state(t)
    t.close()
    u = make(params)
    lb = _run(u, x, tgt, 3)[1:]
    b = _full_state(u)
    u.close()
    assert la == lb and _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


def test_load_checkpoint_checks_the_shapes_before_it_writes(tmp_path):
    params, x, r, tgt, make = _case("si11")
    t = make(params)
    _run(t, x, tgt, 1)
    path = str(tmp_path / "ck.pkl")
    t.save_checkpoint(path)
    t.close()
    p17, _, _, _, make17 = _case("si17")
    u = make17(p17)
    with pytest.raises(ValueError, match="mismatch: got 11 values to set 17 parameters"):
        u.load_checkpoint(path)
    model = str(tmp_path / "model.pkl")
    u.save_model(model)
    with pytest.raises(ValueError, match="not a trainer checkpoint"):
        u.load_checkpoint(model)
    assert _same(u.params(), p17) and u.optimizer_state()['steps'] == 0
    u.close()


# ---------------------------------------------------------------------------------------------- under the guard-band harness
_GUARD_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_train_optim as T
from deepconvsep_amd.runtime import default_context
res = []
for handle in ("si17", "dsd"):
    T._adam_steps(handle, 2)
    params, x, r, tgt, make = T._case(handle)
    t = make(params)
    t.set_optimizer('adam')
    T._run(t, x, tgt, 2)
    st = t.optimizer_state()
    t.set_params(T._case(handle, seed=11)[0])
    t.load_optimizer_state(st)
    T._run(t, x, tgt, 2)
    p, m, v, st = T._full_state(t)
    assert st['steps'] == 4 and all(np.isfinite(a).all() for a in p + m + v)
    res += [a.ravel() for a in p + m + v]
    t.close()
default_context().check_guards()
np.save(sys.argv[2], np.concatenate(res))
"""


def test_guard_harness_red_zones_and_poisons(tmp_path):
    """The Adam update and the set paths (parameters, both slots, on a graph with dead parameters and on one without) with
    red zones around every device buffer of the library and two poison values: no red zone is touched and nothing read
    depends on the poison."""
    outs = []
    for poison in ("255", "127"):
        env = dict(os.environ, DCS_WS_GUARD="4096", DCS_WS_POISON=poison)
        dst = str(tmp_path / ("out_%s.npy" % poison))
        rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst], env=env, timeout=300,
                            capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-3000:]
        outs.append(np.load(dst))
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- the command lines
def _run_script(*a):
    return subprocess.run([sys.executable] + list(a), timeout=300, capture_output=True, text=True)


def test_second_pass_command_line(tmp_path, capsys):
    """train_bach10_si.py --nepochs 6 --second_pass: 6 + 2 epoch blocks, 8 losses, and the saved model is the best epoch's --
    checked against an in-process twin of the schedule on the API (same seeds, so every loss is the same float).  Without
    the flag: the six epochs alone, as before."""
    import test_gpu_train_si as TS
    from deepconvsep_amd.score_training import ScoreFeatureWindows, ScoreTrainer
    from deepconvsep_amd.separation import load_model, write_wav
    db = tmp_path / "Bach10" / "Sources"
    n = 3 * 44100
    pieces = ("01-AchGott", "02-AchLieben")
    for i, piece in enumerate(pieces):
        (db / piece).mkdir(parents=True)
        for k, s in enumerate(("bassoon", "clarinet", "saxphone", "violin")):
            write_wav(str(db / piece / ("%s-%s.wav" % (piece, s))), TS._tone(n, 110.0 * (k + 1) * (i + 1), 10 * i + k), 44100)
        for code in ("_g", "_b"):
            TS._score_dir(db / piece, n / 44100.0, code)
    ex = os.path.join(ROOT, "examples", "bach10_scoreinformed")
    rc = _run_script(os.path.join(ex, "compute_features.py"), "--db", str(db), "--frame_size", "1024")
    assert rc.returncode == 0, rc.stderr[-3000:]
    def read(out):
        with open(str(out / "models" / "loss_m_gt.data"), "rb") as fh:
            return pickle.load(fh), load_model(str(out / "models" / "model_m_gt.pkl"))

    outs = [tmp_path / "out0", tmp_path / "out1"]
    for o in outs:
        o.mkdir()
    common = ["--db", str(db), "--model", "m", "--batch_size", "4", "--frame_size", "1024", "--nepochs", "6", "--skip_sep"]
    rc = _run_script(os.path.join(ex, "train_bach10_si.py"), "--output", str(outs[1]), "--second_pass", *common)
    assert rc.returncode == 0, rc.stderr[-3000:]
    runs = {True: (rc.stdout,) + read(outs[1])}
    # without the flag, in this process (the command line itself is test_gpu_train_si.py's business)
    sys.path.insert(0, ex)
    try:
        import train_bach10_si
    finally:
        sys.path.remove(ex)
    capsys.readouterr()
    train_bach10_si.main(["--output", str(outs[0])] + common)
    runs[False] = (capsys.readouterr().out,) + read(outs[0])
    so, losses, saved = runs[True]
    assert [so.count("Epoch %d of 6 took" % k) for k in range(1, 7)] == [1] * 6
    assert so.count("Epoch 1 of 2 took") == 1 and so.count("Epoch 2 of 2 took") == 1
    assert so.index("Epoch 6 of 6") < so.index("Epoch 1 of 2") < so.index("Epoch 2 of 2")
    assert so.count("  training loss:") == 8 and so.count("training loss for violin") == 8
    assert len(losses) == 8 and np.isfinite(losses).all()
    so0, losses0, saved0 = runs[False]
    assert so0.count(" took ") == 6 and "of 2 took" not in so0 and so0.count("  training loss:") == 6
    assert losses0 == losses[:6]

    # the twin: trainCNNrwc.py:287-354 on the API
    data = ScoreFeatureWindows([str(db / "transforms" / "t3")], 'e', 30, 25, 0.3, 'reference', 4, 0)
    t = ScoreTrainer(branches=4, batch_size=4, time_context=30, feat_size=513, seed=0)
    twin, best, min_loss = [], None, 1e14
    best6 = None

    def epochs(count, first):
        nonlocal best, min_loss
        for e in range(count):
            err = 0.0
            for xb, tb in data.batches(first + e):
                err += t.step(xb, tb)
            twin.append(err / data.iteration_size)
            if twin[-1] < min_loss:
                min_loss, best = twin[-1], t.params()

    epochs(6, 0)
    best6 = best
    if twin[-1] > min_loss:
        t.set_params(best)
    t.set_optimizer('adam')
    epochs(2, 6)
    t.close()
    assert twin == losses
    assert _same(saved, best) and _same(saved0, best6)
    assert min(losses) == losses[int(np.argmin(losses))] == min_loss


def test_three_stage_command_line_and_its_twin_on_the_api(tmp_path):
    """train_dsd_ild_3stages.py --nepochs_mse 2 --nepochs_ILD 1: the three files under the _mseEp=2_ILDEp=1 name, three
    losses, stereo wavs for the one mixture.  The twin runs the stage order on the API with the same seeds -- stage 1, keep
    the optimiser's state, a fresh Adadelta for stage 2, the kept state for stage 3 -- and ends on the bits of the script's
    _ILD_extra_mse.pkl; a twin that gave stage 3 fresh accumulators would not."""
    import scipy.io.wavfile
    import torch
    import test_gpu_train_ild as TI
    from deepconvsep_amd.separation import load_model, write_wav
    from deepconvsep_amd.stereo_training import RAND_STD, StereoFeatureWindows, StereoTrainer
    db = tmp_path / "DSD100"
    out = tmp_path / "out"
    out.mkdir()
    n = 2 * 44100
    sources = ("vocals", "bass", "drums", "other")
    song = "051 - A"
    (db / "Mixtures" / "Dev" / song).mkdir(parents=True)
    (db / "Sources" / "Dev" / song).mkdir(parents=True)
    stems = []
    for k, s in enumerate(sources):
        st = np.stack([TI._tone(n, 110.0 * (k + 1), k) * (0.3 + 0.2 * k), TI._tone(n, 110.0 * (k + 1), k) * (0.9 - 0.2 * k)],
                      axis=1) / 4
        write_wav(str(db / "Sources" / "Dev" / song / (s + ".wav")), st, 44100)
        stems.append(st)
    write_wav(str(db / "Mixtures" / "Dev" / song / "mixture.wav"), sum(stems), 44100)
    ex = os.path.join(ROOT, "examples", "dsd100_2ch_ILD")
    rc = _run_script(os.path.join(ex, "compute_features.py"), "--db", str(db))
    assert rc.returncode == 0, rc.stderr[-3000:]
    rc = _run_script(os.path.join(ex, "train_dsd_ild_3stages.py"), "--db", str(db), "--output", str(out), "--model", "m",
                     "--batch_size", "4", "--windows", "all", "--nepochs_mse", "2", "--nepochs_ILD", "1")
    assert rc.returncode == 0, rc.stderr[-3000:]
    so = rc.stdout
    assert so.index("1st MSE training stage") < so.index("ILD training stage...") < so.index("2nd MSE training stage") \
        < so.index("Separating")
    assert so.count("Epoch 1 of 2") == 2 and so.count("Epoch 2 of 2") == 2 and so.count("Epoch 1 of 1") == 1
    name = "m_mseEp=2_ILDEp=1"
    files = [out / "models" / (name + sfx + ".pkl") for sfx in ("_noILD", "_ILD", "_ILD_extra_mse")]
    assert all(f.is_file() for f in files) and not (out / "models" / (name + ".pkl")).exists()
    with open(str(out / "models" / ("loss_" + name + ".data")), "rb") as fh:
        losses = pickle.load(fh)
    assert len(losses) == 3 and np.isfinite(losses).all()
    for s in sources:
        sr, wav = scipy.io.wavfile.read(str(out / "output" / name / "Sources" / "Dev" / song / (s + ".wav")))
        assert sr == 44100 and wav.shape == (n, 2)

    data = StereoFeatureWindows([str(db / "transforms" / "feature_folder")], 30, 25, 0.3, 0.3, 'all', 4, 0)
    saved = [load_model(str(f)) for f in files]

    def twin(stage3_fresh):
        t = StereoTrainer(batch_size=4, time_context=30, feat_size=data.F, seed=0)
        gen = torch.Generator(device=t.ctx.device)
        gen.manual_seed(0)
        losser, epoch = [], [0]

        def run(count, ild, record):
            for _ in range(count):
                err = 0.0
                for xb, tb in data.batches(epoch[0]):
                    with t.ctx.stream_scope():
                        rr = torch.randn(t.rand_shape, generator=gen, device=t.ctx.device, dtype=torch.float32) * RAND_STD
                    t.set_rand(rr)
                    err += t.step(xb, tb, ild=ild)
                epoch[0] += 1
                if record:
                    losser.append(err / data.iteration_size)

        run(2, False, True)
        p1, kept = t.params(), t.optimizer_state()
        t.set_optimizer('adadelta')
        run(1, True, True)
        p2 = t.params()
        if stage3_fresh:
            t.set_optimizer('adadelta')
        else:
            t.load_optimizer_state(kept)
        run(2, False, False)
        p3 = t.params()
        t.close()
        return losser, p1, p2, p3

    losser, p1, p2, p3 = twin(False)
    assert losser == losses
    assert _same(p1, saved[0]) and _same(p2, saved[1]) and _same(p3, saved[2])
    assert not _same(twin(True)[3], saved[2])
