"""Score-informed Bach10 trainer: the float64 restatement (tests/train_si_ref.py) against the inference oracle and the
reference's own loss lines, the dead-parameter rule, the two layouts against each other, the NumPy feed (tests/
score_feed_ref.py) against the reference's loadFile + filterSpec + products, and Lasagne's initialisation (CPU only)."""
import numpy as np
import pytest
import torch

import score_feed_ref
import train_ref
import train_si_ref
from deepconvsep_amd import score_training, training
from deepconvsep_amd.arch import ARCHS
from oracle import net_ref


def _case(B, tc, F, seed, branches=4):
    rs = np.random.RandomState(seed)
    params = score_training.glorot_init(tc, F, seed, branches)
    last = len(params) - 1
    for i in [1, 2, 4, 5, 7] + list(range(9, last, 2)):
        params[i] = (0.05 * rs.randn(*params[i].shape)).astype(np.float32)
    params[last] = np.float32(0.1) + np.abs(0.05 * rs.randn(*params[last].shape)).astype(np.float32)
    x = (0.3 * rs.uniform(0, 0.25, size=(B, 4, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, 4, tc, F))).astype(np.float32)
    return params, x, r, tgt


@pytest.mark.parametrize("tc,F", [(30, 33), (2, 34), (3, 30), (9, 65)])
@pytest.mark.parametrize("arch", ["bach10_si", "bach10_si1"])
def test_forward_equals_net_ref(arch, tc, F):
    """The tolerance of test_train_bach10_cpu.py for the same comparison."""
    rs = np.random.RandomState(tc + F)
    branches = 4 if arch == "bach10_si" else 1
    params = score_training.glorot_init(tc, F, seed=1, branches=branches)
    params[-1] = np.abs(rs.randn(4 * branches)).astype(np.float32)
    x = rs.uniform(0, 1, size=(2, 4, tc, F))
    p = train_si_ref.forward_np(params, x)
    want = net_ref.forward(arch, params, x).numpy()
    assert p.shape == want.shape == (2, 4 * branches, tc, F)
    np.testing.assert_allclose(p, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())


def test_loss_and_components_match_the_reference_lines(golden):
    g = golden("train_si_loss")
    t = lambda k: torch.as_tensor(g[k])  # noqa: E731
    assert g["p"].shape[1] == 16 and g["x"].shape[1] == 4
    assert (g["p"][:, 4:] > 0).all()             # the dead channels are non-zero: they do not matter
    assert not g["p"][0, 0:4, 0, 0].any()        # the element whose masks are 0 / (eps r)
    got = np.array([float(v) for v in train_si_ref.components(t("p"), t("x"), t("tgt"), t("r"))])
    want = np.array([float(g[k]) for k in ("loss", "error1", "error2", "error3", "error4")])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert np.isclose(got[0], got[1:].sum(), rtol=1e-14)
    # the same from the live channels alone
    got4 = np.array([float(v) for v in train_si_ref.components(t("p")[:, 0:4], t("x"), t("tgt"), t("r"))])
    assert np.array_equal(got, got4)


def test_dead_parameters_get_zero_gradients_and_adadelta_leaves_them():
    params, x, r, tgt = _case(2, 9, 65, seed=3)
    out, g = train_si_ref.loss_and_grads(params, x, tgt, r)
    assert out[0] > 0
    for i in train_si_ref.DEAD:
        assert np.linalg.norm(params[i]) > 0 and not g[i].any(), i
    assert not g[16][4:].any() and g[16][:4].all()
    for i in list(range(10)):
        assert np.linalg.norm(g[i]) > 0, i
    zeros = [np.zeros(p.shape) for p in params]
    P, A, D = train_ref.adadelta(params, g, zeros, [z.copy() for z in zeros])
    for i in train_si_ref.DEAD:
        assert np.array_equal(P[i], np.asarray(params[i], np.float64)) and not A[i].any() and not D[i].any(), i
    assert np.array_equal(P[16][4:], np.asarray(params[16][4:], np.float64)) and not A[16][4:].any() and not D[16][4:].any()
    assert (P[16][:4] != params[16][:4]).all()


@pytest.mark.parametrize("B,tc,F", [(2, 9, 65), (1, 12, 93), (3, 3, 30)])
def test_the_two_layouts_agree(B, tc, F):
    params, x, r, tgt = _case(B, tc, F, seed=B + tc)
    out17, g17 = train_si_ref.loss_and_grads(params, x, tgt, r)
    out11, g11 = train_si_ref.loss_and_grads(train_si_ref.live(params), x, tgt, r)
    np.testing.assert_allclose(out11, out17, rtol=1e-12)
    live17 = train_si_ref.live(g17)
    assert len(g11) == 11
    for i, (a, b) in enumerate(zip(g11, live17)):
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), i
    # arch.live_params cuts the same arrays
    from deepconvsep_amd.arch import live_params
    arch, lp = live_params(ARCHS["bach10_si"], params)
    assert arch.name == "bach10_si1" and all(np.array_equal(a, b) for a, b in zip(lp, train_si_ref.live(params)))


def test_feed_ref_matches_loadfile_filterspec_and_products(golden):
    """gather_np over reference_slots against what the reference's loadFile (with LargeDatasetMask2.filterSpec) and
    trainCNNrwc.py:309-320 produced (tests/golden/train_si_feed.npz), bit for bit."""
    g = golden("train_si_feed")
    files, notes = score_feed_ref.fixture_files(), score_feed_ref.fixture_notes()
    tc, ov, F = score_feed_ref.TC, score_feed_ref.OVERLAP, score_feed_ref.F
    for k, (T, _, mult) in enumerate(score_feed_ref.FILES):
        rows = [(0, s) if s is not None else (-1, 0) for s in training.reference_slots(T, tc, ov)]
        x, t = score_feed_ref.gather_np([files[k]], [notes[k]], rows, tc, F, mult)
        assert x.dtype == np.float32 and x.shape == g["inputs_%d" % k].shape == (len(rows), 4, tc, F)
        assert np.array_equal(x, g["inputs_%d" % k]) and np.array_equal(t, g["targets_%d" % k]), k
    # the cases the fixture must hold
    rows = [(0, s) for s in training.reference_slots(24, tc, ov)]
    assert rows == [(0, 0), (0, 5), (0, 10), (0, 15)]
    m = np.stack([score_feed_ref.masks_np(notes[0], s, tc, tc, F) for _, s in rows])      # [window, inst, t, f]
    one, half, quarter = np.float32(1), np.float32(0.5), np.float32(0.25)
    assert m[1, 0, 0, 2] == one and m[1, 0, 3, 2] == one and m[1, 0, 4, 2] != one          # a note from before the window, ending in it
    assert m[0, 0, 4, 3] == half and m[0, 1, 4, 3] == half                                  # two instruments share a bin
    assert (m[2, :, 2:5] == quarter).all()                                                  # nobody plays: frames 12 .. 14
    assert (m[:, 3] < one).all() and (m[3, 2, 0:3, 0] == one).all()                         # an instrument without notes
    assert (m[3, :, 5:, 8:12] == quarter).all()                                             # MIDI 0 and the frameless note paint nothing
    assert score_feed_ref.FILES[1][0] < tc and not g["inputs_1"][0, :, 5:].any() and g["inputs_1"][0, :, 4].all()
    assert training.reference_slots(8, tc, ov) == [None] and not g["inputs_2"].any() and not g["targets_2"].any()
    # sums: the four masks add to one (float32), so the four inputs add to the scaled mixture within rounding
    x0 = g["inputs_0"].astype(np.float64).sum(axis=1)
    mix = 0.5 * np.stack([files[0][0, s:s + tc] for _, s in rows])
    np.testing.assert_allclose(x0, mix, rtol=3e-7)


def test_shapes_and_glorot_bounds_of_both_layouts():
    for branches, n in ((4, 17), (1, 11)):
        ps = score_training.glorot_init(30, 2049, seed=3, branches=branches) if branches == 1 else None
        shapes = score_training.param_shapes(30, 2049, branches)
        assert len(shapes) == n
        assert shapes[0] == (30, 4, 1, 30) and shapes[3] == (30, 30, 20, 1) and shapes[6] == (166650, 256)
        for i in range(8, n - 1, 2):
            assert shapes[i] == (256, 166650) and shapes[i + 1] == (166650,)
        assert shapes[-1] == (4 * branches,)
        assert shapes == [tuple(s) for s in ARCHS[score_training.arch_name(branches)].param_shapes(30, 2049)]
        if ps is None:      # the 17-array layout at a size that stays small
            ps = score_training.glorot_init(12, 93, seed=3, branches=4)
            shapes = score_training.param_shapes(12, 93, 4)
        assert [p.shape for p in ps] == shapes
        for p in ps:
            assert p.dtype == np.float32
            if p.ndim == 1:
                assert not p.any()
            else:
                rf = int(np.prod(p.shape[2:])) if p.ndim > 2 else 1
                a = np.sqrt(6.0 / ((p.shape[0] + p.shape[1]) * rf))
                assert np.abs(p).max() <= a and np.abs(p).max() > 0.9 * a
    with pytest.raises(ValueError):
        score_training.param_shapes(30, 2049, branches=2)
    assert score_training.COMPONENTS == ("bassoon", "clarinet", "saxophone", "violin") and score_training.SI_EPS == 1e-18


def test_the_mono_trainer_still_refuses_the_score_informed_graph():
    assert training.TRAINABLE == ("dsd", "ikala_nopool", "bach10")
    with pytest.raises(NotImplementedError):
        training.param_shapes("bach10_si", 30, 513)
    import deepconvsep_amd as dcs
    assert dcs.ScoreTrainer is score_training.ScoreTrainer and dcs.ScoreFeatureWindows is score_training.ScoreFeatureWindows
