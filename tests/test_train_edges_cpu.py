"""The checks that keep tests/test_gpu_train_feed.py and tests/test_gpu_train_edges.py honest (CPU only): the NumPy feed
against the reference's loadFile, the exact-zero constructions against the two rectifier conventions a kernel could carry by
mistake, the hyper-parameter case against swapped hyper-parameters, and the table of split-K regimes the edge shapes visit."""
import numpy as np
import pytest
import torch

import feed_ref
import train_edges as E
import train_ref
from deepconvsep_amd import training


# ---------------------------------------------------------------------------------------------- A. the feed
def _feed_cases(g):
    for k, (T, tc, ov, nsrc, F, mult) in enumerate(g["cases"]):
        yield k, int(T), int(tc), int(ov), int(nsrc), int(F), float(mult)


def test_feed_ref_matches_loadfile(golden):
    """gather_np over reference_slots against the inputs / outputs loadFile returned (tests/golden/train_feed.npz).  Equal
    where the scale is a power of two; otherwise within one float32 ulp, because loadFile multiplies in float64 and then
    narrows while the feed narrows the file first (two roundings against one)."""
    g = golden("train_feed")
    seen = set()
    for k, T, tc, ov, nsrc, F, mult in _feed_cases(g):
        data = feed_ref.data_pattern(nsrc, T, F)
        slots = training.reference_slots(T, tc, ov)
        rows = [(0, s) if s is not None else (-1, 0) for s in slots]
        x, t = feed_ref.gather_np([data], rows, tc, F, nsrc, mult)
        want_x, want_t = g["inputs_%d" % k], g["outputs_%d" % k]
        assert x[:, 0].shape == want_x.shape and want_t.shape == (len(rows), tc, nsrc * F)
        got_t = feed_ref.reference_layout(t)
        if np.log2(mult) == np.round(np.log2(mult)):
            assert np.array_equal(x[:, 0], want_x) and np.array_equal(got_t, want_t), k
            seen.add("power of two")
        else:
            assert (np.abs(x[:, 0] - want_x) <= np.spacing(np.abs(want_x))).all(), k
            assert (np.abs(got_t - want_t) <= np.spacing(np.abs(want_t))).all(), k
            seen.add("one ulp")
        # the cases the fixture must hold
        if tc > T:
            assert x[0, 0, T - 1].all() and not x[0, 0, T:].any() and not t[0, :, T:].any()
            seen.add("padded")
        if T == tc:
            assert len(rows) == 1 and rows[0][0] == -1 and not want_x.any() and not want_t.any()
            seen.add("T == tc")
        if T == tc + 1:
            assert rows == [(0, 0)]
            seen.add("T == tc + 1")
        if any(r[0] < 0 for r in rows) and any(r[0] >= 0 for r in rows):
            seen.add("zero slot beside windows")
        seen.add("%d sources" % nsrc)
    assert seen >= {"power of two", "one ulp", "padded", "T == tc", "T == tc + 1", "zero slot beside windows", "2 sources",
                    "4 sources"}, seen


def test_feed_pattern_is_exact_in_float32_and_distinct():
    a = feed_ref.data_pattern(4, 61, 7)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and len(np.unique(a)) == a.size


def test_gather_np_pads_zero_slots_and_layout():
    a, b = feed_ref.data_pattern(2, 5, 3), feed_ref.data_pattern(2, 9, 3, offset=5000)
    x, t = feed_ref.gather_np([a, b], [(1, 4), (-1, 0), (0, 3)], 4, 3, 2, 2.0)
    assert np.array_equal(x[0, 0], 2 * b[0, 4:8]) and np.array_equal(t[0, 1], 2 * b[2, 4:8])
    assert not x[1].any() and not t[1].any()
    assert np.array_equal(x[2, 0, :2], 2 * a[0, 3:5]) and not x[2, 0, 2:].any() and not t[2, :, 2:].any()
    assert np.array_equal(feed_ref.reference_layout(t)[0, :, 3:6], t[0, 1])


# ---------------------------------------------------------------------------------------------- B. exact zeros and ties
def test_relu_tie_switch():
    v = torch.tensor([-1.0, 0.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    for d in (0.0, 0.5, 1.0):
        with train_ref.relu_tie(d):
            y = train_ref.rectify(v)
            (gr,) = torch.autograd.grad(y.sum(), v)
        assert y.tolist() == [0.0, 0.0, 0.0, 2.0] and gr.tolist() == [0.0, d, d, 1.0]
    (gr,) = torch.autograd.grad(train_ref.rectify(v).sum(), v)
    assert gr.tolist() == [0.0, 0.5, 0.5, 1.0]


# which parameters each construction must move (by 100 % or more) under the other two conventions
TIE_PARAMS = {"branch0": lambda g: g.branch, "fc0": lambda g: [6, 7], "q0": lambda g: g.branch + [g.bo]}


@pytest.mark.parametrize("graph", sorted(E.GRAPHS))
@pytest.mark.parametrize("case", E.TIE_CASES)
def test_tie_cases_tell_the_conventions_apart(graph, case):
    """Non-vacuity of the device tie tests: in float64, r'(0) = 0 and r'(0) = 1 each move at least the named parameters'
    gradients by 100 x the device bound (1e-4 relative norm), here by 100 % and more, and every gradient stays finite."""
    g = E.GRAPHS[graph]
    params, x, r, tgt, hyper = E.tie_case(graph, case)
    out, g_half = g.ref.loss_and_grads(params, x, tgt, r, **hyper)
    assert np.isfinite(out).all() and all(np.isfinite(a).all() for a in g_half)
    if case == "q0":
        with torch.no_grad():
            assert not g.ref.forward([train_ref._t(p) for p in params], train_ref._t(x)).any() and x.all()
    for tie in (0.0, 1.0):
        _, g_other = g.ref.loss_and_grads(params, x, tgt, r, tie=tie, **hyper)
        moved = {i: E.rel(g_other[i], g_half[i]) for i in range(g.nparams) if np.linalg.norm(g_half[i]) > 0}
        print(graph, case, "r'(0) = %g moves" % tie, {i: "%.3g" % v for i, v in moved.items() if v > 0})
        for i in TIE_PARAMS[case](g):
            assert np.linalg.norm(g_half[i]) > 0, (tie, i)
            assert moved[i] >= 100 * E.NORM_BOUND and moved[i] >= 0.99, (tie, i, moved[i])


@pytest.mark.parametrize("graph", sorted(E.GRAPHS))
def test_all_zero_batch_is_exactly_zero_in_float64(graph):
    g = E.GRAPHS[graph]
    params, x, r, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=5)
    out, grads = g.ref.loss_and_grads(params, np.zeros_like(x), np.zeros_like(tgt), r)
    assert not out.any() and not any(a.any() for a in grads)


def test_bach10_zero_over_zero_is_nan_in_float64():
    params, x, r, tgt, hyper = E.tie_case("bach10", "q0")
    r[0, 0, 0, 0] = 0.0
    out, _ = E.GRAPHS["bach10"].ref.loss_and_grads(params, x, tgt, r, **hyper)
    assert np.isnan(out[0])


# ---------------------------------------------------------------------------------------------- C. the ends of the ranges
@pytest.mark.parametrize("graph", sorted(E.GRAPHS))
def test_edge_shapes_visit_every_split_regime(graph, capsys):
    seen = set()
    with capsys.disabled():
        print("\n%s: (B, tc, F) gemm (splits, kchunk, K, K %% kchunk) regimes" % graph)
        for shp in E.EDGE_SHAPES[graph]:
            for name, splits, kc, K, rem, hit in E.regimes(graph, *shp):
                print("  %-16r %-4s (%3d, %5d, %7d, %5d) %s" % (shp, name, splits, kc, K, rem, ", ".join(sorted(hit))))
                seen |= hit
    assert seen == set(E.REGIMES), set(E.REGIMES) - seen
    # the cap the graph's plan() names is reached exactly: 64 (DSD), 128 (iKala), 512 (Bach10)
    most = max(row[1] for shp in E.EDGE_SHAPES[graph] for row in E.regimes(graph, *shp))
    caps = {cap for _, _, _, cap in E.split_gemms(graph, 1, E.TIE_SHAPES[graph][1], E.TIE_SHAPES[graph][2]).values()}
    assert most == E.CAPS[graph] == max(caps), (most, caps)


def test_pick_split_restatement_on_known_plans():
    """The figures of the issue's own restatement for DSD: K = 16, 24, 72, 168; (7, 10, 65) has two slices with a last slice
    of 24 and (2, 64, 33) one of 8; and the plans the source comments state (iKala dW2 at B = 32: 47 row tiles)."""
    ks = {row[3] for shp in E.EDGE_SHAPES["dsd"] for row in E.regimes("dsd", *shp)}
    assert {16, 24, 72, 168} <= ks
    assert [r[:5] for r in E.regimes("dsd", 7, 10, 65)][0] == ("dW1", 2, 256, 280, 24)
    assert [r[:5] for r in E.regimes("dsd", 2, 64, 33)][1] == ("dW2", 2, 256, 264, 8)
    assert E.split_gemms("ikala", 32, 30, 513)["dW2"][0] == 47
    assert E.pick_split(1, 10, 512, 64) == (1, 32) and E.pick_split(1, 300, 512, 64) == (2, 256)


def test_edge_shapes_hold_every_bound():
    for graph, lo, hi in (("dsd", (1, 4, 1), (1024, 64, 2049)), ("ikala", (1, 10, 87), (1024, 64, 2049)),
                          ("bach10", (1, 2, 30), (1024, 47, 2049))):
        for axis in range(3):
            vals = {s[axis] for s in E.EDGE_SHAPES[graph]}
            assert lo[axis] in vals and hi[axis] in vals, (graph, axis)
            bad = {s[axis] for s in E.BAD_SHAPES[graph]}
            step = 2 if (graph, axis) == ("dsd", 1) else 1     # DSD's time_context is even
            assert lo[axis] - step in bad and hi[axis] + step in bad, (graph, axis)
    assert {3, 47} <= {s[1] for s in E.EDGE_SHAPES["bach10"]} and 31 in {s[2] for s in E.EDGE_SHAPES["bach10"]}


# ---------------------------------------------------------------------------------------------- D. hyper-parameters
@pytest.mark.parametrize("graph", ["dsd", "ikala"])
def test_swapped_loss_hyper_parameters_show(graph):
    """Control of the device hyper-parameter case: exchanging any two of eps, alpha, beta (beta_acc), beta_voc in the float64
    restatement moves at least one of the reported values by more than 100 x the device tolerance (1e-5 relative)."""
    g = E.GRAPHS[graph]
    params, x, r, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=8)
    hyper = dict(zip(g.hyper_names, E.HYPER[:4]))
    base, _ = g.ref.loss_and_grads(params, x, tgt, r, **hyper)
    names = list(g.hyper_names)
    for i in range(4):
        for j in range(i + 1, 4):
            sw = dict(hyper)
            sw[names[i]], sw[names[j]] = hyper[names[j]], hyper[names[i]]
            out, _ = g.ref.loss_and_grads(params, x, tgt, r, **sw)
            move = np.abs(out - base) / np.abs(base)
            print(graph, names[i], "<->", names[j], "moves", move)
            assert move.max() > 100 * 1e-5, (names[i], names[j], move)
    dflt, _ = g.ref.loss_and_grads(params, x, tgt, r)
    assert (np.abs(dflt - base) / np.abs(base)).max() > 100 * 1e-5


def test_bach10_eps_shows_and_nothing_else_exists():
    """Bach10's loss reads eps alone: the non-default eps moves every value by more than 100 x the tolerance, and the
    restatement takes no alpha / beta / beta_voc at all."""
    g = E.GRAPHS["bach10"]
    params, x, r, tgt = E.setup("bach10", *E.TIE_SHAPES["bach10"], seed=8)
    base, _ = g.ref.loss_and_grads(params, x, tgt, r, eps=E.HYPER[0])
    dflt, _ = g.ref.loss_and_grads(params, x, tgt, r)
    assert (np.abs(dflt - base) / np.abs(base)).min() > 100 * 1e-5
    with pytest.raises(TypeError):
        g.ref.loss_and_grads(params, x, tgt, r, alpha=0.07)


def test_hyper_values_are_distinct_and_not_the_defaults():
    dflt = {training.EPS, training.ALPHA, training.BETA, training.BETA_VOC, training.LEARNING_RATE, training.RHO,
            training.ADA_EPSILON, training.IKALA_ALPHA, training.IKALA_BETA_ACC, training.IKALA_BETA_VOC,
            training.BACH10_EPS}
    assert len(set(E.HYPER)) == 7 and not set(E.HYPER) & dflt


def test_adadelta_restatement_on_a_live_state():
    """delta_accu enters the numerator: from a non-zero state the update differs from the zero-state one."""
    g, a, d = [np.array([0.3, -2.0])], [np.array([0.5, 0.1])], [np.array([0.2, 0.4])]
    P, A, D = train_ref.adadelta([np.ones(2)], g, a, d, lr=0.5, rho=0.9, eps=1e-3)
    a1 = 0.9 * a[0] + 0.1 * g[0] ** 2
    u = g[0] * np.sqrt(d[0] + 1e-3) / np.sqrt(a1 + 1e-3)
    np.testing.assert_allclose(P[0], 1 - 0.5 * u, rtol=1e-15)
    np.testing.assert_allclose(A[0], a1, rtol=1e-15)
    np.testing.assert_allclose(D[0], 0.9 * d[0] + 0.1 * u * u, rtol=1e-15)
