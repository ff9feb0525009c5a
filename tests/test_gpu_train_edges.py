"""The three HIP trainers (csrc/train_core.hip, train_dsd.hip on train_dsd_graph.hip, train_ca.hip with train_ikala.hip and train_bach10.hip) where
a training run goes and the template of test_gpu_train*.py does not: exact zeros and ties at every site that carries Theano's conventions, the
ends of the accepted shape ranges and the split-K regimes behind them, non-default hyper-parameters, and Adadelta on a live
state -- each against the float64 restatements, gradients by norm and by element (tests/train_edges.py).  The controls that
show these cases can fail are in tests/test_train_edges_cpu.py."""
import numpy as np
import pytest
import torch

import train_edges as E
import train_ref

pytestmark = pytest.mark.gpu

GRAPH_NAMES = sorted(E.GRAPHS)


def _trainer_kw(graph, hyper):
    """Keywords of the restatement -> keywords of Trainer (iKala's beta_acc travels as ``beta``)."""
    return {("beta" if k == "beta_acc" else k): v for k, v in hyper.items()}


def _trainer(graph, params, r, **kw):
    from deepconvsep_amd.training import Trainer
    B, _, tc, F = r.shape
    return Trainer(arch=E.GRAPHS[graph].arch, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, **kw)


def _compare(graph, params, x, r, tgt, hyper=None, label="", **trainer_kw):
    """Loss, components and every gradient of one call against float64: rtol 1e-5 on the values, 1e-4 relative norm and the
    elementwise bound of train_edges.check_gradients per gradient.  Returns (trainer, float64 values, float64 gradients)."""
    g = E.GRAPHS[graph]
    hyper = dict(hyper or {})
    want, g64 = g.ref.loss_and_grads(params, x, tgt, r, **hyper)
    _, g32 = g.ref.loss_and_grads(params, x, tgt, r, dtype=torch.float32, **hyper)
    kw = _trainer_kw(graph, hyper)
    kw.update(trainer_kw)
    t = _trainer(graph, params, r, **kw)
    out, grads = t.loss_and_gradients(x, tgt)
    print(label, "out7", out, "float64", want)
    assert len(grads) == g.nparams and not out[g.ncomp:].any()
    np.testing.assert_allclose(out[:g.ncomp], want, rtol=1e-5)
    E.check_gradients(grads, g64, g32, x.shape[0], label)
    # b1 / b1b and b2 / b2b get identical gradients (Theano)
    assert np.array_equal(grads[1], grads[2]) and np.array_equal(grads[4], grads[5])
    n = g.ncomp - 1
    assert t.losses(x, tgt) == pytest.approx(list(want[1:1 + n]), rel=1e-5)
    return t, want, g64


# ---------------------------------------------------------------------------------------------- B. exact zeros and ties
@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("case", E.TIE_CASES)
def test_exact_zero_at_one_site(graph, case):
    """r'(0) = 0.5 on the device at the site ``case`` zeroes (train_edges.tie_case): the GEMM epilogue's EPI_DRELU behind the
    branch layers, the r' of z (the epilogue on DSD, finish_kernel after the split-K sum on iKala and Bach10), the loss
    kernels' q == 0 branch.  The q0 case keeps r >= 0.01 and runs Bach10 at eps = 1e-6 instead of its 1e-18, so that dE/dq ~
    x t / (eps r) stays finite in float32.  test_train_edges_cpu.py shows that 0 or 1 in place of 0.5 moves the gradients named
    there by 100 % and more."""
    params, x, r, tgt, hyper = E.tie_case(graph, case)
    t, _, g64 = _compare(graph, params, x, r, tgt, hyper, "%s %s" % (graph, case))
    assert all(np.isfinite(a).all() for a in t.gradients())
    t.close()


@pytest.mark.parametrize("graph,shape,rows", [("dsd", (7, 10, 33), (1, 4, 5)), ("ikala", (5, 12, 93), (0, 3)),
                                              ("bach10", (5, 6, 37), (2, 4))])
def test_zero_windows_among_live_rows(graph, shape, rows):
    """Some rows of the batch are what a zero slot of the feed gives (inputs and targets zero), the rest well conditioned."""
    params, x, r, tgt = E.setup(graph, *shape, seed=11)
    x, tgt = E.zero_rows(x, tgt, rows)
    t, _, _ = _compare(graph, params, x, r, tgt, label="%s zero rows" % graph)
    t.close()


@pytest.mark.parametrize("graph", GRAPH_NAMES)
def test_all_zero_batch(graph):
    """A batch of zero slots only: the loss and every component are exactly 0, sign(E) = 0 and every gradient is exactly
    zero; ``step`` leaves the parameters bit-identical and both Adadelta accumulators exactly zero."""
    g = E.GRAPHS[graph]
    params, x, r, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=5)
    x, tgt = np.zeros_like(x), np.zeros_like(tgt)
    t = _trainer(graph, params, r)
    out, grads = t.loss_and_gradients(x, tgt)
    assert not out.any(), out
    assert not any(a.any() for a in grads), [i for i, a in enumerate(grads) if a.any()]
    before = t.params()
    for _ in range(2):
        assert t.step(x, tgt) == 0.0
    for i, (a, b, p) in enumerate(zip(t.params(), before, params)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a, p), i
    accu, delta = t.adadelta_state()
    assert not any(a.any() for a in accu) and not any(a.any() for a in delta)
    assert len(before) == g.nparams
    t.close()


def test_bach10_zero_over_zero_stays_nan():
    """All four outputs zero at an element whose draw r is exactly 0: the reference's 0 / 0, in the configuration of the q0
    case (eps 1e-6; eps r = 0 whatever eps is).  The NaN is kept, in float64 and on the device; nothing else is compared."""
    params, x, r, tgt, hyper = E.tie_case("bach10", "q0")
    r[0, 0, 0, 0] = 0.0
    want, _ = E.GRAPHS["bach10"].ref.loss_and_grads(params, x, tgt, r, **hyper)
    assert np.isnan(want[0])
    t = _trainer("bach10", params, r, **hyper)
    out = t.ctx.to_host(t.run(x, tgt, 0)).copy()
    assert np.isnan(out[0]), out
    t.close()


# ---------------------------------------------------------------------------------------------- C. the ends of the ranges
@pytest.mark.parametrize("graph,shape", [(g, s) for g in GRAPH_NAMES for s in E.EDGE_SHAPES[g]])
def test_edges_of_the_accepted_ranges(graph, shape):
    """One gradient-and-loss case at every bound of the trainer's range check, and the shapes that take every split-K GEMM
    through K < 32, K < 256, one slice, a short last slice, a last slice that is no multiple of the K step of 32, and the
    slice cap (the table is printed here and asserted complete in test_train_edges_cpu.py).  The float64 autograd of the
    largest of them takes a few seconds on the CPU, so every bound is checked against float64 itself."""
    for name, splits, kc, K, rem, hit in E.regimes(graph, *shape):
        print("%s %r %s (splits, kchunk, K, K %% kchunk) = (%d, %d, %d, %d) %s" % (graph, shape, name, splits, kc, K, rem,
                                                                                 ", ".join(sorted(hit))))
    B, tc, F = shape
    params, x, r, tgt = E.setup(graph, B, tc, F, seed=B + tc + F)
    t, _, _ = _compare(graph, params, x, r, tgt, label="%s %r" % (graph, shape))
    t.close()


RANGE_MESSAGE = r"time_context -?\d+ \(.*\), F -?\d+ \(.*\), batch -?\d+ \(1 \.\. 1024\)"


def _create_without_parameters(graph, B, tc, F):
    """dcs_trainer_create with a one-element draw and no parameters at all: the range check of the graph's *_trainer_new
    runs first and reads no memory; a shape it accepts comes back as the parameter-count error that follows it."""
    from ctypes import c_double, c_void_p, byref
    from deepconvsep_amd import _lib
    from deepconvsep_amd.arch import ARCHS
    from deepconvsep_amd.runtime import _ptr, default_context
    ctx = default_context()
    with ctx.stream_scope():
        draw = torch.zeros(1, dtype=torch.float32, device=ctx.device)
    hyper = (c_double * 7)(1e-8, 0.001, 0.01, 0.03, 1.0, 0.95, 1e-6)
    h = c_void_p()
    _lib.check(ctx._lib.dcs_trainer_create(ctx._h, ARCHS[E.GRAPHS[graph].arch].code, tc, F, B, None, None, 0, _ptr(draw),
                                           hyper, byref(h)))
    return h


@pytest.mark.parametrize("graph", GRAPH_NAMES)
def test_one_step_past_each_bound_is_a_value_error(graph):
    """Every shape one step past a bound is refused by the range check itself (its message, not the parameter-shape or
    null-argument errors that would follow), and the same call one step inside passes it.  The entry point is called
    without parameters, so that batch 0 and F 0 reach the check too; where Trainer can build the call (parameters shaped for
    the refused shape), it raises the same message."""
    from deepconvsep_amd import training
    from deepconvsep_amd.training import Trainer
    g = E.GRAPHS[graph]
    lo, hi = {"dsd": ((1, 4, 1), (1024, 64, 2049)), "ikala": ((1, 10, 87), (1024, 64, 2049)),
              "bach10": ((1, 2, 30), (1024, 47, 2049))}[graph]
    for B, tc, F in E.BAD_SHAPES[graph]:
        with pytest.raises(ValueError, match=RANGE_MESSAGE):
            _create_without_parameters(graph, B, tc, F)
        # one step inside on the axis that was out of range: the range check passes, the parameter count is refused next
        inside = tuple(min(max(v, a), b) for v, a, b in zip((B, tc, F), lo, hi))
        if graph == "dsd" and inside[1] % 2:
            inside = (inside[0], inside[1] - 1, inside[2])
        assert inside != (B, tc, F)
        with pytest.raises(ValueError, match="got 0 values to set %d parameters" % g.nparams):
            _create_without_parameters(graph, *inside)
        try:
            params = training.glorot_init(g.arch, tc, F)
        except Exception:
            continue
        if B < 1 or any(p.size == 0 for p in params):
            continue
        with pytest.raises(ValueError, match=RANGE_MESSAGE):
            Trainer(arch=g.arch, params=params, batch_size=B, time_context=tc, feat_size=F, rand=np.zeros((B, 1, tc, F)))


# ---------------------------------------------------------------------------------------------- D. hyper-parameters
def _one_update_bounds(graph, t, params, g64, lr, rho, epsilon):
    """The bounds of test_gpu_train.py::test_one_update_matches_float64 (|du/dg| <= 1 for any rho and epsilon)."""
    zeros = [np.zeros(p.shape) for p in params]
    P64, A64, D64 = train_ref.adadelta(params, g64, zeros, zeros, lr=lr, rho=rho, eps=epsilon)
    P = t.params()
    A, D = t.adadelta_state()
    for i in range(len(params)):
        bound = 1e-4 * np.linalg.norm(g64[i]) + 6e-8 * np.linalg.norm(P64[i]) + 1e-12
        assert np.linalg.norm(P[i] - P64[i]) <= bound, (i, np.linalg.norm(P[i] - P64[i]), bound)
        assert E.rel(A[i], A64[i]) <= 3e-4 or np.linalg.norm(A64[i]) < 1e-30, i
        assert E.rel(D[i], D64[i]) <= 3e-4 or np.linalg.norm(D64[i]) < 1e-30, i


@pytest.mark.parametrize("graph", GRAPH_NAMES)
def test_all_seven_hyper_parameters_non_default(graph):
    """eps, alpha, beta (iKala: Trainer's ``beta`` is beta_acc), beta_voc, learning_rate, rho, epsilon all set to
    train_edges.HYPER: loss, components and gradients, then one update.  test_train_edges_cpu.py shows that exchanging any
    two of the loss hyper-parameters moves a component by more than 100 x the tolerance."""
    g = E.GRAPHS[graph]
    params, x, r, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=8)
    eps, alpha, beta, beta_voc, lr, rho, epsilon = E.HYPER
    hyper = dict(zip(g.hyper_names, E.HYPER[:4]))
    kw = dict(eps=eps, alpha=alpha, beta=beta, beta_voc=beta_voc, learning_rate=lr, rho=rho, epsilon=epsilon)
    t, want, g64 = _compare(graph, params, x, r, tgt, hyper, "%s hyper" % graph, **kw)
    dflt, _ = g.ref.loss_and_grads(params, x, tgt, r)
    assert (np.abs(dflt - want) / np.abs(want)).max() > 1e-3      # the defaults would show
    assert t.step(x, tgt) == pytest.approx(want[0], rel=1e-5)
    _one_update_bounds(graph, t, params, g64, lr, rho, epsilon)
    t.close()


def test_bach10_ignores_alpha_beta_and_beta_voc():
    """The Bach10 loss has no such terms: two trainers that differ in them give bit-identical values, gradients and
    updated parameters."""
    params, x, r, tgt = E.setup("bach10", *E.TIE_SHAPES["bach10"], seed=8)
    res = []
    for kw in ({}, dict(alpha=0.07, beta=0.2, beta_voc=0.11)):
        t = _trainer("bach10", params, r, eps=2e-3, **kw)
        out, grads = t.loss_and_gradients(x, tgt)
        t.step(x, tgt)
        res.append([out] + grads + t.params())
        t.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------- E. Adadelta on a live state
U = 2.0 ** -24       # float32 unit roundoff: one correctly rounded operation has relative error <= U
TINY = 2.0 ** -126   # below it float32 products lose relative precision (g^2 and u^2 of vanishing gradients)


@pytest.mark.parametrize("graph,shape", [("dsd", (3, 10, 33)), ("ikala", (2, 12, 93)), ("bach10", (3, 6, 37))])
def test_adadelta_kernel_on_a_live_state(graph, shape):
    """train::adadelta_kernel alone: five steps with non-default learning_rate, rho, epsilon; after each one the float64
    lasagne.updates.adadelta is fed the *device's* previous parameters and state and the *device's* gradient, so the
    gradient error is out of the comparison and what remains is the float32 rounding of the kernel's own operations, each
    correctly rounded (hipcc's default division and sqrtf), relative error <= U = 2^-24 apiece, contraction to FMA only
    removing roundings.  With the float32 values of learning_rate, rho, epsilon on both sides (1 - rho is exact):

        a' = rho a + (1 - rho) g g        g g: U, (1 - rho) .: 2 U, rho a: U, the sum of two non-negative terms: 3 U
        u  = g sqrt(d + e) / sqrt(a' + e) a' + e: 4 U, its root: 2 U + U = 3 U; d + e: U, its root: 1.5 U, times g: 2.5 U;
                                          the quotient: 2.5 + 3 + 1 = 6.5 U
        p' = p - lr u                     lr u: 7.5 U of |lr u|, the difference: half an ulp of p'
        d' = rho d + (1 - rho) u u        u u: 14 U, (1 - rho) .: 15 U, rho d: U, the sum of non-negative terms: 16 U

    Asserted, elementwise: |a' - a'64| <= 4 U a'64, |d' - d'64| <= 17 U d'64 (one U above the first-order count for the
    higher-order terms), |p' - p'64| <= 8 U |lr u64| + ulp(p') / 2; each plus 4 x 2^-126 for products that underflow.
    DSD at (3, 10, 33) has a parameter count of 2 modulo 4: the flat state ends in a pad of two floats, which must stay
    out of what is fetched (the last parameter, the output bias, is compared like every other)."""
    g = E.GRAPHS[graph]
    lr, rho, epsilon = [float(np.float32(v)) for v in E.HYPER[4:]]
    assert float(np.float32(1) - np.float32(rho)) == 1.0 - rho
    params, x, r, tgt = E.setup(graph, *shape, seed=13)
    x2, tgt2 = E.setup(graph, *shape, seed=14)[1::2]
    count = sum(p.size for p in params)
    if graph == "dsd":
        assert count % 4 == 2
    t = _trainer(graph, params, r, learning_rate=lr, rho=rho, epsilon=epsilon)
    P0 = t.params()
    A0, D0 = t.adadelta_state()
    assert all(np.array_equal(a, b) for a, b in zip(P0, params))
    assert not any(a.any() for a in A0 + D0)
    worst = {"accu": 0.0, "delta": 0.0, "param": 0.0}
    for step in range(5):
        xb, tb = (x, tgt) if step % 2 == 0 else (x2, tgt2)
        t.step(xb, tb)
        G = t.gradients()
        P1 = t.params()
        A1, D1 = t.adadelta_state()
        P64, A64, D64 = train_ref.adadelta(P0, G, A0, D0, lr=lr, rho=rho, eps=epsilon)
        for i in range(g.nparams):
            assert P1[i].shape == params[i].shape and A1[i].shape == params[i].shape and D1[i].shape == params[i].shape
            assert np.isfinite(P1[i]).all() and (A1[i] >= 0).all() and (D1[i] >= 0).all()
            lru = np.abs(np.asarray(P0[i], np.float64) - P64[i])
            ea = np.abs(A1[i] - A64[i]) - 4 * TINY
            ed = np.abs(D1[i] - D64[i]) - 4 * TINY
            ep = np.abs(P1[i] - P64[i]) - 4 * TINY - 0.5 * np.spacing(np.abs(P1[i])).astype(np.float64)
            worst["accu"] = max(worst["accu"], float((ea / np.maximum(A64[i], TINY)).max()) / U)
            worst["delta"] = max(worst["delta"], float((ed / np.maximum(D64[i], TINY)).max()) / U)
            worst["param"] = max(worst["param"], float((ep / np.maximum(lru, TINY)).max()) / U)
            assert (ea <= 4 * U * A64[i]).all(), (step, i, "accu", worst)
            assert (ed <= 17 * U * D64[i]).all(), (step, i, "delta_accu", worst)
            assert (ep <= 8 * U * lru).all(), (step, i, "param", worst)
        if step:
            assert any(d.any() for d in D0)      # the state the numerator reads is live from the second step on
        P0, A0, D0 = P1, A1, D1
    print("%s: worst errors in units of U = 2^-24: accu %.2f (bound 4), delta_accu %.2f (17), parameters beyond half an "
          "ulp %.2f of |lr u| (8)" % (graph, worst["accu"], worst["delta"], worst["param"]))
    t.close()
