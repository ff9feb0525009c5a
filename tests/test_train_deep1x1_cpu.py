"""The float64 restatement of the deep score-informed trainer (tests/train_deep1x1_ref.py) and the device-free parts of its
Python surface: no GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

import deep1x1_ref
import train_deep1x1_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def _worst(g, want):
    return max(_rel(a, b) for a, b in zip(g, want) if np.linalg.norm(b) > 0)


@pytest.fixture(scope="module")
def flip_case():
    """(B, tc, F, seed) = (2, 19, 253, 3): the case in which float32 and float64 disagree on the sign of one conv3 unit."""
    params, x, r, tgt = R.setup(2, 19, 253, seed=3)
    out64, g64, info64 = R.loss_and_grads(params, x, tgt, r)
    return params, x, r, tgt, out64, g64, info64


def test_forward_is_the_separators_oracle():
    for B, tc, F in ((2, 19, 253), (1, 20, 257)):
        params, x, _, _ = R.setup(B, tc, F, seed=1)
        want = deep1x1_ref.forward(params, x, branches=1)
        assert np.array_equal(R.forward_np(params, x), want)
        assert np.array_equal(R.forward_np(R.live(params), x), want)


def test_codes_of_a_float32_run_make_float64_agree(flip_case):
    """The two-part criterion on the restatement itself: float32 against float64 at float32's own codes agrees to float32's
    rounding, and its codes pass part 2.  Where a unit changes sign between the precisions (one conv3 unit at 1.5e-8 of its
    layer's maximum in this case, on the machine the criterion was worked out on), the plain comparison fails by far."""
    params, x, r, tgt, out64, g64, info64 = flip_case
    out32, g32, info32 = R.loss_and_grads(params, x, tgt, r, dtype=torch.float32)
    _, g64c, _ = R.loss_and_grads(params, x, tgt, r, codes=info32['codes'])
    at_codes, own = _worst(g32, g64c), _worst(g32, g64)
    ndiff = R.check_codes(info32['codes'], info64['pres'], "float32")
    print("float32 vs float64: at float32's codes %.2e, each at its own %.2e, %d units differ" % (at_codes, own, ndiff))
    assert at_codes <= 1e-5
    assert ndiff <= 1
    if ndiff == 0:
        assert own <= 1e-5
    np.testing.assert_allclose(out32, out64, rtol=1e-5)


def test_one_flipped_unit_moves_the_gradient_past_the_tolerance(flip_case):
    """Why part 1 runs at the device's codes: the conv3 unit nearest to zero, given the other sign, changes a gradient by more
    than the 1e-4 a kernel is allowed (the InverseLayer of conv3 multiplies by the code), while the loss stays within its 1e-5."""
    params, x, r, tgt, out64, g64, info64 = flip_case
    pre = info64['pres'][2]
    at = np.unravel_index(np.argmin(np.abs(pre)), pre.shape)
    assert abs(pre[at]) <= 1e-5 * np.abs(pre).max()
    codes = [c.copy() for c in info64['codes']]
    codes[2][at] = 1.0 - codes[2][at]
    out, g, _ = R.loss_and_grads(params, x, tgt, r, codes=codes)
    print("one flipped conv3 unit: gradient change %.2e" % _worst(g, g64))
    assert _worst(g, g64) > 1e-4
    np.testing.assert_allclose(out, out64, rtol=1e-5)


def test_own_codes_given_back_change_nothing(flip_case):
    params, x, r, tgt, out64, g64, info64 = flip_case
    out, g, _ = R.loss_and_grads(params, x, tgt, r, codes=info64['codes'])
    np.testing.assert_allclose(out, out64, rtol=1e-13)
    assert _worst(g, g64) <= 1e-12


def test_dead_rows_get_exactly_zero_gradient(flip_case):
    g64 = flip_case[5]
    for i in (18, 19, 20):
        assert not g64[i][200:].any() and g64[i][:200].any()
    assert not g64[21][4:].any() and g64[21][:4].all()
    # b_l and bb_l sit on opposite sides of a rectify
    for k in range(7):
        assert _rel(g64[3 * k + 1], g64[3 * k + 2]) > 1e-3


@pytest.mark.parametrize("w", [3, 18])
def test_the_tie_value_changes_the_gradient_of_a_zeroed_filter(w):
    params, x, r, tgt = R.setup(2, 19, 253, seed=12)
    params[w][7] = 0
    params[w + 1][7] = 0
    gs = [R.loss_and_grads(params, x, tgt, r, tie=tie)[1] for tie in (0.0, 0.5, 1.0)]
    assert not gs[0][w][7].any() and not gs[0][w + 1][7]
    assert np.linalg.norm(gs[1][w][7]) > 0
    np.testing.assert_allclose(gs[2][w][7], 2 * gs[1][w][7], rtol=1e-12)
    np.testing.assert_allclose(gs[2][w + 1][7], 2 * gs[1][w + 1][7], rtol=1e-12)


def test_command_line_function_and_model_name():
    sys.path.insert(0, os.path.join(ROOT, "examples", "bach10_scoreinformed"))
    import train_bach10_si as cli
    assert cli.network_function("build_ca_1x1") == "build_ca_1x1"
    for v in ("build_ca", "build_ca_2x2", "", "BUILD_CA_1X1"):
        assert cli.network_function(v) == "build_ca"           # trainCNNrwc.py:630: anything unknown is build_ca
    assert cli.model_name("m", "build_ca_1x1") == "m_x_gt"
    assert cli.model_name("m", "build_ca") == "m_gt"
    with pytest.raises(SystemExit):
        cli.main(["--output", "."])                            # --db is required


def test_trainer_arguments_that_need_no_device():
    from deepconvsep_amd import score_training as st
    from deepconvsep_amd.arch import ARCHS, resolve
    shapes = st.param_shapes(19, 253, function='build_ca_1x1')
    assert len(shapes) == 22 and shapes[18] == (800, 200, 1, 1) and shapes[21] == (16,)
    assert st.param_shapes(19, 253, 1, 'build_ca_1x1')[18] == (200, 200, 1, 1)
    init = st.glorot_init(19, 253, function='build_ca_1x1')
    assert [p.shape for p in init] == shapes and all(p.dtype == np.float32 for p in init)
    assert not init[1].any() and init[0].any()
    assert resolve('bach10_si', init, 19, 253) is ARCHS['bach10_si_1x1']
    assert len(st.param_shapes(12, 93)) == 17                  # the default stays build_ca
    assert st.arch_name(4) == 'bach10_si' and st.arch_name(2, 'build_ca_1x1') == 'bach10_si_1x1'
    for kw in (dict(function='build_ca_2x2'), dict(function='build_ca_1x1', branches=5),
               dict(function='build_ca_1x1', time_context=18, feat_size=253),
               dict(function='build_ca_1x1', time_context=19, feat_size=252), dict(branches=2)):
        with pytest.raises(ValueError):
            st.ScoreTrainer(**kw)
    a = ARCHS['bach10_si_1x1']
    assert a.train_flops_per_tile(30, 2049) > 2 * a.flops_per_tile(30, 2049, live_only=True)
