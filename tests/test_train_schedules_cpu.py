"""What the Adam update and the two schedules built on it decide without a GPU: tests/adam_ref.py (the float64 yardstick
of tests/test_gpu_train_optim.py) against torch.optim.Adam, the second-pass arithmetic of
examples/bach10_scoreinformed/train_bach10_si.py and the model names of examples/dsd100_2ch_ILD/train_dsd_ild_3stages.py."""
import os
import sys

import numpy as np
import pytest
import torch

import adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _d in ("bach10_scoreinformed", "dsd100_2ch_ILD"):
    _p = os.path.join(ROOT, "examples", _d)
    if _p not in sys.path:
        sys.path.insert(0, _p)


def test_adam_ref_matches_torch_adam_where_the_epsilon_placements_coincide():
    """Five steps in float64 on random non-zero gradients with epsilon = 1e-300 in both: there lasagne's
    a_t m / (sqrt(v) + eps) and torch's (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps) are the same number up
    to rounding, so the recursion and the bias correction are pinned to 1e-12 relative."""
    rs = np.random.RandomState(0)
    shapes = [(7, 5), (11,), (3, 2, 4, 1)]
    p0 = [rs.randn(*s) for s in shapes]
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.Adam(tp, lr=1e-3, betas=(0.9, 0.999), eps=1e-300)
    P, M, V = p0, [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    for t in range(5):
        g = [rs.randn(*s) * 10.0 ** rs.randint(-3, 2) for s in shapes]
        assert all((np.abs(a) > 0).all() for a in g)
        for q, a in zip(tp, g):
            q.grad = torch.tensor(a, dtype=torch.float64)
        opt.step()
        P, M, V, S = adam_ref.adam(P, g, M, V, t, epsilon=1e-300)
        for q, a, p_start, s in zip(tp, P, p0, S):
            got = q.detach().numpy()
            np.testing.assert_allclose(got, a, rtol=1e-12, atol=0)
            # and relative to the distance travelled (about 1e-3 a step), so that a wrong step size cannot hide behind |p|:
            # the float64 rounding of p ~ 1 (1e-16 a step) is 1e-13 of it
            assert np.abs(got - a).max() <= 1e-9 * np.abs(a - p_start).max(), (t, np.abs(got - a).max())
            assert np.abs(s).min() > 0
    # the step sizes the GPU tests rely on to tell t = 1, 2, 3 apart
    assert [round(adam_ref.a_t(t) / adam_ref.LR, 3) for t in (1, 2, 3)] == [0.316, 0.235, 0.202]


def test_adam_ref_zero_gradient_gives_zero_step():
    p = [np.array([1.5, -2.0, 0.0, 3e-30]), np.zeros((2, 3))]
    z = [np.zeros(a.shape) for a in p]
    P, M, V = p, z, z
    for t in range(3):
        P, M, V, S = adam_ref.adam(P, z, M, V, t)
        for a, b, m, v, s in zip(P, p, M, V, S):
            assert np.array_equal(a, b) and not m.any() and not v.any() and not s.any()


def test_epsilon_is_outside_the_bias_correction():
    """One step from zero state with a gradient far below epsilon: lasagne's step is a_1 (1 - beta1) g / (sqrt(1 - beta2) |g|
    + eps) ~ lr sqrt(1 - beta2) g / eps; torch's placement would give lr g / eps, 31.6 times as much."""
    g = [np.array([1e-12])]
    P, _, _, S = adam_ref.adam([np.zeros(1)], g, [np.zeros(1)], [np.zeros(1)], 0)
    want = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9) * (0.1 * 1e-12) / (np.sqrt(0.001) * 1e-12 + 1e-8)
    assert S[0][0] == pytest.approx(want, rel=1e-12)
    assert S[0][0] == pytest.approx(1e-3 * np.sqrt(0.001) * 1e-12 / 1e-8, rel=1e-2)


@pytest.mark.parametrize("nepochs,want", [(5, 1), (6, 2), (40, 8), (1, 1), (0, 0)])
def test_second_pass_epochs(nepochs, want):
    import train_bach10_si
    assert train_bach10_si.second_pass_epochs(nepochs) == want


@pytest.mark.parametrize("skip_mse,skip_ild,want", [(False, False, "m_mseEp=30_ILDEp=10"), (True, False, "m_mseEp=0_ILDEp=10"),
                                                    (False, True, "m_mseEp=30_ILDEp=0"), (True, True, "m_mseEp=0_ILDEp=0")])
def test_three_stage_model_names(skip_mse, skip_ild, want, tmp_path):
    import train_dsd_ild_3stages as S
    assert S.model_name("m", 30, 10, skip_mse, skip_ild, load=False) == want
    assert S.model_name("m", 30, 10, skip_mse, skip_ild, load=True) == "m"
    out = str(tmp_path)
    for name in (want, "m"):
        base = os.path.join(out, "models", name)
        assert S.stage_files(out, name) == (base + ".pkl", base + "_noILD.pkl", base + "_ILD.pkl",
                                            base + "_ILD_extra_mse.pkl")


def test_three_stage_skips_that_leave_nothing_to_do_stop_with_a_message(tmp_path):
    import train_dsd_ild_3stages as S
    common = ["--db", str(tmp_path), "--output", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        S.main(common + ["--skip_train_mse", "--skip_train_ILD"])
    assert "leaves no model" in str(e.value)
    with pytest.raises(SystemExit) as e:
        S.main(common + ["--skip_train_ILD"])
    assert "_ILD.pkl" in str(e.value) and "does not exist" in str(e.value)


def test_optimizer_table_holds_lasagnes_defaults():
    from deepconvsep_amd import training
    assert training.OPTIMIZERS['adadelta'] == (0, ('learning_rate', 'rho', 'epsilon'), (1.0, 0.95, 1e-6))
    assert training.OPTIMIZERS['adam'] == (1, ('learning_rate', 'beta1', 'beta2', 'epsilon'),
                                           (adam_ref.LR, adam_ref.BETA1, adam_ref.BETA2, adam_ref.EPSILON))
