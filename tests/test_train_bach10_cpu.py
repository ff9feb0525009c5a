"""Bach10 trainer: the float64 restatement (tests/train_bach10_ref.py) against the inference oracle and the reference's own
loss lines, and Lasagne's initialisation of the 17 arrays (CPU only)."""
import numpy as np
import pytest
import torch

import train_bach10_ref
from deepconvsep_amd import training
from deepconvsep_amd.arch import ARCHS
from oracle import cases, net_ref


@pytest.mark.parametrize("name", ["net_bach10_f129_glorot", "net_bach10_f129_sparse", "net_bach10_f129_tiny"])
def test_forward_equals_the_inference_oracle_goldens(golden, name):
    g = golden(name)
    arch, F, seed, kind = str(g["arch"]), int(g["F"]), int(g["seed"]), str(g["kind"])
    assert arch == "bach10"
    params = cases.case_params(arch, 30, F, seed, kind, g["out_bias"] if kind != "glorot" else None)
    p = train_bach10_ref.forward_np(params, g["x"])
    np.testing.assert_allclose(p, g["p"], rtol=1e-10, atol=1e-10 * np.abs(g["p"]).max())


@pytest.mark.parametrize("tc,F", [(30, 33), (2, 34), (3, 30), (9, 65)])
def test_forward_equals_net_ref_where_conv1t_leaves_edge_columns(tc, F):
    """(F - 30) % 4 != 0 at 33, 65 (and 34): conv1^T gives the last columns no tap, they hold the output bias alone."""
    rs = np.random.RandomState(tc + F)
    params = training.glorot_init("bach10", tc, F, seed=1)
    params[16] = np.abs(rs.randn(4)).astype(np.float32)
    x = rs.uniform(0, 1, size=(2, 1, tc, F))
    p = train_bach10_ref.forward_np(params, x)
    want = net_ref.forward("bach10", params, x).numpy()
    assert p.shape == want.shape == (2, 4, tc, F)
    np.testing.assert_allclose(p, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    if (F - 30) % 4:
        last = 4 * ((F - 30) // 4) + 30
        assert last < F
        for k in range(4):
            assert np.all(p[:, k, :, last:] == max(float(params[16][k]), 0.0))


def test_loss_and_components_match_the_reference_lines(golden):
    g = golden("train_bach10_loss")
    t = lambda k: torch.as_tensor(g[k])  # noqa: E731
    got = np.array([float(v) for v in train_bach10_ref.components(t("p"), t("x"), t("tgt"), t("r"))])
    want = np.array([float(g[k]) for k in ("loss", "error1", "error2", "error3", "error4")])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    assert not g["p"][0, :, 0, 0].any()          # the element whose masks are 0 / (eps r)
    assert np.isclose(got[0], got[1:].sum(), rtol=1e-14)


def test_glorot_init_shapes_and_bounds():
    ps = training.glorot_init("bach10", 30, 2049, seed=3)
    shapes = [tuple(s) for s in ARCHS["bach10"].param_shapes(30, 2049)]
    assert [p.shape for p in ps] == shapes == [tuple(s) for s in training.param_shapes("bach10", 30, 2049)]
    assert len(ps) == 17
    assert shapes[0] == (30, 1, 1, 30) and shapes[3] == (30, 30, 20, 1) and shapes[6] == (166650, 256)
    for i in (8, 10, 12, 14):
        assert shapes[i] == (256, 166650) and shapes[i + 1] == (166650,)
    assert shapes[16] == (4,)
    assert sum(int(np.prod(s)) for s in shapes) == 213997880
    for p in ps:
        assert p.dtype == np.float32
        if p.ndim == 1:
            assert not p.any()
        else:
            rf = int(np.prod(p.shape[2:])) if p.ndim > 2 else 1
            a = np.sqrt(6.0 / ((p.shape[0] + p.shape[1]) * rf))
            assert np.abs(p).max() <= a and np.abs(p).max() > 0.9 * a


def test_trainable_graphs_and_sources():
    assert training.TRAINABLE == ("dsd", "ikala_nopool", "bach10")
    assert training.n_sources("bach10") == 4 and training.n_sources("ikala_nopool") == 2 and training.n_sources("dsd") == 4
    assert training.BACH10_COMPONENTS == ("bassoon", "clarinet", "saxophone", "violin")
    assert training.BACH10_EPS == 1e-18
    for arch in ("ikala", "bach10_si"):
        with pytest.raises(NotImplementedError):
            training.param_shapes(arch, 30, 513)
