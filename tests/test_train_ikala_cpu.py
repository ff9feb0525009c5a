"""iKala trainer: the float64 restatement (tests/train_ikala_ref.py) against the inference oracle and the reference's own loss
lines, Lasagne's initialisation of the 13 arrays, and 3-channel feature files (CPU only)."""
import numpy as np
import pytest
import torch

import train_ikala_ref
from deepconvsep_amd import training
from deepconvsep_amd.arch import ARCHS
from deepconvsep_amd.transform import write_shape_file
from oracle import cases, net_ref


@pytest.mark.parametrize("name", ["net_ikalanp_f150_glorot", "net_ikalanp_f150_sparse"])
def test_forward_equals_the_inference_oracle_goldens(golden, name):
    g = golden(name)
    arch, F, seed, kind = str(g["arch"]), int(g["F"]), int(g["seed"]), str(g["kind"])
    assert arch == "ikala_nopool"
    params = cases.case_params(arch, 30, F, seed, kind, g["out_bias"] if kind != "glorot" else None)
    p = train_ikala_ref.forward_np(params, g["x"])
    np.testing.assert_allclose(p, g["p"], rtol=1e-10, atol=1e-10 * np.abs(g["p"]).max())


@pytest.mark.parametrize("tc,F", [(30, 131), (12, 93), (10, 87)])
def test_forward_equals_net_ref_where_conv1t_leaves_edge_columns(tc, F):
    """(F - 30) % 3 != 0 at 131 and 93: conv1^T gives the last columns no tap, they hold the output bias alone."""
    rs = np.random.RandomState(tc + F)
    params = training.glorot_init("ikala_nopool", tc, F, seed=1)
    params[12] = np.abs(rs.randn(2)).astype(np.float32)
    x = rs.uniform(0, 1, size=(2, 1, tc, F))
    p = train_ikala_ref.forward_np(params, x)
    want = net_ref.forward("ikala_nopool", params, x).numpy()
    np.testing.assert_allclose(p, want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    if (F - 30) % 3:
        last = 3 * ((F - 30) // 3) + 30
        for k in range(2):
            assert np.all(p[:, k, :, last:] == max(float(params[12][k]), 0.0))


@pytest.mark.parametrize("case", ["pos", "neg"])
def test_loss_and_components_match_the_reference_lines(golden, case):
    g = golden("train_ikala_loss")
    t = lambda k: torch.as_tensor(g["%s_%s" % (case, k)])  # noqa: E731
    got = np.array([float(v) for v in train_ikala_ref.components(t("p"), t("x"), t("tgt"), t("r"))])
    np.testing.assert_allclose(got, g["%s_out" % case], rtol=1e-12, atol=1e-300)
    E = got[1] + got[2] - got[3]
    assert (E < 0) == (case == "neg")


def test_gradient_sign_follows_E(golden):
    """loss = |E|: for E < 0 the gradient of the loss is minus that of E (abs' = sign)."""
    g = golden("train_ikala_loss")
    for case, sgn in (("pos", 1.0), ("neg", -1.0)):
        p = torch.as_tensor(g["%s_p" % case]).requires_grad_(True)
        args = [torch.as_tensor(g["%s_%s" % (case, k)]) for k in ("x", "tgt", "r")]
        out = train_ikala_ref.components(p, *args)
        E = out[1] + out[2] - out[3]
        (gl,) = torch.autograd.grad(out[0], p, retain_graph=True)
        (ge,) = torch.autograd.grad(E, p)
        assert np.array_equal(gl.numpy(), sgn * ge.numpy())


def test_glorot_init_shapes_and_bounds():
    ps = training.glorot_init("ikala_nopool", 30, 513, seed=3)
    shapes = [tuple(s) for s in ARCHS["ikala_nopool"].param_shapes(30, 513)]
    assert [p.shape for p in ps] == shapes == [tuple(s) for s in training.param_shapes("ikala_nopool", 30, 513)]
    assert len(ps) == 13
    assert shapes[0] == (30, 1, 1, 30) and shapes[3] == (30, 30, 10, 20) and shapes[6] == (90090, 256)
    assert shapes[8] == (256, 90090) and shapes[12] == (2,)
    assert sum(int(np.prod(s)) for s in shapes) == 69550578
    for p in ps:
        assert p.dtype == np.float32
        if p.ndim == 1:
            assert not p.any()
        else:
            rf = int(np.prod(p.shape[2:])) if p.ndim > 2 else 1
            a = np.sqrt(6.0 / ((p.shape[0] + p.shape[1]) * rf))
            assert np.abs(p).max() <= a and np.abs(p).max() > 0.9 * a
    assert np.isclose(np.sqrt(6.0 / (60 * 200)), np.sqrt(3.0) * np.sqrt(2.0 / (60 * 200)))


def test_pooled_ikala_graph_does_not_train():
    with pytest.raises(NotImplementedError):
        training.param_shapes("ikala", 30, 513)
    assert training.n_sources("ikala_nopool") == 2 and training.n_sources("dsd") == 4


def _files(tmp_path, C, Ts, F=7):
    paths = []
    for i, T in enumerate(Ts):
        stem = str(tmp_path / ("song%d.data" % i))
        np.zeros((C, T, F)).tofile(stem)
        write_shape_file(stem.replace(".data", ".shape"), (C, T, F))
        paths.append(stem)
    return paths


def test_feature_windows_reads_three_channel_files(tmp_path):
    paths = _files(tmp_path, 3, (20, 30, 200))
    fw = training.FeatureWindows(paths, 30, 20, 0.3, batch_size=4, sources=2)
    want = [(0, 0), (-1, 0)] + [(2, s) for s in range(0, 100, 10)]
    assert [tuple(r) for r in fw.table] == want
    assert fw.iteration_size == len(want) // 4 and fw.F == 7 and fw.sources == 2
    fa = training.FeatureWindows(paths, 30, 20, 0.3, windows="all", sources=2)
    assert len(fa.table) == 1 + 1 + 18


def test_feature_windows_rejects_a_channel_mismatch(tmp_path):
    three = _files(tmp_path, 3, (40,))
    with pytest.raises(ValueError):
        training.FeatureWindows(three, 30, 20, 0.3)               # the default is DSD's [5, T, F]
    (tmp_path / "five").mkdir()
    five = _files(tmp_path / "five", 5, (40,))
    with pytest.raises(ValueError):
        training.FeatureWindows(five, 30, 20, 0.3, sources=2)
    assert training.FeatureWindows(five, 30, 20, 0.3).sources == 4
