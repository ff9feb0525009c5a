"""DSD trainer: the float64 restatement (tests/train_ref.py) against the reference's own loss lines and the inference
oracle, the window table against dataset.py's loadFile, Lasagne's initialisation (CPU only)."""
import os

import numpy as np
import pytest
import torch

import train_ref
from deepconvsep_amd import training
from deepconvsep_amd.transform import write_shape_file
from oracle import cases


@pytest.mark.parametrize("name", ["net_dsd_f33_tiny", "net_dsd_f33_sparse", "net_dsd_f33_dominant", "net_dsd_f65_glorot"])
def test_forward_equals_the_inference_oracle(golden, name):
    g = golden(name)
    arch, F, seed, kind = str(g["arch"]), int(g["F"]), int(g["seed"]), str(g["kind"])
    params = cases.case_params(arch, 30, F, seed, kind, g["out_bias"] if kind != "glorot" else None)
    p = train_ref.forward_np(params, g["x"])
    np.testing.assert_allclose(p, g["p"], rtol=1e-10, atol=1e-10 * np.abs(g["p"]).max())


@pytest.mark.parametrize("case", ["pos", "neg"])
def test_loss_and_components_match_the_reference_lines(golden, case):
    g = golden("train_loss")
    t = lambda k: torch.as_tensor(g["%s_%s" % (case, k)])  # noqa: E731
    got = np.array([float(v) for v in train_ref.components(t("p"), t("x"), t("tgt"), t("r"))])
    np.testing.assert_allclose(got, g["%s_out" % case], rtol=1e-12, atol=0)


def test_relu_tie_and_abs_at_zero():
    v = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (gr,) = torch.autograd.grad(train_ref.rectify(v).sum(), v)
    assert gr.tolist() == [0.5, 0.5, 0.5]
    e = torch.zeros((), dtype=torch.float64, requires_grad=True)
    (ga,) = torch.autograd.grad(torch.abs(e), e)
    assert float(ga) == 0.0


def test_first_adadelta_step_closed_form():
    g = [np.array([3.0, -1e-4, 0.0])]
    P, A, D = train_ref.adadelta([np.zeros(3)], g, [np.zeros(3)], [np.zeros(3)])
    u = g[0] * np.sqrt(1e-6) / np.sqrt(0.05 * g[0] ** 2 + 1e-6)
    np.testing.assert_allclose(P[0], -u, rtol=1e-15)
    np.testing.assert_allclose(A[0], 0.05 * g[0] ** 2, rtol=1e-15)
    np.testing.assert_allclose(D[0], 0.05 * u * u, rtol=1e-15)


def _slots_from_fixture(a):
    out = []
    for row in a:
        out.append(None if row[0] == 0 else int(row[0]) - 1)
    return out


def test_window_table_matches_loadfile(golden):
    g = golden("train_windows")
    for key in g.files:
        T, tc, ov = [int(s[s.index(c) + len(c):]) for s, c in zip(key.split("_"), ("T", "tc", "ov"))]
        assert training.reference_slots(T, tc, ov) == _slots_from_fixture(g[key]), key


def test_feature_windows_reads_the_repo_writer(tmp_path):
    paths = []
    for i, T in enumerate((20, 30, 200)):
        stem = str(tmp_path / ("song%d.data" % i))
        np.zeros((5, T, 7)).tofile(stem)
        write_shape_file(stem.replace(".data", ".shape"), (5, T, 7))
        paths.append(stem)
    fw = training.FeatureWindows(paths, 30, 25, 0.3, batch_size=4)
    want = [(0, 0), (-1, 0)] + [(2, s) for s in range(0, 55, 5)]
    assert [tuple(r) for r in fw.table] == want
    assert fw.iteration_size == len(want) // 4 and fw.F == 7
    fa = training.FeatureWindows(paths, 30, 25, 0.3, windows="all")
    assert len(fa.table) == 1 + 1 + 35


def test_glorot_init_shapes_and_bounds():
    ps = training.glorot_init("dsd", 30, 513, seed=3)
    assert [p.shape for p in ps] == [tuple(s) for s in training.param_shapes("dsd", 30, 513)]
    for p in ps:
        assert p.dtype == np.float32
        if p.ndim == 1:
            assert not p.any()
        else:
            rf = int(np.prod(p.shape[2:])) if p.ndim > 2 else 1
            a = np.sqrt(6.0 / ((p.shape[0] + p.shape[1]) * rf))
            assert np.abs(p).max() <= a and np.abs(p).max() > 0.9 * a


def test_trainer_without_a_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError):
        training.Trainer(batch_size=1, time_context=4, feat_size=5)
