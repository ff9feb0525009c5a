"""The handle the three trainers share (training.TrainerHandle) on the MI355X: ``Trainer.set_rand``, the output vector
sized from ``dcs_trainer_out_count`` and ``forward`` without targets, at the smallest shapes of the tie tests."""
from ctypes import byref, c_int

import numpy as np
import pytest
import torch

import train_edges as E

pytestmark = pytest.mark.gpu

MONO = ("dsd", "ikala", "bach10")
# eps 0.05 puts the draw into the masks at a size float32 sees ((p + eps r) / sum, p of the order 0.1); at the graphs'
# defaults (1e-8, 1e-18) two draws give the same float32 loss and the test could not tell them apart
EPS = 0.05


def _trainer(graph, params, r, **kw):
    from deepconvsep_amd.training import Trainer
    B, _, tc, F = r.shape
    return Trainer(arch=E.GRAPHS[graph].arch, params=params, batch_size=B, time_context=tc, feat_size=F, rand=r, **kw)


@pytest.mark.parametrize("graph", MONO)
def test_set_rand_equals_a_trainer_built_with_that_draw(graph):
    params, x, r2, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=3)
    r1 = np.random.RandomState(8).uniform(size=r2.shape).astype(np.float32)
    a, b, c = (_trainer(graph, params, r, eps=EPS) for r in (r1, r2, r1))
    a.set_rand(r2)
    assert a.rand_shape == r2.shape
    la, lb, lc = a.step(x, tgt), b.step(x, tgt), c.step(x, tgt)
    assert la == lb and lc != lb
    for p, q in zip(a.params(), b.params()):
        assert np.array_equal(p, q)
    with pytest.raises(ValueError, match="rand has shape"):
        a.set_rand(r2[:, :, :, :-1])
    for t in (a, b, c):
        t.close()


def _out_count(t):
    from deepconvsep_amd import _lib
    n = c_int()
    _lib.check(t.ctx._lib.dcs_trainer_out_count(t._h, byref(n)))
    return n.value


@pytest.mark.parametrize("graph", MONO)
def test_run_returns_seven_doubles(graph):
    params, x, r, tgt = E.setup(graph, *E.TIE_SHAPES[graph], seed=3)
    t = _trainer(graph, params, r)
    out = t.run(x, tgt, 0)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (_out_count(t),) == (7,)
    assert np.isfinite(t.ctx.to_host(out)).all()
    t.close()


def test_stereo_run_returns_sixteen_doubles():
    from deepconvsep_amd.stereo_training import StereoTrainer, glorot_init
    B, tc, F = 2, 4, 8
    rs = np.random.RandomState(1)
    t = StereoTrainer(params=glorot_init(tc, F, 1), batch_size=B, time_context=tc, feat_size=F)
    x, tgt = 0.3 * rs.uniform(size=(B, 2, tc, F)), 0.1 * rs.uniform(size=(B, 8, tc, F))
    for ild in (False, True):
        out = t.run(x, tgt, 0, ild)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (_out_count(t),) == (16,)
    t.close()


@pytest.mark.parametrize("graph", MONO)
def test_forward_takes_inputs_alone(graph):
    """Against the graph's float64 restatement, at the bound test_gpu_train.py holds the forward pass to."""
    g = E.GRAPHS[graph]
    params, x, r, _ = E.setup(graph, *E.TIE_SHAPES[graph], seed=3)
    t = _trainer(graph, params, r)
    want = g.ref.forward_np(params, x)
    for inputs in (x, t.ctx.to_device(x, np.float32)):
        got = t.ctx.to_host(t.forward(inputs))
        assert got.shape == want.shape == x.shape[:1] + (g.nsrc,) + x.shape[2:]
        assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    with pytest.raises(ValueError, match="inputs"):
        t.forward(x[:, :, :, :-1])
    t.close()
