"""Writes tests/golden/train_si_loss.npz and train_si_feed.npz from the reference's own source.  CPU only; needs the reference
tree (DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_train_si.py

* train_si_loss: examples/bach10_scoreinformed/trainCNNrwc.py:235-236 and :246-275 executed as written, with the NumPy
  stand-ins of make_golden_train_bach10.py (``prediction2`` is a fixed ``p``, ``lasagne.objectives.squared_error`` is
  (a - b) ** 2, ``np.random.uniform`` returns a fixed ``r``): the loss and its four errors for a ``p`` of 16 channels whose
  channels 4 .. 15 are non-zero -- they do not matter -- a four-channel input, and one bin with all four live outputs zero.
* train_si_feed: dataset.py's getNum (:596-602), loadFile (:383-488), initOutput (:509-516), initMasks (:522-524) and
  LargeDatasetMask2.filterSpec (:839-879) executed on a stub dataset (float32 tensors, as trainCNNrwc.py:657 builds it) whose
  files hold tests/feed_ref.py's ``data_pattern`` and whose note tables are tests/score_feed_ref.py's ``fixture_notes``; then
  trainCNNrwc.py:307-320 executed as written on what loadFile returned.  Per file k: ``inputs_k`` (the network input ``mask``
  [n, 4, tc, F]) and ``targets_k`` [n, 4, tc, F].
"""
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_exec  # noqa: E402
import score_feed_ref  # noqa: E402

TRAINER = "examples/bach10_scoreinformed/trainCNNrwc.py"
KEYS = ["loss", "error1", "error2", "error3", "error4"]
DATASET = {"getNum": ("dataset.py", 596, 602), "loadFile": ("dataset.py", 383, 488), "initOutput": ("dataset.py", 509, 516),
           "initMasks": ("dataset.py", 522, 524), "filterSpec": ("dataset.py", 839, 879)}


def run_loss(p, x, tgt, r):
    B, _, tc, F = x.shape
    lasagne = types.SimpleNamespace(objectives=types.SimpleNamespace(squared_error=lambda a, b: (a - b) ** 2))
    npr = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith('__')})
    npr.random = types.SimpleNamespace(uniform=lambda size: r.reshape(size))
    train = types.SimpleNamespace(batch_size=B, time_context=tc, input_size=F)
    ns = dict(np=npr, lasagne=lasagne, train=train, prediction2=p, input_var2=x, target_var2=tgt)
    for first, last in ((235, 236), (246, 275)):
        exec(compile(textwrap.dedent(ref_exec._slice(TRAINER, first, last)), TRAINER, "exec"), ns)
    assert ns["eps"] == 1e-18
    return np.array([float(ns[k]) for k in KEYS])


def loss_case():
    rs = np.random.RandomState(3)
    B, tc, F = 2, 4, 5
    p = np.maximum(rs.randn(B, 16, tc, F), 0.0)
    p[:, 4:] += 0.5          # the twelve dead channels: non-zero everywhere
    p[0, 0:4, 0, 0] = 0.0    # all four live channels zero: the masks are 0 / (eps * r) = 0
    x = rs.uniform(0, 0.5, size=(B, 4, tc, F))
    r = rs.uniform(size=(B, 1, tc, F))
    tgt = rs.uniform(0, 1, size=(B, 4, tc, F))
    vals = run_loss(p, x, tgt, r)
    out = dict(p=p, x=x, r=r, tgt=tgt)
    out.update(zip(KEYS, vals))
    return out


class _Stub(object):
    pitched = extra_features = False
    save_mask = True
    log_in = log_out = False
    nsources = 4
    ninst = 4
    tensortype = np.float32
    timbre_model_path = None
    path_transform_in = path_transform_out = ["in"]
    dirid = [0]
    file_list = ["f.data"]

    def __init__(self, data, notes, tc, ov, mult):
        self.data, self.notes = data, notes
        self.time_context, self.overlap = tc, ov
        self.mult_factor_in = self.mult_factor_out = mult
        self.input_size, self.output_size = data.shape[2], 4 * data.shape[2]

    def get_shape(self, path):
        return self.data.shape

    def loadInputOutput(self, id):
        return self.data[0:1], self.data[1:]

    def loadPitch(self, id):
        return self.notes


def feed_cases():
    ns = {"np": np, "os": os}
    for name, (rel, a, b) in DATASET.items():
        exec(compile(textwrap.dedent(ref_exec._slice(rel, a, b)), rel, "exec"), ns)
        setattr(_Stub, name, ns[name])
    products = textwrap.dedent(ref_exec._slice(TRAINER, 307, 320))
    theano = types.SimpleNamespace(config=types.SimpleNamespace(floatX="float32"))
    out = {}
    files, notes = score_feed_ref.fixture_files(), score_feed_ref.fixture_notes()
    for k, ((T, _, mult), data, tab) in enumerate(zip(score_feed_ref.FILES, files, notes)):
        s = _Stub(data, tab, score_feed_ref.TC, score_feed_ref.OVERLAP, mult)
        s.num_points = [0, s.getNum(0)]
        res = s.loadFile(0)
        assert res["inputs"].dtype == np.float32 and res["masks"].dtype == np.float32
        env = dict(np=np, theano=theano, inputs=res["inputs"], target=res["outputs"], masks=res["masks"])
        exec(compile(products, TRAINER, "exec"), env)
        assert env["mask"].dtype == np.float32 and env["targets"].dtype == np.float32
        out["inputs_%d" % k], out["targets_%d" % k] = env["mask"], env["targets"]
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "train_si_loss.npz"), **loss_case())
    np.savez_compressed(os.path.join(HERE, "train_si_feed.npz"), **feed_cases())
    print("wrote train_si_loss.npz, train_si_feed.npz")


if __name__ == "__main__":
    main()
