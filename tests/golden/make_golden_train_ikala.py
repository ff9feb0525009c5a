"""Writes tests/golden/train_ikala_loss.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_train_ikala.py

examples/ikala/trainCNN.py:155-189 executed as written, with NumPy stand-ins for the network output
(``lasagne.layers.get_output`` returns a fixed ``p``), ``lasagne.objectives.squared_error`` ((a - b) ** 2) and the uniform
draw (``np.random.uniform`` returns a fixed ``r``): the loss and its four components for fixed p, x, targets, r.  Case ``neg``
has the targets equal to the masked sources, so vocals_error and acc_error vanish and E = -negative_error_voc < 0.
"""
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_exec  # noqa: E402

TRAINER = ("examples/ikala/trainCNN.py", 155, 189)
KEYS = ["loss", "vocals_error", "acc_error", "negative_error_voc", "negative_error_acc"]


def run_loss(p, x, tgt, r):
    B, _, tc, F = x.shape
    lasagne = types.SimpleNamespace(layers=types.SimpleNamespace(get_output=lambda net, deterministic=True: p),
                                    objectives=types.SimpleNamespace(squared_error=lambda a, b: (a - b) ** 2))
    npr = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith('__')})
    npr.random = types.SimpleNamespace(uniform=lambda size: r.reshape(size))
    train = types.SimpleNamespace(batch_size=B, time_context=tc, input_size=F)
    ns = dict(np=npr, lasagne=lasagne, train=train, fun=lambda **kw: None, load=False, input_var2=x, target_var2=tgt)
    src = textwrap.dedent(ref_exec._slice(*TRAINER))
    exec(compile(src, TRAINER[0], "exec"), ns)
    return np.array([float(ns[k]) for k in KEYS])


def loss_cases():
    out = {}
    for name, seed in (("pos", 1), ("neg", 2)):
        rs = np.random.RandomState(seed)
        B, tc, F = 2, 4, 5
        p = np.maximum(rs.randn(B, 2, tc, F), 0.0)
        p[0, :, 0, 0] = 0.0      # both channels zero: the masks come from eps * r alone
        x = rs.uniform(0, 2, size=(B, 1, tc, F))
        r = rs.uniform(size=(B, 1, tc, F))
        tgt = rs.uniform(0, 1, size=(B, 2, tc, F))
        if name == "neg":
            s = p + 1e-8 * r
            tgt = s / s.sum(axis=1, keepdims=True) * x
        vals = run_loss(p, x, tgt, r)
        E = vals[1] + vals[2] - vals[3]
        assert (E < 0) == (name == "neg"), (name, E)
        for k, v in (("p", p), ("x", x), ("r", r), ("tgt", tgt), ("out", vals)):
            out["%s_%s" % (name, k)] = v
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "train_ikala_loss.npz"), **loss_cases())
    print("wrote train_ikala_loss.npz")


if __name__ == "__main__":
    main()
