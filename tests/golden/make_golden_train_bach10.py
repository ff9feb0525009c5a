"""Writes tests/golden/train_bach10_loss.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_train_bach10.py

examples/bach10/trainCNNbach10.py:160-198 executed as written, with the NumPy stand-ins of make_golden_train_ikala.py for the
network output (``lasagne.layers.get_output`` returns a fixed ``p``), ``lasagne.objectives.squared_error`` ((a - b) ** 2) and
the uniform draw (``np.random.uniform`` returns a fixed ``r``): the loss and its four errors for fixed p, x, targets, r.
E = error1 + .. + error4 is a sum of squares, so there is no negative case.
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

TRAINER = ("examples/bach10/trainCNNbach10.py", 160, 198)
KEYS = ["loss", "error1", "error2", "error3", "error4"]


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


def loss_case():
    rs = np.random.RandomState(1)
    B, tc, F = 2, 4, 5
    p = np.maximum(rs.randn(B, 4, tc, F), 0.0)
    p[0, :, 0, 0] = 0.0      # all four channels zero: the masks are 0 / (eps * r) = 0
    x = rs.uniform(0, 2, size=(B, 1, tc, F))
    r = rs.uniform(size=(B, 1, tc, F))
    tgt = rs.uniform(0, 1, size=(B, 4, tc, F))
    vals = run_loss(p, x, tgt, r)
    out = dict(p=p, x=x, r=r, tgt=tgt)
    out.update(zip(KEYS, vals))
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "train_bach10_loss.npz"), **loss_case())
    print("wrote train_bach10_loss.npz")


if __name__ == "__main__":
    main()
