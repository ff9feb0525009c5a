"""Writes tests/golden/train_ild_loss.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_train_ild.py

examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:183-198 (the stage-1 loss) and :210-228 (the ILD term) executed as written,
with NumPy stand-ins for Theano: ``T.sum`` / ``T.tile`` are NumPy's, ``dimshuffle`` is a method of an ndarray subclass,
``lasagne.objectives.squared_error`` is (a - b) ** 2, ``prediction`` is a fixed ``p`` and the two normal draws are fixed
``r1`` / ``r2`` (``rand_num`` is given, ``theano_rng.normal`` returns ``r2``).  Per case: p, x, tgt, r = [r1, r2] and ten
values: the stage-2 loss, errors_insts (mic 0's four sources, then mic 1's) and the ILD term abs(sum) / 500; ``loss1`` is
the stage-1 loss.  Case ``zeros`` has bins where all four outputs of a channel (or of both) are zero and bins where a
target pair is silent.
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

TRAINER = "examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py"
STAGE1, STAGE2 = (TRAINER, 183, 198), (TRAINER, 210, 228)


class Arr(np.ndarray):
    def dimshuffle(self, *axes):
        a = np.asarray(self)
        return a.reshape([1 if k == 'x' else a.shape[k] for k in axes]).view(Arr)


def run_loss(p, x, tgt, r1, r2):
    B, _, tc, F = x.shape
    T = types.SimpleNamespace(sum=np.sum, tile=np.tile)
    lasagne = types.SimpleNamespace(objectives=types.SimpleNamespace(squared_error=lambda a, b: (a - b) ** 2))
    theano = types.SimpleNamespace(config=types.SimpleNamespace(floatX='float64'))
    rng = types.SimpleNamespace(normal=lambda size, avg, std, dtype: r2.reshape(size))
    ns = dict(np=np, T=T, lasagne=lasagne, theano=theano, theano_rng=rng, nchannels=2, nsources=4, eps=1e-12,
              batch_size=B, time_context=tc, input_size=F, prediction=p.view(Arr), input_var=x.view(Arr),
              target_var=tgt.view(Arr), rand_num=r1, sourceall=[], errors_insts=[], sep_chann=[], loss=0)
    exec(compile(textwrap.dedent(ref_exec._slice(*STAGE1)), TRAINER, "exec"), ns)
    loss1 = float(ns["loss"])
    exec(compile(textwrap.dedent(ref_exec._slice(*STAGE2)), TRAINER, "exec"), ns)
    errors = np.concatenate([np.asarray(e, np.float64).ravel() for e in ns["errors_insts"]])
    ild = float(abs(ns["train_loss_ild"].sum()) / 500)
    return loss1, np.concatenate([[float(ns["loss"])], errors, [ild]])


def case(seed, zeros):
    rs = np.random.RandomState(seed)
    B, tc, F = 2, 4, 5
    p = np.maximum(rs.randn(B, 8, tc, F), 0.0) + 0.05 * (rs.uniform(size=(B, 8, tc, F)) < 0.3)
    x = rs.uniform(0, 2, size=(B, 2, tc, F))
    tgt = rs.uniform(0, 1, size=(B, 8, tc, F))
    r1 = 0.1 * rs.randn(B, 4, tc, F)
    r2 = 0.1 * rs.randn(B, 4, tc, F)
    if zeros:
        p[0, 0::2, 0, 0] = 0.0       # channel 0's four outputs zero: its masks are 0 / (eps r1)
        p[1, :, 2, 3] = 0.0          # both channels
        p[0, :, :, 4] = 0.0          # a whole bin of one window
        tgt[0, 0:2, 1, :] = 0.0      # vocals silent in both mics: a row of bins
        tgt[1, 4:6, :, 2] = 0.0      # drums silent in a bin
        tgt[1, 2, 3, 1] = 0.0        # bass silent in mic 0 only
    loss1, vals = run_loss(p, x, tgt, r1, r2)
    return dict(p=p, x=x, tgt=tgt, r=np.stack([r1, r2]), loss1=loss1, values=vals)


def main():
    out = {}
    for name, c in (("plain", case(1, False)), ("zeros", case(2, True))):
        for k, v in c.items():
            out["%s_%s" % (name, k)] = v
        print(name, c["loss1"], c["values"])
    np.savez_compressed(os.path.join(HERE, "train_ild_loss.npz"), **out)
    print("wrote train_ild_loss.npz")


if __name__ == "__main__":
    main()
