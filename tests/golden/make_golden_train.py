"""Writes tests/golden/train_loss.npz, train_windows.npz and train_feed.npz from the reference's own source.  CPU only; needs the
reference tree (DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_train.py

* train_loss: examples/dsd100/trainCNN.py:167-219 executed as written, with NumPy stand-ins for the network output
  (``lasagne.layers.get_output`` returns a fixed ``p``), ``lasagne.objectives.squared_error`` ((a - b) ** 2) and the
  uniform draw (``np.random.uniform`` returns a fixed ``r``): the loss and its six components for fixed p, x, targets, r.
  Case ``neg`` has targets 0..2 equal to the masked sources, so E < 0.
* train_windows: dataset.py's getNum (:596-602), loadFile (:383-488) and initOutput (:509-516) executed on a stub
  LargeDataset whose mixture holds frame number + 1 in every bin; the slots' first bin gives the window start + 1, 0 a
  zero frame.
* train_feed: the same three methods on a stub whose data holds ``1000 c + 10 t + f + 1`` at (channel c, frame t, bin f)
  (small integers, exact in float32) with ``mult_factor_in = mult_factor_out`` set and ``tensortype`` float32, as the
  trainers build the class: per case ``(T, tc, overlap, nsources, F, mult)`` the full ``inputs [n, tc, F]`` and
  ``outputs [n, tc, nsources F]`` of loadFile, and ``cases`` = the table of the six numbers.
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

TRAINER = ("examples/dsd100/trainCNN.py", 167, 219)
DATASET = {"getNum": ("dataset.py", 596, 602), "loadFile": ("dataset.py", 383, 488), "initOutput": ("dataset.py", 509, 516)}
WINDOW_CASES = [(20, 30, 25), (30, 30, 25), (31, 30, 25), (200, 30, 25), (200, 30, 20), (200, 30, 0), (95, 30, 20),
                (61, 20, 0)]


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
    keys = ["loss", "vocals_error", "bass_error", "drums_error", "negative_error", "alpha_component", "negative_error_voc"]
    return np.array([float(ns[k]) for k in keys])


def loss_cases():
    out = {}
    for name, seed in (("pos", 1), ("neg", 2)):
        rs = np.random.RandomState(seed)
        B, tc, F = 2, 4, 5
        p = np.maximum(rs.randn(B, 4, tc, F), 0.0)
        p[0, :, 0, 0] = 0.0      # every channel zero: the masks come from eps * r alone
        x = rs.uniform(0, 2, size=(B, 1, tc, F))
        r = rs.uniform(size=(B, 1, tc, F))
        tgt = rs.uniform(0, 1, size=(B, 4, tc, F))
        if name == "neg":
            s = p + 1e-8 * r
            den = s.sum(axis=1, keepdims=True)
            tgt[:, 0:3] = s[:, 0:3] / den * x
        vals = run_loss(p, x, tgt, r)
        E = vals[1] + vals[3] + vals[2] - vals[4] - vals[5] - vals[6]
        assert (E < 0) == (name == "neg"), (name, E)
        for k, v in (("p", p), ("x", x), ("r", r), ("tgt", tgt), ("out", vals)):
            out["%s_%s" % (name, k)] = v
    return out


class _Stub(object):
    pitched = save_mask = extra_features = False
    log_in = log_out = False
    mult_factor_in = mult_factor_out = 1.0
    nsources = 4
    tensortype = np.float64
    input_size = 1
    output_size = 4
    path_transform_in = path_transform_out = ["in"]
    dirid = [0]
    file_list = ["f.data"]

    def __init__(self, T, tc, ov):
        self.T, self.time_context, self.overlap = T, tc, ov

    def get_shape(self, path):
        return (5, self.T, 1)

    def loadInputOutput(self, id):
        frames = np.arange(1, self.T + 1, dtype=np.float64).reshape(1, self.T, 1)
        return frames, np.repeat(frames, 4, axis=0)


def window_cases():
    ns = {"np": np, "os": os}
    for name, (rel, a, b) in DATASET.items():
        exec(compile(textwrap.dedent(ref_exec._slice(rel, a, b)), rel, "exec"), ns)
        setattr(_Stub, name, ns[name])
    out = {}
    for T, tc, ov in WINDOW_CASES:
        s = _Stub(T, tc, ov)
        n = s.getNum(0)
        s.num_points = [0, n]
        res = s.loadFile(0)
        out["T%d_tc%d_ov%d" % (T, tc, ov)] = res["inputs"][:, :, 0]
    return out


# (T, tc, overlap, nsources, F, mult): a file shorter than tc (one padded window), T == tc (loadFile reaches no window:
# one zero slot), T == tc + 1, more slots than windows (one window, one zero slot), overlapping windows, a scale that is
# a power of two and scales that are not, 2 and 4 sources
FEED_CASES = [(7, 10, 5, 4, 5, 0.5), (10, 10, 5, 4, 3, 0.3), (11, 10, 5, 2, 7, 0.3), (60, 30, 0, 4, 3, 0.25),
              (61, 20, 0, 2, 6, 0.3), (40, 10, 8, 4, 4, 0.7), (23, 6, 2, 2, 5, 2.0)]


def feed_data(T, nsources, F):
    """[1 + nsources, T, F] float64: 1000 c + 10 t + f + 1."""
    c, t, f = np.meshgrid(np.arange(1 + nsources), np.arange(T), np.arange(F), indexing="ij")
    return (1000 * c + 10 * t + f + 1).astype(np.float64)


class _FeedStub(_Stub):
    tensortype = np.float32

    def __init__(self, T, tc, ov, nsources, F, mult):
        _Stub.__init__(self, T, tc, ov)
        self.nsources, self.F = nsources, F
        self.input_size, self.output_size = F, nsources * F
        self.mult_factor_in = self.mult_factor_out = mult

    def get_shape(self, path):
        return (1 + self.nsources, self.T, self.F)

    def loadInputOutput(self, id):
        a = feed_data(self.T, self.nsources, self.F)
        return a[0:1], a[1:]


def feed_cases():
    ns = {"np": np, "os": os}
    for name, (rel, a, b) in DATASET.items():
        exec(compile(textwrap.dedent(ref_exec._slice(rel, a, b)), rel, "exec"), ns)
        setattr(_FeedStub, name, ns[name])
    out = {"cases": np.asarray(FEED_CASES, dtype=np.float64)}
    for k, (T, tc, ov, nsrc, F, mult) in enumerate(FEED_CASES):
        s = _FeedStub(T, tc, ov, nsrc, F, mult)
        s.num_points = [0, s.getNum(0)]
        res = s.loadFile(0)
        assert res["inputs"].dtype == np.float32 and res["outputs"].dtype == np.float32
        out["inputs_%d" % k], out["outputs_%d" % k] = res["inputs"], res["outputs"]
    return out


def main():
    np.savez_compressed(os.path.join(HERE, "train_loss.npz"), **loss_cases())
    np.savez_compressed(os.path.join(HERE, "train_windows.npz"), **window_cases())
    np.savez_compressed(os.path.join(HERE, "train_feed.npz"), **feed_cases())
    print("wrote train_loss.npz, train_windows.npz, train_feed.npz")


if __name__ == "__main__":
    main()
