"""NumPy restatement of the trainers' data feed (test infrastructure): what ``FeatureWindows.gather`` /
``dcs_trainer_gather`` / ``dcs_trainer_gather_sources`` (train::gather_kernel, csrc/train_core.hip) must write, element for
element.  dataset.py's loadFile (:383-488) scales the float64 file and narrows it to float32 when it fills its batch; the
trainer keeps the files resident as float32 and multiplies by the float32 scale, one float32 product per element, which has
one correctly rounded result: the comparison with the device is bit for bit."""
import numpy as np


def data_pattern(nsrc, T, F, offset=0):
    """[1 + nsrc, T, F] float64 with a distinct small integer at every (channel, frame, bin): 1000 c + 10 t + f + 1 (+
    ``offset`` to tell files apart), as tests/golden/make_golden_train.py's feed stub holds it."""
    c, t, f = np.meshgrid(np.arange(1 + nsrc), np.arange(T), np.arange(F), indexing="ij")
    return (1000 * c + 10 * t + f + 1 + offset).astype(np.float64)


def gather_np(files, table_rows, tc, F, nsrc, scale):
    """``files``: arrays ``[1 + nsrc, T_i, F]``; ``table_rows``: (file, start) pairs, file -1 = a zero slot.  Returns float32
    inputs ``[B, 1, tc, F]`` and targets ``[B, nsrc, tc, F]``: ``float32(scale) * float32(data)``, zero for file -1 and for
    frames past T_i."""
    rows = np.asarray(table_rows, dtype=np.int64).reshape(-1, 2)
    x = np.zeros((len(rows), 1, tc, F), dtype=np.float32)
    t = np.zeros((len(rows), nsrc, tc, F), dtype=np.float32)
    sc = np.float32(scale)
    for b, (fi, start) in enumerate(rows):
        if fi < 0:
            continue
        a = np.asarray(files[fi], dtype=np.float32)
        assert a.shape[0] == 1 + nsrc and a.shape[2] == F
        n = max(0, min(tc, a.shape[1] - int(start)))
        w = sc * a[:, start:start + n, :]
        assert w.dtype == np.float32
        x[b, 0, :n] = w[0]
        t[b, :, :n] = w[1:]
    return x, t


def reference_layout(targets):
    """Targets ``[n, nsrc, tc, F]`` in loadFile's layout ``outputs[n, t, j F + f]``."""
    n, nsrc, tc, F = targets.shape
    return np.ascontiguousarray(targets.transpose(0, 2, 1, 3)).reshape(n, tc, nsrc * F)
