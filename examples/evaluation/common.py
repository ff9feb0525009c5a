"""Shared by the evaluation command lines: wav reading and the JSON layout of the results."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.evaluation import nanmedian  # noqa: E402
from deepconvsep_amd.separation import read_wav  # noqa: E402


def read(path):
    """wav -> (rate, float64 [samples, channels]); BSS Eval ratios do not depend on a common scale"""
    rate, x = read_wav(path)
    return rate, (x[:, None] if x.ndim == 1 else x)


def find(folder, names):
    """the first of `names` that exists in `folder`, or None"""
    for n in names:
        p = os.path.join(folder, n)
        if os.path.isfile(p):
            return p
    return None


def metrics(names, values, keys):
    """{name: {key: per-window list, 'median': {key: NaN-ignoring median}}} from values[key] [nsrc, nwin] or [nsrc]"""
    out = {}
    for j, n in enumerate(names):
        rec = {}
        for k in keys:
            v = np.atleast_1d(np.asarray(values[k][j], dtype=np.float64))
            rec[k] = [None if np.isnan(x) else float(x) for x in v]
        rec["median"] = {k: nanmedian(values[k][j]) for k in keys}
        out[n] = rec
    return out


def dump(obj, path):
    def clean(o):
        if isinstance(o, dict):
            return {k: clean(v) for k, v in o.items()}
        if isinstance(o, list):
            return [clean(v) for v in o]
        if isinstance(o, float) and np.isnan(o):
            return None
        if isinstance(o, float) and np.isinf(o):
            return "inf" if o > 0 else "-inf"
        return o
    text = json.dumps(clean(obj), indent=1, sort_keys=True)
    if path:
        with open(path, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)
