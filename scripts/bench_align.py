#!/usr/bin/env python3
"""Dynamic time warping on the MI355X (``dcs_dtw``) at T = U = 3446 frames -- 40 s of audio at hop 512 against a score of the
same length -- on unit-norm chroma rows.  Timed warm with HIP events around the whole call (fill, one launch per anti-diagonal
of tiles, backtrack); the NumPy restatement of the same recursion (tests/align_ref.py, float32, one vector operation per
anti-diagonal of cells) is timed on the host's CPU beside it and the two costs are compared.  Prints one JSON line.

    python scripts/bench_align.py [--frames 3446] [--score-frames 3446] [--band N] [--reps 20]

Per-kernel times (tile launches, the backtrack's single walker) come from a kernel trace of this script, in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3446)
    ap.add_argument("--score-frames", type=int, default=3446)
    ap.add_argument("--band", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args(argv)
    import torch
    import align_ref
    from deepconvsep_amd import _lib, align
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    T, U = a.frames, a.score_frames
    A, S = align_ref.unit_features(T, U, seed=0)
    A_t, S_t = ctx.to_device(A, np.float32), ctx.to_device(S, np.float32)
    B = int(_lib.load().dcs_dtw_tile())
    path, cost = align.dtw(ctx, A_t, S_t, band=a.band)                 # warm
    with ctx.stream_scope():
        out_path = torch.empty((T + U - 1, 2), dtype=torch.int32, device=A_t.device)
        n = torch.zeros((1,), dtype=torch.int64, device=A_t.device)
        c = torch.empty((1,), dtype=torch.float32, device=A_t.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            _lib.check(ctx._lib.dcs_dtw(ctx._h, A_t.data_ptr(), T, S_t.data_ptr(), U, -1 if a.band is None else a.band,
                                        out_path.data_ptr(), n.data_ptr(), c.data_ptr()))
            ev[i + 1].record()
        torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps))
    res = dict(T=T, U=U, band=a.band, tile=B, path_points=int(len(path)), cost=cost,
               launches_unbanded=1 + (-(-T // B)) + (-(-U // B)) - 1 + 1, scratch_bytes=align.dtw_bytes(T, U, a.band),
               dtw_ms_median=ms[len(ms) // 2], dtw_ms_min=ms[0], dtw_ms_max=ms[-1])
    if not a.no_numpy:
        t0 = time.perf_counter()
        ref_path, ref_cost, _ = align_ref.dtw(A, S, band=a.band, dtype=np.float32)
        res["numpy_f32_cpu_s"] = time.perf_counter() - t0
        res["cost_minus_numpy"] = cost - ref_cost
        res["same_path_as_numpy"] = bool(np.array_equal(path, ref_path))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
