#!/usr/bin/env python3
"""The score follower on the MI355X (``dcs_follow_push``): 128 frames a push -- one block of 65 536 samples at hop 512 -- on
unit-norm chroma rows against a score of 4000 frames, at windows of 512 and 1024 cells.  Timed warm with HIP events around the
call (scripts/bench_align.py's method); the NumPy restatement of the same recurrence (tests/follow_ref.py, float32) is timed on
the host's CPU beside it, per frame.  Then a followed ``ScoreStream`` push against an unarmed one at the same block size (frames
of 4096 every 512, four instruments): the difference is what following costs.  Prints one JSON line.

    python scripts/bench_follow.py [--frames 128] [--score-frames 4000] [--reps 30]

Per-kernel times come from a kernel trace of this script, in a run of its own.
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


def _median(x):
    x = sorted(x)
    return x[len(x) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--score-frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args(argv)
    import torch
    import align_ref
    import follow_ref
    from deepconvsep_amd import _lib, align, runtime
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    n, U = a.frames, a.score_frames
    A, S = align_ref.unit_features(n * (a.reps + 1), U, seed=0)
    A_t = ctx.to_device(A, np.float32)
    res = dict(frames=n, U=U)
    for W in (512, 1024):
        f = align.ScoreFollower(ctx, S, window=W, max_frames=n)
        with ctx.stream_scope():
            pos = torch.empty((n,), dtype=torch.int32, device=A_t.device)
            _lib.check(ctx._lib.dcs_follow_push(f._h, A_t[:n].data_ptr(), n, pos.data_ptr()))     # warm
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
            ev[0].record()
            for i in range(a.reps):
                _lib.check(ctx._lib.dcs_follow_push(f._h, A_t[(i + 1) * n:(i + 2) * n].data_ptr(), n, pos.data_ptr()))
                ev[i + 1].record()
            torch.cuda.synchronize()
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
        res["W%d" % W] = dict(push_ms_median=_median(ms), push_ms_min=min(ms), us_per_frame=1e3 * _median(ms) / n,
                              bytes=f.device_bytes, last_pos=int(pos[-1].item()))
        if not a.no_numpy:
            t0 = time.perf_counter()
            follow_ref.follow(A[:4 * n], S, W, 2, W // 4, 1.0 / 16, dtype=np.float32)
            res["W%d" % W]["numpy_f32_cpu_us_per_frame"] = 1e6 * (time.perf_counter() - t0) / (4 * n)
        f.close()
    if not a.no_stream:
        from deepconvsep_amd.synth import synth_audio
        import score_stream_ref as ssr
        N, hop, tc, ov, block = 4096, 512, 30, 25, n * 512
        plan = runtime.StftPlan(ctx, N, hop, np.hanning(N))
        audio_t = ctx.to_device(0.5 * synth_audio(block * (a.reps + 2), seed=1), np.float32)
        notes = ssr.synth_table(4, U, N // 2 + 1, nharm=20, boundary=10, seed=0)
        for name in ("unarmed", "followed"):
            kw = {}
            if name == "followed":
                f = align.ScoreFollower(ctx, S, window=512, max_frames=1024)
                kw = dict(follow=f, classes=align.bin_classes(N))
            st = runtime.ScoreStream(plan, 4, notes, tc, ov, scale=0.3, max_push=block, **kw)
            with ctx.stream_scope():
                ms = []
                for i in range(a.reps + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    tiles = st.push(audio_t[i * block:(i + 1) * block])
                    e1.record()
                    p = torch.ones((4,) + tuple(tiles.shape[:1]) + tuple(tiles.shape[2:]), dtype=torch.float32, device=tiles.device)
                    st.pull(p if int(tiles.shape[0]) else None)
                    torch.cuda.synchronize()
                    if i:
                        ms.append(e0.elapsed_time(e1))
            res["stream_push_ms_" + name] = _median(ms)
            res["stream_bytes_" + name] = st.bytes
            st.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
