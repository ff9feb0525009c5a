#!/usr/bin/env python3
"""Times the deep score-informed graph build_ca_1x1 (DCS_ARCH_BACH10_SI_1X1) at the trainer's shape, F = 2049 bins,
time_context 30: one batch of 32 tiles through the live part of the network (dcs_model_forward_masked), and the whole
score-informed path on a 30 s clip (dcs_separate_scoreinformed, library tiler, overlap 25), both with device events after
a warm-up.  Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python3 ...`."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import score  # noqa: E402
from deepconvsep_amd.arch import ARCHS  # noqa: E402
from deepconvsep_amd.runtime import Network, default_context  # noqa: E402
from deepconvsep_amd.synth import synth_audio, synth_params, synth_score_text  # noqa: E402

PEAK_F32_TFLOPS = 157.3


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    tc, F = 30, 2049
    ctx = default_context()
    params = synth_params("bach10_si_1x1", tc, F, seed=1)
    net = Network(ctx, "bach10_si", params, tc, F)
    x = ctx.to_device(np.random.RandomState(0).uniform(0, 1, (a.tiles, 4, tc, F)).astype(np.float32), np.float32)
    for _ in range(a.warmup):
        net.forward_masked(x)
    ms_batch = timed(lambda: net.forward_masked(x), a.reps)
    gflop = ARCHS["bach10_si_1x1"].flops_per_tile(tc, F, live_only=True) / 1e9
    tflops = gflop * a.tiles / ms_batch      # GFLOP / ms = TFLOP / s
    L = int(a.seconds * 44100)
    audio = synth_audio(L, seed=3)
    with tempfile.TemporaryDirectory() as d:
        names = []
        for i in range(4):
            names.append("inst%d.txt" % i)
            with open(os.path.join(d, names[-1]), "w") as fh:
                fh.write(synth_score_text(60 + i, a.seconds + 0.5, 40 + 5 * i, 64 + 6 * i))
        melody = score.melody_table(names, d, int(np.ceil(L / 512.0)) + 2, 44100, 512, 4096)
    sep = dcs.Separator("bach10_si", params, 0.3, tc, 25, 32, F, 4096, 512, dcs.blackmanharris, tiler='library',
                        score_normalise='sum', score_mixture='sum')
    ad = ctx.to_device(audio.astype(np.float32), np.float32)
    for _ in range(a.warmup):
        sep.separate_scoreinformed_device(ad, melody)
    ms_clip = timed(lambda: sep.separate_scoreinformed_device(ad, melody), max(1, a.reps // 2))
    print(json.dumps({"workload": "bach10_si_1x1", "F": F, "time_context": tc, "tiles_per_batch": a.tiles,
                      "ms_per_batch": round(ms_batch, 3), "live_gflop_per_tile": round(gflop, 3),
                      "tflops": round(tflops, 2), "fraction_of_f32_peak": round(tflops / PEAK_F32_TFLOPS, 3),
                      "clip_seconds": a.seconds, "clip_tiles": sep.net.last_tiles, "ms_per_clip": round(ms_clip, 2)}))


if __name__ == "__main__":
    main()
