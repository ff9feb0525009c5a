#!/usr/bin/env python3
"""The sample-rate converter (``dcs_resample_f32``) on the MI355X at the sizes ``Separator.separate(..., sample_rate=)`` runs
it: a 10 s mono clip 48 000 -> 44 100 Hz in front of the separator and its S = 4 sources 44 100 -> 48 000 Hz behind it, next
to the DSD separator's own device time for that clip.  Both placements of the polyphase table (copied into LDS per
workgroup | read from global memory, L2-resident; ``DCS_RESAMPLE_TABLE``) are timed in one process, alternating, ``--rounds``
rounds of ``--reps`` back-to-back launches between two HIP events each.  Prints one JSON line.

    python scripts/bench_resample.py [--seconds 10] [--reps 200] [--rounds 7]

The floor is the traffic of the signal alone, 4 (n_in + n_out) n_clips bytes, at the HBM rate below; the table (43 KB for
these two ratios) is not counted.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0              # MI355X spec HBM3E bandwidth, not measured here


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs the MI355X")
    import deepconvsep_amd as dcs
    from deepconvsep_amd.resample import Resampler
    from deepconvsep_amd.runtime import default_context
    from deepconvsep_amd.synth import synth_audio

    ctx = default_context()

    def event_ms(fn, reps):
        """ms per call of `reps` calls enqueued back to back between two events"""
        with ctx.stream_scope():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / reps

    cases = {"front_48000_to_44100_1_clip": (48000, 44100, 1), "back_44100_to_48000_4_clips": (44100, 48000, 4)}
    result = {"seconds": a.seconds, "reps": a.reps, "rounds": a.rounds, "hbm_TBs": HBM_PEAK_TBS}
    for name, (fi, fo, n_clips) in cases.items():
        L = int(a.seconds * fi)
        x = ctx.to_device(np.stack([synth_audio(L, seed=k, silence=False) for k in range(n_clips)]), np.float32)
        plans, outs = {}, {}
        for where in ("lds", "l2"):
            os.environ["DCS_RESAMPLE_TABLE"] = where
            plans[where] = Resampler(ctx, fi, fo)
        del os.environ["DCS_RESAMPLE_TABLE"]
        M = plans["lds"].out_length(L)
        buf = ctx.empty((n_clips, M), np.float32)
        times = {w: [] for w in plans}
        for w, rs in plans.items():
            event_ms(lambda: rs(x, out=buf), 10)                                                 # warm
            outs[w] = ctx.to_host(buf).copy()
        for _ in range(a.rounds):
            for w, rs in plans.items():
                times[w].append(event_ms(lambda: rs(x, out=buf), a.reps))
        nbytes = 4 * (L + M) * n_clips
        floor_ms = nbytes / (HBM_PEAK_TBS * 1e12) * 1e3
        entry = {"n_in": L, "n_out": M, "clips": n_clips, "signal_MB": round(nbytes / 1e6, 3), "floor_ms": round(floor_ms, 5),
                 "placements_agree_bitwise": bool(np.array_equal(outs["lds"], outs["l2"]))}
        for w in plans:
            med = float(np.median(times[w]))
            entry["table_%s_ms_median" % w] = round(med, 5)
            entry["table_%s_ms_min" % w] = round(min(times[w]), 5)
            entry["table_%s_floor_fraction" % w] = round(floor_ms / med, 4)
        result[name] = entry
        for rs in plans.values():
            rs.close()

    # the separator's own device time for the same clip at 44 100 Hz (STFT -> network -> iSTFT, one dcs_separate call)
    sep = dcs.Separator("dsd", dcs.glorot_init("dsd"), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, ctx=ctx)
    clip = ctx.to_device(synth_audio(int(a.seconds * 44100), seed=9, silence=False), np.float32)
    run = lambda: sep.net.separate(sep.plan, clip, sep.overlap, sep.tiler, sep.scale_factor, None, sep.tie_mode)
    event_ms(run, 5)
    sep_ms = [event_ms(run, max(1, a.reps // 10)) for _ in range(a.rounds)]
    result["dsd_separator_same_clip_ms_median"] = round(float(np.median(sep_ms)), 4)
    result["dsd_separator_same_clip_ms_min"] = round(min(sep_ms), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
