"""Wall time of one streaming step of the DSD graph at 513 bins: push one stride of audio (``st * hop`` = 2560 samples, one new
tile), run the tile through the network, pull the finished samples -- and of the push + pull machinery alone, with the network
left out (a fixed ``p``).  Each step ends with a stream synchronisation, as a live caller that plays the samples would.

    python scripts/bench_stream.py [--steps 200] [--warmup 20] [--channels 2] [--rate 48000] [--score] [--ild [--block 65536]]
                                   [--mwf N [--block 65536]]

``--channels 2`` adds, in the same run, the stereo step on one channel engine (``Separator.stream_channels()``) and the stereo
step composed of three mono ``runtime.Stream`` engines -- L, R and the down-mix -- that share one ``p``, which is what the mono
API allows.  ``--rate R`` adds the step of a ``RateStream`` at ``R`` Hz around the mono stream (and, with ``--channels 2``, around
the stereo one); its block is one stride of audio at that rate.  The launch counts per step are those of the code: append,
frames, tiles, the network call, keep-p, fold, inverse, gather per engine; append and convert per converter.  ``--score`` adds
the score-informed step at the Bach10 shape (frameSize 4096, 2049 bins, four instruments, synthetic weights and a synthetic
score as long as the run: ``Separator.stream_scoreinformed``, one launch more for the masks of the new frames) next to the mono
``bach10`` stream's step at the same shape, and the device bytes of both.  ``--ild`` adds the step of the stereo (ILD) graph's own
stream (``Separator.stream_stereo``: two-channel tiles, ``forward_stereo_tiles``, the per-channel fold; 7 launches + the network
call) next to the mono DSD stream's step, both with blocks of ``--block`` samples (default: one stride), and the bytes of both.
``--mwf N`` adds the steps of the ``dsd`` channel stream and of the ``dsd_ild`` stream with N iterations of the online Wiener
filter per frame (one launch more per step, two when the pull's frames wrap in the rings) next to the same streams' steps without
it, all four with blocks of ``--block`` samples, and the device bytes of the four.

Prints one JSON line: the median and mean wall time per step in milliseconds, next to the block's duration in audio time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--channels", type=int, default=1, choices=(1, 2))
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--ild", action="store_true")
    ap.add_argument("--block", type=int, default=0, help="--ild, --mwf: samples per push (default one stride)")
    ap.add_argument("--mwf", type=int, default=0, help="iterations of the online Wiener filter on the two-channel streams")
    args = ap.parse_args(argv)
    import torch
    import deepconvsep_amd as dcs
    from deepconvsep_amd import runtime
    from deepconvsep_amd.streaming import RateStream
    from deepconvsep_amd.synth import synth_audio, synth_params

    N, hop, F, tc, ov = 1024, 512, 513, 30, 25
    block = (tc - ov) * hop
    sep = dcs.Separator("dsd", synth_params("dsd", tc, F, seed=2), 0.3, tc, ov, 32, F, N, hop, np.hanning)
    ctx = sep.ctx
    total = args.warmup + args.steps
    audio = ctx.to_device(0.5 * synth_audio(block * (total + tc), seed=0), np.float32)
    ss = sep.stream(max_block=block)

    def timed(step, fill=tc):
        for i in range(fill):                           # fill: the first tile needs tc frames
            step(i)
        times = []
        for i in range(fill, fill + total):
            ctx.synchronize()
            t0 = time.perf_counter()
            step(i)
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        return np.array(times[args.warmup:]) * 1e3

    full = timed(lambda i: ss.push_device(audio[i * block:(i + 1) * block]))
    eng = runtime.Stream(sep.plan, sep.net.S, tc, ov, sep.tiler, sep.net.arch.eps_mode, 0.3, max_push=block)
    p = torch.rand((sep.net.S, 1, tc, F), dtype=torch.float32, device=ctx.device) + 0.05

    def machinery(i):
        tiles = eng.push(audio[i * block:(i + 1) * block])
        eng.pull(p if int(tiles.shape[0]) else None)

    mach = timed(machinery)
    extra = {}

    def med(t):
        return round(float(np.median(t)), 4)
    if args.channels == 2:
        a3 = torch.stack([audio, torch.roll(audio, 977), 0.5 * (audio + torch.roll(audio, 977))])
        cs = sep.stream_channels(max_block=block)
        stereo = timed(lambda i: cs.push_device(a3[:, i * block:(i + 1) * block]))
        engines = [runtime.Stream(sep.plan, sep.net.S, tc, ov, sep.tiler, sep.net.arch.eps_mode, 0.3, max_push=block)
                   for _ in range(3)]

        def three(i):
            tiles = [e.push(a3[r, i * block:(i + 1) * block]) for r, e in enumerate(engines)][2]
            q = None
            if int(tiles.shape[0]):
                q = sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:sep.net.S]
            return [e.pull(q) for e in engines]

        composed = timed(three)
        extra.update({"stereo_step_ms_median": med(stereo), "stereo_launches_per_step": 7 + 1,
                      "stereo_three_engines_step_ms_median": med(composed), "stereo_three_engines_launches_per_step": 3 * 7 + 1,
                      "stereo_device_bytes": cs.device_bytes,
                      "stereo_three_engines_device_bytes": sum(e.bytes for e in engines)})
    if args.rate != 44100:
        rblock = block * args.rate // 44100
        raudio = ctx.to_device(0.5 * synth_audio(rblock * (total + tc + 2), seed=1), np.float32)
        rs = RateStream(sep.stream(max_block=rblock), args.rate)
        rated = timed(lambda i: rs.push_device(raudio[i * rblock:(i + 1) * rblock]))
        extra.update({"rate": args.rate, "rate_block_samples": rblock, "rate_step_ms_median": med(rated),
                      "rate_launches_per_step": 7 + 1 + 4, "rate_device_bytes": rs.device_bytes})
        if args.channels == 2:
            r3 = torch.stack([raudio, torch.roll(raudio, 977), 0.5 * (raudio + torch.roll(raudio, 977))])
            rs2 = RateStream(sep.stream_channels(max_block=rblock), args.rate)
            rated2 = timed(lambda i: rs2.push_device(r3[:, i * rblock:(i + 1) * rblock]))
            extra.update({"rate_stereo_step_ms_median": med(rated2), "rate_stereo_device_bytes": rs2.device_bytes})
    if args.score:
        N4, F4 = 4096, 2049
        n_frames = block * (total + tc) // hop + 3
        rs_ = np.random.RandomState(3)
        nharm, per_note = 20, 35                                      # back-to-back notes of 35 frames, 20 harmonic bands each
        n_notes = n_frames // per_note + 1
        melody = np.zeros((4, n_notes, 2 * nharm + 3))
        for j in range(4):
            for m in range(n_notes):
                b0 = int(rs_.randint(8, 60))                          # the fundamental's bin
                melody[j, m, :3] = (m * per_note, min(n_frames, (m + 1) * per_note), 40 + j)
                for k in range(1, nharm + 1):
                    if k * b0 + 3 <= F4:
                        melody[j, m, 1 + 2 * k:3 + 2 * k] = (k * b0 - 2, k * b0 + 3)
        sep_si = dcs.Separator("bach10_si", synth_params("bach10_si", tc, F4, seed=2), 0.3, tc, ov, 32, F4, N4, hop,
                               dcs.blackmanharris, tiler='library', ctx=ctx)
        sep_b = dcs.Separator("bach10", synth_params("bach10", tc, F4, seed=2), 0.3, tc, ov, 32, F4, N4, hop, dcs.blackmanharris,
                              ctx=ctx)
        sc, sb = sep_si.stream_scoreinformed(melody, max_block=block), sep_b.stream(max_block=block)
        scored = timed(lambda i: sc.push_device(audio[i * block:(i + 1) * block]))
        plain = timed(lambda i: sb.push_device(audio[i * block:(i + 1) * block]))
        extra.update({"score_bins": F4, "score_instruments": 4, "score_note_rows": 4 * n_notes,
                      "score_step_ms_median": med(scored), "score_launches_per_step": 8 + 1,
                      "bach10_step_ms_median": med(plain), "score_device_bytes": sc.device_bytes,
                      "bach10_device_bytes": sb.device_bytes})
    if args.ild:
        B = args.block or block
        fill = -(-tc * hop // B) + 1
        base = 0.5 * synth_audio(8 * B, seed=4, channels=2)                                   # repeated: the values do not matter
        a2 = ctx.to_device(np.ascontiguousarray(base.T), np.float32).repeat(1, (total + fill) // 8 + 1)
        sep_i = dcs.Separator("dsd_ild", synth_params("dsd_ild", tc, F, seed=7), 0.3, tc, ov, 32, F, N, hop, np.hanning,
                              tiler='library', ctx=ctx)
        si, sm = sep_i.stream_stereo(max_block=B), sep.stream(max_block=B)
        ild = timed(lambda i: si.push_device(a2[:, i * B:(i + 1) * B]), fill)
        mono = timed(lambda i: sm.push_device(a2[0, i * B:(i + 1) * B]), fill)
        extra.update({"ild_block_samples": B, "ild_step_ms_median": med(ild), "ild_step_ms_max": round(float(ild.max()), 4),
                      "ild_mono_dsd_step_ms_median": med(mono), "ild_launches_per_step": 7 + 1,
                      "ild_device_bytes": si.device_bytes, "ild_mono_dsd_device_bytes": sm.device_bytes})
    if args.mwf:
        B = args.block or block
        fill = -(-tc * hop // B) + 1
        base = 0.5 * synth_audio(8 * B, seed=4, channels=2)                                   # repeated: the values do not matter
        a2 = ctx.to_device(np.ascontiguousarray(base.T), np.float32).repeat(1, (total + fill) // 8 + 1)
        a3 = torch.cat([a2, 0.5 * (a2[:1] + a2[1:])])
        sep_i = dcs.Separator("dsd_ild", synth_params("dsd_ild", tc, F, seed=7), 0.3, tc, ov, 32, F, N, hop, np.hanning,
                              tiler='library', ctx=ctx)
        extra.update({"mwf_iters": args.mwf, "mwf_block_samples": B, "mwf_frames_per_step": B // hop})
        for tag, make, sig in (("channels", sep.stream_channels, a3), ("ild", sep_i.stream_stereo, a2)):
            for name, iters in (("plain", 0), ("mwf", args.mwf)):
                st = make(max_block=B, mwf_iters=iters)
                t = timed(lambda i: st.push_device(sig[:, i * B:(i + 1) * B]), fill)
                extra.update({"mwf_%s_%s_step_ms_median" % (tag, name): med(t),
                              "mwf_%s_%s_step_ms_max" % (tag, name): round(float(t.max()), 4),
                              "mwf_%s_%s_device_bytes" % (tag, name): st.device_bytes})
    print(json.dumps({"bench": "stream", "graph": "dsd", "bins": F, "block_samples": block,
                      "block_audio_ms": round(1e3 * block / 44100.0, 3), "steps": args.steps,
                      "step_ms_median": round(float(np.median(full)), 4), "step_ms_mean": round(float(full.mean()), 4),
                      "step_ms_max": round(float(full.max()), 4),
                      "push_pull_only_ms_median": round(float(np.median(mach)), 4),
                      "push_pull_only_ms_mean": round(float(mach.mean()), 4),
                      "stream_device_bytes": ss.device_bytes, "launches_per_step": 7 + 1, **extra,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
