"""Wall time of one streaming step of the DSD graph at 513 bins: push one stride of audio (``st * hop`` = 2560 samples, one new
tile), run the tile through the network, pull the finished samples -- and of the push + pull machinery alone, with the network
left out (a fixed ``p``).  Each step ends with a stream synchronisation, as a live caller that plays the samples would.

    python scripts/bench_stream.py [--steps 200] [--warmup 20]

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
    args = ap.parse_args(argv)
    import torch
    import deepconvsep_amd as dcs
    from deepconvsep_amd import runtime
    from deepconvsep_amd.synth import synth_audio, synth_params

    N, hop, F, tc, ov = 1024, 512, 513, 30, 25
    block = (tc - ov) * hop
    sep = dcs.Separator("dsd", synth_params("dsd", tc, F, seed=2), 0.3, tc, ov, 32, F, N, hop, np.hanning)
    ctx = sep.ctx
    total = args.warmup + args.steps
    audio = ctx.to_device(0.5 * synth_audio(block * (total + tc), seed=0), np.float32)
    ss = sep.stream(max_block=block)

    def timed(step):
        for i in range(tc):                             # fill: the first tile needs tc frames
            step(i)
        times = []
        for i in range(tc, tc + total):
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
    print(json.dumps({"bench": "stream", "graph": "dsd", "bins": F, "block_samples": block,
                      "block_audio_ms": round(1e3 * block / 44100.0, 3), "steps": args.steps,
                      "step_ms_median": round(float(np.median(full)), 4), "step_ms_mean": round(float(full.mean()), 4),
                      "step_ms_max": round(float(full.max()), 4),
                      "push_pull_only_ms_median": round(float(np.median(mach)), 4),
                      "push_pull_only_ms_mean": round(float(mach.mean()), 4),
                      "stream_device_bytes": ss.device_bytes, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
