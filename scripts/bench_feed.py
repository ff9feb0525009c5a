#!/usr/bin/env python3
"""Feed benchmark of the augmented hiphop trainer: what one batch of training windows costs when it is cut from resident
feature files (``dcs_trainer_gather``, the feed of ``FeatureWindows``), when it is rendered and transformed from resident
source audio with the 14 circular-shift variants (``dcs_trainer_gather_render``, the feed of ``RenderedWindows``), and what
the training step it feeds costs (``dcs_trainer_step``, mode 2).  Prints one JSON line.

    python scripts/bench_feed.py [--batch 32] [--time_context 30] [--seconds 95] [--songs 2] [--steps 200] [--warmup 20]
                                 [--repeats 5] [--source cs|score|score_si]

``--source score`` measures the feed of the Bach10 RWC trainer instead (``dcs_trainer_gather_score_render``, the feed of
``ScoreRenderedWindows``): frame 4096 / hop 512 (F = 2049), four tracks, ``--songs`` virtual files of ``--seconds`` (default
30) assembled from a synthetic note bank (4 instruments x 24 notes of 2 s) by seeded scores of about two notes per second
and track, consecutive notes overlapping by 0.2 s.  Against it: (a) ``dcs_trainer_gather`` on the float64 render of the same
files cast to float32 and resident -- what the new feed replaces -- and (b) ``dcs_trainer_gather_render`` at the same shape
on whole-signal tracks of the same length, which does the same FFT work without the note lookup.

``--source score_si`` measures the feed of the score-informed trainer on the same synthetic files
(``dcs_trainer_gather_score_informed_render``, the feed of ``ScoreInformedRenderedWindows``): every note also has a row in
its file's mask table (its frames, 20 harmonic bands of +-50 cents).  Against it, at the same windows: the existing
``dcs_trainer_gather_score_render`` (the transforms without the masks) and the file-based ``dcs_trainer_gather_score`` on
the float32 render of the same files (the masks without the transforms) -- the two launches the new one fuses.  The new
feed's outputs are compared bit for bit with that composition before anything is timed.  ``--only informed|render|masks``
times one of the three alone, for runs that alternate between fresh processes.

The data: ``--songs`` seeded songs of ``--seconds`` at 44.1 kHz (four sources each), frame 1024 / hop 512, so F = 513; the cs
variants of every song in 30 s chunks; windows='all', seeded permutation.  The resident files of the gather are the float64
render of the same virtual files cast to float32 -- what compute_features.py --augment cs would have written -- so both
feeds serve the same windows.  Each of the three is timed alone: ``--warmup`` calls, a synchronise, ``--steps`` calls on
changing batches of the permutation with no host synchronisation inside, a synchronise; ms = wall time / steps, and the
window is repeated ``--repeats`` times (median and spread are reported).  The window tables are uploaded before the timed
window (the host's per-batch copy of a 32 x 2 int32 table is the same for both feeds).  A kernel breakdown comes from
``rocprofv3 --kernel-trace --stats -- python scripts/bench_feed.py``, in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, n_args, steps, warmup, repeats, sync):
    for i in range(warmup):
        fn(i % n_args)
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i % n_args)
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / steps)
    return out


def synthetic_score_files(songs, seconds, sr, S):
    """The note bank and the seeded virtual files of the score sources; per file and track the pitch index of every note."""
    from deepconvsep_amd import rwc, score_render
    from deepconvsep_amd.synth import synth_audio
    size = int(seconds * sr)
    bank = rwc.NoteBank.from_arrays({(i, p): synth_audio(2 * sr, seed=1000 + 24 * i + p, silence=False) * 0.25
                                     for i in range(S) for p in range(24)}, sr=sr)
    rs = np.random.RandomState(0)
    sfiles, pitches, n_notes = [], [], 0
    for f in range(songs):
        tracks, pt = [], []
        for i in range(S):
            b = np.sort((np.arange(0, seconds, 0.5) + rs.uniform(0, 0.2, int(np.ceil(seconds / 0.5)))) * sr).astype(np.int64)
            b = b[b < size]
            notes, ps = [], []
            for x in b:
                p = int(rs.randint(24))
                e = bank.index[(i, p)]
                notes.append((int(x), e.offset, int(min(e.length, 0.7 * sr, size - x))))
                ps.append(p)
            tracks.append(tuple(notes))
            pt.append(ps)
            n_notes += len(notes)
        sfiles.append(score_render.ScoreFile("file_%d" % f, size, tuple(tracks)))
        pitches.append(pt)
    return bank, sfiles, pitches, n_notes


def main_score_si(a):
    import torch
    import deepconvsep_amd as dcs
    from deepconvsep_amd import _lib, score_render
    from deepconvsep_amd.runtime import _ptr, default_context
    from deepconvsep_amd.score import harmonic_bins
    from deepconvsep_amd.separation import blackmanharris
    ctx = default_context()
    sr, frame, hop, B, tc, S, nh = 44100, 4096, 512, a.batch, a.time_context, 4, 20
    F, width = frame // 2 + 1, 2 * nh + 3
    seconds = 30.0 if a.seconds == 95.0 else a.seconds
    bank, files0, pitches, n_notes = synthetic_score_files(a.songs, seconds, sr, S)
    bins = {p: np.asarray(harmonic_bins(48 + p, size=frame, interval=50, tuning_freq=440, nharmonics=nh, sampleRate=sr))
            for p in range(24)}
    sfiles = []
    for sf, pt in zip(files0, pitches):
        P = max(len(t) for t in sf.tracks)
        table = np.zeros((S, P, width))
        for i, (t, ps) in enumerate(zip(sf.tracks, pt)):
            for m, ((b, _, ln), p) in enumerate(zip(t, ps)):
                table[i, m, :3] = (b // hop, (b + ln) // hop + 1, 48 + p)
                table[i, m, 3:3 + 2 * len(bins[p]):2] = bins[p][:, 0]
                table[i, m, 4:4 + 2 * len(bins[p]):2] = bins[p][:, 1]
        sfiles.append(score_render.ScoreInformedFile(sf.name, sf.size, sf.tracks, table, table))
    sw = score_render.ScoreInformedRenderedWindows(bank, sfiles, 'e', time_context=tc, overlap=a.overlap, mult_factor=0.3,
                                                   windows='all', batch_size=B, seed=0, ctx=ctx, frameSize=frame, hopSize=hop,
                                                   window=blackmanharris)
    sw._upload()
    # the file-based feed: the float32 render of the same files, resident, with the same mask tables
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=sr, window=blackmanharris, precision='float32')
    blocks, files, off = [], [], 0
    for sf in sfiles:
        b = score_render.render_score_features(tt, bank, sf)
        blocks.append(ctx.to_device(b, np.float32).reshape(-1))
        files.append((off, b.shape[1]))
        off += b.size
    with ctx.stream_scope():
        data_d = torch.cat(blocks)
        del blocks
        files_d = torch.from_numpy(np.asarray(files, dtype=np.int64)).to(ctx.device)
        perm = np.random.RandomState(0).permutation(sw.total)
        n_batches = min(sw.iteration_size, 64)
        wins = [torch.from_numpy(np.ascontiguousarray(sw.table[perm[i * B:(i + 1) * B]])).to(ctx.device) for i in range(n_batches)]
        x = torch.empty((B, S, tc, F), dtype=torch.float32, device=ctx.device)
        t = torch.empty((B, S, tc, F), dtype=torch.float32, device=ctx.device)
        x2, t2 = torch.empty_like(x), torch.empty_like(t)
        x3 = torch.empty((B, 1, tc, F), dtype=torch.float32, device=ctx.device)
        t3 = torch.empty_like(t)

        def informed(i):
            _lib.check(ctx._lib.dcs_trainer_gather_score_informed_render(
                ctx._h, sw._plan._h, _ptr(sw._bank_d), bank.length, _ptr(sw._notes_d), len(sw.notes), _ptr(sw._rows_d),
                len(sw.rows), _ptr(sw._masks_d), sw.mask_len, _ptr(sw._mask_files_d), width, _ptr(wins[i]), B, tc, S, 0.3,
                _ptr(x), _ptr(t)))

        def masks(i):
            _lib.check(ctx._lib.dcs_trainer_gather_score(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(sw._masks_d),
                                                         _ptr(sw._mask_files_d), _ptr(wins[i]), B, tc, F, S, width, 0.3, _ptr(x2),
                                                         _ptr(t2)))

        def render(i):
            _lib.check(ctx._lib.dcs_trainer_gather_score_render(
                ctx._h, sw._plan._h, _ptr(sw._bank_d), bank.length, _ptr(sw._notes_d), len(sw.notes), _ptr(sw._rows_d),
                len(sw.rows), _ptr(wins[i]), B, tc, S, 0.3, _ptr(x3), _ptr(t3)))
        equal = True
        for i in range(min(n_batches, 4)):
            informed(i)
            masks(i)
            equal = equal and bool(torch.equal(x, x2)) and bool(torch.equal(t, t2))
        sync = ctx.synchronize
        n, r, m = [], [], []
        for _ in range(a.repeats):          # alternating windows of the three feeds (--only: of one of them)
            if a.only in ("all", "informed"):
                n += timed(informed, n_batches, a.steps, a.warmup, 1, sync)
            if a.only in ("all", "render"):
                r += timed(render, n_batches, a.steps, a.warmup, 1, sync)
            if a.only in ("all", "masks"):
                m += timed(masks, n_batches, a.steps, a.warmup, 1, sync)
    med = lambda v: float(np.median(v)) if v else float("nan")  # noqa: E731
    lo_hi = lambda v: [round(min(v), 4), round(max(v), 4)] if v else []  # noqa: E731
    print(json.dumps(dict(
        source="score_si", batch=B, time_context=tc, feat_size=F, files=a.songs, seconds=seconds, notes=n_notes,
        windows=sw.total, bank_mb=round(bank.length * 4 / 1e6, 1), features_mb=round(off * 4 / 1e6, 1),
        mask_table_kb=round(sw.mask_len * 4 / 1e3, 1), frames_per_batch=B * tc * (1 + S),
        only=a.only, gather_score_informed_render_ms=round(med(n), 4), gather_score_informed_render_ms_min_max=lo_hi(n),
        gather_score_render_ms=round(med(r), 4), gather_score_render_ms_min_max=lo_hi(r),
        gather_score_ms=round(med(m), 4), gather_score_ms_min_max=lo_hi(m),
        informed_over_sum=round(med(n) / (med(r) + med(m)), 3), equal_to_the_composition=equal,
        steps=a.steps, warmup=a.warmup, repeats=a.repeats)), flush=True)


def main_score(a):
    import torch
    import deepconvsep_amd as dcs
    from deepconvsep_amd import _lib, augment, score_render
    from deepconvsep_amd.runtime import _ptr, default_context
    from deepconvsep_amd.separation import blackmanharris
    from deepconvsep_amd.synth import synth_audio
    ctx = default_context()
    sr, frame, hop, B, tc, S = 44100, 4096, 512, a.batch, a.time_context, 4
    F = frame // 2 + 1
    seconds = 30.0 if a.seconds == 95.0 else a.seconds
    size = int(seconds * sr)
    bank, sfiles, _, n_notes = synthetic_score_files(a.songs, seconds, sr, S)
    sw = score_render.ScoreRenderedWindows(bank, sfiles, tc, a.overlap, 0.3, 'all', B, 0, ctx, frame, hop, blackmanharris)
    sw._upload()
    # (b) whole-signal tracks of the same length: the same table of windows
    signals = {(f, i): synth_audio(size, seed=2000 + S * f + i) * 0.25 for f in range(a.songs) for i in range(S)}
    vfiles = [augment.VirtualFile(tuple(augment.Track((f, i), 0, 1.0, 1 + i) for i in range(S)), 1.0, size, ((0, size),),
                                  ("whole_%d" % f,)) for f in range(a.songs)]
    rw = augment.RenderedWindows(signals, vfiles, tc, a.overlap, 0.3, 'all', B, 0, ctx, frame, hop, blackmanharris)
    rw._upload()
    assert np.array_equal(rw.table, sw.table)
    # (a) the same windows from resident float32 feature blocks
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=sr, window=blackmanharris)
    blocks, files, off = [], [], 0
    for sf in sfiles:
        b = score_render.render_score_features(tt, bank, sf)
        blocks.append(ctx.to_device(b, np.float32).reshape(-1))
        files.append((off, b.shape[1]))
        off += b.size
    with ctx.stream_scope():
        data_d = torch.cat(blocks)
        del blocks
        files_d = torch.from_numpy(np.asarray(files, dtype=np.int64)).to(ctx.device)
        perm = np.random.RandomState(0).permutation(sw.total)
        n_batches = min(sw.iteration_size, 64)
        wins = [torch.from_numpy(np.ascontiguousarray(sw.table[perm[i * B:(i + 1) * B]])).to(ctx.device) for i in range(n_batches)]
        x = torch.empty((B, 1, tc, F), dtype=torch.float32, device=ctx.device)
        t = torch.empty((B, S, tc, F), dtype=torch.float32, device=ctx.device)
        x2, t2 = torch.empty_like(x), torch.empty_like(t)
        x3, t3 = torch.empty_like(x), torch.empty_like(t)

        def gather(i):
            _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(wins[i]), B, tc, F, 0.3, _ptr(x),
                                                   _ptr(t)))

        def render(i):
            _lib.check(ctx._lib.dcs_trainer_gather_render(ctx._h, rw._plan._h, _ptr(rw._bank.tensor), rw._bank.length,
                                                          _ptr(rw._rows_d), _ptr(rw._gains_d), len(rw.rows), _ptr(wins[i]), B, tc,
                                                          S, 0.3, _ptr(x2), _ptr(t2)))

        def score(i):
            _lib.check(ctx._lib.dcs_trainer_gather_score_render(
                ctx._h, sw._plan._h, _ptr(sw._bank_d), bank.length, _ptr(sw._notes_d), len(sw.notes), _ptr(sw._rows_d),
                len(sw.rows), _ptr(wins[i]), B, tc, S, 0.3, _ptr(x3), _ptr(t3)))
        err = 0.0
        for i in range(min(n_batches, 4)):
            gather(i)
            score(i)
            err = max(err, float((x - x3).abs().max()), float((t - t3).abs().max()))
        sync = ctx.synchronize
        g = timed(gather, n_batches, a.steps, a.warmup, a.repeats, sync)
        r = timed(render, n_batches, a.steps, a.warmup, a.repeats, sync)
        c = timed(score, n_batches, a.steps, a.warmup, a.repeats, sync)
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps(dict(
        source="score", batch=B, time_context=tc, feat_size=F, files=a.songs, seconds=seconds, notes=n_notes, windows=sw.total,
        bank_mb=round(bank.length * 4 / 1e6, 1), features_mb=round(off * 4 / 1e6, 1), frames_per_batch=B * tc * (1 + S),
        gather_ms=round(med(g), 4), gather_ms_min_max=[round(min(g), 4), round(max(g), 4)],
        gather_render_ms=round(med(r), 4), gather_render_ms_min_max=[round(min(r), 4), round(max(r), 4)],
        gather_score_render_ms=round(med(c), 4), gather_score_render_ms_min_max=[round(min(c), 4), round(max(c), 4)],
        score_over_gather=round(med(c) / med(g), 2), score_over_render=round(med(c) / med(r), 3),
        max_abs_difference_of_the_feeds=err, steps=a.steps, warmup=a.warmup, repeats=a.repeats)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--seconds", type=float, default=95.0)
    ap.add_argument("--songs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--source", choices=("cs", "score", "score_si"), default="cs")
    ap.add_argument("--only", choices=("all", "informed", "render", "masks"), default="all",
                    help="score_si: time one of the three feeds alone (a run per feed, each in a fresh process)")
    a = ap.parse_args()
    if a.source == "score":
        return main_score(a)
    if a.source == "score_si":
        return main_score_si(a)
    import torch
    import deepconvsep_amd as dcs
    from deepconvsep_amd import _lib, augment
    from deepconvsep_amd.runtime import _ptr, default_context
    from deepconvsep_amd.separation import blackmanharris
    from deepconvsep_amd.synth import synth_audio
    from deepconvsep_amd.training import Trainer, glorot_init
    ctx = default_context()
    sr, frame, hop, B, tc = 44100, 1024, 512, a.batch, a.time_context
    F = frame // 2 + 1
    signals, vfiles = {}, []
    for s in range(a.songs):
        ln = {}
        for j, name in enumerate(augment.CHANNELS):
            n = int(a.seconds * sr) + 1000 * j + 333 * s
            signals[(s, name)] = synth_audio(n, seed=100 + 4 * s + j) * 0.25
            ln[name] = n
        vfiles += augment.virtual_files('cs', ln, sr=sr, song=s)
    rw = augment.RenderedWindows(signals, vfiles, tc, a.overlap, 0.3, 'all', B, 0, ctx, frame, hop, blackmanharris)
    rw._upload()
    # the same windows from resident float32 feature blocks
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=sr, window=blackmanharris)
    bank64 = augment.Bank(signals, np.float64, ctx)
    blocks, files, off = [], [], 0
    for vf in vfiles:
        for b in augment.render_features(tt, bank64, vf):
            blocks.append(ctx.to_device(b, np.float32).reshape(-1))
            files.append((off, b.shape[1]))
            off += b.size
    del bank64
    with ctx.stream_scope():
        data_d = torch.cat(blocks)
        del blocks
        files_d = torch.from_numpy(np.asarray(files, dtype=np.int64)).to(ctx.device)
        perm = np.random.RandomState(0).permutation(rw.total)
        n_batches = min(rw.iteration_size, 64)
        wins = [torch.from_numpy(np.ascontiguousarray(rw.table[perm[i * B:(i + 1) * B]])).to(ctx.device) for i in range(n_batches)]
        x = torch.empty((B, 1, tc, F), dtype=torch.float32, device=ctx.device)
        t = torch.empty((B, 4, tc, F), dtype=torch.float32, device=ctx.device)
        x2, t2 = torch.empty_like(x), torch.empty_like(t)

        def gather(i):
            _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(wins[i]), B, tc, F, 0.3, _ptr(x),
                                                   _ptr(t)))

        def render(i):
            _lib.check(ctx._lib.dcs_trainer_gather_render(ctx._h, rw._plan._h, _ptr(rw._bank.tensor), rw._bank.length,
                                                          _ptr(rw._rows_d), _ptr(rw._gains_d), len(rw.rows), _ptr(wins[i]), B, tc,
                                                          4, 0.3, _ptr(x2), _ptr(t2)))
        # the two feeds serve the same windows: largest difference over the batches, before anything is timed
        err = 0.0
        for i in range(min(n_batches, 8)):
            gather(i)
            render(i)
            err = max(err, float((x - x2).abs().max()), float((t - t2).abs().max()))
        trainer = Trainer(ctx, params=glorot_init('dsd', tc, F, 0), batch_size=B, time_context=tc, feat_size=F)

        def step(i):
            trainer.run(x, t, 2)
        sync = ctx.synchronize
        g = timed(gather, n_batches, a.steps, a.warmup, a.repeats, sync)
        r = timed(render, n_batches, a.steps, a.warmup, a.repeats, sync)
        s = timed(step, n_batches, a.steps, a.warmup, a.repeats, sync)
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps(dict(
        batch=B, time_context=tc, feat_size=F, songs=a.songs, seconds=a.seconds, virtual_files=len(rw.rows), windows=rw.total,
        bank_mb=round(rw._bank.length * 4 / 1e6, 1), features_mb=round(off * 4 / 1e6, 1), frames_per_batch=B * tc * 5,
        gather_ms=round(med(g), 4), gather_ms_min_max=[round(min(g), 4), round(max(g), 4)],
        gather_render_ms=round(med(r), 4), gather_render_ms_min_max=[round(min(r), 4), round(max(r), 4)],
        step_ms=round(med(s), 4), step_ms_min_max=[round(min(s), 4), round(max(s), 4)],
        render_over_gather=round(med(r) / med(g), 2), render_over_step=round(med(r) / med(s), 3),
        max_abs_difference_of_the_feeds=err, steps=a.steps, warmup=a.warmup, repeats=a.repeats)), flush=True)


if __name__ == "__main__":
    main()
