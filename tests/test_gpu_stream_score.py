"""Score-informed separation on a stream (``dcs_stream_create_score``, csrc/stream.hip; include/dcs.h has the contract).

Machinery tests drive ``runtime.ScoreStream`` with the synthetic tables of tests/score_stream_ref.py and a synthetic positive
``p`` per tile, no network: the tiles are held bit for bit to ``M * (scale * mag)`` at the device's own magnitudes, the estimates
to ``chanmask_ref.bound`` on the float32 score-informed mixture, the samples to ``stft_ref.BOUND_INV``, and the bits must not
depend on how the signal is cut.  End-to-end tests run the three score-informed graphs on one second of audio at 1024 / 513,
against the float64 whole-file composition at the product's own ``p`` and against the oracle's ``separate_scoreinformed``.
"""
import json
import os
import subprocess
import sys
from ctypes import POINTER, byref, c_double, c_int64, c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import _lib, runtime, score  # noqa: E402
from deepconvsep_amd.arch import ARCHS, EPS_A, EPS_B, TILER_LIBRARY, TILER_SCRIPT, live_params  # noqa: E402
from deepconvsep_amd.resample import ResampleCounts, out_length, ratio  # noqa: E402
from deepconvsep_amd.streaming import RateStream, ScoreStreamSeparator, StreamCounts  # noqa: E402
from deepconvsep_amd.synth import synth_audio, synth_params, synth_score_text  # noqa: E402
from oracle import pipeline, stft_np, tiling_np  # noqa: E402

import chanmask_ref  # noqa: E402
import score_stream_ref as ssr  # noqa: E402
import stft_ref  # noqa: E402
import stream_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TILER_CODE = {tiling_np.SCRIPT: TILER_SCRIPT, tiling_np.LIBRARY: TILER_LIBRARY}
EPS_CODE = {"A": EPS_A, "B": EPS_B}

# (frameSize, hop, time_context, overlap, window), instruments, sources, normalise, mixture
CASES = (
    ((64, 16, 8, 5, "hanning"), 1, 1, "max", "ch0"),
    ((64, 32, 8, 1, "hanning"), 3, 2, "sum", "sum"),
    ((128, 32, 30, 29, "hanning"), 4, 4, "max", "sum"),
    ((1024, 512, 30, 25, "hanning"), 4, 4, "sum", "ch0"),
    ((4096, 512, 30, 25, "blackmanharris"), 4, 4, "max", "ch0"),
)


def _case_id(case):
    return "%s_i%d_S%d_%s_%s" % ((stream_ref.shape_id(case[0]),) + case[1:])


def _drive(stream, audio_t, sizes, seed, counts):
    """the signal through the stream in blocks of ``sizes`` with the synthetic p of stream_ref.tile_p -> host arrays; every count
    the library returned is checked against StreamCounts on the way"""
    ctx = stream.ctx
    mags, phs, ests, pcms, tls, pos, k = [], [], [], [], [], 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = (counts.frames(pos), counts.tiles(pos), counts.emitted(pos))
        tiles, mag, ph = stream.push(audio_t[pos:pos + n] if n else None, last=last, want_frames=True)
        pos += n
        assert stream.last_frames == counts.frames(pos, last) - before[0] == int(mag.shape[0])
        assert stream.last_tiles == counts.tiles(pos, last) - before[1] == int(tiles.shape[0])
        assert stream.last_tiles <= stream.max_tiles and tuple(tiles.shape[1:]) == (stream.ninst, stream.tc, stream.F)
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stream_ref.tile_p(k + j, stream.S, stream.tc, stream.F, seed) for j in range(nt)], axis=1),
                              np.float32)
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        assert stream.last_samples == counts.emitted(pos, last) - before[2] == int(pcm.shape[1])
        mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        tls.append(ctx.to_host(tiles))
    return dict(mag=np.concatenate(mags), phase=np.concatenate(phs), est=np.concatenate(ests, axis=1),
                pcm=np.concatenate(pcms, axis=1), tiles=np.concatenate(tls), n_tiles=k)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_machinery_against_float64_and_across_partitions(case):
    shape, ninst, S, normalise, mixture = case
    N, h, tc, ov, wname = shape
    i = CASES.index(case)
    tiler, conv = stream_ref.TILERS[i % 2], chanmask_ref.CONVENTIONS[(i // 2) % 2]
    L = stream_ref.lengths(N, h, tc, ov)[i % 3]
    win = stream_ref.window(wname, N)
    F, scale, seed = N // 2 + 1, 0.3, 13 * i + 1
    T = stft_np.frame_count(L, h)
    notes = ssr.synth_table(ninst, T, F, nharm=4, boundary=2 * (tc - ov), seed=i)
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, win)
    audio = 0.5 * synth_audio(L, seed=5 + i)
    audio_t = ctx.to_device(audio, np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)
    stream = runtime.ScoreStream(plan, S, notes, tc, ov, TILER_CODE[tiler], EPS_CODE[conv], scale, max_push=L,
                                 normalise=normalise, mixture=mixture)
    nbytes = stream.bytes
    mono = runtime.Stream(plan, S, tc, ov, TILER_CODE[tiler], EPS_CODE[conv], scale, max_push=L)
    assert nbytes > mono.bytes and stream.max_tiles == counts.max_tiles(L)
    mono.close()
    runs = {}
    for kind in ("one", "hop", "empty_last"):
        stream.reset()                                                # reset keeps the score
        runs[kind] = _drive(stream, audio_t, stream_ref.partition(kind, L, h, seed=L), seed, counts)
    one = runs["one"]
    n_tiles = len(tiling_np.tile_starts(T, tc, ov, tiler))
    assert one["mag"].shape == (T, F) and one["est"].shape == (S, T, F) and one["pcm"].shape == (S, L)
    assert one["n_tiles"] == n_tiles >= 1 and one["tiles"].shape == (n_tiles, ninst, tc, F)
    ref = ssr.whole_file_score(audio, N, h, tc, ov, tiler, conv, S, win, scale, notes, normalise, mixture, seed=seed,
                               mag=one["mag"], phase=one["phase"])
    # 1. tiles: M * (scale * mag) at the device's own magnitudes, bit for bit, zero rows past T -- through filterSpec (ref) and
    # through the per-frame definition
    assert np.array_equal(ref["M"], ssr.all_frame_masks(notes, T, F, normalise))
    want = np.zeros((n_tiles, ninst, tc, F), dtype=np.float32)
    prod = np.float32(ref["M"]) * (np.float32(scale) * one["mag"])[None]
    for k in range(n_tiles):
        rows = min(tc, T - k * (tc - ov))
        want[k, :, :rows] = prod[:, k * (tc - ov):k * (tc - ov) + rows]
    assert one["tiles"].dtype == np.float32 and np.array_equal(one["tiles"], want) and np.array_equal(want, ref["tiles"])
    assert one["tiles"].any()
    # 2. estimates and 3. samples
    lim = chanmask_ref.bound(S, tc, ov, ref["mix"].astype(np.float64)[None])[0]
    e_est = np.abs(one["est"] - ref["est"])
    e_pcm = float(np.abs(one["pcm"] - ref["pcm"]).max())
    print("%s: est/bound %.3g pcm %.3g" % (_case_id(case), float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm))
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    assert np.isfinite(one["pcm"]).all() and one["pcm"].any()
    # 4. however the signal is cut: the same bits
    for kind in ("hop", "empty_last"):
        for key in ("mag", "phase", "tiles", "est", "pcm"):
            assert np.array_equal(one[key], runs[kind][key]), (kind, key)
    # 5. reset, the same pushes: the same bits; the stream's memory has not moved
    stream.reset()
    again = _drive(stream, audio_t, stream_ref.partition("empty_last", L, h, seed=L), seed, counts)
    for key in ("mag", "phase", "tiles", "est", "pcm"):
        assert np.array_equal(again[key], runs["empty_last"][key]), key
    assert stream.bytes == nbytes
    stream.close()


# ------------------------------------------------------------------------------------------------ end to end
N, HOP, F, TC, OV = 1024, 512, 513, 30, 25
BLOCK = (TC - OV) * HOP
L_E2E = 44100 + 21
AUDIO_SEED, SCORE_SEED = 12, 60
# graph: (synth_params name, its seed, keep the live arrays only, (normalise, mixture), the oracle's arch)
GRAPHS = {
    "si17": ("bach10_si", 5, False, ("max", "ch0"), "bach10_si"),
    "si11": ("bach10_si", 5, True, ("sum", "sum"), "bach10_si1"),
    "deep": ("bach10_si_1x1", 7, False, ("sum", "sum"), "bach10_si_1x1"),
}
_CACHE = {}


def _melody(L, tmp_dir, frame=N):
    """four seeded scores -> the note table of a signal of L samples at 44 100 Hz"""
    files = []
    for i in range(4):
        files.append("inst%d.txt" % i)
        with open(os.path.join(tmp_dir, files[-1]), "w") as fh:
            fh.write(synth_score_text(SCORE_SEED + i, L / 44100.0 + 0.5, 40 + 5 * i, 64 + 6 * i))
    T = stft_np.frame_count(L, HOP)
    assert T == int(np.ceil(L / float(HOP))) + 2
    return score.melody_table(files, tmp_dir, T, 44100, HOP, frame)


def _setup(graph, tmp_path_factory):
    if graph not in _CACHE:
        name, seed, live, sem, _ = GRAPHS[graph]
        params = synth_params(name, TC, F, seed=seed)
        if live:
            _, params = live_params(ARCHS[name], params)
        sep = dcs.Separator("bach10_si", params, 0.3, TC, OV, 32, F, N, HOP, np.hanning, tiler='library',
                            score_normalise=sem[0], score_mixture=sem[1])
        # 17 arrays load as their live part (the 11-array graph) unless every branch is asked for
        assert len(params) == {"si17": 17, "si11": 11, "deep": 22}[graph] and sep.net.arch.eps_mode == EPS_B
        assert sep.net.arch.name == ("bach10_si_1x1" if graph == "deep" else "bach10_si1")
        if "melody" not in _CACHE:
            _CACHE["audio"] = 0.5 * synth_audio(L_E2E, seed=AUDIO_SEED)
            _CACHE["melody"] = _melody(L_E2E, str(tmp_path_factory.mktemp("scores")))
        _CACHE[graph] = dict(sep=sep, params=params, audio=_CACHE["audio"], melody=_CACHE["melody"])
    return _CACHE[graph]


def _oracle(graph, params, audio, melody):
    """``oracle.pipeline.separate_scoreinformed``; for the deep graph, which the oracle's network does not know, the same
    composition with the float64 restatement tests/deep1x1_ref.py in its place (tests/test_gpu_si1x1.py::_cpu_pipeline)"""
    _, _, _, sem, arch = GRAPHS[graph]
    if graph != "deep":
        return pipeline.separate_scoreinformed(params, audio, melody, 0.3, TC, OV, 32, N, HOP, np.hanning, normalise=sem[0],
                                               mixture=sem[1], arch=arch)
    import deep1x1_ref
    from oracle import score_np
    audio = np.asarray(audio, dtype=np.float64)
    nframes = int(np.ceil(len(audio) / float(HOP))) + 2
    mag, ph = stft_np.compute_file(audio, phase=True, frameSize=N, hopSize=HOP, window=np.hanning)
    mag = 0.3 * mag.astype(np.float32)
    inp = score_np.network_input(mag, np.asarray(melody), nframes, None, normalise=sem[0])
    batches, nchunks = tiling_np.generate_overlapadd(inp, inp.shape[-1], TC, OV, 32, tiler=tiling_np.LIBRARY, fill=0.0)
    out = []
    for b in batches:
        p = deep1x1_ref.forward(params, b, branches=1)
        out.append(list(deep1x1_ref.masked(p, b, EPS_B, sem[1])[:, :, None]))
    mm = tiling_np.overlapadd_multi(np.array(out), nchunks, overlap=OV)
    return np.stack([stft_np.compute_inverse(mm[i, :len(ph)] / 0.3, ph, frameSize=N, hopSize=HOP, window=np.hanning)[:len(audio)]
                     for i in range(mm.shape[0])])


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_end_to_end(graph, tmp_path_factory):
    """push -> ``forward_raw`` -> pull composed here, one stride per push, every ``p`` kept: estimates and samples against the
    float64 whole-file composition at the product's own ``p``, magnitudes and phases; ``ScoreStreamSeparator`` with the same
    blocks returns the same bits; and the stream's samples, like ``Separator.separate_scoreinformed``'s on the same input, lie
    within the project's whole-file bar of 1e-4 of the oracle."""
    s = _setup(graph, tmp_path_factory)
    sep, audio, melody = s["sep"], s["audio"], s["melody"]
    sem = GRAPHS[graph][3]
    S, L, ctx = sep.net.S, audio.size, sep.ctx
    T = stft_np.frame_count(L, HOP)
    a = ctx.to_device(audio, np.float32)
    eng = runtime.ScoreStream(sep.plan, S, melody, TC, OV, sep.tiler, EPS_B, 0.3, max_push=BLOCK, normalise=sem[0],
                              mixture=sem[1])
    mags, phs, ests, pcms, ps = [], [], [], [], []
    starts = list(range(0, L, BLOCK))
    for i in range(len(starts) + 1):
        last = i == len(starts)
        tiles, mag, ph = eng.push(None if last else a[starts[i]:starts[i] + BLOCK], last=last, want_frames=True)
        p = None
        if int(tiles.shape[0]):
            p = sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:S]
            ps.append(ctx.to_host(p))
        pcm, est = eng.pull(p, want_est=True)
        mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
    eng.close()
    run = dict(mag=np.concatenate(mags), phase=np.concatenate(phs), est=np.concatenate(ests, axis=1),
               pcm=np.concatenate(pcms, axis=1), p=np.concatenate(ps, axis=1))
    assert run["p"].shape == (S, len(tiling_np.tile_starts(T, TC, OV, tiling_np.LIBRARY)), TC, F) and (run["p"] >= 0).all()
    assert run["est"].shape == (S, T, F) and run["pcm"].shape == (S, L)
    ref = ssr.whole_file_score(audio, N, HOP, TC, OV, tiling_np.LIBRARY, "B", S, np.hanning(N), 0.3, melody, sem[0], sem[1],
                               p=run["p"], mag=run["mag"], phase=run["phase"])
    lim = chanmask_ref.bound(S, TC, OV, ref["mix"].astype(np.float64)[None])[0]
    e_est = np.abs(run["est"] - ref["est"])
    e_pcm = float(np.abs(run["pcm"] - ref["pcm"]).max())
    print("%s: est/bound %.3g pcm %.3g" % (graph, float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm))
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    # the separator's stream with the same blocks: the same bits
    ss = sep.stream_scoreinformed(melody, max_block=BLOCK)
    assert isinstance(ss, ScoreStreamSeparator) and ss.S == S
    got = [ss.push(audio[b:b + BLOCK]) for b in starts] + [ss.finish()]
    assert len(got) == len(pcms)
    for x, y in zip(got, pcms):
        assert x.dtype == np.float64 and np.array_equal(x, y.astype(np.float64))
    assert sum(x.shape[1] for x in got) == L
    with pytest.raises(ValueError):
        ss.finish()
    # against the oracle: the stream, and the whole-file call on the same input, at the whole-file bar
    want = _oracle(graph, s["params"], audio, melody)
    whole = sep.separate_scoreinformed(audio, melody)
    e_stream = float(np.abs(run["pcm"] - want).max())
    e_whole = float(np.abs(whole - want).max())
    print("%s: |stream - oracle| %.3g  |whole-file - oracle| %.3g  max |oracle| %.3g" % (graph, e_stream, e_whole,
                                                                                       float(np.abs(want).max())))
    assert want.shape == (S, L) and np.abs(want).max() > 1e-3
    assert e_whole < 1e-4
    assert e_stream < 1e-4


# ------------------------------------------------------------------------------------------------ any sample rate
RATE, RATE_BLOCK = 48000, 7000


def test_rate_stream_equals_the_manual_composition(tmp_path_factory):
    """``RateStream`` around a score stream: the whole-file ``Resampler`` down, the inner stream pushed in the 44 100 Hz cuts
    ``ResampleCounts`` predicts, the whole-file ``Resampler`` back, cropped -- bit for bit"""
    import torch
    sep = _setup("si17", tmp_path_factory)["sep"]
    ctx, S = sep.ctx, sep.net.S
    audio = 0.5 * synth_audio(RATE + 33, seed=21)
    L = audio.size
    n44 = out_length(L, *ratio(RATE, 44100))
    melody = _melody(n44, str(tmp_path_factory.mktemp("scores48")))
    sizes = [RATE_BLOCK] * (L // RATE_BLOCK) + [L % RATE_BLOCK]
    rs = RateStream(sep.stream_scoreinformed(melody, max_block=RATE_BLOCK), RATE)
    nbytes = rs.device_bytes
    assert nbytes > rs.inner.device_bytes
    x = ctx.to_device(audio, np.float32)
    outs, pos = [], 0
    for n in sizes:
        outs.append(ctx.to_host(rs.push_device(x[pos:pos + n])))
        pos += n
    outs.append(ctx.to_host(rs.finish_device()))
    got = np.concatenate(outs, axis=1)
    assert got.shape == (S, L) and rs.device_bytes == nbytes
    # the manual composition
    down, up = ctx.resampler(RATE, 44100), ctx.resampler(44100, RATE)
    c = ResampleCounts(down.up, down.down, down.half)
    y = down(x.reshape(1, L))
    assert int(y.shape[1]) == n44
    inner = sep.stream_scoreinformed(melody, max_block=RATE_BLOCK)
    cuts = [c.emitted(P) for P in np.cumsum([0] + list(sizes))] + [c.emitted(L, True)]
    assert cuts[-1] == n44
    pieces = [inner.push_device(y[0, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pieces.append(inner.finish_device())
    with ctx.stream_scope():
        pcm = torch.cat(pieces, dim=-1)
        want = ctx.to_host(up(pcm)[:, :L])
    assert np.isfinite(got).all() and got.any() and np.array_equal(got, want)
    # the host interface: the same bits
    rs.reset()
    host = np.concatenate([rs.push(audio[b:b + RATE_BLOCK]) for b in range(0, L, RATE_BLOCK)] + [rs.finish()], axis=1)
    assert host.dtype == np.float64 and np.array_equal(host, got.astype(np.float64))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(tmp_path_factory):
    s = _setup("si17", tmp_path_factory)
    sep, melody = s["sep"], s["melody"]
    lib, ctx = _lib.load(), sep.ctx
    rise = np.linspace(0., 1., OV)
    rp = rise.ctypes.data_as(POINTER(c_double))
    notes = np.ascontiguousarray(ssr.synth_table(4, 60, F, nharm=4, boundary=5, seed=0))

    def create(notes=notes, ninst=4, n_notes=None, width=None, normalise=0, mixture=0, S=4):
        h = c_void_p()
        rc = lib.dcs_stream_create_score(sep.plan._h, S, TC, OV, TILER_LIBRARY, EPS_B, 0.3, rp, 2048,
                                         notes.ctypes.data_as(POINTER(c_double)), ninst,
                                         notes.shape[1] if n_notes is None else n_notes,
                                         notes.shape[2] if width is None else width, normalise, mixture, byref(h))
        return rc, h
    past = notes.copy()
    row = int(np.argmax((past[0, :, 2] > 0) & (past[0, :, 1] > past[0, :, 0])))     # a row that counts
    past[0, row, 3:5] = (F - 2, F + 1)                                    # a bin range past F
    assert create(notes=past)[0] == _lib.DCS_ESHAPE
    assert create(ninst=0)[0] == _lib.DCS_EINVAL
    nine = np.ascontiguousarray(np.concatenate([notes, notes, notes[:1]]))
    assert create(notes=nine, ninst=9)[0] == _lib.DCS_EINVAL
    even = np.ascontiguousarray(notes[:, :, :-1])
    assert create(notes=even)[0] == _lib.DCS_EINVAL                       # an even width
    assert create(notes=np.ascontiguousarray(notes[:, :, :3]))[0] == _lib.DCS_EINVAL      # no pair at all
    assert create(normalise=2)[0] == _lib.DCS_EINVAL and create(mixture=2)[0] == _lib.DCS_EINVAL
    assert create(S=9)[0] == _lib.DCS_EINVAL                              # what dcs_stream_create refuses
    rc, h = create()
    assert rc == _lib.DCS_OK
    a = ctx.to_device(np.zeros((3, 2048)), np.float32)
    tiles = ctx.empty((int(lib.dcs_stream_max_tiles(h)), 4, TC, F), np.float32)
    pcm = ctx.empty((2, 4, 4096), np.float32)
    nt, nf, no = c_int64(), c_int64(), c_int64()
    assert lib.dcs_stream_push_channels(h, c_void_p(a.data_ptr()), 2048, 16, 0, c_void_p(tiles.data_ptr()), int(tiles.shape[0]),
                                        byref(nt), None, None, 0, 0, byref(nf)) == _lib.DCS_EINVAL
    assert lib.dcs_stream_push(h, c_void_p(a.data_ptr()), 16, 0, c_void_p(tiles.data_ptr()), int(tiles.shape[0]), byref(nt),
                               None, None, 0, byref(nf)) == _lib.DCS_OK and nt.value == 0
    assert lib.dcs_stream_pull_channels(h, None, 0, 0, c_void_p(pcm.data_ptr()), 4 * 4096, 4096, 4096, byref(no), None, 0, 0,
                                        0) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull(h, None, 0, 0, c_void_p(pcm.data_ptr()), 4096, 4096, byref(no), None, 0, 0) == _lib.DCS_OK
    assert lib.dcs_stream_bytes(h) > 0
    ctx.synchronize()
    assert lib.dcs_stream_destroy(h) == _lib.DCS_OK
    # Python
    with pytest.raises(ValueError, match="stream_scoreinformed"):
        sep.stream()                                                      # a multi-channel graph: points to the score stream
    with pytest.raises(ValueError, match="the network takes 4 score channels, the note table has 3"):
        sep.stream_scoreinformed(melody[:3])
    mono = dcs.Separator("dsd", synth_params("dsd", TC, F, seed=7), 0.3, TC, OV, 32, F, N, HOP, np.hanning)
    with pytest.raises(ValueError, match="one input channel"):
        mono.stream_scoreinformed(melody)
    with pytest.raises(ValueError):
        runtime.ScoreStream(sep.plan, 4, melody, TC, OV, normalise='mean')


# ------------------------------------------------------------------------------------------------ guard harness
_CHILD = r'''
import hashlib, json, os, sys, tempfile
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd import score
from deepconvsep_amd.synth import synth_audio, synth_params, synth_score_text
audio = 0.5 * synth_audio(44100 + 21, seed=12)
d = tempfile.mkdtemp()
files = []
for i in range(4):
    files.append("inst%d.txt" % i)
    with open(os.path.join(d, files[-1]), "w") as fh:
        fh.write(synth_score_text(60 + i, audio.size / 44100.0 + 0.5, 40 + 5 * i, 64 + 6 * i))
melody = score.melody_table(files, d, int(np.ceil(audio.size / 512.0)) + 2, 44100, 512, 1024)
sep = dcs.Separator("bach10_si", synth_params("bach10_si", 30, 513, seed=5), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning,
                    tiler='library', score_normalise='sum', score_mixture='sum')
def run(ss):
    return [ss.push(audio[i:i + 4000]) for i in range(0, audio.size, 4000)] + [ss.finish()]
run(sep.stream_scoreinformed(melody, max_block=4000))   # the network makes its own blocks on first need: all of them exist after this
ss = sep.stream_scoreinformed(melody, max_block=4000)
nbytes = ss.device_bytes
blocks0 = sep.ctx.check_guards()
outs = run(ss)
pcm = np.concatenate(outs, axis=1)
blocks1 = sep.ctx.check_guards()                      # raises when a red zone was written
json.dump({"sha256": hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest(), "finite": bool(np.isfinite(pcm).all()),
           "shape": list(pcm.shape), "any": bool(pcm.any()), "blocks_after_create": blocks0, "blocks_after_last_pull": blocks1,
           "bytes_before": nbytes, "bytes_after": ss.device_bytes}, open(OUT, "w"))
'''


def test_guard_harness(tmp_path):
    """one score stream under DCS_WS_GUARD with both poison bytes (the manner of tests/test_gpu_stream.py): no red zone written,
    every output finite -- a mask or magnitude slot read before it was written would be a NaN under 0xFF --, the two runs
    bit-identical, and the stream neither allocates nor grows after its creation"""
    procs = []
    for poison in (255, 75):
        env = dict(os.environ)
        env.update({"DCS_WS_GUARD": "65536", "DCS_WS_POISON": str(poison)})
        out = str(tmp_path / ("guard%d.json" % poison))
        procs.append((poison, out, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, out], env=env, stdout=subprocess.PIPE,
                                                    stderr=subprocess.PIPE, text=True)))
    res = []
    for poison, out, proc in procs:
        so, se = proc.communicate(timeout=300)
        assert proc.returncode == 0, (poison, so[-500:], se[-2500:])
        with open(out) as fh:
            res.append(json.load(fh))
    for r in res:
        assert r["finite"] and r["any"] and r["shape"] == [4, 44100 + 21]
        assert r["blocks_after_create"] == r["blocks_after_last_pull"] >= 9 and r["bytes_before"] == r["bytes_after"] > 0
    assert res[0]["sha256"] == res[1]["sha256"]


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_writes_the_truncated_stream(tmp_path):
    import importlib.util
    import scipy.io.wavfile
    from deepconvsep_amd.separation import SI_SCORE_FILES, SI_SCORE_PARAMS, output_paths, read_wav, save_model, write_wav
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    params = synth_params("bach10_si", 30, 2049, seed=5)
    model, wav, out = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "stems")
    save_model(model, params)
    write_wav(wav, 0.5 * synth_audio(44100, seed=5), 44100)
    for i, name in enumerate(SI_SCORE_FILES):
        (tmp_path / name).write_text(synth_score_text(60 + i, 1.5, 40 + 5 * i, 64 + 6 * i))
    script.main(["-a", "bach10_si", "-i", wav, "-o", out, "-m", model, "--block", "3000"])
    with pytest.raises(SystemExit):
        script.main(["-a", "bach10_si", "-i", wav, "-o", out, "-m", model, "--stereo"])
    _, mono = read_wav(wav)
    melody = score.melody_table(SI_SCORE_FILES, str(tmp_path), int(np.ceil(mono.size / 512.0)) + 2, 44100, 512, 4096,
                                **SI_SCORE_PARAMS)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, 2049, 4096, 512, dcs.blackmanharris, tiler='library')
    ss = sep.stream_scoreinformed(melody, max_block=3000)
    want = np.concatenate([ss.push(mono[i:i + 3000]) for i in range(0, mono.size, 3000)] + [ss.finish()], axis=1)
    paths = output_paths("bach10_si", wav, out)
    assert len(paths) == 4
    for i, path in enumerate(paths):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (mono.size,)
        assert np.array_equal(got, (want[i] * 32767).astype(np.int16)), path
    assert np.abs(want).max() > 1e-3
