"""Stereo streams and streams at any sample rate on the MI355X (``dcs_stream_*_channels`` in csrc/stream.hip,
``dcs_resample_stream`` in csrc/resample.hip; include/dcs.h has the contracts).

Machinery tests drive ``runtime.ChannelStream`` with a synthetic positive ``p`` per tile and no network; the references are the
float64 ones of the mono stream's tests, per channel, evaluated at the device's own magnitudes, estimates and phases, so each
stage is held to its own bound: ``stft_ref.BOUND_MAG`` / ``BOUND_CPX`` for the frames, ``chanmask_ref.bound`` for the estimates,
``stft_ref.BOUND_INV`` for the samples.  With every channel equal to the down-mix the channel stream must return the mono
stream's bits.  End-to-end tests run the DSD graph on one second of stereo audio, at 44 100 Hz and at 48 000 Hz.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd import _lib, runtime
from deepconvsep_amd.arch import EPS_A, EPS_B, TILER_LIBRARY, TILER_SCRIPT
from deepconvsep_amd.resample import ResampleCounts
from deepconvsep_amd.streaming import RateStream, StreamCounts
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import stft_np, tiling_np

import chanmask_ref
import stft_ref
import stream_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = tuple(s for s in stream_ref.SHAPES if s[0] <= 1024)            # (64,16,8,5) (64,32,8,1) (128,32,30,29) (1024,512,30,25)
CHANNELS_SOURCES = ((1, 1), (2, 4), (3, 2))
TILER_CODE = {tiling_np.SCRIPT: TILER_SCRIPT, tiling_np.LIBRARY: TILER_LIBRARY}
EPS_CODE = {"A": EPS_A, "B": EPS_B}
KEYS = ("mag", "phase", "est", "pcm")


def _drive(stream, audio_t, sizes, seed, counts):
    """the rows ``audio_t [rows, L]`` (``[L]`` for a mono stream) through the stream in blocks of ``sizes`` with the synthetic p
    of stream_ref.tile_p -> host arrays with the frame / sample axis last but one / last, and every count the library returned
    checked against StreamCounts on the way"""
    ctx = stream.ctx
    mono = audio_t.dim() == 1
    mags, phs, ests, pcms, tls, pos, k = [], [], [], [], [], 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = (counts.frames(pos), counts.tiles(pos), counts.emitted(pos))
        piece = (audio_t[pos:pos + n] if mono else audio_t[:, pos:pos + n]) if n else None
        tiles, mag, ph = stream.push(piece, last=last, want_frames=True)
        pos += n
        assert stream.last_frames == counts.frames(pos, last) - before[0] == int(mag.shape[-2])
        assert stream.last_tiles == counts.tiles(pos, last) - before[1] == int(tiles.shape[0])
        assert stream.last_tiles <= stream.max_tiles
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stream_ref.tile_p(k + j, stream.S, stream.tc, stream.F, seed) for j in range(nt)], axis=1),
                              np.float32)
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        assert stream.last_samples == counts.emitted(pos, last) - before[2] == int(pcm.shape[-1])
        mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        tls.append(ctx.to_host(tiles))
    return dict(mag=np.concatenate(mags, axis=-2), phase=np.concatenate(phs, axis=-2), est=np.concatenate(ests, axis=-2),
                pcm=np.concatenate(pcms, axis=-1), tiles=np.concatenate(tls), n_tiles=k)


@pytest.mark.parametrize("CS", CHANNELS_SOURCES, ids=lambda cs: "C%d_S%d" % cs)
@pytest.mark.parametrize("shape", SHAPES, ids=stream_ref.shape_id)
def test_machinery_against_float64_and_across_partitions(shape, CS):
    N, h, tc, ov, wname = shape
    C, S = CS
    j = CHANNELS_SOURCES.index(CS)
    i = SHAPES.index(shape) + j
    tiler, conv = stream_ref.TILERS[i % 2], chanmask_ref.CONVENTIONS[(i // 2) % 2]
    L = stream_ref.lengths(N, h, tc, ov)[j]
    win = stream_ref.window(wname, N)
    F, scale, seed = N // 2 + 1, 0.3, 11 * i
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, win)
    chans = np.stack([0.5 * synth_audio(L, seed=3 + i + 17 * c) for c in range(C)])
    rows = np.concatenate([chans, chans.mean(axis=0, keepdims=True)]).astype(np.float32)      # the down-mix last
    audio_t = ctx.to_device(rows, np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)
    stream = runtime.ChannelStream(plan, S, C, tc, ov, TILER_CODE[tiler], EPS_CODE[conv], scale, max_push=L)
    nbytes = stream.bytes
    fp = counts.max_frames(L)
    rf = ff = tc + fp
    rp, rt = -(-tc // (tc - ov)) + counts.max_tiles(L), N // h + ff
    assert nbytes == 4 * ((C + 1) * (N + L) + (C + 1) * rf * F + C * rf * F + S * rp * tc * F + C * S * ff * F + rt * C * S * N + ov)
    assert stream.max_tiles == counts.max_tiles(L)
    runs = {}
    for kind in ("one", "hop", "empty_last"):
        stream.reset()
        runs[kind] = _drive(stream, audio_t, stream_ref.partition(kind, L, h, seed=L), seed, counts)
    one = runs["one"]
    T = stft_np.frame_count(L, h)
    n_tiles = len(tiling_np.tile_starts(T, tc, ov, tiler))
    assert one["mag"].shape == one["phase"].shape == (C, T, F) and one["est"].shape == (C, S, T, F)
    assert one["pcm"].shape == (C, S, L) and one["n_tiles"] == n_tiles >= 1
    # 1. frames, per channel
    e_mag = e_cpx = 0.0
    for c in range(C):
        X = stft_np.stft_norm(rows[c].astype(np.float64), win, float(h), float(N)) / np.sqrt(N)
        e_mag = max(e_mag, float(np.abs(one["mag"][c] - np.abs(X)).max()))
        e_cpx = max(e_cpx, float(np.abs(one["mag"][c] * np.exp(1j * one["phase"][c].astype(np.float64)) - X).max()))
    # 2. estimates at the device's own magnitudes, on every bin
    p = np.stack([stream_ref.tile_p(k, S, tc, F, seed) for k in range(n_tiles)], axis=1)
    want_est, _ = chanmask_ref.chanmask_ref(p, one["mag"], ov, conv, n_frames=T)
    lim = chanmask_ref.bound(S, tc, ov, one["mag"].astype(np.float64))[:, None]
    e_est = np.abs(one["est"] - want_est)
    # 3. samples at the device's own estimates and phases
    e_pcm = 0.0
    for c in range(C):
        for s in range(S):
            want = stft_np.compute_inverse(one["est"][c, s].astype(np.float64), one["phase"][c].astype(np.float64), N, h, win)[:L]
            e_pcm = max(e_pcm, float(np.abs(one["pcm"][c, s] - want).max()))
    print("%s C=%d S=%d: mag %.3g cpx %.3g est/bound %.3g pcm %.3g" % (stream_ref.shape_id(shape), C, S, e_mag, e_cpx,
                                                                     float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm))
    assert e_mag <= stft_ref.BOUND_MAG and e_cpx <= stft_ref.BOUND_CPX
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    assert np.isfinite(one["pcm"]).all() and all(one["pcm"][c].any() for c in range(C))
    # 4. rows past the last tile, and the samples only they reach, are exactly zero
    covered = (n_tiles - 1) * (tc - ov) + tc
    if covered < T:
        assert not one["est"][:, :, covered:].any()
        first = covered * h + N // 2                                 # frame n reaches samples < n h + N / 2
        if first < L:
            assert not one["pcm"][:, :, first:].any()
    # 5. however the signal is cut: the same bits
    for kind in ("hop", "empty_last"):
        for key in KEYS + ("tiles",):
            assert np.array_equal(one[key], runs[kind][key]), (kind, key)
    # 6. reset, the same pushes: the same bits; the stream's memory has not moved
    stream.reset()
    again = _drive(stream, audio_t, stream_ref.partition("empty_last", L, h, seed=L), seed, counts)
    for key in KEYS:
        assert np.array_equal(again[key], runs["empty_last"][key]), key
    assert stream.bytes == nbytes
    stream.close()


@pytest.mark.parametrize("shape", SHAPES, ids=stream_ref.shape_id)
def test_equal_channels_give_the_bits_of_the_mono_stream(shape):
    """every channel row equal to the down-mix row: frames, estimates and samples of each channel and the tiles are those of
    ``runtime.Stream`` on the same blocks and the same p; and each kind of stream refuses the other kind's calls"""
    N, h, tc, ov, wname = shape
    C, S = 2, 3
    i = SHAPES.index(shape)
    tiler, conv = stream_ref.TILERS[(i + 1) % 2], chanmask_ref.CONVENTIONS[i % 2]
    L = stream_ref.lengths(N, h, tc, ov)[2]
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, stream_ref.window(wname, N))
    x = (0.5 * synth_audio(L, seed=40 + i)).astype(np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)
    sizes = stream_ref.partition("random", L, h, seed=L)
    args = (tc, ov, TILER_CODE[tiler], EPS_CODE[conv], 0.3)
    mono = runtime.Stream(plan, S, *args, max_push=2 * h + 2)
    chan = runtime.ChannelStream(plan, S, C, *args, max_push=2 * h + 2)
    a = _drive(mono, ctx.to_device(x, np.float32), sizes, 5, counts)
    b = _drive(chan, ctx.to_device(np.stack([x] * (C + 1)), np.float32), sizes, 5, counts)
    assert np.array_equal(a["tiles"], b["tiles"]) and a["n_tiles"] == b["n_tiles"] >= 1
    for c in range(C):
        for key in KEYS:
            assert np.array_equal(a[key], b[key][c]), (c, key)
    lib = ctx._lib
    assert lib.dcs_stream_push(chan._h, None, 0, 0, None, 0, None, None, None, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull(chan._h, None, 0, 0, None, 0, 0, None, None, 0, 0) == _lib.DCS_EINVAL
    assert lib.dcs_stream_push_channels(mono._h, None, 0, 0, 0, None, 0, None, None, None, 0, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull_channels(mono._h, None, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0) == _lib.DCS_EINVAL
    mono.close()
    chan.close()


def test_channel_stream_refusals():
    from ctypes import POINTER, byref, c_double, c_int64, c_void_p
    ctx = runtime.default_context()
    lib = ctx._lib
    plan = runtime.StftPlan(ctx, 64, 16, np.hanning(64))
    rise = np.linspace(0., 1., 5)
    rp = rise.ctypes.data_as(POINTER(c_double))

    def create(plan, S=2, C=2, tc=8, ov=5, max_push=128):
        h = c_void_p()
        return lib.dcs_stream_create_channels(plan._h, S, C, tc, ov, TILER_SCRIPT, EPS_A, 0.3, rp, max_push, byref(h)), h
    for kw in (dict(C=0), dict(C=9), dict(S=9), dict(ov=8), dict(max_push=0)):
        assert create(plan, **kw)[0] == _lib.DCS_EINVAL, kw
    assert create(runtime.StftPlan(ctx, 64, 48, np.hanning(64)))[0] == _lib.DCS_EINVAL       # hop above frameSize / 2
    assert create(runtime.StftPlan(ctx, 64, 24, np.hanning(64)))[0] == _lib.DCS_EUNSUPPORTED  # hop does not divide frameSize
    rc, h = create(plan)
    assert rc == _lib.DCS_OK
    a = ctx.to_device(np.zeros((3, 128)), np.float32)
    tiles = ctx.empty((int(lib.dcs_stream_max_tiles(h)), 1, 8, 33), np.float32)
    p = ctx.to_device(np.ones((2, int(tiles.shape[0]), 8, 33)), np.float32)
    pcm = ctx.empty((2, 2, 400), np.float32)
    nt, nf, no = c_int64(), c_int64(), c_int64()

    def push(n, last=0, row_stride=128):
        return lib.dcs_stream_push_channels(h, c_void_p(a.data_ptr()), row_stride, n, last, c_void_p(tiles.data_ptr()),
                                            int(tiles.shape[0]), byref(nt), None, None, 0, 0, byref(nf))

    def pull(n, ch_stride=800, stride=400):
        return lib.dcs_stream_pull_channels(h, c_void_p(p.data_ptr()), int(p.stride(0)), n, c_void_p(pcm.data_ptr()), ch_stride,
                                            stride, 400, byref(no), None, 0, 0, 0)
    assert push(129) == _lib.DCS_EINVAL                                   # n > max_push
    assert push(100, row_stride=99) == _lib.DCS_EINVAL                    # rows overlap
    assert pull(0) == _lib.DCS_EINVAL                                     # no push to pull for
    assert push(128) == _lib.DCS_OK and nt.value == 0
    assert push(16) == _lib.DCS_EINVAL                                    # two pushes in a row
    assert pull(1) == _lib.DCS_EINVAL                                     # the wrong tile count
    assert pull(0) == _lib.DCS_OK and no.value == 0
    assert push(128) == _lib.DCS_OK and nt.value == 3                     # 256 samples: 15 frames, tiles at 0, 3 and 6
    assert pull(3, ch_stride=400) == _lib.DCS_EINVAL                      # channels overlap
    assert pull(3) == _lib.DCS_OK and no.value == 9 * 16 - 32
    assert lib.dcs_stream_reset(h) == _lib.DCS_OK and push(0, 1) == _lib.DCS_OK
    assert pull(0) == _lib.DCS_EINVAL                                     # the ended signal gave no tile
    assert push(16) == _lib.DCS_EINVAL                                    # a push after the end
    ctx.synchronize()
    assert lib.dcs_stream_destroy(h) == _lib.DCS_OK


# ------------------------------------------------------------------------------------------------ end to end
N, HOP, F, TC, OV = 1024, 512, 513, 30, 25
BLOCK = (TC - OV) * HOP
_RUN = {}


def _separator():
    if "sep" not in _RUN:
        _RUN["sep"] = dcs.Separator("dsd", synth_params("dsd", TC, F, seed=7), 0.3, TC, OV, 32, F, N, HOP, np.hanning)
    return _RUN["sep"]


def _run():
    """one second of stereo audio through ``runtime.ChannelStream`` composed here, one stride per push, every p kept; and through
    ``ChannelStreamSeparator`` with the same blocks"""
    if "e2e" not in _RUN:
        sep = _separator()
        assert sep.net.arch.eps_mode == EPS_A
        audio = 0.5 * synth_audio(44100 + 21, seed=12, channels=2)                     # [L, 2]
        L, ctx = audio.shape[0], sep.ctx
        a3 = ctx.to_device(np.stack([audio[:, 0], audio[:, 1], (audio[:, 0] + audio[:, 1]) / 2]), np.float32)
        eng = runtime.ChannelStream(sep.plan, sep.net.S, 2, TC, OV, sep.tiler, EPS_A, 0.3, max_push=BLOCK)
        mags, phs, ests, pcms, ps = [], [], [], [], []
        starts = list(range(0, L, BLOCK))
        for i in range(len(starts) + 1):
            last = i == len(starts)
            tiles, mag, ph = eng.push(None if last else a3[:, starts[i]:starts[i] + BLOCK], last=last, want_frames=True)
            p = None
            if int(tiles.shape[0]):
                p = sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:sep.net.S]
                ps.append(ctx.to_host(p))
            pcm, est = eng.pull(p, want_est=True)
            mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        cs = sep.stream_channels(max_block=BLOCK)
        got = [cs.push(audio[s:s + BLOCK]) for s in starts] + [cs.finish()]
        _RUN["e2e"] = dict(sep=sep, audio=audio, mag=np.concatenate(mags, axis=1), phase=np.concatenate(phs, axis=1),
                           est=np.concatenate(ests, axis=2), pcm=np.concatenate(pcms, axis=2), p=np.concatenate(ps, axis=1),
                           pieces=pcms, separator_pieces=got, stream=cs, starts=starts)
    return _RUN["e2e"]


def test_end_to_end_against_the_float64_reference():
    """estimates and samples of both channels against the float64 whole-file composition evaluated at the product's own p,
    magnitudes and phases; each channel's stems add up to that channel where whole tiles cover it (the interval and the 2e-5 of
    the mono stream's test); ``ChannelStreamSeparator`` with the same blocks returns the same bits in the layout of
    ``separate_channels``"""
    run = _run()
    sep, audio = run["sep"], run["audio"]
    S, L = sep.net.S, audio.shape[0]
    T = stft_np.frame_count(L, HOP)
    assert run["p"].shape[0] == S and run["p"].shape[1] == len(tiling_np.tile_starts(T, TC, OV, tiling_np.SCRIPT)) >= 1
    assert run["est"].shape == (2, S, T, F) and run["pcm"].shape == (2, S, L) and (run["p"] >= 0).all()
    hi = ((run["p"].shape[1] - 1) * (TC - OV) + TC - 4) * HOP - N
    assert hi > 4 * N
    for c in range(2):
        ref = stream_ref.whole_file(audio[:, c], N, HOP, TC, OV, tiling_np.SCRIPT, "A", S, np.hanning(N), 0.3, p=run["p"],
                                    mag=run["mag"][c], phase=run["phase"][c])
        lim = chanmask_ref.bound(S, TC, OV, run["mag"][c].astype(np.float64)[None])
        e_est = np.abs(run["est"][c] - ref["est"])
        e_pcm = float(np.abs(run["pcm"][c] - ref["pcm"]).max())
        e_sum = float(np.abs(run["pcm"][c].sum(axis=0)[N:hi] - audio[N:hi, c]).max())
        print("channel %d: est/bound %.3g pcm %.3g sum %.3g" % (c, float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm, e_sum))
        assert np.all(e_est <= lim)
        assert e_pcm <= stft_ref.BOUND_INV
        assert e_sum < 2e-5
    assert len(run["separator_pieces"]) == len(run["pieces"])
    for a, b in zip(run["separator_pieces"], run["pieces"]):
        assert a.dtype == np.float64 and a.shape == (b.shape[2], S, 2) and np.array_equal(a, b.astype(np.float64).transpose(2, 1, 0))
    assert sum(x.shape[0] for x in run["separator_pieces"]) == L
    with pytest.raises(ValueError):
        run["stream"].finish()                                            # a second finish()


def test_equal_channels_give_the_stems_of_the_mono_separator():
    run = _run()
    sep, starts = run["sep"], run["starts"]
    x = run["audio"][:, 0]
    ss, cs = sep.stream(max_block=BLOCK), sep.stream_channels(max_block=BLOCK)
    nbytes = cs.device_bytes
    mono = [ss.push(x[s:s + BLOCK]) for s in starts] + [ss.finish()]
    both = [cs.push(np.stack([x[s:s + BLOCK]] * 2, axis=1)) for s in starts] + [cs.finish()]
    for a, b in zip(mono, both):
        assert b.shape == (a.shape[1], a.shape[0], 2)
        assert np.array_equal(a.T, b[:, :, 0]) and np.array_equal(a.T, b[:, :, 1])
    assert cs.device_bytes == nbytes
    cs.reset()
    cs.push(run["audio"][:5000])
    with pytest.raises(IndexError):                                       # too short for one tile: what separate_channels raises
        cs.finish()
    cs.reset()
    assert cs.push(run["audio"][:100]).shape == (0, sep.net.S, 2)


# ------------------------------------------------------------------------------------------------ any sample rate
RATE, RATE_BLOCK = 48000, 7000


def _manual(sep, rows, sizes, stereo):
    """what RateStream must return for ``rows`` ([1 or 3, L] float32 at RATE) pushed in blocks of ``sizes``: the whole-file
    ``Resampler`` down, the inner stream pushed in the 44 100 Hz cuts ``ResampleCounts`` predicts, the whole-file ``Resampler``
    back, cropped"""
    import torch
    ctx = sep.ctx
    down, up = ctx.resampler(RATE, 44100), ctx.resampler(44100, RATE)
    c = ResampleCounts(down.up, down.down, down.half)
    L = int(rows.shape[1])
    y = down(ctx.to_device(rows, np.float32))
    inner = sep.stream_channels(max_block=RATE_BLOCK) if stereo else sep.stream(max_block=RATE_BLOCK)
    cuts = [c.emitted(P) for P in np.cumsum([0] + list(sizes))] + [c.emitted(L, True)]
    assert cuts[-1] == int(y.shape[1])
    outs = [inner.push_device(y[:, a:b] if stereo else y[0, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    outs.append(inner.finish_device())
    with ctx.stream_scope():
        pcm = torch.cat(outs, dim=-1)
        assert int(pcm.shape[-1]) == cuts[-1]
        back = up(pcm.reshape(-1, cuts[-1]))[:, :L]
        return ctx.to_host(back.reshape(tuple(pcm.shape[:-1]) + (L,)))


@pytest.mark.parametrize("stereo", (False, True), ids=("mono", "stereo"))
def test_rate_stream_equals_the_manual_composition(stereo):
    sep = _separator()
    ctx = sep.ctx
    audio = 0.5 * synth_audio(RATE + 33, seed=21, channels=2)
    L = audio.shape[0]
    rows = np.stack([audio[:, 0], audio[:, 1], (audio[:, 0] + audio[:, 1]) / 2]) if stereo else audio[:, :1].T
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    sizes = [RATE_BLOCK] * (L // RATE_BLOCK) + [L % RATE_BLOCK]
    inner = sep.stream_channels(max_block=RATE_BLOCK) if stereo else sep.stream(max_block=RATE_BLOCK)
    rs = RateStream(inner, RATE)
    nbytes = rs.device_bytes
    assert nbytes > inner.device_bytes
    rows_d = ctx.to_device(rows, np.float32)
    outs, pos, emitted, started = [], 0, 0, False
    for n in sizes:
        out = rs.push_device(rows_d[:, pos:pos + n] if stereo else rows_d[0, pos:pos + n])
        pos += n
        emitted += int(out.shape[-1])
        started = started or emitted > 0
        if started:
            assert pos - emitted < rs.latency_samples(), (pos, emitted)
        outs.append(ctx.to_host(out))
    assert started
    outs.append(ctx.to_host(rs.finish_device()))
    got = np.concatenate(outs, axis=-1)
    S = sep.net.S
    assert got.shape == ((2, S, L) if stereo else (S, L))                  # the lengths add up to the samples pushed
    want = _manual(sep, rows, sizes, stereo)
    assert np.isfinite(got).all() and got.any() and np.array_equal(got, want)
    assert rs.device_bytes == nbytes
    with pytest.raises(ValueError):
        rs.finish_device()
    # the host interface: the same bits in the layouts of separate / separate_channels
    rs.reset()
    blocks = [audio[s:s + RATE_BLOCK] if stereo else audio[s:s + RATE_BLOCK, 0] for s in range(0, L, RATE_BLOCK)]
    host = np.concatenate([rs.push(b) for b in blocks] + [rs.finish()], axis=0 if stereo else 1)
    assert host.dtype == np.float64
    assert np.array_equal(host, got.astype(np.float64).transpose(2, 1, 0) if stereo else got.astype(np.float64))


# ------------------------------------------------------------------------------------------------ guard harness
_CHILD = r'''
import hashlib, json, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd.streaming import RateStream
from deepconvsep_amd.synth import synth_audio, synth_params
sep = dcs.Separator("dsd", synth_params("dsd", 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning)
audio = 0.5 * synth_audio(48000 + 33, seed=21, channels=2)
def run(rs):
    return [rs.push(audio[i:i + 4000]) for i in range(0, audio.shape[0], 4000)] + [rs.finish()]
run(RateStream(sep.stream_channels(max_block=4000), 48000))      # the network and the context make their own blocks on first need
rs = RateStream(sep.stream_channels(max_block=4000), 48000)
nbytes = rs.device_bytes
blocks0 = sep.ctx.check_guards()
outs = run(rs)
pcm = np.concatenate(outs, axis=0)
blocks1 = sep.ctx.check_guards()                      # raises when a red zone was written
json.dump({"sha256": hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest(), "finite": bool(np.isfinite(pcm).all()),
           "shape": list(pcm.shape), "any": bool(pcm.any()), "blocks_after_create": blocks0, "blocks_after_last_pull": blocks1,
           "bytes_before": nbytes, "bytes_after": rs.device_bytes}, open(OUT, "w"))
'''


def test_guard_harness(tmp_path):
    """one stereo 48 kHz RateStream under DCS_WS_GUARD with both poison bytes (the manner of tests/test_gpu_stream.py): no red
    zone written, every output finite -- a ring slot read before it was written would be a NaN under 0xFF --, the two runs
    bit-identical, and neither the stream nor its converters allocate or grow after their creation"""
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
        assert r["finite"] and r["any"] and r["shape"] == [48000 + 33, 4, 2]
        assert r["blocks_after_create"] == r["blocks_after_last_pull"] >= 9 and r["bytes_before"] == r["bytes_after"] > 0
    assert res[0]["sha256"] == res[1]["sha256"]


# ------------------------------------------------------------------------------------------------ command line
def _script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_command_line_stereo_and_resample(tmp_path):
    import scipy.io.wavfile
    from deepconvsep_amd.separation import output_paths, read_wav, save_model, write_wav
    sep, script = _separator(), _script()
    model, wav, wav48 = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "mix48.wav")
    out, out48 = str(tmp_path / "stems"), str(tmp_path / "stems48")
    save_model(model, synth_params("dsd", TC, F, seed=7))
    write_wav(wav, 0.5 * synth_audio(44100, seed=5, channels=2), 44100)
    write_wav(wav48, 0.5 * synth_audio(48000, seed=6, channels=2), 48000)
    # --stereo: the stems of ChannelStreamSeparator with the same blocks
    script.main(["-a", "dsd", "-i", wav, "-o", out, "-m", model, "--block", "3000", "--stereo"])
    _, audio = read_wav(wav)
    cs = sep.stream_channels(max_block=3000)
    want = np.concatenate([cs.push(audio[i:i + 3000]) for i in range(0, audio.shape[0], 3000)] + [cs.finish()], axis=0)
    for i, path in enumerate(output_paths("dsd", wav, out)):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (audio.shape[0], 2)
        assert np.array_equal(got, (want[:, i] * 32767).astype(np.int16)), path
    # --stereo --resample: stems at the file's rate and of the file's length
    script.main(["-a", "dsd", "-i", wav48, "-o", out48, "-m", model, "--block", "6000", "--stereo", "--resample"])
    loud = 0
    for path in output_paths("dsd", wav48, out48):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 48000 and got.dtype == np.int16 and got.shape == (48000, 2)
        loud += int(np.abs(got.astype(np.int64)).max() > 1000)            # the synthetic weights leave some sources silent
    assert loud >= 1
    # without --resample the file is refused as before
    with pytest.raises(SystemExit, match="Sample rate is not 44100"):
        script.main(["-a", "dsd", "-i", wav48, "-o", out48, "-m", model, "--stereo"])
