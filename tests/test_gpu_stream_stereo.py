"""The stereo (ILD) DSD100 graph on a stream on the MI355X: ``dcs_model_forward_stereo`` (csrc/net.hip), ``dcs_stream_*_stereo``
(csrc/stream.hip; include/dcs.h has the contracts), ``StereoStreamSeparator``, ``RateStream`` over it and the command line.

Machinery tests drive ``runtime.StereoStream`` with a synthetic ``p`` per tile and no network, against the float64 statement of
``stereo_stream_ref`` evaluated at the device's own magnitudes, estimates and phases, so each stage is held to its own bound:
``stft_ref.BOUND_MAG`` / ``BOUND_CPX`` for the frames, ``stereo_stream_ref.bound`` for the estimates, ``stft_ref.BOUND_INV`` for the
samples.  The tile forward pass is held to the project's 1e-4 against ``net_ref.forward('dsd_ild')``; the end-to-end tests run one
second of stereo audio, at 44 100 Hz and at 48 000 Hz.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd import _lib, runtime
from deepconvsep_amd.arch import TILER_LIBRARY, TILER_SCRIPT
from deepconvsep_amd.resample import ResampleCounts
from deepconvsep_amd.streaming import (RateStream, StereoStreamSeparator, StreamCounts, stereo_ld, stereo_rows_from_tiles,
                                       stereo_tiles_from_rows)
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import cases, net_ref, pipeline, stft_np, tiling_np

import stereo_stream_ref
import stft_ref
import stream_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILER_CODE = {tiling_np.SCRIPT: TILER_SCRIPT, tiling_np.LIBRARY: TILER_LIBRARY}
SOURCES, CHANNELS = (1, 2, 4), (1, 2, 3)
KEYS = ("mag", "phase", "est", "pcm", "tiles")


def _drive(stream, audio_t, sizes, seed, counts):
    """the rows ``audio_t [C, L]`` through the stream in blocks of ``sizes`` with the synthetic p of stereo_stream_ref.tile_p in
    the Lasagne layout -> host arrays, every count the library returned checked against StreamCounts on the way"""
    ctx = stream.ctx
    mags, phs, ests, pcms, tls, pos, k = [], [], [], [], [], 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = (counts.frames(pos), counts.tiles(pos), counts.emitted(pos))
        tiles, mag, ph = stream.push(audio_t[:, pos:pos + n] if n else None, last=last, want_frames=True)
        pos += n
        assert stream.last_frames == counts.frames(pos, last) - before[0] == int(mag.shape[-2])
        assert stream.last_tiles == counts.tiles(pos, last) - before[1] == int(tiles.shape[0])
        assert stream.last_tiles <= stream.max_tiles
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stereo_stream_ref.tile_p(k + j, stream.S, stream.C, stream.tc, stream.F, seed)
                                        for j in range(nt)], axis=1), np.float32)           # [S C, nt, tc, F]
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        assert stream.last_samples == counts.emitted(pos, last) - before[2] == int(pcm.shape[-1])
        mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        tls.append(ctx.to_host(tiles))
    return dict(mag=np.concatenate(mags, axis=-2), phase=np.concatenate(phs, axis=-2), est=np.concatenate(ests, axis=-2),
                pcm=np.concatenate(pcms, axis=-1), tiles=np.concatenate(tls), n_tiles=k)


@pytest.mark.parametrize("j", (0, 1, 2), ids=lambda j: "len%d" % j)
@pytest.mark.parametrize("shape", stream_ref.SHAPES, ids=stream_ref.shape_id)
def test_machinery_against_float64_and_across_partitions(shape, j):
    N, h, tc, ov, wname = shape
    i = stream_ref.SHAPES.index(shape) + j
    S, C, tiler = SOURCES[i % 3], CHANNELS[(i + i // 3) % 3], stream_ref.TILERS[i % 2]
    L = stream_ref.lengths(N, h, tc, ov)[j]
    win = stream_ref.window(wname, N)
    F, ldt, scale, seed = N // 2 + 1, stereo_ld(N // 2 + 1), 0.3, 13 * i + 1
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, win)
    rows = np.stack([0.5 * synth_audio(L, seed=5 + i + 19 * c) for c in range(C)]).astype(np.float32)
    audio_t = ctx.to_device(rows, np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)
    stream = runtime.StereoStream(plan, S, C, tc, ov, TILER_CODE[tiler], scale, max_push=L)
    nbytes = stream.bytes
    fp = counts.max_frames(L)
    rf = ff = tc + fp
    rp, rt = -(-tc // (tc - ov)) + counts.max_tiles(L), N // h + ff
    assert nbytes == 4 * (C * (N + L) + 2 * C * rf * F + S * C * rp * tc * F + C * S * ff * F + rt * C * S * N + ov)
    assert stream.max_tiles == counts.max_tiles(L)
    runs = {}
    for kind in ("one", "hop", "empty_last"):
        stream.reset()
        runs[kind] = _drive(stream, audio_t, stream_ref.partition(kind, L, h, seed=L), seed, counts)
    one = runs["one"]
    T = stft_np.frame_count(L, h)
    n_tiles = len(tiling_np.tile_starts(T, tc, ov, tiler))
    assert one["mag"].shape == one["phase"].shape == (C, T, F) and one["est"].shape == (C, S, T, F)
    assert one["pcm"].shape == (C, S, L) and one["n_tiles"] == n_tiles >= 1 and one["tiles"].shape == (n_tiles, tc, C, ldt)
    # 1. frames, per channel
    e_mag = e_cpx = 0.0
    for c in range(C):
        X = stft_np.stft_norm(rows[c].astype(np.float64), win, float(h), float(N)) / np.sqrt(N)
        e_mag = max(e_mag, float(np.abs(one["mag"][c] - np.abs(X)).max()))
        e_cpx = max(e_cpx, float(np.abs(one["mag"][c] * np.exp(1j * one["phase"][c].astype(np.float64)) - X).max()))
    # 2. tiles: the float32 product on the device's own rows, zero rows past the end, zero pad columns
    want_tiles = np.zeros((n_tiles, tc, C, ldt), np.float32)
    for k in range(n_tiles):
        hi = min(T, k * (tc - ov) + tc)
        want_tiles[k, :hi - k * (tc - ov), :, :F] = (np.float32(scale) * one["mag"][:, k * (tc - ov):hi]).transpose(1, 0, 2)
    assert np.array_equal(one["tiles"], want_tiles)
    # 3. estimates at the device's own magnitudes, on every bin; 4. samples at the device's own estimates and phases
    p = np.stack([stereo_stream_ref.tile_p(k, S, C, tc, F, seed) for k in range(n_tiles)], axis=1)
    ref = stereo_stream_ref.whole_file(rows.T, N, h, tc, ov, tiler, S, win, scale, stereo_stream_ref.from_lasagne(p, S, C),
                                       mag=one["mag"], phase=one["phase"])
    c0 = stereo_stream_ref.c0_f32(scale)
    lim = stereo_stream_ref.bound(S, tc, ov, one["mag"].astype(np.float64), c0)[:, None]
    e_est = np.abs(one["est"] - ref["est"])
    e_pcm = 0.0
    for c in range(C):
        for s in range(S):
            want = stft_np.compute_inverse(one["est"][c, s].astype(np.float64), one["phase"][c].astype(np.float64), N, h, win)[:L]
            e_pcm = max(e_pcm, float(np.abs(one["pcm"][c, s] - want).max()))
    print("%s C=%d S=%d %s: mag %.3g cpx %.3g est/bound %.3g pcm %.3g" % (stream_ref.shape_id(shape), C, S, tiler, e_mag, e_cpx,
                                                                        float((e_est / lim).max()), e_pcm))
    assert e_mag <= stft_ref.BOUND_MAG and e_cpx <= stft_ref.BOUND_CPX
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    assert np.isfinite(one["pcm"]).all() and all(one["pcm"][c].any() for c in range(C))
    # 5. rows past the last tile, and the samples only they reach, are exactly zero
    covered = (n_tiles - 1) * (tc - ov) + tc
    if covered < T:
        assert not one["est"][:, :, covered:].any()
        first = covered * h + N // 2                                 # frame n reaches samples < n h + N / 2
        if first < L:
            assert not one["pcm"][:, :, first:].any()
    # 6. however the signal is cut: the same bits
    for kind in ("hop", "empty_last"):
        for key in KEYS:
            assert np.array_equal(one[key], runs[kind][key]), (kind, key)
    # 7. reset, the same pushes: the same bits; the stream's memory has not moved
    stream.reset()
    again = _drive(stream, audio_t, stream_ref.partition("empty_last", L, h, seed=L), seed, counts)
    for key in KEYS:
        assert np.array_equal(again[key], runs["empty_last"][key]), key
    assert stream.bytes == nbytes
    stream.close()


def test_both_p_layouts_give_the_same_bits():
    """p handed over as ``forward_stereo_tiles`` leaves it (channels side by side in a row, garbage in the pad columns) and in the
    Lasagne layout: the same estimates and samples"""
    N, h, tc, ov, S, C = 64, 16, 8, 5, 4, 2
    F, ldt = 33, 36
    L = stream_ref.lengths(N, h, tc, ov)[0]
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, np.hanning(N))
    audio_t = ctx.to_device(np.stack([0.5 * synth_audio(L, seed=70 + c) for c in range(C)]), np.float32)
    outs = []
    for layout in ("lasagne", "rows"):
        stream = runtime.StereoStream(plan, S, C, tc, ov, TILER_LIBRARY, 0.3, max_push=L)
        tiles = stream.push(audio_t, last=True)
        n = int(tiles.shape[0])
        p = np.stack([stereo_stream_ref.tile_p(k, S, C, tc, F, 3) for k in range(n)], axis=1)          # [S C, n, tc, F]
        if layout == "rows":
            full = np.full((S, n, tc, C, ldt), np.float32(np.nan))
            full[..., :F] = p.reshape(S, C, n, tc, F).transpose(0, 2, 3, 1, 4)
            p = full
        pcm, est = stream.pull(ctx.to_device(p, np.float32), want_est=True)
        outs.append((ctx.to_host(pcm), ctx.to_host(est)))
        stream.close()
    assert np.isfinite(outs[1][0]).all() and outs[0][0].any()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ tile forward
N, HOP, F, TC, OV = 1024, 512, 513, 30, 25
BLOCK = (TC - OV) * HOP
_RUN = {}


def _params():
    if "params" not in _RUN:
        _RUN["params"] = synth_params("dsd_ild", TC, F, seed=7)
    return _RUN["params"]


def _separator():
    if "sep" not in _RUN:
        _RUN["sep"] = dcs.Separator("dsd_ild", _params(), 0.3, TC, OV, 32, F, N, HOP, np.hanning, tiler='library')
    return _RUN["sep"]


def _forward_case():
    """33 library tiles of synthetic stereo audio x 0.3 and their float64 network output, computed once"""
    if "fwd" not in _RUN:
        L = (32 * (TC - OV) + OV + 3) * HOP
        audio = synth_audio(L, seed=23, channels=2)
        mag = np.stack([stft_np.compute_file(audio[:, c], frameSize=N, hopSize=HOP, window=np.hanning) for c in range(2)])
        mag = 0.3 * mag.astype(np.float32)
        batches, n = tiling_np.generate_overlapadd(mag, F, TC, OV, 33, tiler=tiling_np.LIBRARY)
        assert n >= 33
        tiles = np.ascontiguousarray(batches.reshape(-1, 2, TC, F)[:33], dtype=np.float32)
        want = net_ref.forward('dsd_ild', _params(), tiles, inverse='explicit').numpy()   # [33, S C, tc, F]
        _RUN["fwd"] = (tiles, want)
    return _RUN["fwd"]


def _forward(net, tiles):
    """Lasagne tiles ``[n, C, tc, F]`` -> ``forward_stereo_tiles`` -> ``[n, S C, tc, F]`` on the host"""
    ctx = net.ctx
    out = ctx.to_host(net.forward_stereo_tiles(ctx.to_device(stereo_rows_from_tiles(tiles), np.float32)))   # [S, n, tc, C, ld]
    assert out.shape == (net.S, tiles.shape[0], net.tc, 2, stereo_ld(net.F))
    got = stereo_tiles_from_rows(out, net.F)                                                                # [S, n, C, tc, F]
    return got.transpose(1, 0, 2, 3, 4).reshape(tiles.shape[0], net.S * 2, net.tc, net.F)


@pytest.mark.parametrize("n", (1, 3, 33))
def test_tile_forward_matches_the_float64_graph(n):
    sep = _separator()
    tiles, want = _forward_case()
    got = _forward(sep.net, tiles[:n])
    err = float(np.abs(got - want[:n]).max())
    print("forward_stereo_tiles n=%d: max |err| %.3g, max p %.3g" % (n, err, float(want[:n].max())))
    assert (got >= 0).all() and np.isfinite(got).all() and want[:n].max() > 1e-2
    assert err < 1e-4
    # tile k does not depend on which other tiles are in the call
    if n > 1:
        alone = _forward(sep.net, tiles[n - 1:n])
        other = _forward(sep.net, tiles[1:n])
        assert np.abs(alone[0] - got[n - 1]).max() <= 1e-6 and np.abs(other - got[1:]).max() <= 1e-6


def test_tile_forward_small_fixture(golden):
    g = golden("net_dsdild_f33_glorot")
    arch, Fg, seed, kind = str(g["arch"]), int(g["F"]), int(g["seed"]), str(g["kind"])
    assert arch == "dsd_ild" and kind == "glorot"
    params = cases.case_params(arch, 30, Fg, seed, kind)
    ctx = runtime.default_context()
    net = runtime.Network(ctx, arch, params, 30, Fg)
    x = np.asarray(g["x"], dtype=np.float32)
    got = _forward(net, x)
    want = net_ref.forward('dsd_ild', params, x, inverse='explicit').numpy()
    assert got.shape == g["p"].shape == want.shape
    print("net_dsdild_f33_glorot: max |err| %.3g (fixture %.3g)" % (float(np.abs(got - want).max()), float(np.abs(got - g["p"]).max())))
    assert (got >= 0).all() and np.abs(got - want).max() < 1e-4 and np.abs(got - g["p"]).max() < 1e-4
    # refusals of the Python layer and of the C ABI
    with pytest.raises(ValueError):
        net.forward_stereo_tiles(ctx.to_device(x, np.float32))                               # the Lasagne layout
    mono = runtime.Network(ctx, "dsd", synth_params("dsd", 30, Fg, seed=2), 30, Fg)
    rows = ctx.to_device(stereo_rows_from_tiles(x), np.float32)
    with pytest.raises(ValueError):
        mono.forward_stereo_tiles(rows)
    lib = ctx._lib
    from ctypes import c_void_p
    out = ctx.empty((4, 1, 30, 2, stereo_ld(Fg)), np.float32)
    vp = lambda t: c_void_p(t.data_ptr())
    assert lib.dcs_model_forward_stereo(mono._h, vp(rows), 1, vp(out)) == _lib.DCS_EINVAL
    assert lib.dcs_model_forward_stereo(net._h, None, 1, vp(out)) == _lib.DCS_EINVAL
    assert lib.dcs_model_forward_stereo(net._h, vp(rows), 1, None) == _lib.DCS_EINVAL
    assert lib.dcs_model_forward_stereo(net._h, vp(rows), -1, vp(out)) == _lib.DCS_EINVAL
    assert lib.dcs_model_forward_stereo(net._h, vp(rows), 0, vp(out)) == _lib.DCS_OK
    assert int(net.forward_stereo_tiles(rows[:0]).shape[1]) == 0


# ------------------------------------------------------------------------------------------------ end to end
def _audio():
    L = 44100
    audio = synth_audio(L, seed=61, channels=2)
    audio[L // 3: L // 3 + 5000, 1] = 0.0                                # one channel silent for a while
    return audio


def _run():
    """one second of stereo audio through ``runtime.StereoStream`` composed here, one stride per push, every p kept; and through
    ``StereoStreamSeparator`` with the same blocks"""
    if "e2e" not in _RUN:
        sep = _separator()
        audio = _audio()
        L, ctx = audio.shape[0], sep.ctx
        a2 = ctx.to_device(np.ascontiguousarray(audio.T), np.float32)
        eng = runtime.StereoStream(sep.plan, sep.net.S, 2, TC, OV, TILER_LIBRARY, 0.3, max_push=BLOCK)
        mags, phs, ests, pcms, ps = [], [], [], [], []
        starts = list(range(0, L, BLOCK))
        for i in range(len(starts) + 1):
            last = i == len(starts)
            tiles, mag, ph = eng.push(None if last else a2[:, starts[i]:starts[i] + BLOCK], last=last, want_frames=True)
            p = None
            if int(tiles.shape[0]):
                p = sep.net.forward_stereo_tiles(tiles)
                ps.append(stereo_tiles_from_rows(ctx.to_host(p), F))                          # [S, n, C, tc, F]
            pcm, est = eng.pull(p, want_est=True)
            mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        ss = sep.stream_stereo(max_block=BLOCK)
        got = [ss.push(audio[s:s + BLOCK]) for s in starts] + [ss.finish()]
        _RUN["e2e"] = dict(sep=sep, audio=audio, mag=np.concatenate(mags, axis=1), phase=np.concatenate(phs, axis=1),
                           est=np.concatenate(ests, axis=2), pcm=np.concatenate(pcms, axis=2),
                           p=np.concatenate(ps, axis=1).transpose(0, 2, 1, 3, 4),              # [S, C, n, tc, F]
                           pieces=pcms, separator_pieces=got, stream=ss, starts=starts)
    return _RUN["e2e"]


def test_end_to_end_against_the_float64_reference_and_the_oracle():
    run = _run()
    sep, audio = run["sep"], run["audio"]
    S, L = sep.net.S, audio.shape[0]
    T = stft_np.frame_count(L, HOP)
    n = len(tiling_np.tile_starts(T, TC, OV, tiling_np.LIBRARY))
    assert run["p"].shape == (S, 2, n, TC, F) and n >= 1 and (run["p"] >= 0).all()
    assert run["est"].shape == (2, S, T, F) and run["pcm"].shape == (2, S, L)
    # the stream's own definition at the product's own p, magnitudes and phases
    ref = stereo_stream_ref.whole_file(audio, N, HOP, TC, OV, tiling_np.LIBRARY, S, np.hanning(N), 0.3, run["p"], mag=run["mag"],
                                       phase=run["phase"])
    lim = stereo_stream_ref.bound(S, TC, OV, run["mag"].astype(np.float64), stereo_stream_ref.c0_f32(0.3))[:, None]
    e_est = np.abs(run["est"] - ref["est"])
    e_pcm = 0.0
    for c in range(2):
        for s in range(S):
            want = stft_np.compute_inverse(run["est"][c, s].astype(np.float64), run["phase"][c].astype(np.float64), N, HOP,
                                           np.hanning)[:L]
            e_pcm = max(e_pcm, float(np.abs(run["pcm"][c, s] - want).max()))
    print("est/bound %.3g pcm %.3g" % (float((e_est / lim).max()), e_pcm))
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    # the stems against the oracle and against the whole-file path
    stems = np.ascontiguousarray(run["pcm"].astype(np.float64).transpose(2, 1, 0))             # [L, S, 2]
    want = pipeline.separate_stereo(_params(), audio, 0.3, TC, OV, 32, N, HOP, np.hanning)
    whole = sep.separate_stereo(audio)
    e_oracle, e_whole = float(np.abs(stems - want).max()), float(np.abs(stems - whole).max())
    print("stems: against the oracle %.3g, against separate_stereo %.3g" % (e_oracle, e_whole))
    assert stems.shape == want.shape == whole.shape == (L, S, 2) and np.abs(want).max() > 1e-3
    assert e_oracle < 1e-4
    assert e_whole < 2e-4
    # StereoStreamSeparator with the same blocks: the same bits in the layout of separate_stereo
    assert len(run["separator_pieces"]) == len(run["pieces"])
    for a, b in zip(run["separator_pieces"], run["pieces"]):
        assert a.dtype == np.float64 and a.shape == (b.shape[2], S, 2) and np.array_equal(a, b.astype(np.float64).transpose(2, 1, 0))
    assert sum(x.shape[0] for x in run["separator_pieces"]) == L
    with pytest.raises(ValueError):
        run["stream"].finish()                                            # a second finish()


# ------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refusals():
    from ctypes import POINTER, byref, c_double, c_int64, c_void_p
    ctx = runtime.default_context()
    lib = ctx._lib
    plan = runtime.StftPlan(ctx, 64, 16, np.hanning(64))
    rise = np.linspace(0., 1., 5)
    rp = rise.ctypes.data_as(POINTER(c_double))

    def create(plan, S=2, C=2, tc=8, ov=5, max_push=128, scale=0.3):
        h = c_void_p()
        return lib.dcs_stream_create_stereo(plan._h, S, C, tc, ov, TILER_LIBRARY, scale, rp, max_push, byref(h)), h
    for kw in (dict(C=0), dict(C=9), dict(S=0), dict(S=9), dict(ov=8), dict(ov=0), dict(max_push=0), dict(scale=0.0)):
        assert create(plan, **kw)[0] == _lib.DCS_EINVAL, kw
    assert create(runtime.StftPlan(ctx, 64, 48, np.hanning(64)))[0] == _lib.DCS_EINVAL       # hop above frameSize / 2
    assert create(runtime.StftPlan(ctx, 64, 24, np.hanning(64)))[0] == _lib.DCS_EUNSUPPORTED  # hop does not divide frameSize
    assert create(runtime.StftPlan(ctx, 32, 8, np.hanning(32)))[0] == _lib.DCS_EUNSUPPORTED   # frameSize below 64
    rc, h = create(plan)
    assert rc == _lib.DCS_OK
    a = ctx.to_device(np.zeros((2, 128)), np.float32)
    tiles = ctx.empty((int(lib.dcs_stream_max_tiles(h)), 8, 2, 36), np.float32)
    p = ctx.to_device(np.ones((4, int(tiles.shape[0]), 8, 33)), np.float32)                    # Lasagne [S C][n][tc][F]
    pcm = ctx.empty((2, 2, 400), np.float32)
    nt, nf, no = c_int64(), c_int64(), c_int64()
    vp = lambda t: c_void_p(t.data_ptr())

    def push(n, last=0, row_stride=128):
        return lib.dcs_stream_push_stereo(h, vp(a), row_stride, n, last, vp(tiles), int(tiles.shape[0]), byref(nt), None, None, 0,
                                          0, byref(nf))

    def pull(n, src=None, ch=None, ld=33, ch_stride=800, stride=400):
        rows = int(p.shape[1]) * 8
        return lib.dcs_stream_pull_stereo(h, vp(p), 2 * rows * 33 if src is None else src, rows * 33 if ch is None else ch, ld, n,
                                          vp(pcm), ch_stride, stride, 400, byref(no), None, 0, 0, 0)
    assert push(129) == _lib.DCS_EINVAL                                   # n > max_push
    assert push(100, row_stride=99) == _lib.DCS_EINVAL                    # rows overlap
    assert pull(0) == _lib.DCS_EINVAL                                     # no push to pull for
    assert push(128) == _lib.DCS_OK and nt.value == 0
    assert push(16) == _lib.DCS_EINVAL                                    # two pushes in a row
    assert pull(1) == _lib.DCS_EINVAL                                     # the wrong tile count
    assert pull(0) == _lib.DCS_OK and no.value == 0
    assert push(128) == _lib.DCS_OK and nt.value == 3                     # 256 samples: 15 frames, tiles at 0, 3 and 6
    assert pull(3, ld=32) == _lib.DCS_EINVAL                              # rows below the bins
    assert pull(3, ch=40) == _lib.DCS_EINVAL                              # channels neither planes nor side by side
    assert pull(3, src=100) == _lib.DCS_EINVAL                            # sources overlap
    assert pull(3, ch_stride=400) == _lib.DCS_EINVAL                      # output channels overlap
    # the other kinds' calls on a stereo stream
    assert lib.dcs_stream_push(h, None, 0, 0, None, 0, None, None, None, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull(h, None, 0, 0, None, 0, 0, None, None, 0, 0) == _lib.DCS_EINVAL
    assert lib.dcs_stream_push_channels(h, None, 0, 0, 0, None, 0, None, None, None, 0, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull_channels(h, None, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0) == _lib.DCS_EINVAL
    assert pull(3) == _lib.DCS_OK and no.value == 9 * 16 - 32
    assert lib.dcs_stream_reset(h) == _lib.DCS_OK and push(0, 1) == _lib.DCS_OK
    assert pull(0) == _lib.DCS_EINVAL                                     # the ended signal gave no tile
    assert push(16) == _lib.DCS_EINVAL                                    # a push after the end
    # the stereo calls on the other kinds of stream
    mono = runtime.Stream(plan, 2, 8, 5, max_push=128)
    chan = runtime.ChannelStream(plan, 2, 2, 8, 5, max_push=128)
    for other in (mono, chan):
        assert lib.dcs_stream_push_stereo(other._h, None, 0, 0, 0, None, 0, None, None, None, 0, 0, None) == _lib.DCS_EINVAL
        assert lib.dcs_stream_pull_stereo(other._h, None, 0, 0, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0) == _lib.DCS_EINVAL
        other.close()
    assert lib.dcs_stream_push_stereo(None, None, 0, 0, 0, None, 0, None, None, None, 0, 0, None) == _lib.DCS_EINVAL
    ctx.synchronize()
    assert lib.dcs_stream_destroy(h) == _lib.DCS_OK


def test_public_interface_refusals():
    sep, audio = _separator(), _audio()
    mono = dcs.Separator("dsd", synth_params("dsd", TC, F, seed=7), 0.3, TC, OV, 32, F, N, HOP, np.hanning)
    with pytest.raises(ValueError):
        mono.stream_stereo()
    with pytest.raises(ValueError):
        sep.stream()
    with pytest.raises(ValueError):
        sep.stream_channels()
    ss = sep.stream_stereo(max_block=4096)
    nbytes = ss.device_bytes
    assert isinstance(ss, StereoStreamSeparator)
    with pytest.raises(ValueError):
        ss.push(audio[:100, 0])                                           # a mono block
    with pytest.raises(ValueError):
        ss.push_device(sep.ctx.to_device(np.zeros((3, 100)), np.float32)) # three rows: the channel stream's layout
    assert ss.push(audio[:5000]).shape == (0, sep.net.S, 2)
    with pytest.raises(IndexError, match="tuple index out of range"):     # too short for one tile
        ss.finish()
    ss.reset()
    assert ss.push(audio[:100]).shape == (0, sep.net.S, 2) and ss.device_bytes == nbytes


# ------------------------------------------------------------------------------------------------ any sample rate
RATE, RATE_BLOCK = 48000, 7000


def test_rate_stream_equals_the_manual_composition():
    import torch
    sep = _separator()
    ctx = sep.ctx
    audio = 0.5 * synth_audio(RATE + 33, seed=21, channels=2)
    L = audio.shape[0]
    rows = np.ascontiguousarray(audio.T, dtype=np.float32)
    sizes = [RATE_BLOCK] * (L // RATE_BLOCK) + [L % RATE_BLOCK]
    rs = RateStream(sep.stream_stereo(max_block=RATE_BLOCK), RATE)
    nbytes = rs.device_bytes
    assert nbytes > rs.inner.device_bytes
    rows_d = ctx.to_device(rows, np.float32)
    outs, pos, emitted, started = [], 0, 0, False
    for n in sizes:
        out = rs.push_device(rows_d[:, pos:pos + n])
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
    assert got.shape == (2, S, L)                                          # the lengths add up to the samples pushed
    # the manual composition: whole-file Resampler down, the inner stream cut where the converter's counts cut it, Resampler back
    down, up = ctx.resampler(RATE, 44100), ctx.resampler(44100, RATE)
    c = ResampleCounts(down.up, down.down, down.half)
    y = down(rows_d)
    inner = sep.stream_stereo(max_block=RATE_BLOCK)
    cuts = [c.emitted(P) for P in np.cumsum([0] + list(sizes))] + [c.emitted(L, True)]
    assert cuts[-1] == int(y.shape[1])
    pieces = [inner.push_device(y[:, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pieces.append(inner.finish_device())
    with ctx.stream_scope():
        pcm = torch.cat(pieces, dim=-1)
        assert int(pcm.shape[-1]) == cuts[-1]
        want = ctx.to_host(up(pcm.reshape(-1, cuts[-1]))[:, :L].reshape(2, S, L))
    assert np.isfinite(got).all() and got.any() and np.array_equal(got, want)
    assert rs.device_bytes == nbytes
    with pytest.raises(ValueError):
        rs.finish_device()
    # the host interface: the same bits in the layout of separate_stereo
    rs.reset()
    host = np.concatenate([rs.push(audio[s:s + RATE_BLOCK]) for s in range(0, L, RATE_BLOCK)] + [rs.finish()], axis=0)
    assert host.dtype == np.float64 and np.array_equal(host, got.astype(np.float64).transpose(2, 1, 0))


# ------------------------------------------------------------------------------------------------ guard harness
_CHILD = r'''
import hashlib, json, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd.synth import synth_audio, synth_params
sep = dcs.Separator("dsd_ild", synth_params("dsd_ild", 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, tiler="library")
audio = 0.5 * synth_audio(44100 + 33, seed=21, channels=2)
def run(ss):
    outs, blocks, nbytes = [], None, None
    for i in range(0, audio.shape[0], 4000):
        outs.append(ss.push(audio[i:i + 4000]))
        if blocks is None:                                # after the first pull
            blocks, nbytes = sep.ctx.check_guards(), ss.device_bytes
    return outs + [ss.finish()], blocks, nbytes
run(sep.stream_stereo(max_block=4000))                    # the network and the context make their own blocks on first need
ss = sep.stream_stereo(max_block=4000)
outs, blocks0, nbytes = run(ss)
pcm = np.concatenate(outs, axis=0)
blocks1 = sep.ctx.check_guards()                          # raises when a red zone was written
json.dump({"sha256": hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest(), "finite": bool(np.isfinite(pcm).all()),
           "shape": list(pcm.shape), "any": bool(pcm.any()), "blocks_after_first_pull": blocks0, "blocks_after_last_pull": blocks1,
           "bytes_before": nbytes, "bytes_after": ss.device_bytes}, open(OUT, "w"))
'''


def test_guard_harness(tmp_path):
    """one stereo (ILD) stream under DCS_WS_GUARD with both poison bytes (the manner of tests/test_gpu_stream.py): no red zone
    written, every output finite -- a ring slot or a pad column read before it was written would be a NaN under 0xFF --, the two
    runs bit-identical, and neither the block count nor the stream's bytes change after the first pull"""
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
        assert r["finite"] and r["any"] and r["shape"] == [44100 + 33, 4, 2]
        assert r["blocks_after_first_pull"] == r["blocks_after_last_pull"] >= 7 and r["bytes_before"] == r["bytes_after"] > 0
    assert res[0]["sha256"] == res[1]["sha256"]


# ------------------------------------------------------------------------------------------------ command line
def _script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_command_line(tmp_path):
    import scipy.io.wavfile
    from deepconvsep_amd.separation import read_wav, save_model, write_wav
    from deepconvsep_amd.stereo_training import SOURCES as NAMES
    sep, script = _separator(), _script()
    model, wav, wav48 = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "mix48.wav")
    out, out48 = str(tmp_path / "stems"), str(tmp_path / "stems48")
    save_model(model, synth_params("dsd_ild", TC, F, seed=7))
    write_wav(wav, 0.5 * synth_audio(44100, seed=5, channels=2), 44100)
    write_wav(wav48, 0.5 * synth_audio(48000, seed=6, channels=2), 48000)
    # the truncated int16 stems of StereoStreamSeparator with the same blocks, as two-channel files
    script.main(["-a", "dsd_ild", "-i", wav, "-o", out, "-m", model, "--block", "3000"])
    _, audio = read_wav(wav)
    ss = sep.stream_stereo(max_block=3000)
    want = np.concatenate([ss.push(audio[i:i + 3000]) for i in range(0, audio.shape[0], 3000)] + [ss.finish()], axis=0)
    assert sorted(os.listdir(out)) == sorted(s + ".wav" for s in NAMES)
    loud = 0
    for i, s in enumerate(NAMES):
        rate, got = scipy.io.wavfile.read(os.path.join(out, s + ".wav"))
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (audio.shape[0], 2)
        assert np.array_equal(got, (want[:, i] * 32767).astype(np.int16)), s
        loud += int(np.abs(got.astype(np.int64)).max() > 1000)
    assert loud >= 1
    # --resample (and --stereo, implied and accepted): stems at the file's rate and of the file's length
    script.main(["-a", "dsd_ild", "-i", wav48, "-o", out48, "-m", model, "--block", "6000", "--stereo", "--resample"])
    loud = 0
    for s in NAMES:
        rate, got = scipy.io.wavfile.read(os.path.join(out48, s + ".wav"))
        assert rate == 48000 and got.dtype == np.int16 and got.shape == (48000, 2)
        loud += int(np.abs(got.astype(np.int64)).max() > 1000)
    assert loud >= 1
    with pytest.raises(SystemExit, match="Sample rate is not 44100"):
        script.main(["-a", "dsd_ild", "-i", wav48, "-o", out48, "-m", model])
