"""Streaming separation on the MI355X (csrc/stream.hip; include/dcs.h has the contract).

Machinery tests drive ``dcs_stream_push`` / ``dcs_stream_pull`` (through ``runtime.Stream``, which only allocates the outputs)
with a synthetic positive ``p`` per tile and no network, over the shapes of tests/stream_ref.py with 1, 2 and 4 sources; the
references are the whole-file float64 ones evaluated at the device's own magnitudes and phases, so each stage is held to its own
bound: ``stft_ref.BOUND_MAG`` / ``BOUND_CPX`` for the frames, ``chanmask_ref.bound`` for the estimates, ``stft_ref.BOUND_INV``
for the samples.  End-to-end tests run the DSD and iKala graphs on one second of audio.
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
from deepconvsep_amd.streaming import StreamCounts
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import stft_np, tiling_np

import chanmask_ref
import stft_ref
import stream_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = (1, 2, 4)
TILER_CODE = {tiling_np.SCRIPT: TILER_SCRIPT, tiling_np.LIBRARY: TILER_LIBRARY}
EPS_CODE = {"A": EPS_A, "B": EPS_B}


def _drive(stream, audio_t, sizes, seed, counts):
    """the signal through the stream in blocks of ``sizes`` with the synthetic p of stream_ref.tile_p -> host arrays, and every
    count the library returned checked against StreamCounts on the way"""
    ctx = stream.ctx
    mags, phs, ests, pcms, pos, k = [], [], [], [], 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = (counts.frames(pos), counts.tiles(pos), counts.emitted(pos))
        tiles, mag, ph = stream.push(audio_t[pos:pos + n] if n else None, last=last, want_frames=True)
        pos += n
        assert stream.last_frames == counts.frames(pos, last) - before[0] == int(mag.shape[0])
        assert stream.last_tiles == counts.tiles(pos, last) - before[1] == int(tiles.shape[0])
        assert stream.last_tiles <= stream.max_tiles
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stream_ref.tile_p(k + j, stream.S, stream.tc, stream.F, seed) for j in range(nt)], axis=1),
                              np.float32)
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        assert stream.last_samples == counts.emitted(pos, last) - before[2] == int(pcm.shape[1])
        mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
    return dict(mag=np.concatenate(mags), phase=np.concatenate(phs), est=np.concatenate(ests, axis=1),
                pcm=np.concatenate(pcms, axis=1), tiles=k)


@pytest.mark.parametrize("S", SOURCES)
@pytest.mark.parametrize("shape", stream_ref.SHAPES, ids=stream_ref.shape_id)
def test_machinery_against_float64_and_across_partitions(shape, S):
    N, h, tc, ov, wname = shape
    i = stream_ref.SHAPES.index(shape) + SOURCES.index(S)
    tiler, conv = stream_ref.TILERS[i % 2], chanmask_ref.CONVENTIONS[(i // 2) % 2]
    L = stream_ref.lengths(N, h, tc, ov)[SOURCES.index(S)]
    win = stream_ref.window(wname, N)
    F, scale, seed = N // 2 + 1, 0.3, 11 * i
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, win)
    audio = 0.5 * synth_audio(L, seed=3 + i)
    audio_t = ctx.to_device(audio, np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)
    stream = runtime.Stream(plan, S, tc, ov, TILER_CODE[tiler], EPS_CODE[conv], scale, max_push=L)
    nbytes = stream.bytes
    assert nbytes > 0 and stream.max_tiles == counts.max_tiles(L)
    runs = {}
    for kind in ("one", "hop", "empty_last"):
        stream.reset()
        runs[kind] = _drive(stream, audio_t, stream_ref.partition(kind, L, h, seed=L), seed, counts)
    one = runs["one"]
    T = stft_np.frame_count(L, h)
    n_tiles = len(tiling_np.tile_starts(T, tc, ov, tiler))
    assert one["mag"].shape == one["phase"].shape == (T, F) and one["est"].shape == (S, T, F) and one["pcm"].shape == (S, L)
    assert one["tiles"] == n_tiles >= 1
    # 1. frames
    X = stft_np.stft_norm(audio.astype(np.float32).astype(np.float64), win, float(h), float(N)) / np.sqrt(N)
    e_mag = float(np.abs(one["mag"] - np.abs(X)).max())
    e_cpx = float(np.abs(one["mag"] * np.exp(1j * one["phase"].astype(np.float64)) - X).max())
    # 2. estimates and 3. samples, at the device's own magnitudes and phases
    ref = stream_ref.whole_file(audio, N, h, tc, ov, tiler, conv, S, win, scale, seed, mag=one["mag"], phase=one["phase"])
    lim = chanmask_ref.bound(S, tc, ov, one["mag"].astype(np.float64)[None])
    e_est = np.abs(one["est"] - ref["est"])
    e_pcm = float(np.abs(one["pcm"] - ref["pcm"]).max())
    print("%s S=%d: mag %.3g cpx %.3g est/bound %.3g pcm %.3g" % (stream_ref.shape_id(shape), S, e_mag, e_cpx,
                                                                float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm))
    assert e_mag <= stft_ref.BOUND_MAG and e_cpx <= stft_ref.BOUND_CPX
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    assert np.isfinite(one["pcm"]).all() and one["pcm"].any()
    # 4. rows past the last tile, and the samples only they reach, are exactly zero
    rows = (n_tiles - 1) * (tc - ov) + tc
    if rows < T:
        assert not one["est"][:, rows:].any()
        first = rows * h + N // 2                                    # frame n reaches samples < n h + N / 2
        if first < L:
            assert not one["pcm"][:, first:].any()
    # 6. however the signal is cut: the same bits
    for kind in ("hop", "empty_last"):
        for key in ("mag", "phase", "est", "pcm"):
            assert np.array_equal(one[key], runs[kind][key]), (kind, key)
    # 7. reset, the same pushes: the same bits; the stream's memory has not moved
    stream.reset()
    again = _drive(stream, audio_t, stream_ref.partition("empty_last", L, h, seed=L), seed, counts)
    for key in ("mag", "phase", "est", "pcm"):
        assert np.array_equal(again[key], runs["empty_last"][key]), key
    assert stream.bytes == nbytes
    stream.close()


# ------------------------------------------------------------------------------------------------ end to end
N, HOP, F, TC = 1024, 512, 513, 30
OVERLAP = {"dsd": 25, "ikala": 20}
_RUNS = {}


def _run(arch):
    if arch not in _RUNS:
        ov = OVERLAP[arch]
        sep = dcs.Separator(arch, synth_params(arch, TC, F, seed=7), 0.3, TC, ov, 32, F, N, HOP, np.hanning)
        assert sep.net.arch.eps_mode == EPS_A
        audio = 0.5 * synth_audio(44100 + 21, seed=12)
        L, block = audio.size, (TC - ov) * HOP
        ctx = sep.ctx
        a = ctx.to_device(audio, np.float32)
        eng = runtime.Stream(sep.plan, sep.net.S, TC, ov, sep.tiler, EPS_A, 0.3, max_push=block)
        mags, phs, ests, pcms, ps = [], [], [], [], []
        starts = list(range(0, L, block))
        for i in range(len(starts) + 1):
            last = i == len(starts)
            tiles, mag, ph = eng.push(None if last else a[starts[i]:starts[i] + block], last=last, want_frames=True)
            p = None
            if int(tiles.shape[0]):
                p = sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:sep.net.S]
                ps.append(ctx.to_host(p))
            pcm, est = eng.pull(p, want_est=True)
            mags.append(ctx.to_host(mag)); phs.append(ctx.to_host(ph)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm))
        ss = sep.stream(max_block=block)
        got = [ss.push(audio[s:s + block]) for s in starts] + [ss.finish()]
        _RUNS[arch] = dict(arch=arch, ov=ov, sep=sep, audio=audio, block=block, mag=np.concatenate(mags), phase=np.concatenate(phs),
                           est=np.concatenate(ests, axis=1), pcm=np.concatenate(pcms, axis=1), p=np.concatenate(ps, axis=1),
                           pieces=pcms, separator_pieces=got, stream=ss)
    return _RUNS[arch]


@pytest.mark.parametrize("arch", ["dsd", "ikala"])
def test_end_to_end_against_the_float64_reference(arch):
    """push -> ``forward_raw`` -> pull composed here, one stride (``st * hop`` samples) per push, every ``p`` kept; estimates and
    samples against the float64 whole-file reference evaluated at the product's own ``p``, magnitudes and phases; the stems add
    up to the mixture where whole tiles cover it; ``StreamSeparator`` with the same blocks returns the same bits.  No bitwise
    claim is made against ``Separator.separate`` or across block sizes end to end: which kernel family the network runs depends
    on the tile count of a call, so its ``p`` differs in the last bits between groupings of the same tiles."""
    run = _run(arch)
    sep, audio, ov = run["sep"], run["audio"], run["ov"]
    S, L = sep.net.S, audio.size
    T = stft_np.frame_count(L, HOP)
    assert run["p"].shape[0] == S and run["p"].shape[1] == len(tiling_np.tile_starts(T, TC, ov, tiling_np.SCRIPT)) >= 1
    assert run["est"].shape == (S, T, F) and run["pcm"].shape == (S, L) and (run["p"] >= 0).all()
    ref = stream_ref.whole_file(audio, N, HOP, TC, ov, tiling_np.SCRIPT, "A", S, np.hanning(N), 0.3, p=run["p"], mag=run["mag"],
                                phase=run["phase"])
    lim = chanmask_ref.bound(S, TC, ov, run["mag"].astype(np.float64)[None])
    e_est = np.abs(run["est"] - ref["est"])
    e_pcm = float(np.abs(run["pcm"] - ref["pcm"]).max())
    hi = ((run["p"].shape[1] - 1) * (TC - ov) + TC - 4) * HOP - N
    assert hi > 4 * N
    e_sum = float(np.abs(run["pcm"].sum(axis=0)[N:hi] - audio[N:hi]).max())
    print("%s: est/bound %.3g pcm %.3g sum %.3g" % (arch, float((e_est / np.where(lim > 0, lim, 1.0)).max()), e_pcm, e_sum))
    assert np.all(e_est <= lim)
    assert e_pcm <= stft_ref.BOUND_INV
    assert e_sum < 2e-5
    assert len(run["separator_pieces"]) == len(run["pieces"])
    for a, b in zip(run["separator_pieces"], run["pieces"]):
        assert a.dtype == np.float64 and np.array_equal(a, b.astype(np.float64))
    assert sum(x.shape[1] for x in run["separator_pieces"]) == L
    with pytest.raises(ValueError):
        run["stream"].finish()                                            # a second finish()


def test_bad_input_is_refused():
    run = _run("dsd")
    sep = run["sep"]
    ss = sep.stream(max_block=4096)
    ss.push(run["audio"][:5000])
    with pytest.raises(IndexError):                                       # too short for one tile: what separate_channels raises
        ss.finish()
    ss.reset()
    assert ss.push(run["audio"][:100]).shape == (sep.net.S, 0)
    lib, ctx = _lib.load(), sep.ctx
    from ctypes import POINTER, byref, c_double, c_int64, c_void_p
    rise = np.linspace(0., 1., 25)
    rp = rise.ctypes.data_as(POINTER(c_double))

    def create(plan, S=4, tc=30, ov=25, max_push=2048):
        h = c_void_p()
        return lib.dcs_stream_create(plan._h, S, tc, ov, TILER_SCRIPT, EPS_A, 0.3, rp, max_push, byref(h)), h
    assert create(sep.plan, S=9)[0] == _lib.DCS_EINVAL
    assert create(sep.plan, ov=30)[0] == _lib.DCS_EINVAL
    wide = runtime.StftPlan(ctx, 1024, 700, np.hanning(1024))
    assert create(wide)[0] == _lib.DCS_EINVAL                             # hop above frameSize / 2
    rc, h = create(sep.plan)
    assert rc == _lib.DCS_OK
    a = ctx.to_device(run["audio"][:4096], np.float32)
    tiles = ctx.empty((int(lib.dcs_stream_max_tiles(h)), 1, 30, 513), np.float32)
    pcm = ctx.empty((4, 40000), np.float32)
    nt, nf, no = c_int64(), c_int64(), c_int64()

    def push(n, last=0):
        return lib.dcs_stream_push(h, c_void_p(a.data_ptr()), n, last, c_void_p(tiles.data_ptr()), int(tiles.shape[0]), byref(nt),
                                   None, None, 0, byref(nf))

    def pull(n):
        return lib.dcs_stream_pull(h, c_void_p(tiles.data_ptr()), 30 * 513, n, c_void_p(pcm.data_ptr()), 40000, 40000, byref(no),
                                   None, 0, 0)
    assert push(2049) == _lib.DCS_EINVAL                                  # n > max_push
    assert pull(0) == _lib.DCS_EINVAL                                     # no push to pull for
    assert push(2048) == _lib.DCS_OK and nt.value == 0
    assert push(16) == _lib.DCS_EINVAL                                    # two pushes in a row
    assert pull(1) == _lib.DCS_EINVAL                                     # the wrong tile count
    assert pull(0) == _lib.DCS_OK and no.value == 0
    assert push(0, 1) == _lib.DCS_OK
    assert pull(0) == _lib.DCS_EINVAL                                     # the ended signal gave no tile
    assert push(16) == _lib.DCS_EINVAL                                    # a push after the end
    assert lib.dcs_stream_reset(h) == _lib.DCS_OK and push(16) == _lib.DCS_OK and pull(0) == _lib.DCS_OK
    ctx.synchronize()
    assert lib.dcs_stream_destroy(h) == _lib.DCS_OK


# ------------------------------------------------------------------------------------------------ guard harness
_CHILD = r'''
import hashlib, json, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd.synth import synth_audio, synth_params
sep = dcs.Separator("dsd", synth_params("dsd", 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning)
audio = 0.5 * synth_audio(44100 + 21, seed=12)
def run(ss):
    return [ss.push(audio[i:i + 4000]) for i in range(0, audio.size, 4000)] + [ss.finish()]
run(sep.stream(max_block=4000))                       # the network makes its own blocks on first need: all of them exist after this
ss = sep.stream(max_block=4000)
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
    """one DSD stream under DCS_WS_GUARD with both poison bytes (the manner of tests/test_gpu_guard.py): no red zone written,
    every output finite -- a ring slot read before it was written would be a NaN under 0xFF --, the two runs bit-identical, and the
    stream neither allocates nor grows after its creation"""
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
        assert r["blocks_after_create"] == r["blocks_after_last_pull"] >= 7 and r["bytes_before"] == r["bytes_after"] > 0
    assert res[0]["sha256"] == res[1]["sha256"]


# ------------------------------------------------------------------------------------------------ command line
def test_command_line_writes_the_truncated_stream(tmp_path):
    import importlib.util
    import scipy.io.wavfile
    from deepconvsep_amd.separation import output_paths, read_wav, save_model, to_mono, write_wav
    run = _run("dsd")
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    model, wav, out = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "stems")
    save_model(model, synth_params("dsd", TC, F, seed=7))
    write_wav(wav, 0.5 * synth_audio(44100, seed=5, channels=2), 44100)
    script.main(["-a", "dsd", "-i", wav, "-o", out, "-m", model, "--block", "3000"])
    _, audio = read_wav(wav)
    mono = to_mono(audio, "dsd")
    ss = run["sep"].stream(max_block=3000)
    want = np.concatenate([ss.push(mono[i:i + 3000]) for i in range(0, mono.size, 3000)] + [ss.finish()], axis=1)
    for i, path in enumerate(output_paths("dsd", wav, out)):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (mono.size,)
        assert np.array_equal(got, (want[i] * 32767).astype(np.int16)), path
