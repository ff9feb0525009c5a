"""The online multichannel Wiener filter on the two-channel streams, on the MI355X (``dcs_stream_set_mwf`` /
``dcs_stream_mwf_last`` in csrc/stream.hip, ``dcs_mwf_online_*`` in csrc/mwf_online.hip; include/dcs.h has the contracts).

Machinery tests drive ``runtime.ChannelStream`` and ``runtime.StereoStream`` with a synthetic positive ``p`` per tile and no
network, staged like tests/test_gpu_stream_channels.py: what the filter does not touch must keep the bits of the same stream
with the filter off; the filtered rows must be the bits of ``runtime.MwfOnline`` on the stream's own magnitudes, phases and
estimates in ONE push, and within the bound of tests/test_gpu_mwf_online.py of the float64 oracle; the samples are held to
``stft_ref.BOUND_INV`` against the float64 inverse of the device's own filtered rows.  The signal goes through a stream with
room for all of it in one push and through a small one whose rings wrap (there a pull's frames reach the filter in two
pieces): the same bits.  End-to-end tests run the DSD and the stereo (ILD) graphs on one second of stereo audio.
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

import mwf_online_ref
import mwf_ref
import stft_ref
import stream_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = tuple(s for s in stream_ref.SHAPES if s[:4] in ((64, 16, 8, 5), (128, 32, 30, 29)))
SOURCES = (2, 4)
KINDS = ("channels", "stereo")
KEYS = ("mag", "phase", "est", "pcm", "fmag", "fphase")
MWF = dict(niter=2, forget=0.95, loading=1e-3, eps=1e-10)
CEILING = 1e-5                                   # tests/test_gpu_mwf.py has the reasons


def _make(kind, plan, S, tc, ov, tiler, scale, max_push):
    if kind == "channels":
        return runtime.ChannelStream(plan, S, 2, tc, ov, tiler, EPS_A, scale, max_push=max_push)
    return runtime.StereoStream(plan, S, 2, tc, ov, tiler, scale, max_push=max_push)


def _drive(stream, audio_t, sizes, seed, counts, filtered=True):
    """the rows ``audio_t`` through the stream in blocks of ``sizes`` with the synthetic p of stream_ref.tile_p (a stereo stream:
    the Lasagne layout, channel ``s C + c``) -> host arrays, frame / sample axis last but one / last"""
    ctx = stream.ctx
    n_p = stream.S * (2 if isinstance(stream, runtime.StereoStream) else 1)
    out = {k: [] for k in KEYS + ("tiles",)}
    pos, k = 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        tiles, mag, ph = stream.push(audio_t[:, pos:pos + n] if n else None, last=last, want_frames=True)
        pos += n
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stream_ref.tile_p(k + j, n_p, stream.tc, stream.F, seed) for j in range(nt)], axis=1),
                              np.float32)
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        assert stream.last_samples == int(pcm.shape[-1]) and stream.last_folded == int(est.shape[-2])
        fm, fp = stream.last_mwf() if filtered else (est, est)
        assert tuple(fm.shape) == tuple(fp.shape) == tuple(est.shape)
        for key, t in zip(KEYS + ("tiles",), (mag, ph, est, pcm, fm, fp, tiles)):
            out[key].append(ctx.to_host(t))
    axis = dict(pcm=-1, tiles=0)
    return {key: np.concatenate(v, axis=axis.get(key, -2)) for key, v in out.items()}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=stream_ref.shape_id)
def test_machinery(shape, S, kind):
    N, h, tc, ov, wname = shape
    C = 2
    i = SHAPES.index(shape) + SOURCES.index(S)
    tiler = tiling_np.LIBRARY if kind == "stereo" else stream_ref.TILERS[i % 2]
    code = {tiling_np.SCRIPT: TILER_SCRIPT, tiling_np.LIBRARY: TILER_LIBRARY}[tiler]
    L = stream_ref.lengths(N, h, tc, ov)[i % 3] + 16 * h                # long enough for the small stream's rings to wrap
    win = stream_ref.window(wname, N)
    F, scale, seed = N // 2 + 1, 0.3, 13 * i + 1
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, h, win)
    chans = np.stack([0.5 * synth_audio(L, seed=3 + i + 17 * c) for c in range(C)])
    rows = chans if kind == "stereo" else np.concatenate([chans, chans.mean(axis=0, keepdims=True)])
    audio_t = ctx.to_device(rows.astype(np.float32), np.float32)
    counts = StreamCounts(N, h, tc, ov, tiler)

    def closed_form(P):
        fp = counts.max_frames(P)
        rf = ff = tc + fp
        rp, rt = -(-tc // (tc - ov)) + counts.max_tiles(P), N // h + ff
        if kind == "stereo":
            base = 4 * (C * (N + P) + 2 * C * rf * F + S * C * rp * tc * F + C * S * ff * F + rt * C * S * N + ov)
        else:
            base = 4 * ((C + 1) * (N + P) + (C + 1) * rf * F + C * rf * F + S * rp * tc * F + C * S * ff * F + rt * C * S * N + ov)
        return base, base + 2 * 4 * C * S * ff * F + (S * 4 * F * 8 + 255) // 256 * 256

    small_push = 2 * h + 2
    big, small, plain = (_make(kind, plan, S, tc, ov, code, scale, P) for P in (L, small_push, L))
    # 6. bytes: the closed form, before and after arming, and back
    assert big.bytes == plain.bytes == closed_form(L)[0] and small.bytes == closed_form(small_push)[0]
    big.set_mwf(**MWF)
    small.set_mwf(**MWF)
    assert big.bytes == closed_form(L)[1] and small.bytes == closed_form(small_push)[1]
    big.set_mwf(0)
    assert big.bytes == closed_form(L)[0]
    big.set_mwf(**MWF)
    nbytes = big.bytes

    one = _drive(big, audio_t, stream_ref.partition("one", L, h, seed=L), seed, counts)
    off = _drive(plain, audio_t, stream_ref.partition("one", L, h, seed=L), seed, counts, filtered=False)
    T = stft_np.frame_count(L, h)
    assert T > tc + counts.max_frames(small_push)                     # the small stream's rings wrap
    assert one["mag"].shape == (C, T, F) and one["est"].shape == one["fmag"].shape == one["fphase"].shape == (C, S, T, F)
    assert one["pcm"].shape == (C, S, L)
    # 1. what the filter does not touch: the bits of the stream without it
    for key in ("tiles", "mag", "phase", "est"):
        assert np.array_equal(one[key], off[key]), key
    assert not np.array_equal(one["pcm"], off["pcm"])
    # 2. the filtered rows: MwfOnline on the concatenated device arrays in one push, bit for bit; the float64 oracle within the bound
    f = runtime.MwfOnline(ctx, F, S, MWF["niter"], forget=MWF["forget"], loading=MWF["loading"], eps=MWF["eps"])
    om, op = f.push(*(ctx.to_device(one[k], np.float32) for k in ("mag", "phase", "est")))
    assert f.frames == T
    assert np.array_equal(ctx.to_host(om), one["fmag"]) and np.array_equal(ctx.to_host(op), one["fphase"])
    f.close()
    args = (one["mag"], one["phase"], one["est"], MWF["niter"], MWF["forget"], MWF["loading"], MWF["eps"])
    y64, _ = mwf_online_ref.mwf_online_em(*args)
    y32, _ = mwf_online_ref.mwf_online_em(*args, precision="c64")
    peak = float(np.abs(mwf_ref.mixture(one["mag"], one["phase"])).max())
    c64 = 4.0 * float(np.abs(y32 - y64).max()) / peak
    bound = c64 if c64 < CEILING else CEILING
    e_mwf = float(np.abs(mwf_ref.polar(one["fmag"], one["fphase"]) - y64).max()) / peak
    assert np.isfinite(one["fmag"]).all() and np.isfinite(one["fphase"]).all()
    # 3. samples at the device's own filtered magnitudes and phases, per (channel, source)
    e_pcm = 0.0
    for c in range(C):
        for s in range(S):
            want = stft_np.compute_inverse(one["fmag"][c, s].astype(np.float64), one["fphase"][c, s].astype(np.float64), N, h, win)[:L]
            e_pcm = max(e_pcm, float(np.abs(one["pcm"][c, s] - want).max()))
    print("%s %s S=%d: max |y_gpu - y_f64| / max |X| = %.3g (bound %.3g), pcm %.3g" % (stream_ref.shape_id(shape), kind, S, e_mwf,
                                                                                     bound, e_pcm))
    assert e_mwf <= bound
    assert e_pcm <= stft_ref.BOUND_INV
    assert np.isfinite(one["pcm"]).all() and all(one["pcm"][c].any() for c in range(C))
    # 4. however the signal is cut, and whatever the length of the rings: the same bits
    runs = {}
    for part in ("hop", "empty_last"):
        small.reset()
        runs[part] = _drive(small, audio_t, stream_ref.partition(part, L, h, seed=L), seed, counts)
        for key in KEYS + ("tiles",):
            assert np.array_equal(one[key], runs[part][key]), (part, key)
    # 5. reset, the same pushes: the same bits; the stream's memory has not moved
    for stream, part, want in ((big, "one", one), (small, "empty_last", runs["empty_last"])):
        stream.reset()
        again = _drive(stream, audio_t, stream_ref.partition(part, L, h, seed=L), seed, counts)
        for key in KEYS:
            assert np.array_equal(again[key], want[key]), (part, key)
    assert big.bytes == nbytes
    for s in (big, small, plain):
        s.close()


def test_set_mwf_refusals():
    import score_stream_ref as ssr
    ctx = runtime.default_context()
    lib = ctx._lib
    plan = runtime.StftPlan(ctx, 64, 16, np.hanning(64))
    good = (2, 1.0, 1e-3, 1e-10)
    mono = runtime.Stream(plan, 2, 8, 5, TILER_SCRIPT, EPS_A, 0.3, max_push=64)
    score = runtime.ScoreStream(plan, 2, ssr.synth_table(2, 20, 33, nharm=4, boundary=6, seed=0), 8, 5, TILER_LIBRARY, EPS_A, 0.3,
                                max_push=64)
    for s in (mono, score):
        nbytes = s.bytes
        assert lib.dcs_stream_set_mwf(s._h, *good) == _lib.DCS_EINVAL
        assert lib.dcs_stream_mwf_last(s._h, None, None, 0, 0, 33) == _lib.DCS_EINVAL
        assert s.bytes == nbytes
    assert lib.dcs_stream_set_mwf(None, *good) == _lib.DCS_EINVAL and lib.dcs_stream_mwf_last(None, None, None, 0, 0, 33) == _lib.DCS_EINVAL
    for C in (1, 3):
        for s in (runtime.ChannelStream(plan, 2, C, 8, 5, TILER_SCRIPT, EPS_A, 0.3, max_push=64),
                  runtime.StereoStream(plan, 2, C, 8, 5, TILER_LIBRARY, 0.3, max_push=64)):
            with pytest.raises(ValueError):
                s.set_mwf(2)
            s.close()
    for s in (runtime.ChannelStream(plan, 2, 2, 8, 5, TILER_SCRIPT, EPS_A, 0.3, max_push=64),
              runtime.StereoStream(plan, 2, 2, 8, 5, TILER_LIBRARY, 0.3, max_push=64)):
        nbytes = s.bytes
        rows = 3 if isinstance(s, runtime.ChannelStream) else 2
        with pytest.raises(ValueError):
            s.last_mwf()                                                  # the filter is off
        # every value dcs_mwf_online_create refuses
        for bad in ((-1, 1.0, 1e-3, 1e-10), (101, 1.0, 1e-3, 1e-10), (2, 0.0, 1e-3, 1e-10), (2, 1.5, 1e-3, 1e-10),
                    (2, float("nan"), 1e-3, 1e-10), (2, 1.0, -1e-3, 1e-10), (2, 1.0, float("inf"), 1e-10),
                    (2, 1.0, float("nan"), 1e-10), (2, 1.0, 1e-3, 0.0), (2, 1.0, 1e-3, -1e-10), (2, 1.0, 1e-3, 1e-320)):
            assert lib.dcs_stream_set_mwf(s._h, *bad) == _lib.DCS_EINVAL, bad
            assert s.bytes == nbytes
        s.set_mwf(2)
        armed = s.bytes
        assert armed > nbytes
        assert lib.dcs_stream_set_mwf(s._h, 2, 2.0, 1e-3, 1e-10) == _lib.DCS_EINVAL and s.bytes == armed     # refused: still armed
        s.push(ctx.to_device(np.zeros((rows, 40)), np.float32))
        with pytest.raises(ValueError):
            s.set_mwf(2)                                                  # the stream has samples
        s.pull(None)
        with pytest.raises(ValueError):
            s.set_mwf(0)
        s.reset()
        s.set_mwf(1, forget=0.9)                                          # after a reset
        s.set_mwf(0)
        assert s.bytes == nbytes
        s.close()
    mono.close()
    score.close()


# ------------------------------------------------------------------------------------------------ end to end
N, HOP, F, TC, OV = 1024, 512, 513, 30, 25
BLOCK = (TC - OV) * HOP
_RUN = {}


def _separator(arch):
    if arch not in _RUN:
        kw = dict(tiler="library") if arch == "dsd_ild" else {}
        _RUN[arch] = dcs.Separator(arch, synth_params(arch, TC, F, seed=7), 0.3, TC, OV, 32, F, N, HOP, np.hanning, **kw)
    return _RUN[arch]


@pytest.mark.parametrize("arch", ("dsd", "dsd_ild"))
def test_separator_equals_the_manual_composition(arch):
    """``Separator.stream_channels(mwf_iters=2)`` / ``stream_stereo(mwf_iters=2)``: push -> network -> pull on a stream with
    ``set_mwf``, bit for bit; the filter changes the stems; the same stream without it returns what it returned before"""
    sep = _separator(arch)
    ctx, S = sep.ctx, sep.net.S
    audio = 0.5 * synth_audio(44100 + 21, seed=12, channels=2)                         # [L, 2]
    L = audio.shape[0]
    starts = list(range(0, L, BLOCK))
    if arch == "dsd":
        a = ctx.to_device(np.stack([audio[:, 0], audio[:, 1], (audio[:, 0] + audio[:, 1]) / 2]), np.float32)
        eng = runtime.ChannelStream(sep.plan, S, 2, TC, OV, sep.tiler, EPS_A, 0.3, max_push=BLOCK)
        make = sep.stream_channels
    else:
        a = ctx.to_device(np.ascontiguousarray(audio.T), np.float32)
        eng = runtime.StereoStream(sep.plan, S, 2, TC, OV, TILER_LIBRARY, 0.3, max_push=BLOCK)
        make = sep.stream_stereo
    eng.set_mwf(2, forget=0.97, loading=2e-3)
    pcms = []
    for i in range(len(starts) + 1):
        last = i == len(starts)
        tiles = eng.push(None if last else a[:, starts[i]:starts[i] + BLOCK], last=last)
        p = None
        if int(tiles.shape[0]):
            p = (sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:S] if arch == "dsd"
                 else sep.net.forward_stereo_tiles(tiles))
        pcms.append(ctx.to_host(eng.pull(p)))
    eng.close()
    st = make(max_block=BLOCK, mwf_iters=2, mwf_forget=0.97, mwf_loading=2e-3)
    got = [st.push(audio[s:s + BLOCK]) for s in starts] + [st.finish()]
    assert len(got) == len(pcms)
    for x, y in zip(got, pcms):
        assert x.dtype == np.float64 and np.array_equal(x, y.astype(np.float64).transpose(2, 1, 0))
    got = np.concatenate(got, axis=0)
    assert got.shape == (L, S, 2) and np.isfinite(got).all() and got.any()
    off, zero = make(max_block=BLOCK), make(max_block=BLOCK, mwf_iters=0)
    plain = np.concatenate([off.push(audio[s:s + BLOCK]) for s in starts] + [off.finish()], axis=0)
    same = np.concatenate([zero.push(audio[s:s + BLOCK]) for s in starts] + [zero.finish()], axis=0)
    assert np.array_equal(plain, same) and not np.array_equal(plain, got)
    assert st.device_bytes > off.device_bytes == zero.device_bytes
    with pytest.raises(ValueError):
        make(max_block=BLOCK, mwf_iters=-1)
    with pytest.raises(ValueError):
        make(max_block=BLOCK, mwf_iters=2, mwf_forget=0.0).device_bytes


def _script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_command_line(tmp_path, capsys):
    import scipy.io.wavfile
    from deepconvsep_amd.separation import output_paths, read_wav, save_model, write_wav
    sep, script = _separator("dsd"), _script()
    model, wav, out = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "stems")
    save_model(model, synth_params("dsd", TC, F, seed=7))
    write_wav(wav, 0.5 * synth_audio(44100, seed=5, channels=2), 44100)
    script.main(["-a", "dsd", "-i", wav, "-o", out, "-m", model, "--block", "3000", "--stereo", "--mwf", "1"])
    _, audio = read_wav(wav)
    cs = sep.stream_channels(max_block=3000, mwf_iters=1)
    want = np.concatenate([cs.push(audio[i:i + 3000]) for i in range(0, audio.shape[0], 3000)] + [cs.finish()], axis=0)
    for i, path in enumerate(output_paths("dsd", wav, out)):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (audio.shape[0], 2)
        assert np.array_equal(got, (want[:, i] * 32767).astype(np.int16)), path
    # --mwf without --stereo: the usage error of the whole-file scripts
    capsys.readouterr()
    with pytest.raises(SystemExit) as exc:
        script.main(["-a", "dsd", "-i", wav, "-o", out, "-m", model, "--mwf", "1"])
    assert exc.value.code == 2
    assert "usage:" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ guard harness
_CHILD = r'''
import hashlib, json, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd.synth import synth_audio, synth_params
audio = 0.5 * synth_audio(44100 + 33, seed=21, channels=2)
res = {}
for arch in ("dsd", "dsd_ild"):
    kw = dict(tiler="library") if arch == "dsd_ild" else {}
    sep = dcs.Separator(arch, synth_params(arch, 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, **kw)
    make = sep.stream_stereo if arch == "dsd_ild" else sep.stream_channels
    def run(st):
        return [st.push(audio[i:i + 4000]) for i in range(0, audio.shape[0], 4000)] + [st.finish()]
    run(make(max_block=4000, mwf_iters=2))          # the network and the context make their own blocks on first need
    st = make(max_block=4000, mwf_iters=2)
    nbytes = st.device_bytes
    blocks0 = sep.ctx.check_guards()
    pcm = np.concatenate(run(st), axis=0)
    blocks1 = sep.ctx.check_guards()                # raises when a red zone was written
    st.reset()
    again = np.concatenate(run(st), axis=0)
    res[arch] = {"sha256": hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest(), "finite": bool(np.isfinite(pcm).all()),
                 "shape": list(pcm.shape), "any": bool(pcm.any()), "blocks_after_create": blocks0, "blocks_after_last_pull": blocks1,
                 "bytes_before": nbytes, "bytes_after": st.device_bytes, "same_after_reset": bool(np.array_equal(pcm, again))}
json.dump(res, open(OUT, "w"))
'''


def test_guard_harness(tmp_path):
    """both filtered streams under DCS_WS_GUARD with both poison bytes (the manner of tests/test_gpu_stream_channels.py): no red
    zone written, every output finite -- filter state or a filtered row read before it was written would be a NaN under 0xFF --,
    the two runs bit-identical, and the streams neither allocate nor grow after their creation"""
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
        for arch in ("dsd", "dsd_ild"):
            a = r[arch]
            assert a["finite"] and a["any"] and a["shape"] == [44100 + 33, 4, 2] and a["same_after_reset"]
            assert a["blocks_after_create"] == a["blocks_after_last_pull"] >= 12 and a["bytes_before"] == a["bytes_after"] > 0
    for arch in ("dsd", "dsd_ild"):
        assert res[0][arch]["sha256"] == res[1][arch]["sha256"]
