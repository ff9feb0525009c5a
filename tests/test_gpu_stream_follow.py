"""A followed score stream (``dcs_stream_set_follow``, csrc/stream.hip; include/dcs.h has the contract): the score is at nominal
tempo, a push computes the chroma of its new frames, asks the follower (csrc/follow.hip) where in the score they are and paints
audio frame ``t`` from score frame ``pos[t]``.

The machinery tests drive ``runtime.ScoreStream`` on the end-to-end plan of tests/test_gpu_stream_score.py (frames of 1024 every
512, tiles of 30 frames overlapping by 25) with three seconds of the synthetic piece of tests/align_ref.py, blocks of an odd
size and the synthetic ``p`` of tests/stream_ref.py, no network: the stream is held, bit for bit, to its parts -- ``chroma`` of
its own magnitudes through a standalone ``ScoreFollower``, then ``score_stream_ref.frame_masks`` at the positions.
"""
import os
import sys
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import _lib, align, runtime, score  # noqa: E402
from deepconvsep_amd.arch import EPS_B, TILER_LIBRARY  # noqa: E402
from deepconvsep_amd.streaming import RateStream, StreamCounts, score_frames  # noqa: E402
from deepconvsep_amd.synth import synth_audio, synth_params, synth_score_text  # noqa: E402

import align_ref  # noqa: E402
import score_stream_ref as ssr  # noqa: E402
import stream_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N, HOP, F, TC, OV = 1024, 512, 513, 30, 25
ST = TC - OV
S, SCALE, SEED = 4, 0.3, 3
L = 3 * 44100 + 17
BLOCK = 7001                                             # odd, and no multiple of the hop
FILES = ("bassoon_b.txt", "clarinet_b.txt", "saxophone_b.txt", "violin_b.txt")
NHARM = 6                                                # a narrow table: the masks are checked frame by frame on the host


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """the piece's first three seconds, its score at nominal tempo as a note table in SCORE time and as chroma"""
    from deepconvsep_amd.score import write_score
    scores, audio = align_ref.piece()
    d = str(tmp_path_factory.mktemp("scores"))
    for f, (on, off, names) in zip(FILES, scores):
        write_score(os.path.join(d, f), on, off, names)
    U = score_frames(scores, HOP)
    assert U == align_ref.score_frames(scores)
    notes = score.melody_table(FILES, d, U, 44100, HOP, N, nharmonics=NHARM)
    ctx = runtime.default_context()
    plan = runtime.StftPlan(ctx, N, HOP, np.hanning(N))
    return dict(scores=scores, audio=np.ascontiguousarray(audio[:L]), U=U, notes=notes, ctx=ctx, plan=plan, dir=d,
                S=align.score_chroma(scores, U, HOP, 44100), classes=align.bin_classes(N), counts=StreamCounts(N, HOP, TC, OV, 'library'))


def _follower(s, S_rows=None, max_push=BLOCK, **kw):
    kw.setdefault("window", 64)
    return align.ScoreFollower(s["ctx"], s["S"] if S_rows is None else S_rows, max_frames=s["counts"].max_frames(max_push), **kw)


def _stream(s, notes, normalise='max', mixture='ch0', follow=None, max_push=BLOCK):
    kw = dict(follow=follow, classes=s["classes"]) if follow is not None else {}
    return runtime.ScoreStream(s["plan"], S, notes, TC, OV, TILER_LIBRARY, EPS_B, SCALE, max_push=max_push, normalise=normalise,
                               mixture=mixture, **kw)


def _drive(stream, audio_t, sizes):
    """the signal in blocks of ``sizes`` (the last one ends it) with the synthetic p of stream_ref.tile_p -> host arrays"""
    ctx = stream.ctx
    mags, ests, pcms, tls, poss, at, k = [], [], [], [], [], 0, 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        tiles, mag, _ = stream.push(audio_t[at:at + n] if n else None, last=last, want_frames=True)
        at += n
        if stream.follow is not None:
            pos = stream.positions()
            assert pos.dtype == runtime._torch().int32 and int(pos.shape[0]) == int(mag.shape[0]) == stream.last_frames
            poss.append(ctx.to_host(pos))
        nt = int(tiles.shape[0])
        p = None
        if nt:
            p = ctx.to_device(np.stack([stream_ref.tile_p(k + j, S, TC, F, SEED) for j in range(nt)], axis=1), np.float32)
            k += nt
        pcm, est = stream.pull(p, want_est=True)
        mags.append(ctx.to_host(mag)); ests.append(ctx.to_host(est)); pcms.append(ctx.to_host(pcm)); tls.append(ctx.to_host(tiles))
    out = dict(mag=np.concatenate(mags), est=np.concatenate(ests, axis=1), pcm=np.concatenate(pcms, axis=1), tiles=np.concatenate(tls))
    if poss:
        out["pos"] = np.concatenate(poss)
    return out


def _blocks(total, block=BLOCK):
    return [block] * (total // block) + [total % block]


def _want_tiles(notes, pos, mag, normalise):
    """tiles[k][j][r] = frame_masks(notes, pos[t])[j] * (scale * mag[t]), t = k st + r, zero rows past the signal"""
    T = mag.shape[0]
    masks = {}
    n_tiles = (T - OV - 1) // ST + 1
    want = np.zeros((n_tiles, notes.shape[0], TC, F), dtype=np.float32)
    scaled = np.float32(SCALE) * mag
    for k in range(n_tiles):
        for r in range(min(TC, T - k * ST)):
            t = k * ST + r
            u = int(pos[t])
            if u not in masks:
                masks[u] = np.float32(ssr.frame_masks(notes, u, F, normalise))
            want[k, :, r] = masks[u] * scaled[t][None]
    return want


@pytest.mark.parametrize("mixture", ["ch0", "sum"])
@pytest.mark.parametrize("normalise", ["max", "sum"])
def test_followed_stream_against_its_parts(setup, normalise, mixture):
    s = setup
    ctx = s["ctx"]
    audio_t = ctx.to_device(s["audio"], np.float32)
    follower = _follower(s)
    stream = _stream(s, s["notes"], normalise, mixture, follow=follower)
    nbytes, fbytes = stream.bytes, follower.device_bytes
    run = _drive(stream, audio_t, _blocks(L))
    T = s["counts"].frames(L, True)
    assert run["mag"].shape == (T, F) and run["pos"].shape == (T,) and run["pcm"].shape == (S, L)
    # 1. the positions: a standalone follower fed the chroma of the same frames
    alone = _follower(s)
    want_pos = ctx.to_host(alone.push(align.chroma(ctx, ctx.to_device(run["mag"], np.float32), s["classes"])))
    assert np.array_equal(run["pos"], want_pos)
    assert run["pos"][-1] > 100 and (np.diff(run["pos"]) >= 0).all()        # it did follow: three seconds at about 86 frames a second
    # 2. every tile row, bit for bit
    want = _want_tiles(s["notes"], run["pos"], run["mag"], normalise)
    assert run["tiles"].shape == want.shape and np.array_equal(run["tiles"], want) and run["tiles"].any()
    assert np.isfinite(run["pcm"]).all() and run["pcm"].any()
    # 3. the memory does not depend on the signal's length
    assert stream.bytes == nbytes and follower.device_bytes == fbytes
    if (normalise, mixture) == ('max', 'ch0'):
        # 4. however the signal is cut, and after a reset: the same bits
        for sizes in ([HOP] * (L // HOP) + [L % HOP], _blocks(L, 3001) + [0]):
            stream.reset()
            assert follower.frames == 0
            again = _drive(stream, audio_t, sizes)
            for key in ("mag", "pos", "tiles", "est", "pcm"):
                assert np.array_equal(run[key], again[key]), (len(sizes), key)
    stream.close()
    follower.close()
    alone.close()


def test_constructed_identity_track_equals_the_unfollowed_stream(setup):
    """Score chroma rows made equal to the audio's own chroma rows and K = 1: the diagonal costs 1 - |a|^2, a few 2^-24, every
    other path at least the penalty of one step that is not 1, so pos[t] == t by construction -- and then the stems must equal
    the unarmed stream's bit for bit (the same table, read in audio time)."""
    s = setup
    ctx = s["ctx"]
    audio_t = ctx.to_device(s["audio"], np.float32)
    T = s["counts"].frames(L, True)
    notes = ssr.synth_table(4, T, F, nharm=4, boundary=2 * ST, seed=1)
    plain = _stream(s, notes, 'sum', 'sum')
    nbytes = plain.bytes
    base = _drive(plain, audio_t, _blocks(L))
    own = ctx.to_host(align.chroma(ctx, ctx.to_device(base["mag"], np.float32), s["classes"]))
    follower = _follower(s, S_rows=own, max_step=1)
    armed = _stream(s, notes, 'sum', 'sum', follow=follower)
    run = _drive(armed, audio_t, _blocks(L))
    assert np.array_equal(run["pos"], np.arange(T, dtype=np.int32))
    for key in ("mag", "tiles", "est", "pcm"):
        assert np.array_equal(run[key], base[key]), key
    # an unarmed stream is what it was: its bytes are those of a second stream that was never armed, the armed one's are
    # larger by the chroma rows and positions of one push's frames and the class table
    second = _stream(s, notes, 'sum', 'sum')
    fp = s["counts"].max_frames(BLOCK)
    assert plain.bytes == nbytes == second.bytes
    assert armed.bytes == nbytes + fp * 12 * 4 + fp * 4 + (F + 255) // 256 * 256
    for x in (plain, armed, second):
        x.close()
    follower.close()


def test_refusals(setup):
    s = setup
    ctx, lib = s["ctx"], _lib.load()
    cls = np.ascontiguousarray(s["classes"])
    cp = c_void_p(cls.ctypes.data)
    fp = s["counts"].max_frames(BLOCK)

    def arm(stream, follower, classes=cp, floor=1e-6):
        return lib.dcs_stream_set_follow(stream._h, follower._h if follower is not None else None, classes, floor)
    follower = _follower(s)
    mono = runtime.Stream(s["plan"], S, TC, OV, TILER_LIBRARY, EPS_B, SCALE, max_push=BLOCK)
    assert arm(mono, follower) == _lib.DCS_EINVAL                         # not a score stream
    stream = _stream(s, s["notes"])
    assert arm(stream, None) == _lib.DCS_EINVAL and arm(stream, follower, classes=None) == _lib.DCS_EINVAL
    assert arm(stream, follower, floor=-1.0) == _lib.DCS_EINVAL
    bad = cls.copy()
    bad[5] = 12
    assert arm(stream, follower, classes=c_void_p(bad.ctypes.data)) == _lib.DCS_EINVAL
    small = align.ScoreFollower(ctx, s["S"], window=64, max_frames=fp - 1)
    assert arm(stream, small) == _lib.DCS_EINVAL                          # one push of the stream can complete more frames
    n = c_int64(-1)
    torch = runtime._torch()
    pos = torch.empty((fp,), dtype=torch.int32, device=ctx.device)
    assert lib.dcs_stream_follow_last(stream._h, c_void_p(pos.data_ptr()), fp, byref(n)) == _lib.DCS_EINVAL and n.value == -1
    nbytes = stream.bytes
    used = _follower(s)
    used.push(ctx.to_device(s["S"][:3], np.float32))
    assert arm(stream, used) == _lib.DCS_EINVAL                           # the follower has taken frames
    assert stream.bytes == nbytes                                         # a refused call leaves the stream as it was
    stream.push(ctx.to_device(s["audio"][:4000], np.float32))
    stream.pull(None)
    assert arm(stream, follower) == _lib.DCS_EINVAL                       # the stream has taken samples
    stream.reset()
    assert arm(stream, follower) == _lib.DCS_OK and stream.bytes > nbytes
    assert lib.dcs_stream_follow_last(stream._h, c_void_p(pos.data_ptr()), fp, byref(n)) == _lib.DCS_OK and n.value == 0
    assert lib.dcs_stream_follow_last(stream._h, c_void_p(pos.data_ptr()), fp, None) == _lib.DCS_EINVAL
    # Python
    with pytest.raises(ValueError, match="pitch classes"):
        runtime.ScoreStream(s["plan"], S, s["notes"], TC, OV, follow=follower)
    with pytest.raises(ValueError, match="follows no score"):
        _stream(s, s["notes"]).positions()
    ctx.synchronize()
    for x in (mono, stream):
        x.close()
    for x in (follower, small, used):
        x.close()


@pytest.fixture(scope="module")
def separator():
    return dcs.Separator("bach10_si", synth_params("bach10_si", TC, F, seed=5), 0.3, TC, OV, 32, F, N, HOP, np.hanning,
                         tiler='library')


def test_separator_stream_follows(setup, separator):
    """``Separator.stream_scoreinformed(melody, follow_scores=...)``: the stems of the armed engine driven by hand, the positions
    of a push, the refusals of the constructor; ``RateStream`` keeps wrapping it."""
    s = setup
    sep, ctx = separator, separator.ctx
    audio = s["audio"][:44100 + 21]
    ss = sep.stream_scoreinformed(s["notes"], max_block=BLOCK, follow_scores=s["scores"], window=64)
    nbytes = ss.device_bytes
    outs, pos = [], []
    for b in range(0, audio.size, BLOCK):
        outs.append(ss.push(audio[b:b + BLOCK]))
        pos.append(ss.positions())
    outs.append(ss.finish())
    pos.append(ss.positions())
    got = np.concatenate(outs, axis=1)
    assert got.shape == (sep.net.S, audio.size) and np.isfinite(got).all() and got.any() and ss.device_bytes == nbytes
    pos = np.concatenate(pos)
    assert pos.dtype == np.int32 and pos.shape == (s["counts"].frames(audio.size, True),) and (np.diff(pos) >= 0).all()
    # the engine by hand
    follower = _follower(s)
    eng = _stream(s, s["notes"], follow=follower)
    a = ctx.to_device(audio, np.float32)
    pcms, want_pos = [], []
    starts = list(range(0, audio.size, BLOCK))
    for i in range(len(starts) + 1):
        last = i == len(starts)
        tiles = eng.push(None if last else a[starts[i]:starts[i] + BLOCK], last=last)
        want_pos.append(ctx.to_host(eng.positions()))
        p = sep.net.forward_raw(tiles, sep.tie_mode, channel_major=True)[:sep.net.S] if int(tiles.shape[0]) else None
        pcms.append(ctx.to_host(eng.pull(p)))
    assert np.array_equal(pos, np.concatenate(want_pos))
    assert np.array_equal(got, np.concatenate(pcms, axis=1).astype(np.float64))
    eng.close()
    follower.close()
    # reset starts the score again
    ss.reset()
    assert ss.positions().size == 0                                       # the last signal's positions do not outlive it
    again = np.concatenate([ss.push(audio[b:b + BLOCK]) for b in range(0, audio.size, BLOCK)] + [ss.finish()], axis=1)
    assert np.array_equal(again, got)
    ss.close()                                                            # the stream first, then the follower it reads
    assert ss._engine is None and ss._follow._h is None
    ss.close()
    assert isinstance(RateStream(sep.stream_scoreinformed(s["notes"], max_block=BLOCK, follow_scores=s["scores"]), 48000).inner,
                      dcs.ScoreStreamSeparator)
    with pytest.raises(ValueError, match="instruments"):
        sep.stream_scoreinformed(s["notes"], follow_scores=s["scores"][:3])
    with pytest.raises(ValueError, match="score time"):
        late = s["notes"].copy()
        late[0, 0, 1] = s["U"] + 5
        sep.stream_scoreinformed(late, follow_scores=s["scores"])
    with pytest.raises(TypeError):
        sep.stream_scoreinformed(s["notes"], window=64)
    with pytest.raises(ValueError, match="follows no score"):
        sep.stream_scoreinformed(s["notes"]).positions()


def test_command_line_follows(tmp_path):
    """``separate_stream.py -a bach10_si --follow``: four stems of the input's length, what the separator's followed stream gives
    on the table in score time, truncated to int16"""
    import importlib.util
    import scipy.io.wavfile
    from deepconvsep_amd.score import read_score
    from deepconvsep_amd.separation import SI_SCORE_FILES, SI_SCORE_PARAMS, output_paths, read_wav, save_model, write_wav
    spec = importlib.util.spec_from_file_location("separate_stream_follow", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    params = synth_params("bach10_si", 30, 2049, seed=5)
    model, wav, out = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "stems")
    save_model(model, params)
    write_wav(wav, 0.5 * synth_audio(22050, seed=5), 44100)
    for i, name in enumerate(SI_SCORE_FILES):
        (tmp_path / name).write_text(synth_score_text(60 + i, 1.5, 40 + 5 * i, 64 + 6 * i))
    script.main(["-a", "bach10_si", "-i", wav, "-o", out, "-m", model, "--block", "3001", "--follow", "--follow-window", "128",
                 "--follow-step", "3", "--follow-penalty", "0.125"])
    with pytest.raises(SystemExit):
        script.main(["-a", "dsd", "-i", wav, "-o", out, "-m", model, "--follow"])
    _, mono = read_wav(wav)
    scores = [read_score(str(tmp_path / f)) for f in SI_SCORE_FILES]
    melody = score.melody_table(SI_SCORE_FILES, str(tmp_path), score_frames(scores, 512), 44100, 512, 4096, **SI_SCORE_PARAMS)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, 2049, 4096, 512, dcs.blackmanharris, tiler='library')
    ss = sep.stream_scoreinformed(melody, max_block=3001, follow_scores=scores, window=128, max_step=3, penalty=0.125)
    want = np.concatenate([ss.push(mono[i:i + 3001]) for i in range(0, mono.size, 3001)] + [ss.finish()], axis=1)
    assert ss.positions().size and len(output_paths("bach10_si", wav, out)) == 4
    for i, path in enumerate(output_paths("bach10_si", wav, out)):
        rate, got = scipy.io.wavfile.read(path)
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (mono.size,)
        assert np.array_equal(got, (want[i] * 32767).astype(np.int16)), path
    assert np.abs(want).max() > 1e-3
