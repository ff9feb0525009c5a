"""``dcs_resample_f32`` on the MI355X against the float64 restatement tests/resample_ref.py, the rule that one output's sum has
one order whatever the call looks like, and the separators, ``train_auto`` and ``deepconvsep_amd.resample`` on top of it.

The elementwise bound, for output m with K taps, x the float32-rounded input and h the float64 taps:
    |y_gpu[m] - y_ref[m]| <= (K + 2) 2^-24 sum_n |x[n]| |h[m down - n up]|
-- a float32 dot product of length K in any order, plus one rounding each for storing the tap and the result."""
import ctypes
import os

import numpy as np
import pytest

import resample_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)
# ratio up/down -> (fi, fo, design options, lengths, clip counts)
LONG = (1, 2, 5, 73, 1024, 3001)
SHORT = (1, 5, 3001)
CASES = {
    "147/160": (48000, 44100, {}, LONG, (1, 3)),
    "160/147": (44100, 48000, {}, LONG, (1, 3)),
    "2/1": (22050, 44100, {}, LONG, (1, 3)),
    "1/2": (44100, 22050, {}, LONG, (1, 3)),
    "441/320": (32000, 44100, {}, SHORT, (1,)),
    "147/320": (96000, 44100, {}, SHORT, (1,)),
    "3/2 Z=2": (2, 3, dict(zero_crossings=2), SHORT, (1,)),
}


@pytest.fixture(scope="module")
def ctx():
    from deepconvsep_amd.runtime import default_context
    return default_context()


_signals, _refs = {}, {}


def signal(L, k):
    """clip k of length L, float32, seeded; never changed"""
    if (L, k) not in _signals:
        x = np.random.RandomState(1000 * k + L).uniform(-1.0, 1.0, L).astype(np.float32)
        x.setflags(write=False)
        _signals[(L, k)] = x
    return _signals[(L, k)]


def reference(name, L, k):
    """(y, K, mass) of clip k of length L in float64, computed once per case"""
    key = (name, L, k)
    if key not in _refs:
        fi, fo, opts, _, _ = CASES[name]
        up, down = ref.lowest_terms(fi, fo)
        h, H = ref.taps(up, down, **opts)
        _refs[key] = ref.resample(signal(L, k).astype(np.float64), up, down, h, H, want_bound=True)
    return _refs[key]


def raw_call(ctx, rs, clips, in_stride=None, out_stride=None, tail=0):
    """dcs_resample_f32 on clips [n][L] laid out with the given strides: NaN between the inputs, a sentinel between and
    behind the outputs.  Returns (rc, outputs [n, M], the whole output buffer, mask of the samples that belong to outputs)."""
    import torch
    n, L = len(clips), (len(clips[0]) if len(clips) else 0)
    M = rs.out_length(L)
    in_stride = L if in_stride is None else in_stride
    out_stride = M if out_stride is None else out_stride
    src = np.full(max(1, n * in_stride), np.nan, dtype=np.float32)
    for k, c in enumerate(clips):
        src[k * in_stride:k * in_stride + L] = c
    dst = np.full(max(1, n * out_stride + tail), SENTINEL, dtype=np.float32)
    with ctx.stream_scope():
        src_d, dst_d = torch.from_numpy(src).to(ctx.device), torch.from_numpy(dst).to(ctx.device)
        rc = ctx._lib.dcs_resample_f32(rs._h, ctypes.c_void_p(src_d.data_ptr()), L, n, in_stride,
                                       ctypes.c_void_p(dst_d.data_ptr()), out_stride)
        got = ctx.to_host(dst_d)
    mask = np.zeros(got.shape, dtype=bool)
    for k in range(n):
        mask[k * out_stride:k * out_stride + M] = True
    outs = np.stack([got[k * out_stride:k * out_stride + M] for k in range(n)]) if n else np.zeros((0, M), np.float32)
    return rc, outs, got, mask


@pytest.mark.parametrize("name", list(CASES))
def test_every_sample_within_the_float32_bound(ctx, name):
    fi, fo, opts, lengths, clip_counts = CASES[name]
    rs = ctx.resampler(fi, fo, **opts)
    assert (rs.up, rs.down) == ref.lowest_terms(fi, fo)
    for L in lengths:
        for n in clip_counts:
            clips = [signal(L, k) for k in range(n)]
            M = ref.length(L, rs.up, rs.down)
            if n == 1:
                rc, outs, got, mask = raw_call(ctx, rs, clips, tail=64)
            else:       # strides larger than the lengths: NaN in the input gaps, the sentinel in the output gaps and the tail
                rc, outs, got, mask = raw_call(ctx, rs, clips, in_stride=L + 37, out_stride=M + 29, tail=64)
            assert rc == 0 and outs.shape == (n, M)
            assert not np.isnan(got).any(), (name, L, n)
            assert (got[~mask] == SENTINEL).all(), (name, L, n)
            worst = 0.0
            for k in range(n):
                y, K, mass = reference(name, L, k)
                bound = (K + 2) * 2.0 ** -24 * mass
                err = np.abs(outs[k].astype(np.float64) - y)
                worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                assert (err <= bound).all(), (name, L, n, k, int(np.argmax(err - bound)), float(np.max(err - bound)))
            print("%s L %d clips %d: largest error / bound = %.3f" % (name, L, n, worst))


def test_small_case_by_hand(ctx):
    """3/2 with two zero crossings, x = one unit sample at n = 2: output m is h[2 m - 6] itself (one product, x = 1)."""
    rs = ctx.resampler(2, 3, zero_crossings=2)
    h, H = ref.taps(3, 2, zero_crossings=2)
    x = np.zeros(9, dtype=np.float32)
    x[2] = 1.0
    _, outs, _, _ = raw_call(ctx, rs, [x])
    want = np.array([h[2 * m - 6 + H] if abs(2 * m - 6) <= H else 0.0 for m in range(14)])
    assert outs.shape == (1, 14) and np.array_equal(outs[0], want.astype(np.float32))


@pytest.mark.parametrize("name", ["147/160", "160/147", "1/2"])
def test_order_rule_batched_equals_single(ctx, name):
    fi, fo, opts, _, _ = CASES[name]
    rs = ctx.resampler(fi, fo, **opts)
    clips = [signal(3001, k) for k in range(3)]
    M = rs.out_length(3001)
    _, batched, _, _ = raw_call(ctx, rs, clips, in_stride=3001 + 37, out_stride=M + 29)
    for k in range(3):
        _, single, _, _ = raw_call(ctx, rs, [clips[k]])
        assert np.array_equal(batched[k], single[0]), (name, k)


@pytest.mark.parametrize("name", ["147/160", "160/147", "2/1", "147/320"])
def test_order_rule_prefix(ctx, name):
    """Output m of a 3001-sample clip and of its first 1500 samples agree bit for bit wherever the window of m ends inside
    the prefix (that includes the outputs whose window starts before sample 0)."""
    fi, fo, opts, _, _ = CASES[name]
    rs = ctx.resampler(fi, fo, **opts)
    x = signal(3001, 0)
    _, whole, _, _ = raw_call(ctx, rs, [x])
    _, part, _, _ = raw_call(ctx, rs, [x[:1500]])
    m = np.arange(part.shape[1])
    inside = (m * rs.down + rs.half) // rs.up <= 1499
    assert inside.sum() > 100 and not inside.all()
    assert np.array_equal(whole[0][:part.shape[1]][inside], part[0][inside])


@pytest.mark.parametrize("name", ["160/147", "441/320"])
def test_table_placements_agree(ctx, name, monkeypatch):
    """The table read from global memory and the table copied into LDS run the same chain per output: the same bits."""
    from deepconvsep_amd.resample import Resampler
    fi, fo, opts, _, _ = CASES[name]
    x = [signal(3001, k) for k in range(2)]
    outs = {}
    for where in ("lds", "l2"):
        monkeypatch.setenv("DCS_RESAMPLE_TABLE", where)
        rs = Resampler(ctx, fi, fo, **opts)
        rc, outs[where], _, _ = raw_call(ctx, rs, x, in_stride=3100, out_stride=rs.out_length(3001) + 11)
        assert rc == 0
        rs.close()
    monkeypatch.setenv("DCS_RESAMPLE_TABLE", "registers")
    with pytest.raises(ValueError):
        Resampler(ctx, fi, fo, **opts)
    assert np.array_equal(outs["lds"], outs["l2"])
    y, K, mass = reference(name, 3001, 1)
    assert (np.abs(outs["l2"][1] - y) <= (K + 2) * 2.0 ** -24 * mass).all()


def test_no_ops_and_argument_checks(ctx):
    import torch
    from deepconvsep_amd import _lib
    rs = ctx.resampler(48000, 44100)
    buf = torch.full((64,), float(SENTINEL), dtype=torch.float32, device=ctx.device)
    src = torch.zeros((64,), dtype=torch.float32, device=ctx.device)
    call = ctx._lib.dcs_resample_f32
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert call(rs._h, p(src), 0, 3, 8, p(buf), 8) == _lib.DCS_OK           # n_in = 0
    assert call(rs._h, p(src), 8, 0, 8, p(buf), 8) == _lib.DCS_OK           # n_clips = 0
    assert call(rs._h, None, 0, 0, 0, None, 0) == _lib.DCS_OK
    assert call(rs._h, p(src), -1, 1, 8, p(buf), 8) == _lib.DCS_EINVAL
    assert call(rs._h, p(src), 8, 2, 7, p(buf), 8) == _lib.DCS_EINVAL        # input stride below the length
    assert call(rs._h, p(src), 8, 2, 8, p(buf), 7) == _lib.DCS_EINVAL        # output stride below ceil(8 * 147 / 160) = 8
    assert call(rs._h, None, 8, 1, 8, p(buf), 8) == _lib.DCS_EINVAL
    assert (ctx.to_host(buf) == SENTINEL).all()
    assert tuple(rs(src[:0]).shape) == (0,) and tuple(rs(src[:0].reshape(2, 0)).shape) == (2, 0)
    # what the plan cannot hold
    h = ctypes.c_void_p()
    taps = np.zeros(2 * 400000 + 1)
    rc = ctx._lib.dcs_resample_plan(ctx._h, 3, 2, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 400000, ctypes.byref(h))
    assert rc == _lib.DCS_EUNSUPPORTED and not h.value                      # 3 x 266 668 float32 > 1 MiB


def test_python_surface(ctx):
    import deepconvsep_amd as dcs
    x = signal(3001, 0).astype(np.float64)
    y = dcs.resample(x, 48000, 44100)
    assert y.shape == (ref.length(3001, 147, 160),) and y.dtype == np.float64
    X = np.stack([signal(3001, k) for k in range(3)]).astype(np.float64)
    Y = dcs.resample(X, 48000, 44100, ctx=ctx)
    assert Y.shape == (3, y.size) and Y.dtype == np.float64 and np.array_equal(Y[0], y)
    ref_y, K, mass = reference("147/160", 3001, 2)
    assert (np.abs(Y[2] - ref_y) <= (K + 2) * 2.0 ** -24 * mass).all()
    same = dcs.resample(x, 44100, 44100)
    assert same is not x and same.dtype == np.float64 and np.array_equal(same, x)
    assert not np.shares_memory(same, x)
    assert ctx.resampler(48000, 44100) is ctx.resampler(48000, 44100)                          # one plan per rate pair
    assert ctx.resampler(48000, 44100) is not ctx.resampler(48000, 44100, zero_crossings=16)
    assert isinstance(ctx.resampler(48000, 44100), dcs.Resampler)
    with pytest.raises(ValueError):
        dcs.resample(np.zeros((2, 2, 2)), 48000, 44100)


@pytest.fixture(scope="module")
def dsd_separator(ctx):
    import deepconvsep_amd as dcs
    return dcs.Separator("dsd", dcs.glorot_init("dsd"), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, ctx=ctx)


def clip_48k():
    from deepconvsep_amd.synth import synth_audio
    return np.asarray(synth_audio(int(0.6 * 48000), seed=3), dtype=np.float64)


def test_separator_converts_on_the_device(ctx, dsd_separator):
    """The device chain and the same kernels composed through the host (every hop round-trips float32 values exactly)."""
    import deepconvsep_amd as dcs
    sep, x = dsd_separator, clip_48k()
    got = sep.separate(x, sample_rate=48000)
    assert got.shape == (4, len(x)) and got.dtype == np.float64 and np.isfinite(got).all()
    want = dcs.resample(sep.separate(dcs.resample(x, 48000, 44100, ctx=ctx)), 44100, 48000, ctx=ctx)[:, :len(x)]
    assert np.array_equal(got, want)
    assert np.abs(got).max() > 1e-4
    x44 = x[:20000]
    assert np.array_equal(sep.separate(x44, sample_rate=44100), sep.separate(x44))


def test_stereo_separator_converts_on_the_device(ctx):
    import deepconvsep_amd as dcs
    from deepconvsep_amd.synth import synth_audio, synth_params
    sep = dcs.Separator("dsd_ild", synth_params("dsd_ild", 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning,
                        tiler='library', ctx=ctx)
    x = np.asarray(synth_audio(int(0.6 * 22050), seed=5, channels=2), dtype=np.float64)            # [L, 2]
    L = x.shape[0]
    got = sep.separate_stereo(x, mwf_iters=0, sample_rate=22050)
    assert got.shape == (L, sep.net.S, 2)
    x44 = dcs.resample(x.T, 22050, 44100, ctx=ctx).T                                               # [L', 2]
    mid = sep.separate_stereo(x44, mwf_iters=0)                                                    # [L', S, 2]
    back = dcs.resample(mid.transpose(2, 1, 0).reshape(2 * sep.net.S, -1), 44100, 22050, ctx=ctx)[:, :L]
    assert np.array_equal(got, back.reshape(2, sep.net.S, L).transpose(2, 1, 0))
    assert np.array_equal(sep.separate_stereo(x44, sample_rate=44100), mid)


def test_train_auto_writes_at_the_files_own_rate(ctx, dsd_separator, tmp_path, capsys):
    import scipy.io.wavfile
    import deepconvsep_amd as dcs
    from deepconvsep_amd.separation import read_wav, write_wav
    x = clip_48k()
    src = str(tmp_path / "mix.wav")
    scipy.io.wavfile.write(src, 48000, (x * 32767).astype(np.int16))
    params = dcs.glorot_init("dsd")
    names = ["bass.wav", "drums.wav", "other.wav", "vocals.wav"]

    off = tmp_path / "off"
    off.mkdir()
    dcs.train_auto("dsd", src, str(off), params, 0.3, 30, 25, 32, 513)                 # as before: refused, nothing written
    assert "Sample rate is not 44100" in capsys.readouterr().out
    assert os.listdir(str(off)) == []

    on = tmp_path / "on"
    on.mkdir()
    dcs.train_auto("dsd", src, str(on), params, 0.3, 30, 25, 32, 513, resample=True)
    assert "Sample rate is not 44100" not in capsys.readouterr().out
    assert sorted(os.listdir(str(on))) == sorted(names)
    rate, audio = read_wav(src)
    pcm = dsd_separator.separate(audio, sample_rate=rate)
    for path, sig in zip(dcs.separation.output_paths("dsd", src, str(on)), pcm):
        want = str(tmp_path / "want.wav")
        write_wav(want, sig, 48000)
        got_rate, got = scipy.io.wavfile.read(path)
        assert got_rate == 48000 and got.shape == (len(x),) and got.dtype == np.int16
        assert np.array_equal(got, scipy.io.wavfile.read(want)[1])
