"""The stereo (ILD) stream without a GPU: its float64 statement (``stereo_stream_ref``) against the reference's own expression
(``oracle.pipeline.separate_stereo``), the row-layout helpers, ``RateStream``'s type check and the command line's argument
handling for ``-a dsd_ild``."""
import importlib.util
import os

import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd.streaming import (ChannelStreamSeparator, RateStream, StereoStreamSeparator, StreamSeparator, stereo_ld,
                                       stereo_rows_from_tiles, stereo_tiles_from_rows)
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import net_ref, pipeline, tiling_np

import chanmask_ref
import stereo_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_whole_file_reproduces_the_reference_expression():
    """``whole_file`` -- masks folded, times the unscaled magnitudes, plus e / scale -- against the stereo trainer's separation
    block, which folds ``mask * (scale * mag) + e``: equal in exact arithmetic, so in float64 they differ by rounding alone.

    Both sides evaluate, per (tile, bin), S - 1 additions, the eps addition and a division, then per fold step two products and
    an addition (m - 1 steps for m covering tiles), a product with the magnitudes and the constant's addition; the stream's side
    divides the constant and the oracle's the spectra by ``scale``.  That is at most S + 3 m + 4 roundings on either side, each
    relative to a partial result bounded by ``mag + c0`` (masks and weights are at most one): spectra within
    ``2 (S + 3 m + 4) 2^-53 (mag + c0)``.  A sample is ``1 / sum w^2`` times a sum over its frames of ``w irfft(.)``, and one bin's
    error ``d`` moves an irfft sample by at most ``2 sqrt(N) d / N`` summed over F bins, ``< 2 sqrt(N) d``; the inverse's own
    rounding is of the same order on values below one.  Samples within ``2 sqrt(N) max(bound) max_q(sum w / sum w^2)`` over the
    frames that cover sample q, plus ``64 * 2^-53``."""
    N, h, tc, ov, scale, S, C = 64, 16, 8, 5, 0.3, 4, 2
    F = N // 2 + 1
    L = 350
    params = synth_params('dsd_ild', tc, F, seed=5)
    audio = 0.5 * synth_audio(L, seed=9, channels=2)
    want_pcm, want_spec, mag32, phs = pipeline.separate_stereo(params, audio, scale, tc, ov, 32, N, h, np.hanning,
                                                               return_spectra=True)          # [L, S, 2], [S, C, T, F], scaled
    T = mag32.shape[1]
    batches, n = tiling_np.generate_overlapadd(mag32, F, tc, ov, 32, tiler=tiling_np.LIBRARY)
    assert n >= 3 and (n - 1) * (tc - ov) + tc > T                       # a zero-padded last tile
    tiles = batches.reshape(-1, C, tc, F)[:n]
    p = net_ref.forward('dsd_ild', params, tiles, inverse='explicit').numpy()                # [n, S C, tc, F] float64
    p = stereo_stream_ref.from_lasagne(p.transpose(1, 0, 2, 3), S, C)
    e = net_ref.EPS_ILD * net_ref.RAND_ILD
    mag = mag32.astype(np.float64) / scale
    ref = stereo_stream_ref.whole_file(audio, N, h, tc, ov, tiling_np.LIBRARY, S, np.hanning(N), scale, p, mag=mag, phase=phs,
                                       c0=e / scale, eps=e)
    assert ref["T"] == T and ref["n_tiles"] == n and ref["est"].shape == (C, S, T, F)
    m = chanmask_ref.covering_tiles(tc, ov)
    lim = 2 * (S + 3 * m + 4) * 2.0 ** -53 * (mag + e / scale)                                # [C, T, F]
    err = np.abs(ref["est"] - want_spec.transpose(1, 0, 2, 3) / scale)
    assert np.all(err <= lim[:, None]), float((err / lim[:, None]).max())
    w, amp = np.hanning(N), 0.0
    for q in range(L):                                                    # the frames n < T that cover sample q
        offs = np.array([q + N // 2 - k * h for k in range(T) if 0 <= q + N // 2 - k * h < N])
        amp = max(amp, float(w[offs].sum() / (w[offs] ** 2).sum()))
    lim_pcm = 2 * np.sqrt(N) * amp * lim.max() + 64 * 2.0 ** -53
    e_pcm = float(np.abs(ref["pcm"].transpose(2, 1, 0) - want_pcm).max())
    assert e_pcm <= lim_pcm, (e_pcm, lim_pcm)
    assert np.abs(want_pcm).max() > 1e-3                                  # something was separated


def test_masks_zeros_and_the_bound_rule():
    rs = np.random.RandomState(3)
    S, C, n, tc, F = 4, 2, 3, 8, 33
    p = stereo_stream_ref.from_lasagne(stereo_stream_ref.make_p(rs, S, C, n, tc, F), S, C)
    assert p.shape == (S, C, n, tc, F) and p.dtype == np.float32
    assert not p[..., 3].any() and not p[1:, ..., 5].any() and (p[0, ..., 5] > 0).all()
    zeros = float((p == 0).mean())
    assert 0.3 < zeros < 0.5
    m = stereo_stream_ref.tile_masks_ild(p)
    assert m.shape == p.shape and (m >= 0).all() and (m.sum(axis=0) <= 1).all()
    assert not m[..., 3].any()                                            # every source zero: masks 0, not NaN
    # per channel: channel 1's outputs do not move channel 0's masks
    q = p.copy()
    q[:, 1] *= 7
    assert np.array_equal(stereo_stream_ref.tile_masks_ild(q)[:, 0], m[:, 0])
    # tile k of tile_p is a function of (k, seed) alone, in the Lasagne channel order s C + c
    a = stereo_stream_ref.tile_p(5, S, C, tc, F, seed=2)
    assert a.shape == (S * C, tc, F) and np.array_equal(a, stereo_stream_ref.tile_p(5, S, C, tc, F, seed=2))
    assert not np.array_equal(a, stereo_stream_ref.tile_p(6, S, C, tc, F, seed=2))
    assert np.array_equal(stereo_stream_ref.from_lasagne(a[:, None], S, C)[2, 1, 0], a[2 * C + 1])
    # the bound: chanmask_ref's count plus one, on mag + c0
    c0 = stereo_stream_ref.c0_f32(0.3)
    assert c0 == float(np.float32(np.float32(1e-13) / np.float32(0.3)))
    assert stereo_stream_ref.bound(4, 30, 25, 2.0, c0) == (4 + 2 * 6 + 5) * 2.0 ** -23 * (2.0 + c0)
    assert np.isclose(stereo_stream_ref.bound(4, 30, 25, 2.0), chanmask_ref.bound(4, 30, 25, 2.0) * 21 / 20)
    # rows past the last tile are zeros without c0
    audio = 0.5 * synth_audio(16 * 16 + 3, seed=1, channels=2)
    T = 16 + 1 + 2
    n_s = len(tiling_np.tile_starts(T, 8, 5, tiling_np.SCRIPT))
    covered = (n_s - 1) * 3 + 8
    assert covered < T
    ps = np.stack([stereo_stream_ref.tile_p(k, 2, 2, 8, 33) for k in range(n_s)], axis=1)
    ref = stereo_stream_ref.whole_file(audio, 64, 16, 8, 5, tiling_np.SCRIPT, 2, np.hanning(64), 0.3,
                                       stereo_stream_ref.from_lasagne(ps, 2, 2))
    assert ref["covered"] == covered and not ref["est"][:, :, covered:].any() and (ref["est"][:, :, :covered] >= c0).all()


def test_row_layout_helpers():
    assert [stereo_ld(F) for F in (33, 36, 513, 2049)] == [36, 36, 516, 2052]
    rs = np.random.RandomState(0)
    tiles = rs.rand(3, 2, 8, 33).astype(np.float32)
    rows = stereo_rows_from_tiles(tiles)
    assert rows.shape == (3, 8, 2, 36) and rows.dtype == np.float32 and not rows[..., 33:].any()
    for k, c, j in ((0, 0, 0), (2, 1, 7), (1, 1, 3)):
        assert np.array_equal(rows[k, j, c, :33], tiles[k, c, j])
    assert np.array_equal(stereo_tiles_from_rows(rows, 33), tiles)
    out = rs.rand(4, 3, 8, 2, 36).astype(np.float32)                      # [S, n, tc, C, ld] as forward_stereo_tiles returns it
    back = stereo_tiles_from_rows(out, 33)
    assert back.shape == (4, 3, 2, 8, 33) and np.array_equal(back[3, 1, 1, 5], out[3, 1, 5, 1, :33])
    with pytest.raises(ValueError):
        stereo_tiles_from_rows(out, 37)


class _Net(object):
    def __init__(self, C):
        self.S = 4
        self.arch = type("A", (), {"C": C, "eps_mode": 0})()


class _Separator(object):
    """what the stream separators read of a Separator before they touch the device"""
    frameSize, hopSize, tc, overlap, tiler, scale_factor, tie_mode, ctx, plan = 1024, 512, 30, 25, 0, 0.3, 0, None, None

    def __init__(self, arch_name, C):
        self.arch_name, self.net = arch_name, _Net(C)

    _require_mono_graph = dcs.Separator._require_mono_graph
    stream_stereo = dcs.Separator.stream_stereo


def test_refusals_and_rate_stream_types_that_need_no_device():
    with pytest.raises(ValueError, match="stereo \\(ILD\\)"):
        StereoStreamSeparator(_Separator("dsd", 1))
    with pytest.raises(ValueError, match="stereo \\(ILD\\)"):
        _Separator("bach10_si", 4).stream_stereo()
    with pytest.raises(ValueError):
        StereoStreamSeparator(_Separator("dsd_ild", 2), max_block=0)
    with pytest.raises(ValueError):                                       # the other streams keep refusing the graph
        StreamSeparator(_Separator("dsd_ild", 2))
    with pytest.raises(ValueError, match="single-input-channel"):
        ChannelStreamSeparator(_Separator("dsd_ild", 2))
    ss = _Separator("dsd_ild", 2).stream_stereo(max_block=4096)
    assert isinstance(ss, StereoStreamSeparator) and ss.S == 4 and ss.rows_in == 2 and ss.max_block == 4096
    assert ss.counts.tiler == dcs.arch.TILER_LIBRARY                      # the library tiler whatever the separator's
    assert ss.counts.latency_samples() == 30 * 512 + 1024
    with pytest.raises(ValueError, match="stereo"):
        ss.push(np.zeros(10))
    with pytest.raises(ValueError, match="stereo"):
        ss.push(np.zeros((10, 3)))
    with pytest.raises(IndexError, match="tuple index out of range"):     # an empty signal gives no tile
        ss.finish()
    with pytest.raises(ValueError, match="already"):
        ss.finish()
    with pytest.raises(ValueError, match="ended"):
        ss.push(np.zeros((10, 2)))
    ss.reset()
    rs = RateStream(ss, 48000)
    assert rs.stereo and not rs.passthrough and rs.max_block == 4096 and rs.S == 4
    assert rs.latency_samples() > ss.counts.latency_samples() * 48000 / 44100.0
    with pytest.raises(ValueError, match="stereo"):
        rs.push(np.zeros(10))
    assert RateStream(ss, 44100).passthrough
    for other in (object(), ss.counts, "dsd_ild"):
        with pytest.raises(TypeError):
            RateStream(other, 48000)


def _script():
    spec = importlib.util.spec_from_file_location("separate_stream", os.path.join(ROOT, "examples", "separate_stream.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    return script


def test_command_line_argument_handling(tmp_path):
    """what ``-a dsd_ild`` decides before it touches the device"""
    from deepconvsep_amd.separation import write_wav
    script = _script()
    assert "dsd_ild" in script.ARCHS and script.ILD_DEFAULTS[:2] == (1024, 512) and script.ILD_DEFAULTS[3:] == (25, 513)
    mono, st48 = str(tmp_path / "mono.wav"), str(tmp_path / "st48.wav")
    write_wav(mono, 0.5 * synth_audio(3000, seed=1), 44100)
    write_wav(st48, 0.5 * synth_audio(3000, seed=2, channels=2), 48000)
    base = ["-a", "dsd_ild", "-o", str(tmp_path / "out"), "-m", str(tmp_path / "none.pkl")]
    with pytest.raises(SystemExit, match="two-channel"):                  # a mono file, with and without --stereo
        script.main(base + ["-i", mono])
    with pytest.raises(SystemExit, match="two-channel"):
        script.main(base + ["-i", mono, "--stereo"])
    with pytest.raises(SystemExit, match="Sample rate is not 44100"):     # another rate without --resample
        script.main(base + ["-i", st48])
    with pytest.raises(SystemExit, match="bach10_si only"):
        script.main(base + ["-i", st48, "--trainer-semantics"])
    assert not os.path.exists(str(tmp_path / "out"))
