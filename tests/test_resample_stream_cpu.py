"""CPU checks of the streaming sample-rate conversion and of the stereo / any-rate streams (no GPU): ``ResampleCounts`` against
brute force over the tap ranges of tests/resample_ref.py, the history bound the ring is sized by, the C ABI declared, exported
and bound, and what ``ChannelStreamSeparator`` / ``RateStream`` refuse before they touch a device."""
import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd import _lib
from deepconvsep_amd.resample import ResampleCounts, design
from deepconvsep_amd.streaming import ChannelStreamSeparator, RateStream, StreamSeparator

import resample_ref as ref

NEW_SYMBOLS = ["dcs_stream_create_channels", "dcs_stream_push_channels", "dcs_stream_pull_channels",
               "dcs_resample_stream_create", "dcs_resample_stream_destroy", "dcs_resample_stream_reset",
               "dcs_resample_stream_bytes", "dcs_resample_stream_push"]
ZERO_CROSSINGS = (32, 4)
GRID = list(range(0, 51)) + [2999, 3000, 3001, 4097]


def _brute_emitted(P, up, down, H):
    """outputs whose every tap index, the signal taken as endless, lies below P: they form a prefix, m = 0, 1, .."""
    m = 0
    while (m * down + H) // up < P:                      # the highest n with |m down - n up| <= H
        m += 1
    return m


@pytest.mark.parametrize("Z", ZERO_CROSSINGS)
@pytest.mark.parametrize("pair", ref.PAIRS, ids=lambda p: "%d_%d" % p)
def test_counts_against_brute_force(pair, Z):
    fi, fo = pair
    up, down = ref.RATIOS[pair]
    _, H = ref.taps(up, down, zero_crossings=Z)
    u2, d2, _, H2 = design(fi, fo, zero_crossings=Z)
    assert (u2, d2, H2) == (up, down, H)
    c = ResampleCounts(up, down, H)
    assert c.history() == 2 * H // up + 2 and c.delay_samples() == H / float(up)
    prev, worst = 0, 0
    for P in GRID:
        M = c.emitted(P)
        assert M == _brute_emitted(P, up, down, H), (P, M)
        assert prev <= M <= ref.length(P, up, down)
        prev = M
        assert c.emitted(P, True) == ref.length(P, up, down)
        # the definition, through tap_range on a longer signal: output M - 1 ends below P, output M does not
        if M:
            assert ref.tap_range(M - 1, P + 10 ** 6, up, down, H)[1] < P
        assert ref.tap_range(M, P + 10 ** 6, up, down, H)[1] >= P
        # the oldest input an output not yet emitted can reach, behind P
        if P:
            n_lo = -((H - M * down) // up)                # ceil((M down - H) / up), not clamped at 0
            worst = max(worst, P - max(n_lo, 0))
            assert P - n_lo < c.history(), (P, n_lo)
    assert 0 < worst < c.history()


def test_delays_of_the_common_rates():
    for (fi, fo), want in (((48000, 44100), 36.7), ((44100, 48000), 33.7), ((96000, 44100), 73.3)):
        up, down, _, H = design(fi, fo)
        assert abs(ResampleCounts(up, down, H).delay_samples() - want) < 0.05
    assert ResampleCounts(147, 160, 5390).history() == 75 and ResampleCounts(147, 320, 10779).history() == 148
    with pytest.raises(ValueError):
        ResampleCounts(0, 1, 3)


def test_symbols_are_declared_exported_and_bound():
    names = _lib.header_symbols()
    assert set(NEW_SYMBOLS) <= set(names)
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert getattr(lib, n).argtypes is not None, n
    assert lib.dcs_resample_stream_bytes(None) == -1
    assert lib.dcs_resample_stream_destroy(None) == _lib.DCS_OK
    assert lib.dcs_resample_stream_reset(None) == _lib.DCS_EINVAL
    assert lib.dcs_resample_stream_create(None, 1, 16, None) == _lib.DCS_EINVAL
    assert lib.dcs_resample_stream_push(None, None, 0, 0, 0, None, 0, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_create_channels(None, 4, 2, 30, 25, 0, 0, 0.3, None, 16, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_push_channels(None, None, 0, 0, 0, None, 0, None, None, None, 0, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull_channels(None, None, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0) == _lib.DCS_EINVAL
    for name in ("ChannelStreamSeparator", "RateStream", "ResampleCounts", "StreamResampler"):
        assert name in dcs.__all__ and hasattr(dcs, name), name
    assert hasattr(dcs.Separator, "stream_channels")


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


def test_refusals_that_need_no_device():
    with pytest.raises(ValueError, match="single-input-channel"):
        ChannelStreamSeparator(_Separator("dsd_ild", 2))
    with pytest.raises(ValueError, match="single-input-channel"):
        ChannelStreamSeparator(_Separator("bach10_si", 4))
    with pytest.raises(ValueError):
        ChannelStreamSeparator(_Separator("dsd", 1), max_block=0)
    cs = ChannelStreamSeparator(_Separator("dsd", 1), max_block=4096)
    assert cs.counts.latency_samples() == 30 * 512 + 1024 and cs.S == 4
    with pytest.raises(ValueError, match="stereo"):
        cs.push(np.zeros(10))
    with pytest.raises(IndexError):           # an empty signal gives no tile: what separate_channels raises
        cs.finish()
    with pytest.raises(ValueError, match="already"):
        cs.finish()
    with pytest.raises(ValueError, match="ended"):
        cs.push(np.zeros((10, 2)))

    with pytest.raises(TypeError):
        RateStream(object(), 48000)
    with pytest.raises(ValueError):
        RateStream(StreamSeparator(_Separator("dsd", 1)), 0)
    with pytest.raises(ValueError):
        RateStream(StreamSeparator(_Separator("dsd", 1)), 44100.5)
    inner = StreamSeparator(_Separator("dsd", 1), max_block=4096)
    rs = RateStream(inner, 48000)
    assert not rs.stereo and not rs.passthrough and rs.max_block == 4096 and rs.S == 4
    up, down, _, H = design(48000, 44100)
    u2, d2, _, H2 = design(44100, 48000)
    want = (H + 1) / up + (inner.counts.latency_samples() * u2 + H2 + 1) / d2
    assert rs.latency_samples() == int(np.ceil(want)) > inner.counts.latency_samples() * 48000 / 44100.0
    with pytest.raises(ValueError, match="mono"):
        rs.push(np.zeros((10, 2)))
    rs2 = RateStream(ChannelStreamSeparator(_Separator("dsd", 1)), 48000)
    assert rs2.stereo
    with pytest.raises(ValueError, match="stereo"):
        rs2.push(np.zeros(10))
    same = RateStream(StreamSeparator(_Separator("dsd", 1)), 44100)
    assert same.passthrough and same.latency_samples() == inner.counts.latency_samples()
    with pytest.raises(IndexError):
        same.finish()
    # the pins of the mono stream stay
    with pytest.raises(ValueError, match="44 100"):
        StreamSeparator(_Separator("dsd", 1), sample_rate=48000)
