"""CPU checks of the streaming separation (no GPU): the float64 statement of the streaming computation (tests/stream_ref.py)
reproduces the whole-file composition however the signal is cut into blocks, ``StreamCounts`` is the oracle's framing at the
end and keeps its promises mid-stream, ``StreamSeparator`` refuses what it cannot do before it touches a device, and the C ABI
is declared, exported and bound."""
import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd import _lib
from deepconvsep_amd.streaming import StreamCounts, StreamSeparator
from oracle import stft_np, tiling_np

import chanmask_ref
import stream_ref

STREAM_SYMBOLS = ["dcs_stream_create", "dcs_stream_destroy", "dcs_stream_reset", "dcs_stream_max_tiles", "dcs_stream_bytes",
                  "dcs_stream_push", "dcs_stream_pull"]
ROUND_OFF = 1e-12

_WHOLE = {}


def _whole(shape, tiler, conv, L):
    key = (shape, tiler, conv, L)
    if key not in _WHOLE:
        N, h, tc, ov, wname = shape
        ref = stream_ref.whole_file(stream_ref.signal(L), N, h, tc, ov, tiler, conv, 2, stream_ref.window(wname, N), scale=0.3)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WHOLE[key] = ref
    return _WHOLE[key]


@pytest.mark.parametrize("conv", chanmask_ref.CONVENTIONS)
@pytest.mark.parametrize("tiler", stream_ref.TILERS)
@pytest.mark.parametrize("shape", stream_ref.SHAPES, ids=stream_ref.shape_id)
def test_stream_equals_the_whole_file_composition(shape, tiler, conv):
    """frames, tiles, estimates and samples of every partition against stft_np -> tiling_np -> chanmask_ref -> compute_inverse of
    the complete signal, to float64 round-off; the state held never grows past what one push needs"""
    N, h, tc, ov, wname = shape
    win = stream_ref.window(wname, N)
    Ls = stream_ref.lengths(N, h, tc, ov)
    assert Ls[0] % h and not Ls[1] % h
    for L in Ls:
        want = _whole(shape, tiler, conv, L)
        assert want["n_tiles"] >= 1
        audio = stream_ref.signal(L)
        for kind in stream_ref.PARTITIONS:
            sizes = stream_ref.partition(kind, L, h, seed=L)
            assert sum(sizes) == L and (kind != "random" or 0 in sizes) and (kind != "empty_last" or sizes[-1] == 0)
            got = stream_ref.StreamRef(N, h, tc, ov, tiler, conv, 2, win, scale=0.3).run(audio, sizes)
            assert got["X"].shape == want["X"].shape and got["tiles"].shape == want["tiles"].shape
            assert got["est"].shape == want["est"].shape and got["pcm"].shape == want["pcm"].shape == (2, L)
            assert np.abs(got["X"] - want["X"]).max() <= ROUND_OFF
            assert np.abs(got["tiles"] - want["tiles"]).max() <= ROUND_OFF
            assert np.abs(got["est"] - want["est"]).max() <= ROUND_OFF
            assert np.abs(got["pcm"] - want["pcm"]).max() <= ROUND_OFF, (L, kind)
            if kind != "one":
                c = StreamCounts(N, h, tc, ov, tiler)
                mp = max(sizes)
                st = got["state"]
                assert st["samples"] <= N and st["rows"] <= tc + c.max_frames(mp) and st["tf"] <= N // h + tc + c.max_frames(mp)
                assert st["masks"] <= -(-tc // (tc - ov)) + c.max_tiles(mp)
    # the third length: the script tiler drops a tail the library tiler pads; the rows past the last tile are zero
    T = stft_np.frame_count(Ls[2], h)
    ks, kl = (len(tiling_np.tile_starts(T, tc, ov, t)) for t in stream_ref.TILERS)
    assert kl > ks >= 1
    if tiler == tiling_np.SCRIPT:
        tail = _whole(shape, tiler, conv, Ls[2])["est"][:, (ks - 1) * (tc - ov) + tc:]
        assert tail.shape[1] >= min(2, tc - ov) and not tail.any()


def test_counts_match_the_oracle_at_the_end_and_keep_their_promises_mid_stream():
    for N, h in stream_ref.GRID_FRAMES:
        for tc, ov in stream_ref.GRID_TILES:
            for tiler in stream_ref.TILERS:
                c = StreamCounts(N, h, tc, ov, tiler)
                assert c.latency_samples() == tc * h + N
                span = (tc + 4 * (tc - ov) + 3) * h + N
                grid = sorted(set(list(range(0, 3 * h + 2)) + list(range(0, span, max(1, h // 3))) +
                                  [k * h + d for k in range(0, span // h) for d in (-1, 0, 1) if k * h + d >= 0]))
                worst = None
                for P in grid:
                    T = stft_np.frame_count(P, h)
                    n_tiles = len(tiling_np.tile_starts(T, tc, ov, tiler))
                    assert c.frames(P, True) == T and c.tiles(P, True) == n_tiles
                    assert c.folded(P, True) == T and c.emitted(P, True) == P
                    A, K, Tf, E = c.frames(P), c.tiles(P), c.folded(P), c.emitted(P)
                    assert A == sum(1 for n in range(A + 2) if n * h - N // 2 + N <= P)       # frames whose N samples are in
                    assert K == len([s for s in range(0, max(A, 1), tc - ov) if s + tc <= A])
                    assert K <= n_tiles and A + 1 <= T and Tf == K * (tc - ov) and Tf <= A
                    assert 0 <= E <= P and E == max(0, Tf * h - N // 2)
                    if A >= tc:
                        assert E > P - tc * h - N
                        worst = max(worst or 0, P - E)
                assert worst is not None and worst < c.latency_samples()
                # what one push can produce: the bounds the rings are sized by hold for every push size on the grid
                for mp in (1, h - 1, h, 3 * h + 1):
                    for P in grid[::7]:
                        for ended in (False, True):
                            assert c.frames(P + mp, ended) - c.frames(P) <= c.max_frames(mp)
                            assert c.tiles(P + mp, ended) - c.tiles(P) <= c.max_tiles(mp)
    for bad in ((1000, 500, 30, 25), (1024, 768, 30, 25), (1024, 384, 30, 25), (1024, 512, 30, 30), (1024, 512, 30, 0)):
        with pytest.raises(ValueError):
            StreamCounts(*bad)


class _Net(object):
    def __init__(self, C):
        self.S = 4
        self.arch = type("A", (), {"C": C, "eps_mode": 0})()


class _Separator(object):
    """what StreamSeparator reads of a Separator before it touches the device"""
    frameSize, hopSize, tc, overlap, tiler, scale_factor, tie_mode, ctx, plan = 1024, 512, 30, 25, 0, 0.3, 0, None, None

    def __init__(self, arch_name, C):
        self.arch_name, self.net = arch_name, _Net(C)

    _require_mono_graph = dcs.Separator._require_mono_graph


def test_stream_separator_refusals():
    with pytest.raises(ValueError, match="single-input-channel"):
        StreamSeparator(_Separator("dsd_ild", 2))
    with pytest.raises(ValueError, match="single-input-channel"):
        StreamSeparator(_Separator("bach10_si", 4))
    with pytest.raises(ValueError, match="44 100"):
        StreamSeparator(_Separator("dsd", 1), sample_rate=48000)
    with pytest.raises(ValueError):
        StreamSeparator(_Separator("dsd", 1), max_block=0)
    ss = StreamSeparator(_Separator("dsd", 1), max_block=4096)
    assert ss.counts.latency_samples() == 30 * 512 + 1024
    with pytest.raises(IndexError):           # an empty signal gives no tile: what separate_channels raises
        ss.finish()
    with pytest.raises(ValueError, match="already"):
        ss.finish()
    with pytest.raises(ValueError, match="ended"):
        ss.push(np.zeros(10))
    assert hasattr(dcs.Separator, "stream")


def test_stream_symbols_are_declared_exported_and_bound():
    names = _lib.header_symbols()
    assert set(STREAM_SYMBOLS) <= set(names)
    lib = _lib.load()
    for n in STREAM_SYMBOLS:
        fn = getattr(lib, n)
        assert fn.argtypes is not None, n
    assert lib.dcs_stream_max_tiles(None) == -1 and lib.dcs_stream_bytes(None) == -1
    assert lib.dcs_stream_destroy(None) == _lib.DCS_OK
    assert lib.dcs_stream_reset(None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_push(None, None, 0, 0, None, 0, None, None, None, 0, None) == _lib.DCS_EINVAL
    assert lib.dcs_stream_pull(None, None, 0, 0, None, 0, 0, None, None, 0, 0) == _lib.DCS_EINVAL
    assert "StreamSeparator" in dcs.__all__ and "StreamCounts" in dcs.__all__
