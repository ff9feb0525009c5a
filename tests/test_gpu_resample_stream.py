"""``dcs_resample_stream`` on the MI355X: however the signal is cut, the concatenated outputs are ``dcs_resample_f32``'s on the
complete signal bit for bit, every count is ``ResampleCounts``', the one-block output keeps the float32 bound of
tests/test_gpu_resample.py against the float64 restatement, and bad calls are refused before anything is launched or written."""
import ctypes
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

from deepconvsep_amd import _lib
from deepconvsep_amd.resample import ResampleCounts, StreamResampler

import resample_ref as ref

pytestmark = pytest.mark.gpu

L_LONG, L_SINGLES, PAD = 3001, 700, 37
SENTINEL = np.float32(-1234.5)
_signals, _whole = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from deepconvsep_amd.runtime import default_context
    return default_context()


def signal(rows, L):
    """[rows, L] float32, seeded; never changed"""
    if (rows, L) not in _signals:
        x = np.random.RandomState(100 * rows + L).uniform(-1.0, 1.0, (rows, L)).astype(np.float32)
        x.setflags(write=False)
        _signals[(rows, L)] = x
    return _signals[(rows, L)]


def whole(ctx, pair, rows, L):
    """``Resampler`` on the complete signal, once per case"""
    key = (pair, rows, L)
    if key not in _whole:
        y = ctx.to_host(ctx.resampler(*pair)(ctx.to_device(np.array(signal(rows, L)), np.float32)))
        y.setflags(write=False)
        _whole[key] = y
    return _whole[key]


def partitions(L, seed):
    rs = np.random.RandomState(seed)
    sizes, left = [], L
    while left:
        n = 0 if rs.rand() < 0.2 else int(min(left, rs.randint(1, 400)))
        sizes.append(n)
        left -= n
    sizes.insert(len(sizes) // 2, 0)                   # an empty push mid-stream, whatever the draw
    return {"one": [L], "random": sizes, "empty_last": sizes + [0]}


def drive(ctx, st, x, sizes):
    """x [rows, L] through the stream in blocks of ``sizes`` (the last one ends the signal); with more than one row the blocks
    are views of a buffer whose row stride is larger than any block.  Every n_out is checked against ResampleCounts."""
    import torch
    rows, L = x.shape
    buf = np.full((rows, L + PAD), np.nan, dtype=np.float32)
    buf[:, :L] = x
    buf_d = ctx.to_device(buf, np.float32)
    c, pos, outs = st.counts, 0, []
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        before = c.emitted(pos)
        piece = buf_d[:, pos:pos + n] if rows > 1 else buf_d[:, pos:pos + n].contiguous()
        y = st.push(piece if n else None, last=last)
        pos += n
        assert int(y.shape[1]) == c.emitted(pos, last) - before and tuple(y.shape[:1]) == (rows,)
        outs.append(y)
    assert pos == L and st.pushed == L
    with ctx.stream_scope():
        return ctx.to_host(torch.cat(outs, dim=1))


@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("pair", ref.PAIRS, ids=lambda p: "%d_%d" % p)
def test_bits_of_the_whole_file_conversion_however_the_signal_is_cut(ctx, pair, rows):
    x = signal(rows, L_LONG)
    want = whole(ctx, pair, rows, L_LONG)
    st = StreamResampler(ctx, pair[0], pair[1], rows, max_block=L_LONG)
    assert (st.counts.up, st.counts.down) == ref.RATIOS[pair]
    nbytes = st.device_bytes
    assert nbytes == rows * (L_LONG + st.counts.history()) * 4
    parts = partitions(L_LONG, seed=L_LONG + rows)
    assert 0 in parts["random"][:-1] and parts["empty_last"][-1] == 0
    for kind in ("one", "random", "empty_last"):
        st.reset()
        got = drive(ctx, st, x, parts[kind])
        assert got.shape == want.shape == (rows, ref.length(L_LONG, *ref.RATIOS[pair]))
        assert not np.isnan(got).any() and np.array_equal(got, want), (pair, rows, kind)
    st.reset()                                         # reset, the same pushes: the same bits; the memory has not moved
    assert np.array_equal(drive(ctx, st, x, parts["empty_last"]), want)
    assert st.device_bytes == nbytes
    st.close()
    # every block a single sample, on a ring of 1 + history samples
    xs = signal(rows, L_SINGLES)
    st = StreamResampler(ctx, pair[0], pair[1], rows, max_block=1)
    assert st.device_bytes == rows * (1 + st.counts.history()) * 4
    got = drive(ctx, st, xs, [1] * L_SINGLES + [0])
    assert np.array_equal(got, whole(ctx, pair, rows, L_SINGLES)), (pair, rows, "singles")
    st.close()


@pytest.mark.parametrize("pair", ref.PAIRS, ids=lambda p: "%d_%d" % p)
def test_one_block_within_the_float32_bound(ctx, pair):
    """|y_gpu[m] - y_ref[m]| <= (K + 2) 2^-24 sum_n |x[n]| |h[m down - n up]|, the bound of tests/test_gpu_resample.py"""
    up, down = ref.RATIOS[pair]
    h, H = ref.taps(up, down)
    x = signal(1, L_LONG)
    y, K, mass = ref.resample(x[0].astype(np.float64), up, down, h, H, want_bound=True)
    st = StreamResampler(ctx, pair[0], pair[1], 1, max_block=L_LONG)
    got = drive(ctx, st, x, [L_LONG])[0]
    st.close()
    bound = (K + 2) * 2.0 ** -24 * mass
    err = np.abs(got.astype(np.float64) - y)
    print("%d -> %d: largest error / bound = %.3f" % (pair[0], pair[1], float(np.max(err / np.maximum(bound, 1e-300)))))
    assert got.shape == y.shape and (err <= bound).all(), (int(np.argmax(err - bound)), float(np.max(err - bound)))


def test_bad_calls_are_refused_before_anything_is_written(ctx):
    lib = ctx._lib
    rs = ctx.resampler(48000, 44100)
    counts = ResampleCounts(rs.up, rs.down, rs.half)

    def create(rows, max_push):
        h = c_void_p()
        return lib.dcs_resample_stream_create(rs._h, rows, max_push, byref(h)), h
    for rows, max_push in ((0, 64), (65, 64), (1, 0), (1, 2 ** 30 + 1)):
        assert create(rows, max_push)[0] == _lib.DCS_EINVAL, (rows, max_push)
    rc, h = create(3, 256)
    assert rc == _lib.DCS_OK and lib.dcs_resample_stream_bytes(h) == 3 * (256 + counts.history()) * 4
    x = ctx.to_device(signal(3, L_LONG)[:, :300], np.float32)
    out = ctx.to_device(np.full((3, 400), SENTINEL, np.float32), np.float32)
    got = c_int64(-7)

    def push(n, last=0, in_stride=300, out_stride=400, cap=400, at=0):
        return lib.dcs_resample_stream_push(h, c_void_p(x.data_ptr() + 4 * at), in_stride, n, last, c_void_p(out.data_ptr()), out_stride,
                                            cap, byref(got))

    def untouched():
        return bool((ctx.to_host(out) == SENTINEL).all())
    assert push(257) == _lib.DCS_EINVAL and push(-1) == _lib.DCS_EINVAL                 # n out of range
    assert push(200, in_stride=199) == _lib.DCS_EINVAL                                  # input stride below the count
    due = counts.emitted(200)
    assert due > 1
    assert push(200, cap=due - 1) == _lib.DCS_EINVAL                                    # no room for what becomes final
    assert push(200, out_stride=due - 1) == _lib.DCS_EINVAL                             # output stride below the count
    assert got.value == -7 and untouched()
    assert push(20) == _lib.DCS_OK and got.value == counts.emitted(20) == 0 and untouched()     # nothing is due yet
    assert push(180, at=20) == _lib.DCS_OK and got.value == due                               # the refused calls left no trace
    first = ctx.to_host(out)[:, :due].copy()
    assert push(0, last=1) == _lib.DCS_OK and got.value == counts.emitted(200, True) - due
    assert push(1) == _lib.DCS_EINVAL and push(0, last=1) == _lib.DCS_EINVAL            # a push after the end
    assert lib.dcs_resample_stream_reset(h) == _lib.DCS_OK
    assert push(200) == _lib.DCS_OK and got.value == due
    assert np.array_equal(ctx.to_host(out)[:, :due], first) and (ctx.to_host(out)[:, due:] == SENTINEL).all()
    ctx.synchronize()
    assert lib.dcs_resample_stream_destroy(h) == _lib.DCS_OK
