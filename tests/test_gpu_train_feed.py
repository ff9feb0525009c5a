"""The trainers' data feed on the MI355X (train::gather_kernel of csrc/train_core.hip behind dcs_trainer_gather,
dcs_trainer_gather_sources and FeatureWindows) against its NumPy restatement tests/feed_ref.py, bit for bit: one float32
multiply has one result, so every comparison here is equality of the 32-bit patterns, never a tolerance."""
from ctypes import c_void_p

import numpy as np
import pytest

import feed_ref

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert not len(bad), (what, "first difference at", tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


def _write(tmp_path, arrays):
    from deepconvsep_amd.transform import write_shape_file
    paths = []
    for i, a in enumerate(arrays):
        stem = str(tmp_path / ("song%d.data" % i))
        np.asarray(a, dtype=np.float64).tofile(stem)
        write_shape_file(stem.replace(".data", ".shape"), a.shape)
        paths.append(stem)
    return paths


def _files(nsrc, F, Ts):
    """One pattern file per T, told apart by an offset; all values are integers below 2^24."""
    return [feed_ref.data_pattern(nsrc, T, F, offset=10000 * i) for i, T in enumerate(Ts)]


def _feed(tmp_path, files, tc, ov, mult, nsrc, **kw):
    from deepconvsep_amd.training import FeatureWindows
    return FeatureWindows(_write(tmp_path, files), tc, ov, mult, sources=nsrc, **kw)


def _table(files, tc, ov, windows):
    """The window table from the slot functions alone (checked against loadFile in test_train_cpu.py), not from the feed."""
    from deepconvsep_amd import training
    slots = training.reference_slots if windows == "reference" else training.all_slots
    return np.asarray([(i, s) if s is not None else (-1, 0) for i, a in enumerate(files)
                       for s in slots(a.shape[1], tc, ov)], dtype=np.int64).reshape(-1, 2)


def _check(fw, files, rows, tc, ov, mult, windows="reference", what=""):
    """gather(rows) against feed_ref on the test's own tc, overlap, scale, F and source count and its own window table."""
    nsrc, F = files[0].shape[0] - 1, files[0].shape[2]
    table = _table(files, tc, ov, windows)
    assert fw.total == len(table) and np.array_equal(fw.table, table)
    x, t = fw.gather(rows)
    wx, wt = feed_ref.gather_np(files, table[np.asarray(rows, dtype=np.int64)], tc, F, nsrc, mult)
    _same(fw.ctx.to_host(x), wx, what + " inputs")
    _same(fw.ctx.to_host(t), wt, what + " targets")
    return wx, wt


def test_fixture_cases_equal_feed_ref_and_loadfile(tmp_path, golden):
    """The cases of tests/golden/train_feed.npz: the device equals feed_ref bit for bit, and loadFile's own arrays exactly
    where the scale is a power of two, within one float32 ulp otherwise (loadFile scales in float64 before it narrows)."""
    g = golden("train_feed")
    for k, (T, tc, ov, nsrc, F, mult) in enumerate(g["cases"]):
        T, tc, ov, nsrc, F, mult = int(T), int(tc), int(ov), int(nsrc), int(F), float(mult)
        sub = tmp_path / str(k)
        sub.mkdir()
        files = [feed_ref.data_pattern(nsrc, T, F)]
        fw = _feed(sub, files, tc, ov, mult, nsrc)
        wx, wt = _check(fw, files, np.arange(fw.total), tc, ov, mult, what="case %d" % k)
        ref_x, ref_t = g["inputs_%d" % k], g["outputs_%d" % k]
        got_t = feed_ref.reference_layout(wt)
        if np.log2(mult) == np.round(np.log2(mult)):
            assert np.array_equal(wx[:, 0], ref_x) and np.array_equal(got_t, ref_t), k
        else:
            assert (np.abs(wx[:, 0] - ref_x) <= np.spacing(np.abs(ref_x))).all(), k
            assert (np.abs(got_t - ref_t) <= np.spacing(np.abs(ref_t))).all(), k


@pytest.mark.parametrize("windows", ["reference", "all"])
@pytest.mark.parametrize("nsrc", [1, 2, 4, 8])
@pytest.mark.parametrize("F", [1, 3, 6, 7])
def test_rows_across_files_in_one_batch(tmp_path, windows, nsrc, F):
    """Files of different T in one table (shorter than tc, T == tc, T == tc + 1, zero slots, many windows), every row once in
    one batch in a shuffled order, then a second batch with repeats."""
    tc, ov = 8, 5
    files = _files(nsrc, F, (5, 8, 9, 40, 16, 23))
    fw = _feed(tmp_path, files, tc, ov, 0.3, nsrc, windows=windows)
    assert len(set(fw.table[:, 0])) >= 5 and (windows == "all" or (fw.table[:, 0] < 0).any())
    rs = np.random.RandomState(F + nsrc)
    _check(fw, files, rs.permutation(fw.total), tc, ov, 0.3, windows, "every row")
    _check(fw, files, rs.randint(0, fw.total, size=11), tc, ov, 0.3, windows, "repeats")


def test_a_batch_of_one_row_and_a_batch_of_zero_slots(tmp_path):
    files = _files(4, 5, (12, 12, 30))
    fw = _feed(tmp_path, files, 12, 6, 0.3, 4)
    zero = np.flatnonzero(fw.table[:, 0] < 0)
    live = np.flatnonzero(fw.table[:, 0] >= 0)
    assert len(zero) >= 2 and len(live) >= 2
    for row in (live[-1], zero[0]):
        _check(fw, files, [row], 12, 6, 0.3, what="one row")
    wx, wt = _check(fw, files, zero, 12, 6, 0.3, what="zero slots only")
    assert not wx.any() and not wt.any()


def test_batches_order_drop_last_and_seeding(tmp_path):
    files = _files(2, 4, (40, 7, 25))
    for windows in ("reference", "all"):
        fw = _feed(tmp_path, files, 6, 2, 0.7, 2, windows=windows, batch_size=4, seed=5)
        again = _feed(tmp_path, files, 6, 2, 0.7, 2, windows=windows, batch_size=4, seed=5)
        assert fw.total % 4 and fw.iteration_size == fw.total // 4     # a last partial batch exists and is dropped
        perms = []
        for epoch in (0, 1):
            perm = np.random.RandomState(5 + epoch).permutation(fw.total)
            perms.append(perm)
            got, got2 = list(fw.batches(epoch)), list(again.batches(epoch))
            assert len(got) == fw.iteration_size == len(got2)
            for b, ((x, t), (x2, t2)) in enumerate(zip(got, got2)):
                rows = _table(files, 6, 2, windows)[perm[4 * b:4 * b + 4]]
                wx, wt = feed_ref.gather_np(files, rows, 6, 4, 2, 0.7)
                _same(fw.ctx.to_host(x), wx, "epoch %d batch %d inputs" % (epoch, b))
                _same(fw.ctx.to_host(t), wt, "epoch %d batch %d targets" % (epoch, b))
                _same(again.ctx.to_host(x2), wx)
                _same(again.ctx.to_host(t2), wt)
        assert not np.array_equal(perms[0], perms[1])


# ---------------------------------------------------------------------------------------------- the C entry points directly
SENTINEL = 0x5CA1AB1E      # a finite float32 bit pattern no product of the feed gives


def _raw_gather(ctx, torch, data_d, files, rows, tc, F, nsrc, scale, entry, guard=0):
    """Call ``entry`` ('gather' or 'sources') with output buffers that carry ``guard`` sentinel words on both sides; returns
    the whole buffers (uint32 view) and the windows."""
    B = len(rows)
    nx, nt = B * tc * F, B * nsrc * tc * F
    with ctx.stream_scope():
        files_d = torch.from_numpy(np.asarray(files, dtype=np.int64).reshape(-1, 2)).to(ctx.device)
        win_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)).to(ctx.device)
        xb = torch.full((nx + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        tb = torch.full((nt + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        ptr = lambda t, off=0: c_void_p(t.data_ptr() + 4 * off)  # noqa: E731
        from deepconvsep_amd import _lib
        if entry == "gather":
            assert nsrc == 4
            _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, ptr(data_d), ptr(files_d), ptr(win_d), B, tc, F, scale,
                                                   ptr(xb, guard), ptr(tb, guard)))
        else:
            _lib.check(ctx._lib.dcs_trainer_gather_sources(ctx._h, ptr(data_d), ptr(files_d), ptr(win_d), B, tc, F, nsrc,
                                                           scale, ptr(xb, guard), ptr(tb, guard)))
        return xb.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32)


def _resident(ctx, torch, files):
    table, off = [], 0
    for a in files:
        table.append((off, a.shape[1]))
        off += a.size
    with ctx.stream_scope():
        data_d = torch.from_numpy(np.concatenate([a.astype(np.float32).ravel() for a in files])).to(ctx.device)
    return data_d, table


@pytest.mark.parametrize("nsrc,F", [(4, 5), (4, 1), (1, 3), (8, 6)])
def test_entry_points_write_nothing_outside_their_outputs(nsrc, F):
    """The outputs of FeatureWindows.gather are torch tensors, outside the DCS_WS_GUARD harness: here both output buffers
    are larger than needed and filled with a sentinel on both sides, and every word outside inputs / targets must be
    untouched, every word inside equal to feed_ref.  Four sources go through both entry points and give identical bytes."""
    import torch
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    tc, guard = 7, 4096
    files = _files(nsrc, F, (4, 7, 30, 8))
    data_d, table = _resident(ctx, torch, files)
    rows = [(2, 23), (-1, 0), (0, 0), (3, 1), (2, 0), (1, 0), (3, 0), (-1, 0), (2, 11)]   # (2, 23): the file's last window
    wx, wt = feed_ref.gather_np(files, rows, tc, F, nsrc, 0.3)
    outs = []
    for entry in (("gather", "sources") if nsrc == 4 else ("sources",)):
        xb, tb = _raw_gather(ctx, torch, data_d, table, rows, tc, F, nsrc, 0.3, entry, guard)
        for name, buf, want in (("inputs", xb, wx), ("targets", tb, wt)):
            assert (buf[:guard] == SENTINEL).all() and (buf[-guard:] == SENTINEL).all(), (entry, name, "guard words changed")
            assert np.array_equal(buf[guard:-guard], _bits(want).ravel()), (entry, name)
        outs.append((xb, tb))
    if nsrc == 4:
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_bad_arguments_of_the_entry_points():
    import torch
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    files = _files(2, 3, (9,))
    data_d, table = _resident(ctx, torch, files)
    for nsrc in (0, 9):
        with pytest.raises(ValueError):
            _raw_gather(ctx, torch, data_d, table, [(0, 0)], 4, 3, nsrc, 1.0, "sources")
    from deepconvsep_amd.training import FeatureWindows
    for nsrc in (0, 9):
        with pytest.raises(ValueError):
            FeatureWindows([], sources=nsrc)


def test_element_offsets_past_two_to_the_31():
    """A resident training set of the DSD100 size is of the order of 10 GB of float32: element offsets pass 2^31.  A device
    buffer of 2^31 + 4096 float32 elements, zeroed on the device (no host copy), holds three small files: one at offset 0,
    one that straddles element 2^31 and one that starts past it; their windows come back exactly."""
    import torch
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    nsrc, T, F, tc = 4, 9, 5, 4
    n = 2 ** 31 + 4096
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 4 * n:
        pytest.skip("%.1f GiB of device memory free, the test wants four times its %.1f GiB buffer"
                    % (free / 2.0 ** 30, 4 * n / 2.0 ** 30))
    files = _files(nsrc, F, (T, T, T))
    size = files[0].size
    bases = [0, 2 ** 31 - size // 2 - 1, 2 ** 31 + 1000]
    assert bases[1] < 2 ** 31 < bases[1] + size and bases[2] + size <= n
    with ctx.stream_scope():
        data_d = torch.zeros(n, dtype=torch.float32, device=ctx.device)
        for a, base in zip(files, bases):
            data_d[base:base + size] = torch.from_numpy(a.astype(np.float32).ravel()).to(ctx.device)
    table = [(b, T) for b in bases]
    rows = [(2, 5), (1, 0), (0, 2), (1, 5), (-1, 0), (2, 0), (1, 7), (2, 8)]     # the last two run past T: padded
    wx, wt = feed_ref.gather_np(files, rows, tc, F, nsrc, 0.3)
    assert wx[1].all() and wx[3].all() and wx[0].all()
    for entry in ("gather", "sources"):
        xb, tb = _raw_gather(ctx, torch, data_d, table, rows, tc, F, nsrc, 0.3, entry, 64)
        assert (xb[:64] == SENTINEL).all() and (xb[-64:] == SENTINEL).all()
        assert (tb[:64] == SENTINEL).all() and (tb[-64:] == SENTINEL).all()
        assert np.array_equal(xb[64:-64], _bits(wx).ravel()) and np.array_equal(tb[64:-64], _bits(wt).ravel()), entry
    del data_d
    torch.cuda.empty_cache()
