"""The score-rendered STFT on the MI355X (csrc/fft_score_render.hip): ``dcs_stft_forward_score_render_f64`` bit for bit
against the existing float64 kernel on host-rendered audio (score_render.render_score_audio, itself equal to the reference's
render lines: tests/test_score_render_cpu.py) and within 1e-11 of the reference's own blocks (tests/golden/score_render.npz);
``dcs_trainer_gather_score_render`` against ``dcs_trainer_gather`` on those float64 blocks cast to float32, the path
``FeatureWindows`` serves today; both under the guard-band harness; files and rendered windows train alike; the Sibelius
files through the existing render entry point.

Shapes: the seeded tree and scores of tests/score_render_ref.py at sr = 1000 -- a virtual file is a 2 s chunk, 1800 - 2000
samples, 34 frames at hop 64 and 6 at hop 512, with every case of the overwrite rule in it
(test_score_render_cpu.py::test_the_fixture_holds_every_case) -- and hand-built files for 1, 3 and 8 tracks, empty tracks
and the frame of 4096."""
import os
import subprocess
import sys
from ctypes import POINTER, c_int64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

import score_render_ref as R  # noqa: E402
import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import _lib, augment, rwc, score_render as sr  # noqa: E402
from deepconvsep_amd.runtime import StftPlan, _ptr, default_context  # noqa: E402
from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from deepconvsep_amd.synth import synth_audio  # noqa: E402
from oracle import stft_np  # noqa: E402
from test_gpu_augment import FEED_TOL, SENTINEL  # noqa: E402      the project's float32 feed bound, 2e-5

FRAMES = [(256, 64), (1024, 512)]
_CACHE = {}


def _inputs():
    """(bank, the four recorded virtual files, all nine of the three combinations), built once per process."""
    if not _CACHE:
        import tempfile
        tmp = tempfile.mkdtemp()
        tree = R.write_rwc_tree(os.path.join(tmp, "rwc"))
        piece = R.write_scores(os.path.join(tmp, "db"))
        bank = rwc.NoteBank.from_instruments(
            [rwc.Instrument(tree, i, list(R.STYLES), list(R.CASES), list(R.DYNAMICS)) for i in R.INSTRUMENT_IDS])
        every = sr.score_files(piece, R.PIECE, bank, R.COMBOS, R.CHUNK, R.SR, 64)
        assert len(every) == 9
        _CACHE.update(bank=bank, every=every, recorded=[every[3 * ci + chnk] for ci, chnk, _, _ in R.RENDERS])
    return _CACHE["bank"], _CACHE["recorded"], _CACHE["every"]


def _hand_built():
    """name -> (bank, virtual file): what the scores do not reach."""
    arrays = {k: synth_audio(n, seed=70 + k, silence=False) * 0.25 for k, n in enumerate((900, 2500, 333, 1200, 64, 4000, 700, 1))}
    bank = rwc.NoteBank.from_arrays(arrays, sr=R.SR)
    off = [bank.index[k].offset for k in range(8)]
    ln = [bank.index[k].length for k in range(8)]
    rs = np.random.RandomState(9)

    def track(size, n, longest):
        b = np.sort(rs.randint(0, size, n))
        out = []
        for x in b:
            k = int(rs.randint(0, 8))
            out.append((int(x), off[k], int(min(ln[k], rs.randint(1, longest), size - x))))
        return tuple(out)
    return {
        # 6000 samples at frame 4096: the float64 kernel keeps its twiddles in global memory; dense and sparse tracks
        'long': (bank, sr.ScoreFile('long', 6000, (track(6000, 40, 900), track(6000, 3, 2500), track(6000, 12, 300),
                                                    track(6000, 1, 4000)))),
        # one track; a note of one sample; a note of length 0; two notes at the same b; a note at the last sample
        'one': (bank, sr.ScoreFile('one', 1500, (((0, off[7], 1), (5, off[0], 0), (5, off[0], 300), (5, off[2], 100),
                                                   (1499, off[3], 1)),))),
        # three tracks, the middle one without notes, the last one silent until past the first frames
        'three': (bank, sr.ScoreFile('three', 1111, (track(1111, 9, 500), (), ((900, off[1], 211),)))),
        # eight tracks, odd size; notes that reach past size are cut by the kernel as by the host render
        'eight': (bank, sr.ScoreFile('eight', 777, tuple(((0, off[s], min(ln[s], 2000)),) + track(777, 3, 400)
                                                        for s in range(8)))),
    }


HAND = _hand_built()


@pytest.fixture(scope="module")
def ctx():
    return default_context()


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "score_render.npz"))


def _tt(frame, hop):
    return dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=R.SR, window=blackmanharris)


@pytest.fixture(scope="module")
def blocks64(ctx):
    """(frame, hop, index into all nine files) -> the float64 block of the device render, computed once and shared."""
    cache = {}

    def get(frame, hop, i):
        if (frame, hop, i) not in cache:
            bank, _, every = _inputs()
            cache[(frame, hop, i)] = sr.render_score_features(_tt(frame, hop), bank, every[i])
        return cache[(frame, hop, i)]
    return get


def _check_f64(bank, sf, frame, hop, got=None):
    tt = _tt(frame, hop)
    got = sr.render_score_features(tt, bank, sf) if got is None else got
    audio = sr.render_score_audio(bank, sf)
    S = len(sf.tracks)
    assert got.shape == (1 + S, _lib.frame_count(sf.size, hop), frame // 2 + 1) and got.dtype == np.float64
    dev = tt.compute_transform(audio, phase=False, save=False)
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(dev).view(np.uint64)), sf.name
    win = blackmanharris(frame)
    want = np.stack([stft_np.compute_file(audio[:, j], frameSize=frame, hopSize=hop, window=win) for j in range(1 + S)])
    err = float(np.max(np.abs(got - want)))
    print("score render f64 %r (%d, %d): max |device - oracle| = %.3e" % (sf.name[:8], frame, hop, err))
    assert got[0].any() and err < 1e-11            # the float64 STFT's bound in tests/test_gpu_parity.py


# ------------------------------------------------------------------------------------------ (i) float64, the file path
@pytest.mark.parametrize("frame,hop", FRAMES)
@pytest.mark.parametrize("k", range(len(R.RENDERS)))
def test_score_render_f64_equals_the_existing_kernel_on_host_rendered_audio(blocks64, k, frame, hop):
    bank, _, every = _inputs()
    ci, chnk = R.RENDERS[k][:2]
    _check_f64(bank, every[3 * ci + chnk], frame, hop, blocks64(frame, hop, 3 * ci + chnk))


@pytest.mark.parametrize("name,frame,hop", [('long', 4096, 512), ('long', 256, 64), ('one', 256, 64), ('three', 1024, 512),
                                            ('three', 256, 64), ('eight', 256, 64), ('eight', 4096, 512)])
def test_score_render_f64_hand_built_files(ctx, name, frame, hop):
    bank, sf = HAND[name]
    _check_f64(bank, sf, frame, hop)


def test_hand_built_files_reach_what_the_scores_do_not():
    long_ = HAND['long'][1]
    assert long_.size == 6000 and len(long_.tracks[0]) == 40
    one = HAND['one'][1].tracks[0]
    assert [n[2] for n in one][:2] == [1, 0] and one[2][0] == one[3][0] and one[-1][0] == HAND['one'][1].size - 1
    assert HAND['three'][1].tracks[1] == ()
    eight = HAND['eight'][1]
    assert len(eight.tracks) == 8 and any(n[0] + n[2] > eight.size for t in eight.tracks for n in t)
    a = sr.render_score_audio(*HAND['one'])
    assert a[5, 1] == HAND['one'][0].data[one[3][1]]               # of two notes at the same b the later one is heard


# ------------------------------------------------------------------------------------------ (ii) the reference's blocks
@pytest.mark.parametrize("k", [k for k, r in enumerate(R.RENDERS) if r[2]])
def test_score_render_f64_against_the_reference_blocks(ctx, g, k):
    """The reference's own render lines (compute_features_bach10rwc.py:112-139 at 1000 Hz) transformed by its stft_norm:
    within 1e-11, and bit for bit against the existing kernel on the reference's rendered audio."""
    bank, recorded, _ = _inputs()
    _, _, frame, hop = R.RENDERS[k]
    tt = _tt(frame, hop)
    got = sr.render_score_features(tt, bank, recorded[k])
    want = g["block_%d" % k]
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    print("golden %d (%d, %d): %.3e" % (k, frame, hop, err))
    assert err < 1e-11
    dev = tt.compute_transform(np.ascontiguousarray(g["audio_%d" % k]), phase=False, save=False)
    assert np.array_equal(got, dev)


def test_render_score_features_writes_the_reference_files(ctx, blocks64, tmp_path):
    bank, _, every = _inputs()
    tt = _tt(256, 64)
    path = sr.render_score_features(tt, bank, every[4], str(tmp_path))
    assert os.path.basename(path) == every[4].name + "__m_.data"
    shape = tt.get_shape(path.replace('.data', '.shape'))
    want = blocks64(256, 64, 4)
    assert shape == want.shape and np.array_equal(np.fromfile(path).reshape(shape), want)


# ------------------------------------------------------------------------------------------ (iii) float32, the feed
def _feed_windows(T, tc, batch):
    """(file, first frame) windows: from frame 0, ending exactly at T, running past T, a dead slot, a file index past the
    table, a window that begins past T, windows of every file; cycled to ``batch``."""
    longest = int(np.argmax(T))
    assert T[longest] > tc
    base = [(longest, 0), (longest, T[longest] - tc), (longest, T[longest] - tc + 3), (-1, 0), (len(T), 0), (0, T[0] + 2)]
    for i in range(len(T)):
        base.append((i, (5 * i) % max(1, T[i] - 1)))
    return np.asarray([base[i % len(base)] for i in range(batch)], dtype=np.int32)


def _raw_feed(ctx, plan, bank_t, bank_len, notes, rows, win, tc, S, scale, guard=0, n_notes=None, n_files=None):
    """dcs_trainer_gather_score_render into buffers with ``guard`` sentinel words on either side; rc and the whole buffers."""
    import torch
    B, F = len(win), plan.bins
    nx, nt = B * max(tc, 1) * F, B * max(S, 1) * max(tc, 1) * F
    with ctx.stream_scope():
        notes_d = torch.from_numpy(np.ascontiguousarray(notes, dtype=np.int64)).to(ctx.device)
        rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(ctx.device)
        win_d = torch.from_numpy(np.ascontiguousarray(win, dtype=np.int32)).to(ctx.device)
        xb = torch.full((nx + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        tb = torch.full((nt + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        rc = ctx._lib.dcs_trainer_gather_score_render(
            ctx._h, plan._h, _ptr(bank_t), bank_len, _ptr(notes_d), len(notes) if n_notes is None else n_notes, _ptr(rows_d),
            len(rows) if n_files is None else n_files, _ptr(win_d), B, tc, S, scale, xb.data_ptr() + 4 * guard,
            tb.data_ptr() + 4 * guard)
        return rc, xb.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32)


def _unguard(buf, guard, shape):
    assert (buf[:guard] == SENTINEL).all() and (buf[len(buf) - guard:] == SENTINEL).all(), "the margins were written"
    return buf[guard:len(buf) - guard].view(np.float32).reshape(shape)


def _feed_case(ctx, blocks64, frame, hop, tc, batch, scale, guard=0):
    import torch
    bank, _, every = _inputs()
    notes, rows = sr.pack_tables(every, bank.length, hop)
    T = [int(r[1]) for r in rows]
    win = _feed_windows(T, tc, batch)
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    rc, xb, tb = _raw_feed(ctx, plan, bank.device(np.float32, ctx), bank.length, notes, rows, win, tc, 4, scale, guard)
    _lib.check(rc)
    F = plan.bins
    x, t = _unguard(xb, guard, (batch, 1, tc, F)), _unguard(tb, guard, (batch, 4, tc, F))
    # the parent's feed: the float64 blocks cast to float32, resident, cut by dcs_trainer_gather
    blocks = [blocks64(frame, hop, i).astype(np.float32) for i in range(len(every))]
    table, off = [], 0
    for b in blocks:
        table.append((off, b.shape[1]))
        off += b.size
    with ctx.stream_scope():
        data_d = torch.from_numpy(np.concatenate([b.ravel() for b in blocks])).to(ctx.device)
        files_d = torch.from_numpy(np.asarray(table, dtype=np.int64)).to(ctx.device)
        # dcs_trainer_gather takes no file count and bounds only file < 0: a file past the table is a dead slot for it
        win_ref = win.copy()
        win_ref[win_ref[:, 0] >= len(table)] = (-1, 0)
        win_d = torch.from_numpy(win_ref).to(ctx.device)
        xr = torch.empty((batch, 1, tc, F), dtype=torch.float32, device=ctx.device)
        tr = torch.empty((batch, 4, tc, F), dtype=torch.float32, device=ctx.device)
        _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(win_d), batch, tc, F, scale, _ptr(xr),
                                               _ptr(tr)))
        xr, tr = xr.cpu().numpy(), tr.cpu().numpy()
    return T, win, (x, t), (xr, tr)


# every (frame, hop, tc) x scale x batch of the first two shapes, and the frame of 4096 once: above 48 KiB of LDS the launch
# raises the kernel's dynamic shared-memory limit first
@pytest.mark.parametrize("frame,hop,tc,scale,batch",
                         [(f, h, tc, s, b) for f, h, tc in [(1024, 512, 4), (256, 64, 8)] for s in [1.0, 0.3] for b in [1, 32]]
                         + [(4096, 512, 3, 0.3, 2)])
def test_gather_score_render_against_gather_on_the_float64_blocks(ctx, blocks64, frame, hop, tc, scale, batch):
    T, win, (x, t), (xr, tr) = _feed_case(ctx, blocks64, frame, hop, tc, batch, scale)
    ex, et = float(np.max(np.abs(x - xr))), float(np.max(np.abs(t - tr)))
    print("score feed (%d, %d) tc %d scale %.1f batch %d: max error inputs %.3e targets %.3e (bound %.1e)"
          % (frame, hop, tc, scale, batch, ex, et, FEED_TOL * scale))
    assert xr.any() and tr.any()
    for b, (fi, start) in enumerate(win):
        n = 0 if fi < 0 or fi >= len(T) else max(0, min(tc, T[fi] - int(start)))
        # (iv) dead slots, files outside the table and frames past T: exactly zero, in both feeds
        assert not x[b, :, n:].any() and not t[b, :, n:].any(), b
        assert not xr[b, :, n:].any() and not tr[b, :, n:].any(), b
    assert ex <= FEED_TOL * scale and et <= FEED_TOL * scale


# ------------------------------------------------------------------------------------------ (iv) guard bands
def _raw_render(ctx, plan, bank_t, bank_len, tracks, size, guard=0, S=None, out_rows=None, ld=None, f64=True):
    """dcs_stft_forward_score_render into a buffer with ``guard`` sentinel words on either side; (rc, buffer as uint32, T)."""
    import torch
    S = len(tracks) if S is None else S
    counts = np.asarray([len(t) for t in tracks], dtype=np.int64)
    notes = np.asarray([n for t in tracks for n in t], dtype=np.int64).reshape(-1, 3)
    T = _lib.frame_count(max(int(size), 0), plan.hop)
    rows = (1 + max(S, 0)) * T if out_rows is None else out_rows
    words = 2 if f64 else 1
    got = c_int64(-1)
    with ctx.stream_scope():
        buf = torch.full((max(rows, 1) * plan.bins * words + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        fn = ctx._lib.dcs_stft_forward_score_render_f64 if f64 else ctx._lib.dcs_stft_forward_score_render_f32
        rc = fn(plan._h, _ptr(bank_t), bank_len, S, notes.ctypes.data, counts.ctypes.data, int(size), buf.data_ptr() + 4 * guard,
                plan.bins if ld is None else ld, rows, POINTER(c_int64)(got))
        return rc, buf.cpu().numpy().view(np.uint32), got.value


def guarded_calls(out_path):
    """Body of the guard-band child process: one render call and one feed call with poisoned margins around the outputs."""
    ctx = default_context()
    bank, _, every = _inputs()
    guard, frame, hop = 4096, 256, 64
    sf = every[3]
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    rc, buf, T = _raw_render(ctx, plan, bank.device(np.float64, ctx), bank.length, sf.tracks, sf.size, guard)
    _lib.check(rc)
    assert T == _lib.frame_count(sf.size, hop)
    assert (buf[:guard] == SENTINEL).all() and (buf[len(buf) - guard:] == SENTINEL).all(), "render wrote its margins"
    got = buf[guard:len(buf) - guard].view(np.float64)
    tt = _tt(frame, hop)
    cache = {}

    def blocks64(fr, hp, i):
        if i not in cache:
            cache[i] = sr.render_score_features(tt, bank, every[i])
        return cache[i]
    assert np.array_equal(got, blocks64(frame, hop, 3).ravel()) and not np.isnan(got).any()
    _, _, (x, t), (xr, tr) = _feed_case(ctx, blocks64, frame, hop, 8, 32, 0.3, guard)
    assert np.max(np.abs(x - xr)) <= FEED_TOL * 0.3 and np.max(np.abs(t - tr)) <= FEED_TOL * 0.3
    n = ctx.check_guards()
    assert n > 0
    np.save(out_path, np.concatenate([got.astype(np.float32), x.ravel(), t.ravel()]))


_GUARD_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_score_render as T
T.guarded_calls(sys.argv[2])
"""


def test_guard_harness_red_zones_and_poisons(tmp_path):
    outs = []
    for poison in ("255", "127"):
        env = dict(os.environ, DCS_WS_GUARD="4096", DCS_WS_POISON=poison)
        dst = str(tmp_path / ("out_%s.npy" % poison))
        rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst], env=env, timeout=300, capture_output=True,
                            text=True)
        assert rc.returncode == 0, rc.stderr[-3000:]
        outs.append(np.load(dst))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ------------------------------------------------------------------------------------------ (v) validation
def test_entry_points_reject_bad_arguments(ctx):
    bank, sf = HAND['three']
    b64, b32 = bank.device(np.float64, ctx), bank.device(np.float32, ctx)
    plan = StftPlan(ctx, 256, 64, blackmanharris(256))
    T = _lib.frame_count(sf.size, 64)

    def render(**kw):
        args = dict(tracks=sf.tracks, size=sf.size, S=None, bank_len=bank.length, out_rows=None, ld=None)
        args.update(kw)
        rc, buf, _ = _raw_render(ctx, plan, b64, args['bank_len'], args['tracks'], args['size'], 16, args['S'],
                                 args['out_rows'], args['ld'])
        if rc != _lib.DCS_OK:
            assert (buf == SENTINEL).all()          # a rejected call writes nothing
        return rc
    assert render() == _lib.DCS_OK
    assert render(S=0, tracks=()) == _lib.DCS_EINVAL
    assert render(S=9, tracks=(sf.tracks * 3)) == _lib.DCS_EINVAL
    assert render(out_rows=4 * T - 1) == _lib.DCS_EINVAL
    assert render(ld=128) == _lib.DCS_EINVAL
    assert render(size=-1) == _lib.DCS_EINVAL
    last = sf.tracks[2][0]
    assert render(bank_len=last[1] + last[2] - 1) == _lib.DCS_EINVAL                       # a note past the bank
    for bad in ((last, (last[0] - 1, last[1], 5)),                                          # b decreases
                ((-1, 0, 5),), ((0, -1, 5),), ((0, 0, -5),), ((0, bank.length, 1),)):
        assert render(tracks=(sf.tracks[0], (), bad)) == _lib.DCS_EINVAL, bad
    with pytest.raises(ValueError):
        sr.render_score_features(_tt(256, 64), bank, sf._replace(tracks=(sf.tracks[0], (), ((9, 0, 5), (8, 0, 5)))))

    notes, rows = sr.pack_tables([sf], bank.length, 64)
    win = np.asarray([(0, 0)], dtype=np.int32)
    for S, tc, n_files in ((0, 8, 1), (9, 8, 1), (3, 0, 1), (3, 8, 0)):
        rc, xb, tb = _raw_feed(ctx, plan, b32, bank.length, notes, rows, win, tc, S, 0.3, 16, n_files=n_files)
        assert rc == _lib.DCS_EINVAL, (S, tc, n_files)
        assert (xb == SENTINEL).all() and (tb == SENTINEL).all()
    rc, xb, tb = _raw_feed(ctx, plan, b32, bank.length, notes, rows, win, 8, 3, 0.3, 16, n_notes=-1)
    assert rc == _lib.DCS_EINVAL and (xb == SENTINEL).all() and (tb == SENTINEL).all()
    rc, xb, tb = _raw_feed(ctx, plan, b32, bank.length, notes, rows, win, 8, 3, 0.3, 16)
    assert rc == _lib.DCS_OK and not (xb[16:-16] == SENTINEL).any() and not (tb[16:-16] == SENTINEL).any()


def test_the_feed_bounds_its_device_tables(ctx):
    """The tables of the feed live on the device, where the host cannot validate them: a track whose notes lie outside the
    note table is silent, a note whose segment reaches past the bank reads zeros there, and nothing outside the outputs is
    written."""
    bank, sf = HAND['three']
    plan = StftPlan(ctx, 256, 64, blackmanharris(256))
    notes, rows = sr.pack_tables([sf], bank.length, 64)
    win = np.asarray([(0, 0), (0, 9)], dtype=np.int32)
    b32 = bank.device(np.float32, ctx)
    _, xb, tb = _raw_feed(ctx, plan, b32, bank.length, notes, rows, win, 8, 3, 1.0, 16)
    good = _unguard(tb, 16, (2, 3, 8, 129))
    bad_rows = rows.copy()
    bad_rows[0, 2 + 2 * 2] = len(notes)                         # track 2 begins at the table's end with a count of 1
    rc, xb, tb = _raw_feed(ctx, plan, b32, bank.length, notes, bad_rows, win, 8, 3, 1.0, 16)
    t = _unguard(tb, 16, (2, 3, 8, 129))
    assert rc == _lib.DCS_OK and not t[:, 2].any() and np.array_equal(t[:, 0], good[:, 0])
    _unguard(xb, 16, (2, 1, 8, 129))
    # a bank declared shorter than the notes reach: what lies past its end reads as zero, bit for bit what a bank with
    # zeros there gives
    short = int(sf.tracks[2][0][1] + sf.tracks[2][0][2] - 100)
    rc, xb, tb = _raw_feed(ctx, plan, b32, short, notes, rows, win, 8, 3, 1.0, 16)
    assert rc == _lib.DCS_OK
    zeroed = bank.data.copy()
    zeroed[short:] = 0
    rc, xz, tz = _raw_feed(ctx, plan, ctx.to_device(zeroed, np.float32), bank.length, notes, rows, win, 8, 3, 1.0, 16)
    assert rc == _lib.DCS_OK and np.array_equal(xb, xz) and np.array_equal(tb, tz)
    t = _unguard(tb, 16, (2, 3, 8, 129))
    assert np.isfinite(t).all() and not np.array_equal(t[:, 2], good[:, 2])


# ------------------------------------------------------------------------------------------ (vi) end to end, tiny
def test_end_to_end_files_and_rendered_windows_train_alike(ctx, tmp_path):
    """F = 129 (frame 256): the smallest feature size of tests/test_gpu_train_bach10.py that is frame / 2 + 1 of a frame the
    render tests cover."""
    from deepconvsep_amd.training import FeatureWindows, Trainer, glorot_init
    bank, _, every = _inputs()
    frame, hop, tc, ov, B, scale = 256, 64, 9, 5, 8, 0.3
    tt = _tt(frame, hop)
    paths = [sr.render_score_features(tt, bank, sf, str(tmp_path)) for sf in every]
    rw = sr.ScoreRenderedWindows(bank, every, tc, ov, scale, 'reference', B, 0, ctx, frame, hop, blackmanharris)
    fw = FeatureWindows(paths, tc, ov, scale, 'reference', B, 0, ctx)
    assert np.array_equal(fw.table, rw.table) and (fw.F, fw.total, fw.iteration_size) == (rw.F, rw.total, rw.iteration_size)
    assert rw.F == 129 and rw.iteration_size >= 3
    params = glorot_init('bach10', tc, rw.F, seed=1)
    first = []
    for data in (fw, rw):
        tr = Trainer(ctx, arch='bach10', params=params, batch_size=B, time_context=tc, feat_size=rw.F, seed=1)
        losses = []
        for k, (x, t) in enumerate(data.batches(0)):
            if k == 3:
                break
            if data is rw:
                xf, tf = fw.gather(np.random.RandomState(0).permutation(fw.total)[k * B:(k + 1) * B])
                ex, et = float((x - xf).abs().max()), float((t - tf).abs().max())
                print("end to end batch %d: inputs %.3e targets %.3e" % (k, ex, et))
                assert ex <= FEED_TOL * scale and et <= FEED_TOL * scale
            if k == 0:
                n_t, t_rms = t.numel(), float(t.double().pow(2).mean().sqrt())
            losses.append(tr.step(x, t))
        assert len(losses) == 3 and np.isfinite(losses).all()
        first.append(losses[0])
        tr.close()
    # The margin test_gpu_augment.py::test_end_to_end_files_and_rendered_windows_train_alike derives: the loss is a weighted
    # sum of squared differences e = mask(x) x - target with |weights| <= 1, so |dL| <= 2 |e| |de| to first order; every
    # input and target element moves by at most delta = FEED_TOL * scale, so |d target| <= delta sqrt(n); the masked
    # prediction is taken to move by at most K = 10 times as much in norm.  Hence |dL| / L <= 2 (1 + K) delta sqrt(n) / sqrt(L).
    delta, K = FEED_TOL * scale, 10.0
    margin = 2 * (1 + K) * delta * np.sqrt(n_t) / np.sqrt(first[0])
    rel = abs(first[0] - first[1]) / first[0]
    print("first losses %.9g (files) %.9g (rendered): relative difference %.3e, margin %.3e, target rms %.3e"
          % (first[0], first[1], rel, margin, t_rms))
    assert first[0] > 0 and rel <= margin


def _load(script):
    import importlib.util
    spec = importlib.util.spec_from_file_location(os.path.basename(script)[:-3] + "_sr", os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_lines_write_the_files_and_train_without_them(ctx, tmp_path):
    """compute_features_rwc.py writes what render_score_features gives for the files of dataset_files; train_bach10.py --rwc
    --render trains one epoch from the tree alone."""
    tree = R.write_rwc_tree(str(tmp_path / "rwc"))
    db = str(tmp_path / "db")
    R.write_scores(db)
    os.makedirs(os.path.join(db, "notes"))                       # no digit in front: not a piece
    out = str(tmp_path / "features")
    common = ["--rwc", tree, "--chunk_size", "2", "--sample_size", "3", "--seed", "4", "--sample_rate", str(R.SR)]
    _load("examples/bach10/compute_features_rwc.py").main(["--db", db, "--feature_path", out] + common)
    bank = sr.load_bank(tree)
    ((piece, style, sfiles),) = sr.dataset_files(db, bank, 2, 3, True, 4, R.SR)
    assert (piece, style) == (R.PIECE, 'original') and len(sfiles) == 9
    tt = _tt(4096, 512)
    d = os.path.join(out, R.PIECE, 'original')
    assert sorted(os.listdir(d)) == sorted(sf.name + e for sf in sfiles for e in ("__m_.data", "__m_.shape"))
    want = sr.render_score_features(tt, bank, sfiles[5])
    shape = tt.get_shape(os.path.join(d, sfiles[5].name + "__m_.shape"))
    assert shape == want.shape == (5, _lib.frame_count(sfiles[5].size, 512), 2049)
    assert np.array_equal(np.fromfile(os.path.join(d, sfiles[5].name + "__m_.data")).reshape(shape), want)
    # training: 9 virtual files of 6 frames at hop 512, windows of 4 frames
    sources = str(tmp_path / "sources")
    os.makedirs(os.path.join(sources, R.PIECE))
    outdir = str(tmp_path / "out")
    os.makedirs(outdir)
    _load("examples/bach10/train_bach10.py").main(
        ["--db", sources, "--dbs", db, "--output", outdir, "--model", "m", "--render", "--frame_size", "1024", "--batch_size", "4",
         "--time_context", "4", "--overlap", "2", "--nepochs", "1", "--skip_sep"] + common)
    model = _load("examples/bach10/separate_bach10.py").load_model(os.path.join(outdir, "models", "model_m.pkl"))
    assert len(model) == 17 and all(np.isfinite(p).all() for p in model)


# ------------------------------------------------------------------------------------------ (vii) Sibelius
def test_sibelius_files_through_the_existing_render(ctx, g):
    """compute_features_bach10sibelius.py needs no new kernel: its files are ``augment.VirtualFile``s."""
    frame, hop = 4096, 512
    vfs = sr.sibelius_files(R.SIB_LENGTHS, R.SIB_SHIFTS, R.SIB_GAINS, R.SR, name='p')
    signals = {('p', i): x for i, x in enumerate(R.sibelius_sources())}
    bank = augment.Bank(signals, np.float64, ctx)
    tt = _tt(frame, hop)
    for k, ci in enumerate(R.SIB_PICK):
        (got,) = augment.render_features(tt, bank, vfs[ci])
        audio = np.ascontiguousarray(g["sib_audio_%d" % k])
        assert got.shape == (5, _lib.frame_count(len(audio), hop), frame // 2 + 1)
        assert np.array_equal(got, tt.compute_transform(audio, phase=False, save=False))
        if k == R.SIB_BLOCK:
            err = float(np.max(np.abs(got - g["sib_block_%d" % k])))
            print("sibelius %d: %.3e" % (k, err))
            assert err < 1e-11
