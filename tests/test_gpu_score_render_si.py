"""The score-informed feed on rendered data on the MI355X (csrc/fft_score_render.hip: ``stft_score_informed_kernel``,
``dcs_trainer_gather_score_informed_render``): bit for bit against the composition of the entry points it fuses --
``dcs_stft_forward_score_render_f32`` on every virtual file, then ``dcs_trainer_gather_score`` on those blocks with the same
windows and mask tables.  Both sides run the same float32 operations, so inputs and targets are compared as bit patterns.
Hand-built mask tables against the NumPy restatement tests/score_feed_ref.py; the device tables are bounded; bad arguments;
the files ``render_score_informed_features`` writes; files and rendered windows train alike; the command lines.

Shapes: the seeded tree and pieces of tests/score_render_si_ref.py at sr = 1000 -- a virtual file is a 2 s chunk, 34 frames
at hop 64 and 6 at hop 512 -- and the hand-built files of tests/test_gpu_score_render.py for 1, 4 and 8 tracks and the frame
of 4096."""
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

import score_render_ref as R  # noqa: E402
import score_render_si_ref as SI  # noqa: E402
import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import _lib, rwc, score_render as sr  # noqa: E402
from deepconvsep_amd.runtime import Context, StftPlan, _ptr, default_context  # noqa: E402
from deepconvsep_amd.score_training import ScoreFeatureWindows, ScoreTrainer, glorot_init, pack_notes  # noqa: E402
from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from score_feed_ref import _note, gather_np  # noqa: E402
from test_gpu_augment import FEED_TOL, SENTINEL  # noqa: E402      the project's float32 feed bound, 2e-5
from test_gpu_score_render import HAND, _feed_windows, _unguard  # noqa: E402

_CACHE = {}


def _inputs(hop, frame):
    """(bank, the nine virtual files of the main piece at this hop and frame), built once per process."""
    if "bank" not in _CACHE:
        import tempfile
        tmp = tempfile.mkdtemp()
        tree = R.write_rwc_tree(os.path.join(tmp, "rwc"))
        _CACHE["db"] = SI.write_pieces(os.path.join(tmp, "db"))
        _CACHE["tree"] = tree
        _CACHE["bank"] = rwc.NoteBank.from_instruments(
            [rwc.Instrument(tree, i, list(R.STYLES), list(R.CASES), list(R.DYNAMICS)) for i in R.INSTRUMENT_IDS])
    if (hop, frame) not in _CACHE:
        every = sr.score_informed_files(SI.piece_dir(_CACHE["db"], R.PIECE), _CACHE["bank"], R.COMBOS, SI.CHUNK, SI.SR, hop, frame)
        assert len(every) == 9
        _CACHE[(hop, frame)] = every
    return _CACHE["bank"], _CACHE[(hop, frame)]


@pytest.fixture(scope="module")
def ctx():
    return default_context()


def _tt(frame, hop, precision='float64'):
    return dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=SI.SR, window=blackmanharris, precision=precision)


_BLOCKS = {}


def _block32(key, frame, hop, bank, sf):
    """The float32 block of ``dcs_stft_forward_score_render_f32`` for one virtual file, computed once and left unchanged."""
    k = (key, frame, hop)
    if k not in _BLOCKS:
        b = sr.render_score_features(_tt(frame, hop, 'float32'), bank, sf)
        b32 = b.astype(np.float32)
        assert np.array_equal(b32.astype(np.float64), b)           # the float32 kernel's values, exactly
        b32.setflags(write=False)
        _BLOCKS[k] = b32
    return _BLOCKS[k]


def _pack_masks(ctx, tables, F):
    packed, mask_files, off = [], [], 0
    for t in tables:
        m = pack_notes(ctx._lib, t, F)
        packed.append(m.ravel())
        mask_files.append((off, t.shape[1]))
        off += m.size
    return np.concatenate(packed + [np.zeros(1, np.int32)]), np.asarray(mask_files, dtype=np.int64).reshape(-1, 2), off


def _raw(ctx, plan, bank_t, bank_len, notes, rows, masks, mask_files, mask_len, width, win, tc, S, scale, guard=0, n_notes=None,
         n_files=None, null=None, other_ctx=None):
    """dcs_trainer_gather_score_informed_render into buffers with ``guard`` sentinel words on either side; rc and the whole
    buffers as uint32."""
    import torch
    B, F = len(win), plan.bins
    n = max(B, 1) * max(S, 1) * max(tc, 1) * F
    with ctx.stream_scope():
        dev = dict(notes=torch.from_numpy(np.ascontiguousarray(notes, dtype=np.int64)).to(ctx.device),
                   rows=torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(ctx.device),
                   masks=torch.from_numpy(np.ascontiguousarray(masks, dtype=np.int32)).to(ctx.device),
                   mask_files=torch.from_numpy(np.ascontiguousarray(mask_files, dtype=np.int64)).to(ctx.device),
                   win=torch.from_numpy(np.ascontiguousarray(win, dtype=np.int32)).to(ctx.device))
        xb = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        tb = torch.full((n + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        p = dict(ctx=ctx._h if other_ctx is None else other_ctx._h, plan=plan._h, bank=_ptr(bank_t), x=xb.data_ptr() + 4 * guard,
                 t=tb.data_ptr() + 4 * guard)
        p.update({k: _ptr(v) for k, v in dev.items()})
        if null is not None:
            p[null] = c_void_p(None)
        rc = ctx._lib.dcs_trainer_gather_score_informed_render(
            p['ctx'], p['plan'], p['bank'], bank_len, p['notes'], len(notes) if n_notes is None else n_notes, p['rows'],
            len(rows) if n_files is None else n_files, p['masks'], mask_len, p['mask_files'], width, p['win'], B, tc, S, scale,
            p['x'], p['t'])
        return rc, xb.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32)


def _composition(ctx, blocks, masks, mask_files, width, win, tc, S, scale):
    """The oracle: ``dcs_trainer_gather_score`` on the resident float32 blocks.  It takes no file count and bounds only
    file < 0: a file past the table is a dead slot for it."""
    import torch
    F = blocks[0].shape[2]
    table, off = [], 0
    for b in blocks:
        table.append((off, b.shape[1]))
        off += b.size
    ref = np.array(win, dtype=np.int32)
    ref[ref[:, 0] >= len(blocks)] = (-1, 0)
    B = len(ref)
    with ctx.stream_scope():
        data_d = torch.from_numpy(np.concatenate([b.ravel() for b in blocks])).to(ctx.device)
        files_d = torch.from_numpy(np.asarray(table, dtype=np.int64)).to(ctx.device)
        masks_d = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.int32)).to(ctx.device)
        mf_d = torch.from_numpy(np.ascontiguousarray(mask_files, dtype=np.int64)).to(ctx.device)
        win_d = torch.from_numpy(ref).to(ctx.device)
        x = torch.empty((B, S, tc, F), dtype=torch.float32, device=ctx.device)
        t = torch.empty((B, S, tc, F), dtype=torch.float32, device=ctx.device)
        _lib.check(ctx._lib.dcs_trainer_gather_score(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(masks_d), _ptr(mf_d), _ptr(win_d),
                                                     B, tc, F, S, width, scale, _ptr(x), _ptr(t)))
        return x.cpu().numpy(), t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(ctx, name, bank, sfiles, tables, frame, hop, tc, win, scale, guard=0):
    """Both sides for the virtual files ``sfiles`` with the mask tables ``tables``; returns (new feed, composition)."""
    S = len(sfiles[0].tracks)
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    F = plan.bins
    notes, rows = sr.pack_tables(sfiles, bank.length, hop)
    masks, mask_files, mask_len = _pack_masks(ctx, tables, F)
    width = tables[0].shape[2]
    rc, xb, tb = _raw(ctx, plan, bank.device(np.float32, ctx), bank.length, notes, rows, masks, mask_files, mask_len, width, win,
                      tc, S, scale, guard)
    _lib.check(rc)
    shape = (len(win), S, tc, F)
    x, t = _unguard(xb, guard, shape), _unguard(tb, guard, shape)
    blocks = [_block32((name, i), frame, hop, bank, sf) for i, sf in enumerate(sfiles)]
    xr, tr = _composition(ctx, blocks, masks, mask_files, width, win, tc, S, scale)
    return (x, t), (xr, tr), [int(r[1]) for r in rows], blocks


def _assert_zero_rows(win, T, tc, x, t):
    for b, (fi, start) in enumerate(win):
        n = 0 if fi < 0 or fi >= len(T) else max(0, min(tc, T[fi] - int(start)))
        assert not x[b, :, n:].any() and not t[b, :, n:].any(), b


# ------------------------------------------------------------------------------------------ (i) the composition, bit for bit
@pytest.mark.parametrize("pitch_code", ['g', 'e'])
@pytest.mark.parametrize("batch", [1, 32])
@pytest.mark.parametrize("scale", [1.0, 0.3])
@pytest.mark.parametrize("frame,hop,tc", [(256, 64, 8), (1024, 512, 4)])
def test_the_feed_equals_the_composition_of_the_existing_entry_points(ctx, frame, hop, tc, scale, batch, pitch_code):
    bank, every = _inputs(hop, frame)
    tables = [sf.melody_g if pitch_code == 'g' else sf.melody_e for sf in every]
    T = [_lib.frame_count(sf.size, hop) for sf in every]
    win = _feed_windows(T, tc, batch)
    (x, t), (xr, tr), T2, _ = _case(ctx, ('main', hop), bank, every, tables, frame, hop, tc, win, scale)
    assert T == T2
    if batch == 32:
        assert (win[:, 0] == -1).any() and (win[:, 0] == len(T)).any() and (win[:, 1] == 0).any()
        assert any(0 <= fi < len(T) and 0 < T[fi] - st < tc for fi, st in win)          # some frames past T
        assert xr.any() and tr.any()
        # the masks do something: the four input rows of a window differ
        assert not np.array_equal(x[0, 0], x[0, 1])
    _assert_zero_rows(win, T, tc, x, t)
    dx, dt = int(np.count_nonzero(_bits(x) != _bits(xr))), int(np.count_nonzero(_bits(t) != _bits(tr)))
    print("si feed (%d, %d) tc %d scale %.1f batch %d %s: differing words inputs %d targets %d"
          % (frame, hop, tc, scale, batch, pitch_code, dx, dt))
    assert dx == 0 and dt == 0


def _random_masks(rs, S, P, width, T, F):
    """A mask table [S, P, width]: random frame spans inside and around [0, T), random bands inside [0, F], some rows with
    MIDI number 0, some bands empty."""
    t = np.zeros((S, P, width))
    for i in range(S):
        for m in range(P):
            a = int(rs.randint(-2, T))
            bands = []
            for _ in range((width - 3) // 2):
                f0 = int(rs.randint(0, F))
                bands.append((f0, min(F, f0 + int(rs.randint(0, 40)))))
            t[i, m] = _note(max(a, 0), a + int(rs.randint(0, 6)), 0 if rs.rand() < 0.15 else 60 + m, bands, width)
    return t


def test_the_feed_equals_the_composition_at_frame_4096(ctx):
    """F = 2049 on the hand-built long file (14 frames): the mixture's flags share the FFT's free buffer."""
    bank, sf = HAND['long']
    frame, hop, tc = 4096, 512, 3
    T = _lib.frame_count(sf.size, hop)
    table = _random_masks(np.random.RandomState(3), 4, 9, 43, T, frame // 2 + 1)
    table[1, 0] = _note(0, T, 64, [(2040, 2049), (0, 1)], 43)                  # a band that ends at F, one at bin 0
    win = np.asarray([(0, 0), (0, T - tc), (0, T - 1), (-1, 0), (1, 0), (0, 5)], dtype=np.int32)
    (x, t), (xr, tr), _, _ = _case(ctx, 'long', bank, [sf], [table], frame, hop, tc, win, 0.3)
    _assert_zero_rows(win, [T], tc, x, t)
    assert x.shape == (6, 4, 3, 2049) and xr.any() and tr.any()
    assert np.array_equal(_bits(x), _bits(xr)) and np.array_equal(_bits(t), _bits(tr))


# ------------------------------------------------------------------------------------------ (ii) hand-built mask tables
def _hand_masks(S, width, F):
    """[S, 4, width], frames 0 .. 7 of a file: frame 0: nobody sounds; frames 1 .. 2: instrument 0 on bins 3 .. 9 (and, width
    permitting, a band that ends at F); frame 2 .. 3: the last instrument on the same bins 3 .. 9; a note with end == 4 and
    one with first == 4 on different bins of instrument 0; a row with MIDI number 0 that the packer drops."""
    t = np.zeros((S, 4, width))
    bands = [(3, 10)] + ([(F - 5, F)] if width >= 7 else [])
    t[0, 0] = _note(1, 3, 60, bands, width)
    t[S - 1, 1] = _note(2, 4, 62, [(3, 10)], width)
    t[0, 2] = _note(3, 4, 64, [(20, 25)], width)          # end == 4: frame 4 is not painted
    t[0, 3] = _note(4, 6, 65, [(30, 35)], width)          # first == 4: frame 4 is painted
    t[S - 1, 0] = _note(0, 8, 0, [(40, 50)], width)       # MIDI 0: dropped by the packer
    if S > 1:
        t[S - 1, 2] = _note(5, 6, 66, [(F - 1, F)], width)   # the last bin alone
    return t


@pytest.mark.parametrize("S,name,width", [(1, 'one', 5), (1, 'one', 43), (4, 'long', 5), (4, 'long', 43), (8, 'eight', 5),
                                         (8, 'eight', 43)])
def test_hand_built_masks(ctx, S, name, width):
    bank, sf = HAND[name]
    assert len(sf.tracks) == S
    frame, hop, tc, scale = 256, 64, 8, 0.3
    F = frame // 2 + 1
    table = _hand_masks(S, width, F)
    win = np.asarray([(0, 0), (0, 3)], dtype=np.int32)
    (x, t), (xr, tr), T, blocks = _case(ctx, name, bank, [sf], [table], frame, hop, tc, win, scale)
    assert T[0] >= 11
    assert np.array_equal(_bits(x), _bits(xr)) and np.array_equal(_bits(t), _bits(tr))
    # the NumPy restatement of the reference's feed on the same float32 block
    xn, tn = gather_np(blocks, [table], win, tc, F, scale)
    assert np.array_equal(_bits(x), _bits(xn)) and np.array_equal(_bits(t), _bits(tn))
    mix = np.float32(scale) * blocks[0][0]
    assert mix[:6].any()
    one, tiny = np.float32(1.0), np.float32(1e-18)

    def share(n_on, on):
        """mask value of an instrument that sounds (on) or not where n_on of the S instruments sound, added in order."""
        tot = np.float32(0)
        vals = [one] * n_on + [tiny] * (S - n_on)
        # the order of the additions matters only through rounding; with values 1 and 1e-18 every order gives the same sum
        for k, v in enumerate(vals):
            tot = v if k == 0 else np.float32(tot + v)
        return np.float32((one if on else tiny) / tot)
    # frame 0: nobody sounds -- every mask is 1 / S up to the float32 sum of S times 1e-18
    for j in range(S):
        assert np.array_equal(x[0, j, 0], share(0, False) * mix[0])
    # frame 1, bins 3 .. 9: instrument 0 alone; the other bins as in frame 0
    assert np.array_equal(x[0, 0, 1, 3:10], share(1, True) * mix[1, 3:10])
    assert np.array_equal(x[0, 0, 1, 10:20], share(0, False) * mix[1, 10:20])
    if S > 1:
        assert np.array_equal(x[0, S - 1, 1, 3:10], share(1, False) * mix[1, 3:10])
        # frame 2: instrument 0 and the last one on the same bins
        assert np.array_equal(x[0, 0, 2, 3:10], share(2, True) * mix[2, 3:10])
        assert np.array_equal(x[0, S - 1, 2, 3:10], share(2, True) * mix[2, 3:10])
        assert np.array_equal(x[0, 1, 2, 3:10], share(2, False) * mix[2, 3:10])
        # the last bin alone, frame 5
        assert np.array_equal(x[0, S - 1, 5, F - 1:], share(1, True) * mix[5, F - 1:])
        assert np.array_equal(x[0, S - 1, 5, F - 2:F - 1], share(0, False) * mix[5, F - 2:F - 1])
    if width >= 7:                                  # a band that ends at F
        assert np.array_equal(x[0, 0, 1, F - 5:], share(1, True) * mix[1, F - 5:])
    # end == 4 is excluded, first == 4 is included (window 0 frame 4 = window 1 frame 1)
    assert np.array_equal(x[0, 0, 3, 20:25], share(1, True) * mix[3, 20:25])
    assert np.array_equal(x[0, 0, 4, 20:25], share(0, False) * mix[4, 20:25])
    assert np.array_equal(x[0, 0, 4, 30:35], share(1, True) * mix[4, 30:35])
    assert np.array_equal(x[1, 0, 1, 30:35], x[0, 0, 4, 30:35]) and np.array_equal(x[1, :, :5], x[0, :, 3:])
    # the row with MIDI number 0 paints nothing
    assert np.array_equal(x[0, S - 1, 0, 40:50], share(0, False) * mix[0, 40:50])
    # the targets are the render feed's
    assert np.array_equal(t[0, :, :8], np.float32(scale) * blocks[0][1:, :8])


# ------------------------------------------------------------------------------------------ (iii) the device tables are bounded
def bounded_calls(out_path=None):
    """A mask offset past the given length paints nothing; a render note index past n_notes is a silent track; in both cases
    nothing outside the outputs is written.  Also the body of the guard-band child process."""
    ctx = default_context()
    bank, sf = HAND['long']
    frame, hop, tc, scale, guard, S = 256, 64, 8, 0.3, 4096, 4
    F = frame // 2 + 1
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    notes, rows = sr.pack_tables([sf], bank.length, hop)
    table = _hand_masks(S, 43, F)
    masks, mask_files, mask_len = _pack_masks(ctx, [table], F)
    win = np.asarray([(0, 0), (0, 30)], dtype=np.int32)
    b32 = bank.device(np.float32, ctx)
    shape = (2, S, tc, F)

    def call(**kw):
        a = dict(notes=notes, rows=rows, mask_files=mask_files, mask_len=mask_len, n_notes=None)
        a.update(kw)
        rc, xb, tb = _raw(ctx, plan, b32, bank.length, a['notes'], a['rows'], masks, a['mask_files'], a['mask_len'], 43, win, tc,
                          S, scale, guard, n_notes=a['n_notes'])
        assert rc == _lib.DCS_OK
        return _unguard(xb, guard, shape), _unguard(tb, guard, shape)
    x, t = call()
    # no mask table at all: what every out-of-range table must give
    none = np.zeros((S, 1, 43))
    m0, f0, l0 = _pack_masks(ctx, [none], F)
    rc, xb, tb = _raw(ctx, plan, b32, bank.length, notes, rows, m0, f0, l0, 43, win, tc, S, scale, guard)
    x_none, t_none = _unguard(xb, guard, shape), _unguard(tb, guard, shape)
    assert rc == _lib.DCS_OK and not np.array_equal(x, x_none) and np.array_equal(t, t_none)
    outs = [x, t]
    for bad in (dict(mask_files=np.asarray([[mask_len, 4]], dtype=np.int64)),           # begins at the end
                dict(mask_files=np.asarray([[1, 4]], dtype=np.int64)),                  # its last int lies past the length
                dict(mask_files=np.asarray([[-8, 4]], dtype=np.int64)),
                dict(mask_files=np.asarray([[0, -1]], dtype=np.int64)),
                dict(mask_files=np.asarray([[0, 1 << 40]], dtype=np.int64)),
                dict(mask_len=mask_len - 1), dict(mask_len=0)):
        xb_, tb_ = call(**bad)
        assert np.array_equal(_bits(xb_), _bits(x_none)) and np.array_equal(_bits(tb_), _bits(t)), bad
    # a render note index past n_notes: track 2 is silent (zero targets), the mixture is what the other tracks give
    bad_rows = rows.copy()
    bad_rows[0, 2 + 2 * 2] = len(notes)
    xs, ts = call(rows=bad_rows)
    assert not ts[:, 2].any() and np.array_equal(ts[:, 0], t[:, 0]) and np.isfinite(xs).all()
    xs2, ts2 = call(n_notes=int(rows[0, 2 + 2 * 3]))          # the table declared shorter: track 3 lies outside it
    assert not ts2[:, 3].any() and np.array_equal(ts2[:, :3], t[:, :3])
    silent = sf._replace(tracks=sf.tracks[:3] + ((),))
    n3, r3 = sr.pack_tables([silent], bank.length, hop)
    x3, t3 = call(notes=n3, rows=r3)
    assert np.array_equal(_bits(xs2), _bits(x3)) and np.array_equal(_bits(ts2), _bits(t3))
    outs += [xs, ts, xs2, ts2]
    if out_path is not None:
        n = ctx.check_guards()
        assert n > 0
        np.save(out_path, np.concatenate([o.ravel() for o in outs]))


def test_the_feed_bounds_its_device_tables(ctx):
    bounded_calls()


_GUARD_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_score_render_si as T
T.bounded_calls(sys.argv[2])
"""


def test_guard_harness_reports_no_damage(tmp_path):
    env = dict(os.environ, DCS_WS_GUARD="4096")
    dst = str(tmp_path / "out.npy")
    rc = subprocess.run([sys.executable, "-c", _GUARD_CHILD, ROOT, dst], env=env, timeout=300, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-3000:]
    assert np.isfinite(np.load(dst)).all()


# ------------------------------------------------------------------------------------------ (iv) validation
def test_the_entry_point_rejects_bad_arguments(ctx):
    bank, sf = HAND['long']
    frame, hop, F = 256, 64, 129
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    notes, rows = sr.pack_tables([sf], bank.length, hop)
    masks, mask_files, mask_len = _pack_masks(ctx, [_hand_masks(4, 43, F)], F)
    win = np.asarray([(0, 0)], dtype=np.int32)
    b32 = bank.device(np.float32, ctx)

    def call(S=4, tc=8, width=43, bank_len=bank.length, win=win, **kw):
        rc, xb, tb = _raw(ctx, plan, b32, bank_len, notes, rows, masks, mask_files, mask_len, width, win, tc, S, 0.3, 16, **kw)
        if rc != _lib.DCS_OK:
            assert (xb == SENTINEL).all() and (tb == SENTINEL).all()           # a rejected call launches nothing
        return rc
    assert call() == _lib.DCS_OK
    for null in ('ctx', 'plan', 'bank', 'notes', 'rows', 'masks', 'mask_files', 'win', 'x', 't'):
        assert call(null=null) == _lib.DCS_EINVAL, null
    assert call(other_ctx=Context()) == _lib.DCS_EINVAL                     # the plan belongs to ctx
    for S in (0, 9, -1):
        assert call(S=S) == _lib.DCS_EINVAL, S
    for width in (4, 3, 0, -1, 6, 44, 42):
        assert call(width=width) == _lib.DCS_EINVAL, width
    assert call(win=np.zeros((0, 2), np.int32)) == _lib.DCS_EINVAL            # batch 0
    assert call(tc=0) == _lib.DCS_EINVAL
    assert call(n_files=0) == _lib.DCS_EINVAL
    assert call(bank_len=0) == _lib.DCS_EINVAL
    assert call(n_notes=-1) == _lib.DCS_EINVAL
    assert call(width=5) == _lib.DCS_OK          # a narrower reading of the same ints: in bounds, defined


# ------------------------------------------------------------------------------------------ (v) files
@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "score_render_si.npz"))


def test_render_score_informed_features_writes_what_the_reference_writes(ctx, g, tmp_path):
    """The golden pairs at frame 256 / hop 50: the block is the existing float64 transform of the reference's audio bit for bit,
    the tables are the reference's, and ScoreFeatureWindows loads the files."""
    bank, _ = _inputs(64, 256)
    tt = _tt(SI.FRAME, SI.HOP)
    for k, (piece, style, ci, chnk) in enumerate(SI.RENDERS):
        sfs = sr.score_informed_files(SI.piece_dir(_CACHE["db"], piece), bank, [R.COMBOS[ci]], SI.CHUNK, SI.SR, SI.HOP, SI.FRAME,
                                      SI.STYLE_MIDI[style])
        sf = sfs[chnk]
        out_dir = str(tmp_path / piece / style)
        path = sr.render_score_informed_features(tt, bank, sf, out_dir)
        stem = bytes(g["stem_%d" % k]).decode('ascii')
        assert path == os.path.join(str(tmp_path), stem + "__m_.data")
        want = tt.compute_transform(np.ascontiguousarray(g["audio_%d" % k]), phase=False, save=False)
        shape = tt.get_shape(path.replace('.data', '.shape'))
        assert shape == want.shape == (5, _lib.frame_count(sf.size, SI.HOP), SI.FRAME // 2 + 1)
        assert np.array_equal(np.fromfile(path).reshape(shape).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
        for code in ('g', 'e'):
            q = path.replace('__m_', '__%s_' % code)
            tshape = tt.get_shape(q.replace('.data', '.shape'))
            assert np.array_equal(np.fromfile(q).reshape(tshape), g["melody_%s_%d" % (code, k)])
        block, mg, me = sr.render_score_informed_features(tt, bank, sf)
        assert np.array_equal(block, want) and np.array_equal(mg, sf.melody_g) and np.array_equal(me, sf.melody_e)
    d = str(tmp_path / R.PIECE / 'original')
    fw = ScoreFeatureWindows([d], 'e', 8, 3, 0.3, 'reference', 2, 0, ctx)
    assert len(fw.pairs) == 3 and fw.F == SI.FRAME // 2 + 1 and fw.width == 43
    x, t = fw.gather([0, 1])
    assert tuple(x.shape) == (2, 4, 8, 129) and bool(x.any()) and bool(t.any())


# ------------------------------------------------------------------------------------------ (vi) end to end, tiny
def test_end_to_end_files_and_rendered_windows_train_alike(ctx, tmp_path):
    """Three ScoreTrainer steps, B = 2, tc = 30, frame 256 (F = 129), on the files just written and on rendered windows."""
    frame, hop, tc, ov, B, scale = 256, 64, 30, 25, 2, 0.3
    bank, every = _inputs(hop, frame)
    tt = _tt(frame, hop)
    paths = [sr.render_score_informed_features(tt, bank, sf, str(tmp_path)) for sf in every]
    assert len(set(paths)) == 9
    fw = ScoreFeatureWindows(sorted(paths), 'e', tc, ov, scale, 'reference', B, 0, ctx)
    # ScoreFeatureWindows sorts its files by name; the rendered windows keep the order they were given
    order = [paths.index(p) for p, _ in fw.pairs]
    rw = sr.ScoreInformedRenderedWindows(bank, [every[i] for i in order], 'e', time_context=tc, overlap=ov, mult_factor=scale,
                                         windows='reference', batch_size=B, seed=0, ctx=ctx, frameSize=frame, hopSize=hop,
                                         window=blackmanharris)
    assert rw.pitch_code == 'e' and np.array_equal(fw.table, rw.table)
    assert (fw.F, fw.total, fw.iteration_size) == (rw.F, rw.total, rw.iteration_size) and rw.F == 129 and rw.iteration_size >= 3
    params = glorot_init(tc, rw.F, seed=1)
    first = []
    for data in (fw, rw):
        tr = ScoreTrainer(ctx, params=params, batch_size=B, time_context=tc, feat_size=rw.F, seed=1)
        losses = []
        for k, (x, t) in enumerate(data.batches(0)):
            if k == 3:
                break
            assert tuple(x.shape) == tuple(t.shape) == (B, 4, tc, rw.F)
            if data is rw:
                xf, tf = fw.gather(np.random.RandomState(0).permutation(fw.total)[k * B:(k + 1) * B])
                ex, et = float((x - xf).abs().max()), float((t - tf).abs().max())
                print("end to end batch %d: inputs %.3e targets %.3e" % (k, ex, et))
                assert ex <= FEED_TOL * scale and et <= FEED_TOL * scale
            if k == 0:
                n_t = t.numel()
            losses.append(tr.step(x, t))
        assert len(losses) == 3 and np.isfinite(losses).all()
        first.append(losses[0])
        tr.close()
    # The bound of tests/test_gpu_score_render.py::test_end_to_end_files_and_rendered_windows_train_alike, for the same reason
    # (float64 files cast to float32 against a float32 bank): every input and target element moves by at most delta =
    # FEED_TOL * scale, the masked prediction by at most K = 10 times as much in norm, so
    # |dL| / L <= 2 (1 + K) delta sqrt(n) / sqrt(L).
    delta, K = FEED_TOL * scale, 10.0
    margin = 2 * (1 + K) * delta * np.sqrt(n_t) / np.sqrt(first[0])
    rel = abs(first[0] - first[1]) / first[0]
    print("first losses %.9g (files) %.9g (rendered): relative difference %.3e, margin %.3e" % (first[0], first[1], rel, margin))
    assert first[0] > 0 and rel <= margin


def _load(script):
    import importlib.util
    spec = importlib.util.spec_from_file_location(os.path.basename(script)[:-3] + "_si", os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_lines_write_the_files_and_train_without_them(ctx, tmp_path):
    """compute_features_rwc.py writes what render_score_informed_features gives for the files of si_dataset_files;
    train_bach10_si.py --render runs two batches from the trees alone."""
    tree = R.write_rwc_tree(str(tmp_path / "rwc"))
    db = str(tmp_path / "db")
    R.write_scores(db)
    os.makedirs(os.path.join(db, "notes"))                       # no digit in front: not a piece
    out = str(tmp_path / "features")
    common = ["--rwc", tree, "--chunk_size", "2", "--sample_size", "2", "--seed", "4", "--sample_rate", str(SI.SR)]
    _load("examples/bach10_scoreinformed/compute_features_rwc.py").main(["--db", db, "--feature_path", out] + common)
    bank = sr.load_bank(tree)
    ((piece, style, sfiles),) = sr.si_dataset_files(db, bank, 2.0, 2, True, 4, SI.SR)
    assert (piece, style) == (R.PIECE, 'original') and len(sfiles) == 6
    tt = _tt(4096, 512)
    d = os.path.join(out, R.PIECE, 'original')
    assert sorted(os.listdir(d)) == sorted(sf.name + e for sf in sfiles for e in
                                           ("__m_.data", "__m_.shape", "__g_.data", "__g_.shape", "__e_.data", "__e_.shape"))
    want, mg, me = sr.render_score_informed_features(tt, bank, sfiles[3])
    shape = tt.get_shape(os.path.join(d, sfiles[3].name + "__m_.shape"))
    assert shape == want.shape == (5, _lib.frame_count(sfiles[3].size, 512), 2049)
    assert np.array_equal(np.fromfile(os.path.join(d, sfiles[3].name + "__m_.data")).reshape(shape), want)
    assert np.array_equal(np.fromfile(os.path.join(d, sfiles[3].name + "__e_.data")).reshape(me.shape), me)
    # training: 6 virtual files of 6 frames at hop 512, windows of 4 frames, two batches of 3
    sources = str(tmp_path / "sources")
    os.makedirs(os.path.join(sources, R.PIECE))
    outdir = str(tmp_path / "out")
    os.makedirs(outdir)
    _load("examples/bach10_scoreinformed/train_bach10_si.py").main(
        ["--db", sources, "--dbs", db, "--output", outdir, "--model", "m", "--render", "--frame_size", "1024", "--batch_size", "3",
         "--time_context", "4", "--overlap", "2", "--nepochs", "1", "--skip_sep", "--branches", "1"] + common)
    from deepconvsep_amd.separation import load_model
    model = load_model(os.path.join(outdir, "models", "model_m_gt.pkl"))
    assert len(model) == 11 and all(np.isfinite(p).all() for p in model)
