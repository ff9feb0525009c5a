"""The rendered STFT on the MI355X (csrc/fft_render.hip): ``dcs_stft_forward_render_f64`` bit for bit against the existing
float64 kernel on host-rendered audio (tests/augment_ref.py) and within 1e-11 of the reference's own blocks
(tests/golden/augment_cs.npz); ``dcs_trainer_gather_render`` against ``dcs_trainer_gather`` on those float64 blocks cast to
float32, the path ``FeatureWindows`` serves today; both under the guard-band harness; the hiphop command lines end to end.

Shapes: frame / hop (1024, 512) and (256, 64), sources of 3 000 - 7 000 samples, chunks of 2 048 samples at sr = 1000 -- a
file has up to three chunks and a rest -- the smallest at which every bound of the loader (chunk, rendered length, source
length) falls inside a frame."""
import importlib.util
import os
import shutil
import subprocess
import sys
from ctypes import POINTER, c_double, c_int64

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

import augment_ref  # noqa: E402
import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd import _lib, augment  # noqa: E402
from deepconvsep_amd.augment import Track, VirtualFile  # noqa: E402
from deepconvsep_amd.runtime import StftPlan, _ptr, default_context  # noqa: E402
from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from deepconvsep_amd.synth import synth_audio  # noqa: E402

SR, CHUNK = 1000, 2048
FRAMES = [(1024, 512), (256, 64)]
SENTINEL = 0x5CA1AB1E      # a finite float32 bit pattern no product of the feed gives
# the float32 STFT kernel's bound on inputs of this amplitude (tests/test_gpu_parity.py::test_compute_file_matches_reference)
FEED_TOL = 2e-5


def _signals():
    """Song A: sources of four lengths; songs B, C, D for the four-song mixture.  synth_audio * 0.25: a mixture of four
    stays in the amplitude range the STFT bounds were established for."""
    lengths = {('A', 'vocals'): 7000, ('A', 'bass'): 6000, ('A', 'drums'): 5000, ('A', 'other'): 3000,
               ('B', 'bass'): 4500, ('C', 'drums'): 6100, ('D', 'other'): 5203, ('B', 'vocals'): 4099}
    return {k: synth_audio(L, seed=20 + i) * 0.25 for i, (k, L) in enumerate(sorted(lengths.items()))}


def _vf(tracks, m, size, rest=True):
    chunks = augment.chunk_bounds(size, SR, rest, CHUNK)
    return VirtualFile(tuple(tracks), float(m), int(size), tuple(chunks), tuple("f_%d" % i for i in range(len(chunks))))


def _cases():
    """name -> (virtual file, bit-exact against the host render?).  Gains in {0, 1} and m in {1, 1/4} are the only values
    the reference uses; every product is exact for them."""
    A = lambda s: ('A', s)  # noqa: E731
    ln = {s: n for s, n in (('vocals', 7000), ('bass', 6000), ('drums', 5000), ('other', 3000))}
    cs = augment.virtual_files('cs', ln, sr=SR, chunk=CHUNK, song='A')
    instr = augment.virtual_files('instr', ln, sr=SR, chunk=CHUNK, song='A')
    return {
        # shift 0, size = len(other) = 3000: every other source is longer than the rendered signal
        'plain': (augment.virtual_files('none', ln, sr=SR, chunk=CHUNK, song='A')[0], True),
        # +200 on bass and other; size 6800 is no multiple of either hop; bass, drums and other end before `size`, vocals
        # go on after it; chunks 1 and 2 have song on both sides; the rest chunk (656) is shorter than a 1024 frame
        'cs_0101': (cs[4], True),
        'cs_1000': (cs[7], True),
        # a negative, an odd positive, no shift, and a shift past `size`: an all-zero channel that still counts in the sum
        'odd': (_vf([Track(A('vocals'), -333, 1.0, 1), Track(A('bass'), 77, 1.0, 2), Track(A('drums'), 0, 1.0, 3),
                     Track(A('other'), 9001, 1.0, 4)], 1.0, 6500), True),
        # drums muted, mixture / 4, targets unscaled
        'muted': (instr[1], True),
        # four songs of four lengths, whole blocks only, mixture / 4
        'four_songs': (_vf([Track(('B', 'bass'), 0, 1.0, 2), Track(('C', 'drums'), 0, 1.0, 3), Track(('D', 'other'), 0, 1.0, 4),
                            Track(('B', 'vocals'), 0, 1.0, 1)], 0.25, 4099, rest=False), True),
        # a rest of 300 samples: fewer frames than any time context used below
        'short_rest': (_vf([Track(A('bass'), 0, 1.0, 2), Track(A('drums'), -1, 1.0, 3), Track(A('other'), 1, 1.0, 4),
                            Track(A('vocals'), 0, 1.0, 1)], 1.0, CHUNK + 300), True),
        # gains whose products round: within 1e-11 of the oracle only
        'gains': (_vf([Track(A('vocals'), 0, 0.5, 1), Track(A('bass'), 13, 0.3, 2), Track(A('drums'), -6, 0.3, 3),
                       Track(A('other'), 0, 0.5, 4)], 1.0, 5000), False),
    }


CASES = _cases()


@pytest.fixture(scope="module")
def ctx():
    return default_context()


@pytest.fixture(scope="module")
def signals():
    return _signals()


@pytest.fixture(scope="module")
def bank64(ctx, signals):
    return augment.Bank(signals, np.float64, ctx)


@pytest.fixture(scope="module")
def blocks64(ctx, bank64):
    """(frame, hop, case) -> the float64 blocks of the device render, computed once and shared."""
    cache = {}

    def get(frame, hop, name):
        key = (frame, hop, name)
        if key not in cache:
            tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=SR, window=blackmanharris)
            cache[key] = augment.render_features(tt, bank64, CASES[name][0])
        return cache[key]
    return get


def _host_render(signals, vf):
    return augment_ref.render([(signals[t.signal], t.k, t.g, t.c) for t in vf.tracks], vf.m, vf.size)


# ------------------------------------------------------------------------------------------ 1. float64, the file path
@pytest.mark.parametrize("frame,hop", FRAMES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_render_f64_equals_the_existing_kernel_on_host_rendered_audio(signals, blocks64, name, frame, hop):
    vf, exact = CASES[name]
    got = blocks64(frame, hop, name)
    rendered = _host_render(signals, vf)
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=SR, window=blackmanharris)
    want_np = augment_ref.blocks_np(rendered, vf.chunks, frame, hop, blackmanharris(frame))
    assert len(got) == len(vf.chunks) == len(want_np)
    worst = 0.0
    for (a, Lc), g, w in zip(vf.chunks, got, want_np):
        assert g.shape == w.shape == (5, _lib.frame_count(Lc, hop), frame // 2 + 1) and g.dtype == np.float64
        worst = max(worst, float(np.max(np.abs(g - w))))
        if exact:
            dev = tt.compute_transform(augment_ref.chunk_audio(rendered, a, Lc), phase=False, save=False)
            assert np.array_equal(g.view(np.uint64), np.ascontiguousarray(dev).view(np.uint64)), (name, a, Lc)
    print("render f64 %s (%d, %d): max |device - oracle| = %.3e" % (name, frame, hop, worst))
    assert worst < 1e-11           # the float64 STFT's bound in tests/test_gpu_parity.py


def test_cases_cover_the_loader_bounds(signals):
    """The shapes above are only worth their time if they reach every bound; this pins them."""
    ks = [t.k for n in CASES for t in CASES[n][0].tracks]
    assert 0 in ks and any(k > 0 for k in ks) and any(k < 0 for k in ks) and any(k % 2 for k in ks)
    odd = CASES['odd'][0]
    assert odd.tracks[3].k > odd.size and not _host_render(signals, odd)[4].any()
    cs = CASES['cs_0101'][0]
    assert cs.size % 512 and cs.size % 64 and len(cs.chunks) == 4 and cs.chunks[3][1] < 1024
    lens = [len(signals[t.signal]) for t in cs.tracks]
    assert min(lens) < cs.size < max(lens)
    r = _host_render(signals, cs)
    a, Lc = cs.chunks[1]
    assert r[0, a - 1] != 0 and r[0, a + Lc] != 0                     # song on both sides of an inner chunk
    assert 0.0 in [t.g for t in CASES['muted'][0].tracks] and CASES['muted'][0].m == 0.25
    assert len(set(len(signals[t.signal]) for t in CASES['four_songs'][0].tracks)) == 4


@pytest.mark.parametrize("tag", ["a", "b"])
def test_render_f64_against_the_reference_blocks(ctx, tag):
    """The reference's own render and chunk lines (compute_features_cs_aug.py:92-147 at 25 Hz, so that its 30 s chunk is 750
    samples) transformed by its stft_norm: within 1e-11, and bit for bit against the existing kernel on the reference's
    rendered audio."""
    g = np.load(os.path.join(HERE, "golden", "augment_cs.npz"))
    sr, c, size = int(g["sr"]), g[tag + "_c"], int(g[tag + "_size"])
    frame, hop = (int(v) for v in g[tag + "_frame_hop"])
    src = {('song', s): g["src_" + s] for s in augment.CHANNELS}
    tracks = tuple(Track(('song', s), augment.shift_samples(c[j, 0], sr), float(c[j, 1]), 1 + j)
                   for j, s in enumerate(augment.ADD_ORDER['cs']))
    chunks = tuple(augment.chunk_bounds(size, sr))
    vf = VirtualFile(tracks, 1.0, size, chunks, tuple("g_%d" % i for i in range(len(chunks))))
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=sr, window=blackmanharris)
    got = augment.render_features(tt, augment.Bank(src, np.float64, ctx), vf)
    assert [Lc for _, Lc in chunks] == list(g[tag + "_chunk_lengths"])
    for i, ((a, Lc), b) in enumerate(zip(chunks, got)):
        want = g["%s_block_%d" % (tag, i)]
        assert b.shape == want.shape
        err = float(np.max(np.abs(b - want)))
        print("golden %s chunk %d: %.3e" % (tag, i, err))
        assert err < 1e-11
        dev = tt.compute_transform(augment_ref.chunk_audio(g[tag + "_rendered"], a, Lc), phase=False, save=False)
        assert np.array_equal(b, dev)


def test_render_features_writes_the_reference_files(ctx, bank64, blocks64, tmp_path):
    frame, hop = 256, 64
    vf = CASES['cs_0101'][0]
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=SR, window=blackmanharris)
    paths = augment.render_features(tt, bank64, vf, str(tmp_path))
    assert [os.path.basename(p) for p in paths] == [n + "__m_.data" for n in vf.names]
    for p, b in zip(paths, blocks64(frame, hop, 'cs_0101')):
        shape = tt.get_shape(p.replace('.data', '.shape'))
        assert shape == b.shape and np.array_equal(np.fromfile(p).reshape(shape), b)


# ------------------------------------------------------------------------------------------ 2. float32, the feed
def _feed_files(frame, hop):
    """The (case, chunk) pairs that stand for .data files, as virtual files of one chunk each."""
    out = []
    for name in ('cs_0101', 'odd', 'muted', 'four_songs', 'short_rest', 'plain'):
        vf = CASES[name][0]
        out += [(name, i) for i in range(len(vf.chunks))]
    return out


def _feed_windows(files, rows, tc, batch):
    """(file, first frame) windows: from frame 0, ending exactly at T, running past T, a zero slot, a file shorter than tc,
    windows of different files and chunks; cycled to ``batch``."""
    T = [int(r[3]) for r in rows]
    longest = int(np.argmax(T))
    short = [i for i, t in enumerate(T) if t < tc]
    assert short and T[longest] > tc
    base = [(longest, 0), (longest, T[longest] - tc), (longest, T[longest] - tc + 3), (-1, 0), (short[0], 0)]
    for i in range(len(files)):
        base.append((i, (3 * i) % max(1, T[i] - 1)))
    return np.asarray([base[i % len(base)] for i in range(batch)], dtype=np.int32)


def _raw_feed(ctx, plan, bank_t, bank_len, rows, gains, win, tc, S, scale, guard=0):
    """dcs_trainer_gather_render into buffers with ``guard`` sentinel words on either side; returns rc and the whole buffers."""
    import torch
    B, F = len(win), plan.bins
    nx, nt = B * tc * F, B * max(S, 1) * tc * F
    with ctx.stream_scope():
        rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(ctx.device)
        gains_d = torch.from_numpy(np.ascontiguousarray(gains, dtype=np.float64)).to(ctx.device)
        win_d = torch.from_numpy(np.ascontiguousarray(win, dtype=np.int32)).to(ctx.device)
        xb = torch.full((nx + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        tb = torch.full((nt + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        rc = ctx._lib.dcs_trainer_gather_render(ctx._h, plan._h, _ptr(bank_t), bank_len, _ptr(rows_d), _ptr(gains_d), len(rows),
                                                _ptr(win_d), B, tc, S, scale, xb.data_ptr() + 4 * guard,
                                                tb.data_ptr() + 4 * guard)
        return rc, xb.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32)


def _unguard(buf, guard, shape):
    assert (buf[:guard] == SENTINEL).all() and (buf[len(buf) - guard:] == SENTINEL).all(), "the margins were written"
    return buf[guard:len(buf) - guard].view(np.float32).reshape(shape)


def _feed_case(ctx, signals, blocks64, frame, hop, tc, batch, scale, guard=0):
    import torch
    files = _feed_files(frame, hop)
    vfs = [CASES[n][0]._replace(chunks=(CASES[n][0].chunks[i],), names=("x",)) for n, i in files]
    bank = augment.Bank(signals, np.float32, ctx)
    rows, gains = augment.table_rows(vfs, bank.index, hop)
    win = _feed_windows(files, rows, tc, batch)
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    rc, xb, tb = _raw_feed(ctx, plan, bank.tensor, bank.length, rows, gains, win, tc, 4, scale, guard)
    _lib.check(rc)
    F = plan.bins
    x, t = _unguard(xb, guard, (batch, 1, tc, F)), _unguard(tb, guard, (batch, 4, tc, F))
    # the parent's feed: the float64 blocks cast to float32, resident, cut by dcs_trainer_gather
    blocks = [blocks64(frame, hop, n)[i].astype(np.float32) for n, i in files]
    table, off = [], 0
    for b in blocks:
        table.append((off, b.shape[1]))
        off += b.size
    with ctx.stream_scope():
        data_d = torch.from_numpy(np.concatenate([b.ravel() for b in blocks])).to(ctx.device)
        files_d = torch.from_numpy(np.asarray(table, dtype=np.int64)).to(ctx.device)
        win_d = torch.from_numpy(win).to(ctx.device)
        xr = torch.empty((batch, 1, tc, F), dtype=torch.float32, device=ctx.device)
        tr = torch.empty((batch, 4, tc, F), dtype=torch.float32, device=ctx.device)
        _lib.check(ctx._lib.dcs_trainer_gather(ctx._h, _ptr(data_d), _ptr(files_d), _ptr(win_d), batch, tc, F, scale, _ptr(xr),
                                               _ptr(tr)))
        xr, tr = xr.cpu().numpy(), tr.cpu().numpy()
    return rows, win, (x, t), (xr, tr)


@pytest.mark.parametrize("batch", [1, 32])
@pytest.mark.parametrize("scale", [1.0, 0.3])
@pytest.mark.parametrize("frame,hop,tc", [(1024, 512, 4), (256, 64, 8)])
def test_gather_render_against_gather_on_the_float64_blocks(ctx, signals, blocks64, frame, hop, tc, scale, batch):
    rows, win, (x, t), (xr, tr) = _feed_case(ctx, signals, blocks64, frame, hop, tc, batch, scale)
    ex, et = float(np.max(np.abs(x - xr))), float(np.max(np.abs(t - tr)))
    print("feed (%d, %d) tc %d scale %.1f batch %d: max error inputs %.3e targets %.3e (bound %.1e)"
          % (frame, hop, tc, scale, batch, ex, et, FEED_TOL * scale))
    assert xr.any() and tr.any()
    for b, (fi, start) in enumerate(win):
        n = 0 if fi < 0 else max(0, min(tc, int(rows[fi][3]) - int(start)))
        assert not x[b, :, n:].any() and not t[b, :, n:].any(), b       # zero slots and frames past T: exactly zero
        assert not xr[b, :, n:].any() and not tr[b, :, n:].any(), b
    assert ex <= FEED_TOL * scale and et <= FEED_TOL * scale


# ------------------------------------------------------------------------------------------ 3. guard bands
def _raw_render(ctx, plan, bank_t, bank_len, tracks, gains, size, chunks, guard=0, S=None, out_rows=None, f64=True):
    """dcs_stft_forward_render into a buffer with ``guard`` sentinel words on either side; (rc, buffer as uint32, frames)."""
    import torch
    S = len(tracks) if S is None else S
    tracks = np.ascontiguousarray(tracks, dtype=np.int64)
    gains = np.ascontiguousarray(gains, dtype=np.float64)
    chunks = np.ascontiguousarray(chunks, dtype=np.int64).reshape(-1, 2)
    frames = [_lib.frame_count(max(int(Lc), 0), plan.hop) for _, Lc in chunks]
    rows = (1 + max(S, 0)) * sum(frames) if out_rows is None else out_rows
    words = 2 if f64 else 1
    got = (c_int64 * max(len(chunks), 1))()
    with ctx.stream_scope():
        buf = torch.full((rows * plan.bins * words + 2 * guard,), SENTINEL, dtype=torch.int32, device=ctx.device)
        fn = ctx._lib.dcs_stft_forward_render_f64 if f64 else ctx._lib.dcs_stft_forward_render_f32
        rc = fn(plan._h, _ptr(bank_t), bank_len, S, tracks.ctypes.data_as(POINTER(c_int64)),
                gains.ctypes.data_as(POINTER(c_double)), int(size), chunks.ctypes.data_as(POINTER(c_int64)), len(chunks),
                buf.data_ptr() + 4 * guard, plan.bins, rows, got)
        return rc, buf.cpu().numpy().view(np.uint32), list(got)[:len(chunks)]


def guarded_calls(out_path):
    """Body of the guard-band child process: one render call and one feed call with poisoned margins around the outputs."""
    ctx = default_context()
    signals = _signals()
    guard = 4096
    frame, hop = 256, 64
    vf = CASES['odd'][0]
    bank = augment.Bank(signals, np.float64, ctx)
    plan = StftPlan(ctx, frame, hop, blackmanharris(frame))
    tracks = [list(bank.index[t.signal]) + [t.k, t.c] for t in vf.tracks]
    rc, buf, frames = _raw_render(ctx, plan, bank.tensor, bank.length, tracks, [vf.m] + [t.g for t in vf.tracks], vf.size,
                                  vf.chunks, guard)
    _lib.check(rc)
    assert (buf[:guard] == SENTINEL).all() and (buf[len(buf) - guard:] == SENTINEL).all(), "render wrote its margins"
    got = buf[guard:len(buf) - guard].view(np.float64)
    tt = dcs.transformFFT(frameSize=frame, hopSize=hop, sampleRate=SR, window=blackmanharris)
    want = np.concatenate([b.ravel() for b in augment.render_features(tt, bank, vf)])
    assert np.array_equal(got, want) and not np.isnan(got).any()
    cache = {}

    def blocks64(fr, hp, name):
        if name not in cache:
            cache[name] = augment.render_features(tt, bank, CASES[name][0])
        return cache[name]
    _, _, (x, t), (xr, tr) = _feed_case(ctx, signals, blocks64, frame, hop, 8, 32, 0.3, guard)
    assert np.max(np.abs(x - xr)) <= FEED_TOL * 0.3 and np.max(np.abs(t - tr)) <= FEED_TOL * 0.3
    n = ctx.check_guards()
    assert n > 0
    np.save(out_path, np.concatenate([got.astype(np.float32), x.ravel(), t.ravel()]))


_GUARD_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_augment as T
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
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------ 4. end to end, tiny
def _load(script):
    spec = importlib.util.spec_from_file_location(os.path.basename(script)[:-3] + "_hh", os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_db(db):
    from deepconvsep_amd.separation import write_wav
    for i, song in enumerate(("s1", "s2", "s3", "s4")):
        os.makedirs(os.path.join(db, "Mixtures", "Dev", song))
        d = os.path.join(db, "Sources", "Dev", song)
        os.makedirs(d)
        for j, s in enumerate(augment.CHANNELS):
            write_wav(os.path.join(d, s + ".wav"), synth_audio(3000 + 417 * ((i + j) % 4) + 50 * i, seed=40 + 4 * i + j) * 0.25, SR)


def test_end_to_end_files_and_rendered_windows_train_alike(ctx, tmp_path):
    from deepconvsep_amd.training import FeatureWindows, Trainer, glorot_init
    db = str(tmp_path / "db")
    _write_db(db)
    frame, hop, tc, ov, B, scale = 256, 64, 8, 5, 32, 0.3
    common = ["--db", db, "--augment", "cs", "--frameSize", str(frame), "--hopSize", str(hop), "--sample_rate", str(SR),
              "--chunk", str(CHUNK)]
    _load("examples/hiphopss/compute_features.py").main(common)
    signals, vfiles, _ = augment.dataset_signals(db, 'cs', SR, CHUNK)
    assert len(vfiles) == 4 * 14
    rw = augment.RenderedWindows(signals, vfiles, tc, ov, scale, 'reference', B, 0, ctx, frame, hop, blackmanharris)
    feature_path = os.path.join(db, "transforms", "t1_cs_aug")
    paths = [os.path.join(feature_path, n + "__m_.data") for n in rw.names]
    assert sorted(os.path.basename(p) for p in paths) == sorted(f for f in os.listdir(feature_path) if f.endswith(".data"))
    fw = FeatureWindows(paths, tc, ov, scale, 'reference', B, 0, ctx)
    assert np.array_equal(fw.table, rw.table) and (fw.F, fw.total, fw.iteration_size) == (rw.F, rw.total, rw.iteration_size)
    assert rw.F == 129 and rw.iteration_size >= 3
    params = glorot_init('dsd', tc, rw.F, seed=1)
    first = []
    for data in (fw, rw):
        tr = Trainer(ctx, params=params, batch_size=B, time_context=tc, feat_size=rw.F, seed=1)
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
    # Margin, fixed before any run.  The loss is a weighted sum of squared differences e = mask(x) x - target, |weights| <= 1
    # (alpha, beta, beta_voc <= 0.03 weigh the cross terms), so L ~ |e|^2 and |dL| <= 2 |e| |de| to first order.  Every
    # input and target element moves by at most delta = FEED_TOL * scale (case 2), so |d target| <= delta sqrt(n); the
    # masked prediction is taken to move by at most K = 10 times as much in norm -- masks lie in [0, 1], and the
    # network at Glorot initialisation does not amplify a relative input change by more than that.  Hence
    # |dL| / L <= 2 (1 + K) delta sqrt(n) / sqrt(L).
    delta, K = FEED_TOL * scale, 10.0
    margin = 2 * (1 + K) * delta * np.sqrt(n_t) / np.sqrt(first[0])
    rel = abs(first[0] - first[1]) / first[0]
    print("first losses %.9g (files) %.9g (rendered): relative difference %.3e, margin %.3e, target rms %.3e"
          % (first[0], first[1], rel, margin, t_rms))
    assert first[0] > 0 and rel <= margin
    shutil.rmtree(feature_path)                      # --render reads the wav files only
    _load("examples/hiphopss/train_hhds.py").main(common + ["--render", "--nepochs", "1", "--skip_sep", "--time_context", str(tc),
                                                              "--overlap", str(ov), "--batch_size", str(B)])
    pkl = os.path.join(db, "models", "model_hh_cs_aug_fft_1024.pkl")
    model = _load("examples/hiphopss/separate_hhds.py").load_model(pkl)
    assert len(model) == 15 and [tuple(p.shape) for p in model] == [tuple(p.shape) for p in params]
    assert all(np.isfinite(p).all() for p in model)


# ------------------------------------------------------------------------------------------ 5. validation
def test_entry_points_reject_bad_arguments(ctx, signals):
    bank = augment.Bank(signals, np.float64, ctx)
    bank32 = augment.Bank(signals, np.float32, ctx)
    plan = StftPlan(ctx, 256, 64, blackmanharris(256))
    vf = CASES['plain'][0]
    tracks = [list(bank.index[t.signal]) + [t.k, t.c] for t in vf.tracks]
    gains = [vf.m] + [t.g for t in vf.tracks]

    def render(**kw):
        args = dict(tracks=tracks, gains=gains, size=vf.size, chunks=vf.chunks, S=None, bank_len=bank.length)
        args.update(kw)
        rc, buf, _ = _raw_render(ctx, plan, bank.tensor, args['bank_len'], args['tracks'], args['gains'], args['size'],
                                 args['chunks'], 16, args['S'], out_rows=5 * 200)
        if rc != _lib.DCS_OK:
            assert (buf == SENTINEL).all()          # a rejected call writes nothing
        return rc
    assert render() == _lib.DCS_OK
    assert render(S=0) == _lib.DCS_EINVAL
    assert render(S=9, tracks=(tracks * 3)[:9], gains=(gains * 3)[:10]) == _lib.DCS_EINVAL
    assert render(chunks=[(0, 2048), (2048, vf.size - 2048 + 1)]) == _lib.DCS_EINVAL          # a + Lc > size
    past = [list(t) for t in tracks]
    past[2][1] = bank.length - past[2][0] + 1                                                    # a track past the bank
    assert render(tracks=past) == _lib.DCS_EINVAL
    assert render(bank_len=tracks[0][0] + tracks[0][1] - 1) == _lib.DCS_EINVAL
    twice = [list(t) for t in tracks]
    twice[0][3] = twice[1][3]
    assert render(tracks=twice) == _lib.DCS_EINVAL                                               # a channel used twice

    rows, g = augment.table_rows([vf], bank32.index, 64)
    win = np.asarray([(0, 0)], dtype=np.int32)
    for S, tc in ((0, 8), (9, 8), (4, 0)):
        rc, xb, tb = _raw_feed(ctx, plan, bank32.tensor, bank32.length, rows, g, win, tc, S, 0.3, 16)
        assert rc == _lib.DCS_EINVAL, (S, tc)
        assert (xb == SENTINEL).all() and (tb == SENTINEL).all()
    rc, xb, tb = _raw_feed(ctx, plan, bank32.tensor, bank32.length, rows, g, win, 8, 4, 0.3, 16)
    assert rc == _lib.DCS_OK and not (xb[16:-16] == SENTINEL).any()
