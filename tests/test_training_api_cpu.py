"""What the three trainers and the six window feeds share (training.TrainerHandle, training.WindowFeed, training.glorot_arrays):
the initialiser against a restatement of its docstring, the slot table and the epoch order of every feed, and the arguments
every class refuses before it touches a device.  CPU only."""
import numpy as np
import pytest
import torch

from deepconvsep_amd import augment, rwc, score_render, score_training, stereo_training, training
from deepconvsep_amd.transform import write_shape_file

# ------------------------------------------------------------------------------------------------ Glorot initialiser
# layout -> (tc, shapes(tc, F), glorot_init(tc, F, seed))
LAYOUTS = {
    'dsd': (30, lambda tc, F: training.param_shapes('dsd', tc, F), lambda tc, F, s: training.glorot_init('dsd', tc, F, s)),
    'ikala_nopool': (30, lambda tc, F: training.param_shapes('ikala_nopool', tc, F),
                     lambda tc, F, s: training.glorot_init('ikala_nopool', tc, F, s)),
    'bach10': (30, lambda tc, F: training.param_shapes('bach10', tc, F),
               lambda tc, F, s: training.glorot_init('bach10', tc, F, s)),
    'dsd_ild': (30, stereo_training.param_shapes, stereo_training.glorot_init),
    'bach10_si': (30, lambda tc, F: score_training.param_shapes(tc, F, 4), lambda tc, F, s: score_training.glorot_init(tc, F, s, 4)),
    'bach10_si1': (30, lambda tc, F: score_training.param_shapes(tc, F, 1), lambda tc, F, s: score_training.glorot_init(tc, F, s, 1)),
    'bach10_si_1x1 branches 1': (19, lambda tc, F: score_training.param_shapes(tc, F, 1, 'build_ca_1x1'),
                                 lambda tc, F, s: score_training.glorot_init(tc, F, s, 1, 'build_ca_1x1')),
    'bach10_si_1x1 branches 4': (19, lambda tc, F: score_training.param_shapes(tc, F, 4, 'build_ca_1x1'),
                                 lambda tc, F, s: score_training.glorot_init(tc, F, s, 4, 'build_ca_1x1')),
}


def _glorot(shapes, seed):
    """The docstring's formula: W uniform in +-sqrt(3) sqrt(2 / ((n1 + n2) receptive field)), biases 0, float32, one
    RandomState in parameter order."""
    rs = np.random.RandomState(seed)
    out = []
    for shp in shapes:
        if len(shp) == 1:
            out.append(np.zeros(shp, dtype=np.float32))
            continue
        field = 1
        for n in shp[2:]:
            field *= n
        bound = np.sqrt(3.0) * np.sqrt(2.0 / ((shp[0] + shp[1]) * field))
        out.append(rs.uniform(-bound, bound, size=shp).astype(np.float32))
    return out


@pytest.mark.parametrize("seed", [0, 3])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_glorot_init_is_the_docstring_s_formula(layout, seed):
    tc, shapes, init = LAYOUTS[layout]
    got, want = init(tc, 253, seed), _glorot(shapes(tc, 253), seed)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the six feeds, tiny
# T = 7 < tc: one padded window; at tc 10 / overlap 5 loadFile reaches every slot of T = 30, 31 and 95, and leaves the only
# slot of T = 10 and the last of T = 20 unfilled: their rows are (-1, 0)
FRAMES, TC, OVERLAP, F, BATCH = (7, 30, 31, 95, 10, 20), 10, 5, 4, 4
HOP, FRAME = 4, 6                                     # frame // 2 + 1 = F; T = ceil(samples / hop) + 2
FEEDS = {c.__name__: c for c in (training.FeatureWindows, stereo_training.StereoFeatureWindows,
                                 score_training.ScoreFeatureWindows, augment.RenderedWindows,
                                 score_render.ScoreRenderedWindows, score_render.ScoreInformedRenderedWindows)}


def _write(path, shape):
    np.zeros(shape).tofile(path)
    write_shape_file(path.replace('.data', '.shape'), shape)
    return path


def _feed(name, d, cls=None, **kw):
    """Feed ``name`` (or its subclass ``cls``) over files of FRAMES frames: written into ``d``, or virtual."""
    cls = cls or FEEDS[name]
    kw = dict(dict(time_context=TC, overlap=OVERLAP, batch_size=BATCH), **kw)
    d.mkdir(exist_ok=True)
    stem = lambda i, tail: str(d / ("f%d_%s.data" % (i, tail)))  # noqa: E731
    if name == 'FeatureWindows':
        return cls([_write(stem(i, 'x'), (5, T, F)) for i, T in enumerate(FRAMES)], **kw)
    if name == 'StereoFeatureWindows':
        for i, T in enumerate(FRAMES):
            _write(stem(i, 'in_m_'), (2, T, F))
            _write(stem(i, 'out_m_'), (8, T, F))
        return cls([str(d)], **kw)
    if name == 'ScoreFeatureWindows':
        for i, T in enumerate(FRAMES):
            _write(stem(i, 'm_'), (5, T, F))
            _write(stem(i, 'e_'), (4, 2, 5))
        return cls([str(d)], **kw)
    sizes = [(T - 2) * HOP for T in FRAMES]
    kw.update(frameSize=FRAME, hopSize=HOP)
    if name == 'RenderedWindows':
        vfs = [augment.VirtualFile((augment.Track('a', 0, 1.0, 1),), 1.0, n, ((0, n),), ('v%d' % i,)) for i, n in enumerate(sizes)]
        return cls({'a': np.zeros(8)}, vfs, **kw)
    bank = rwc.NoteBank.from_arrays({'a': np.zeros(8)})
    if name == 'ScoreRenderedWindows':
        sfs = [score_render.ScoreFile('s%d' % i, n, (((0, 0, 8),),)) for i, n in enumerate(sizes)]
        return cls(bank, sfs, **kw)
    notes = np.zeros((1, 2, 5))
    sfs = [score_render.ScoreInformedFile('s%d' % i, n, (((0, 0, 8),),), notes, notes) for i, n in enumerate(sizes)]
    return cls(bank, sfs, **kw)


@pytest.mark.parametrize("windows", ['reference', 'all'])
@pytest.mark.parametrize("name", sorted(FEEDS))
def test_slot_table(name, windows, tmp_path):
    slots = training.reference_slots if windows == 'reference' else training.all_slots
    want = []
    for i, T in enumerate(FRAMES):
        want += [(-1, 0) if s is None else (i, s) for s in slots(T, TC, OVERLAP)]
    assert want[0] == (0, 0) and want[1][0] == 1                   # T = 7 < tc: the single padded window
    assert want.count((-1, 0)) == (2 if windows == 'reference' else 0)
    w = _feed(name, tmp_path / "files", windows=windows)
    assert w.F == F
    assert w.table.dtype == np.int32 and w.table.shape == (len(want), 2) and w.table.tolist() == [list(v) for v in want]
    assert w.total == len(want) and w.iteration_size == len(want) // BATCH


@pytest.mark.parametrize("name", sorted(FEEDS))
def test_batches_follow_the_seeded_permutation(name, tmp_path):
    echo = type('Echo' + name, (FEEDS[name],), {'gather': lambda self, rows: rows})
    w = _feed(name, tmp_path / "files", cls=echo, seed=5)
    assert w.total % BATCH                                          # a remainder to drop
    for epoch in (0, 2):
        perm = np.random.RandomState(5 + epoch).permutation(w.total)
        got = list(w.batches(epoch))
        assert len(got) == w.iteration_size == w.total // BATCH
        for b, rows in enumerate(got):
            assert np.array_equal(rows, perm[b * BATCH:(b + 1) * BATCH])


@pytest.mark.parametrize("name", sorted(FEEDS))
def test_feeds_refuse_an_unknown_windows_value(name, tmp_path):
    with pytest.raises(ValueError, match="windows must be"):
        _feed(name, tmp_path / "files", windows='some')


# ------------------------------------------------------------------------------------------------ trainers
class _NoDevice(object):
    """Stands for the context: any use of it is a device call."""

    def __getattr__(self, name):
        raise AssertionError("the trainer reached for ctx.%s" % name)


@pytest.mark.parametrize("make", [
    lambda p: training.Trainer(ctx=_NoDevice(), params=p, batch_size=1, time_context=4, feat_size=5),
    lambda p: stereo_training.StereoTrainer(ctx=_NoDevice(), params=p, batch_size=1, time_context=4, feat_size=5),
    lambda p: score_training.ScoreTrainer(ctx=_NoDevice(), params=p, batch_size=1, time_context=4, feat_size=5),
], ids=['Trainer', 'StereoTrainer', 'ScoreTrainer'])
def test_a_parameter_with_five_axes_is_refused_before_any_device_call(make, monkeypatch):
    monkeypatch.setattr(training, 'require_gpu', lambda: torch)
    with pytest.raises(ValueError, match="parameter 1 has 5 axes"):
        make([np.zeros((2, 3)), np.zeros((1, 1, 1, 1, 1))])
