"""``dcs_chroma`` and ``dcs_dtw`` (csrc/align.hip) on the MI355X against the float64 oracle of tests/align_ref.py, and the
alignment they make up: ``align_scores`` on a seeded synthetic piece and the two command lines.

The kernel cases run through the C ABI in a child process started with ``DCS_WS_GUARD`` (libdcs's scratch -- the strips between
the DTW's tiles, the path from the back, the direction codes -- between poisoned red zones, its payload poisoned too), on
buffers carved out of an arena of this file's own: a 64 KiB red zone on either side of every input and output, outputs and the
padding columns ``F .. ld-1`` poisoned.  Two children, poison 0xFF (float32 NaN) and 0x4B (1.3e7), run side by side; each runs
every case twice.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

FLOOR = 1e-6
EPS = 2.0 ** -24


def _tile():
    from deepconvsep_amd import _lib
    return int(_lib.load().dcs_dtw_tile())


# ------------------------------------------------------------------------------------------------ the cases
def chroma_cases():
    """name -> dict(mag [T, F] float32, ld, cls int8 [F])"""
    from deepconvsep_amd import align
    rs = np.random.RandomState(11)
    cases = {}

    def add(name, T, F, ld, cls=None):
        mag = rs.uniform(0.0, 2.0, (T, F)).astype(np.float32) ** 2
        if cls is None:
            cls = rs.randint(-1, 12, F).astype(np.int8)
        cases[name] = dict(mag=mag, ld=ld, cls=np.asarray(cls, dtype=np.int8))
        return cases[name]

    add("one_bin", 1, 1, 1, cls=[7])
    c = add("odd", 37, 70, 72)
    c["mag"][3:5] = 0.0                                          # frames of zeros ...
    c["mag"][7:9] = rs.uniform(0.0, 1e-9, (2, 70))               # ... and of values whose norm is far below the floor
    add("unused", 37, 70, 72, cls=np.full(70, -1))               # no bin is used: every row uniform
    add("bins2049", 5, 2049, 2052, cls=align.bin_classes(4096))  # the table of the separation's own analysis
    return cases


def dtw_cases():
    """name -> dict(A [T, 12], S [U, 12] float32, band, exact): exact = dyadic features, the path must EQUAL the oracle's"""
    import align_ref
    B = _tile()
    cases = {}
    for i, (T, U) in enumerate(((1, 1), (1, 7), (9, 1), (B - 1, B + 1), (B, B), (2 * B + 2, B + 3), (3 * B + 5, 4 * B + 1))):
        A, S = align_ref.dyadic_features(T, U, seed=20 + i)
        cases["exact_%dx%d" % (T, U)] = dict(A=A, S=S, band=None, exact=True)
    for i, (T, U) in enumerate(((3 * B + 5, 4 * B + 1), (B + 1, 3 * B))):
        A, S = align_ref.unit_features(T, U, seed=40 + i)
        cases["unit_%dx%d" % (T, U)] = dict(A=A, S=S, band=None, exact=False)
    T, U = 3 * B + 5, 4 * B + 1
    for band in (B // 2, 5):
        A, S = align_ref.dyadic_features(T, U, seed=50 + band)
        cases["exact_band%d" % band] = dict(A=A, S=S, band=band, exact=True)
        A, S = align_ref.unit_features(T, U, seed=60 + band)
        cases["unit_band%d" % band] = dict(A=A, S=S, band=band, exact=False)
    return cases


# ------------------------------------------------------------------------------------------------ the child process
def _child(poison, out_path):
    sys.path.insert(0, ROOT)
    import torch
    from deepconvsep_amd import _lib
    from deepconvsep_amd.runtime import default_context

    G = 1 << 16
    blocks = []

    def alloc(shape, dtype=torch.float32):
        """[red zone | payload | red zone], all poisoned"""
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        pay = (n + 255) // 256 * 256
        raw = torch.full((pay + 2 * G,), poison, dtype=torch.uint8, device="cuda")
        blocks.append((raw, n))
        return raw[G:G + n].view(dtype).view(tuple(shape))

    def red_zone_damage():
        torch.cuda.synchronize()
        return sum(int((raw[:G] != poison).sum().item()) + int((raw[G + n:] != poison).sum().item()) for raw, n in blocks)

    def put(data, ld):
        t = alloc(data.shape[:-1] + (ld,))
        t[..., :data.shape[-1]].copy_(torch.from_numpy(np.ascontiguousarray(data)))
        return t

    def untouched(t):
        return bool((t.contiguous().view(torch.uint8) == poison).all().item())

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:                                            # damaged scratch red zone: reported, not raised
            return -1, str(exc)

    ctx = default_context()
    lib = ctx._lib
    vp = ctypes.c_void_p
    arrays, report = {}, {}

    for name, c in chroma_cases().items():
        T, F = c["mag"].shape
        mag_t = put(c["mag"], c["ld"])
        outs = []
        for _ in range(2):
            o = alloc((T, 12))
            rc = lib.dcs_chroma(ctx._h, vp(mag_t.data_ptr()), c["ld"], T, F, vp(c["cls"].ctypes.data), FLOOR, vp(o.data_ptr()))
            ctx.synchronize()
            outs.append((o, rc))
        n_ws, err = guards()
        report["chroma/" + name] = dict(rc=[outs[0][1], outs[1][1]], same_twice=bool(torch.equal(outs[0][0].view(torch.int32),
                                                                                                outs[1][0].view(torch.int32))),
                                        scratch_blocks=n_ws, scratch_guard=err, red_zone_bytes_damaged=red_zone_damage())
        arrays["chroma/" + name] = outs[0][0].cpu().numpy()

    def run_dtw(A_t, S_t, T, U, band, h=None, null=None):
        path, n, cost = alloc((T + U - 1, 2), torch.int32), alloc((1,), torch.int64), alloc((1,), torch.float32)
        ptr = [vp(t.data_ptr()) for t in (A_t, S_t, path, n, cost)]
        if null is not None:
            ptr[null] = vp(None)
        rc = lib.dcs_dtw(ctx._h if h is None else h, ptr[0], T, ptr[1], U, -1 if band is None else band, ptr[2], ptr[3], ptr[4])
        ctx.synchronize()
        return rc, path, n, cost

    for name, c in dtw_cases().items():
        T, U = len(c["A"]), len(c["S"])
        A_t, S_t = put(c["A"], 12), put(c["S"], 12)
        outs = [run_dtw(A_t, S_t, T, U, c["band"]) for _ in range(2)]
        (rc, path, n, cost), (rc2, path2, n2, cost2) = outs
        n_h = int(n.item()) if rc == 0 else 0
        n_ws, err = guards()
        report["dtw/" + name] = dict(rc=[rc, rc2], n=n_h, cost=float(cost.item()) if rc == 0 else None,
                                     same_twice=bool(torch.equal(path[:n_h], path2[:n_h]) and torch.equal(n, n2) and
                                                     torch.equal(cost.view(torch.int32), cost2.view(torch.int32))),
                                     tail_kept=untouched(path[n_h:]) if n_h < T + U - 1 else True,
                                     scratch_blocks=n_ws, scratch_guard=err, red_zone_bytes_damaged=red_zone_damage())
        arrays["dtw/" + name] = path[:n_h].cpu().numpy()

    # arguments: refused, nothing written
    import align_ref
    A, S = align_ref.unit_features(10, 100, seed=1)
    A_t, S_t = put(A, 12), put(S, 12)
    args = {}
    for label, kw in {"band too narrow": dict(band=2), "band=-2": dict(band=-2), "T=0": dict(T=0), "U=0": dict(U=0),
                      "T>2^20": dict(T=(1 << 20) + 1), "null ctx": dict(h=vp(None)), "null a": dict(null=0), "null s": dict(null=1),
                      "null path": dict(null=2), "null n": dict(null=3), "null cost": dict(null=4)}.items():
        T, U = kw.pop("T", 10), kw.pop("U", 100)
        path, n, cost = alloc((10 + 100 - 1, 2), torch.int32), alloc((1,), torch.int64), alloc((1,), torch.float32)
        ptr = [vp(t.data_ptr()) for t in (A_t, S_t, path, n, cost)]
        if "null" in kw:
            ptr[kw["null"]] = vp(None)
        rc = lib.dcs_dtw(kw.get("h", ctx._h), ptr[0], T, ptr[1], U, kw.get("band", 6), ptr[2], ptr[3], ptr[4])
        ctx.synchronize()
        args[label] = dict(rc=rc, untouched=untouched(path) and untouched(n) and untouched(cost))
    mag_t, o = put(np.ones((4, 6), np.float32), 8), alloc((4, 12))
    cls = np.zeros(6, np.int8)
    bad_cls = np.array([0, 1, 12, 3, 4, 5], np.int8)
    for label, a in {"F=0": (8, 4, 0, cls, FLOOR), "ld<F": (5, 4, 6, cls, FLOOR), "n_frames<0": (8, -1, 6, cls, FLOOR),
                     "floor<0": (8, 4, 6, cls, -1.0), "class 12": (8, 4, 6, bad_cls, FLOOR)}.items():
        rc = lib.dcs_chroma(ctx._h, vp(mag_t.data_ptr()), a[0], a[1], a[2], vp(a[3].ctypes.data), a[4], vp(o.data_ptr()))
        ctx.synchronize()
        args["chroma " + label] = dict(rc=rc, untouched=untouched(o))
    rc = lib.dcs_chroma(ctx._h, vp(mag_t.data_ptr()), 8, 0, 6, vp(cls.ctypes.data), FLOOR, vp(o.data_ptr()))
    ctx.synchronize()
    args["chroma n_frames=0"] = dict(rc=rc, untouched=untouched(o))
    report["_args"] = args
    report["_red_zone_bytes_damaged"] = red_zone_damage()
    n_ws, err = guards()
    report["_scratch"] = dict(blocks=n_ws, guard=err)

    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


# ------------------------------------------------------------------------------------------------ the tests
def _start(poison, out):
    env = dict(os.environ)
    env.update({"DCS_WS_GUARD": "65536", "DCS_WS_POISON": str(poison)})
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), str(poison), out], env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)


def _finish(proc, out):
    so, se = proc.communicate(timeout=300)
    assert proc.returncode == 0, (so[-800:], se[-2500:])
    z = np.load(out)
    report = json.loads(bytes(z["_report"]).decode())
    return {k: z[k] for k in z.files if k != "_report"}, report


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """both children, side by side; the oracle's results are computed while they run"""
    import align_ref
    d = tmp_path_factory.mktemp("align")
    f_nan, f_big = str(d / "nan.npz"), str(d / "big.npz")
    p_nan, p_big = _start(0xFF, f_nan), _start(0x4B, f_big)
    try:
        cc, dc = chroma_cases(), dtw_cases()
        refs = {"chroma/" + k: align_ref.chroma(c["mag"], c["cls"], FLOOR) for k, c in cc.items()}
        for k, c in dc.items():
            refs["dtw/" + k] = align_ref.dtw(c["A"], c["S"], band=c["band"])
        for v in refs.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        nan_run, big_run = _finish(p_nan, f_nan), _finish(p_big, f_big)
    finally:
        for p in (p_nan, p_big):                        # whatever went wrong, no child outlives the fixture
            if p.poll() is None:
                p.kill()
                p.communicate()
    return dict(nan=nan_run, big=big_run, refs=refs, chroma=cc, dtw=dc)


@pytest.mark.parametrize("name", ["one_bin", "odd", "unused", "bins2049"])
def test_chroma_against_float64(runs, name):
    """Bound per component (F + 16) 2^-24: components are <= 1 and a sum of F non-negative float32 terms is relatively exact
    to F 2^-24; the rest is the squares, the root and the division.  Uniform rows are held to 2^-24."""
    arrays, report = runs["nan"]
    key = "chroma/" + name
    c, want = runs["chroma"][name], runs["refs"][key]
    got = arrays[key]
    assert report[key]["rc"] == [0, 0] and got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(got).all()
    F = c["mag"].shape[1]
    err = float(np.abs(got - want).max())
    print("%s: max |chroma - float64| = %.3g, bound %.3g" % (name, err, (F + 16) * EPS))
    assert err <= (F + 16) * EPS
    uniform = np.sqrt((np.asarray(c["mag"], np.float64) ** 2).sum(axis=1)) < 1e-7
    if name == "unused":
        uniform[:] = True
    if name == "odd":
        assert uniform[3:5].all() and uniform[7:9].all() and uniform.sum() == 4
    assert np.abs(got[uniform] - 1 / np.sqrt(12.0)).max(initial=0.0) <= EPS
    live = ~uniform
    # the rows' own norm: twelve roundings in the sum of squares, halved by the root, the root's and the division's own
    assert np.abs(np.sqrt((got[live].astype(np.float64) ** 2).sum(axis=1)) - 1.0).max(initial=0.0) <= 16 * EPS


def _dtw_result(runs, name):
    arrays, report = runs["nan"]
    key = "dtw/" + name
    r = report[key]
    assert r["rc"] == [0, 0], r
    path = arrays[key]
    assert path.dtype == np.int32 and path.shape == (r["n"], 2) and r["n"] > 0
    return path, r["cost"], runs["refs"][key], runs["dtw"][name]


def test_dtw_exact_case_list_straddles_the_tile():
    B = _tile()
    names = set(dtw_cases())
    assert {"exact_1x1", "exact_1x7", "exact_9x1", "exact_%dx%d" % (B - 1, B + 1), "exact_%dx%d" % (B, B),
            "exact_%dx%d" % (2 * B + 2, B + 3), "exact_%dx%d" % (3 * B + 5, 4 * B + 1)} <= names


@pytest.mark.parametrize("index", range(7))
def test_dtw_equals_the_oracle_on_dyadic_features(runs, index):
    """every product and partial sum is exact in float32 and ties are everywhere: path and cost must EQUAL the float64 oracle's"""
    name = [k for k in runs["dtw"] if k.startswith("exact_") and "band" not in k][index]
    path, cost, (want_path, want_cost, _), _ = _dtw_result(runs, name)
    assert cost == want_cost, (name, cost, want_cost)
    assert np.array_equal(path, want_path), name


def _check_valid_and_near_optimal(runs, name):
    import align_ref
    path, cost, (want_path, want_cost, D), c = _dtw_result(runs, name)
    T, U = len(c["A"]), len(c["S"])
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (T - 1, U - 1)
    steps = set(map(tuple, np.diff(path, axis=0).tolist()))
    assert steps <= {(1, 1), (1, 0), (0, 1)}, steps
    assert align_ref.in_band(T, U, c["band"])[path[:, 0], path[:, 1]].all()
    # a 13-term rounding per cell on values <= 2 plus one rounding of D per cell, along at most T + U cells
    bound = (T + U) * EPS * (32 + float(np.abs(D[np.isfinite(D)]).max()))
    along = align_ref.path_cost(c["A"], c["S"], path)
    print("%s: cost %.6f, float64 cost along the path %.6f, oracle optimum %.6f, bound %.3g" % (name, cost, along, want_cost, bound))
    assert abs(cost - want_cost) <= bound and abs(along - want_cost) <= bound
    return path, want_path


@pytest.mark.parametrize("index", range(2))
def test_dtw_on_unit_norm_rows(runs, index):
    name = [k for k in runs["dtw"] if k.startswith("unit_") and "band" not in k][index]
    _check_valid_and_near_optimal(runs, name)


@pytest.mark.parametrize("kind", ["exact", "unit"])
@pytest.mark.parametrize("band_in_tiles", [0.5, 0])
def test_dtw_band(runs, band_in_tiles, kind):
    """(3B+5, 4B+1) with band B/2 and band 5 against the banded oracle: equality on dyadic features, the validity and the
    derived bound on real-valued ones"""
    band = int(band_in_tiles * _tile()) or 5
    name = "%s_band%d" % (kind, band)
    if kind == "exact":
        path, cost, (want_path, want_cost, _), _ = _dtw_result(runs, name)
        assert cost == want_cost and np.array_equal(path, want_path)
    _check_valid_and_near_optimal(runs, name)


def test_dtw_scratch_follows_the_band():
    from deepconvsep_amd import _lib
    lib = _lib.load()
    assert 0 < lib.dcs_dtw_bytes(20000, 20000, 200) * 5 <= lib.dcs_dtw_bytes(20000, 20000, -1)


def test_bad_arguments_are_refused_and_write_nothing(runs):
    from deepconvsep_amd import _lib
    for _, report in (runs["nan"], runs["big"]):
        args = dict(report["_args"])
        noop = args.pop("chroma n_frames=0")
        assert noop == dict(rc=_lib.DCS_OK, untouched=True), noop
        assert args.pop("T>2^20") == dict(rc=_lib.DCS_ESHAPE, untouched=True)
        assert len(args) == 15
        for label, r in args.items():
            assert r == dict(rc=_lib.DCS_EINVAL, untouched=True), (label, r)       # (10, 100) with band 2 among them


def test_memory_and_determinism(runs):
    (a_nan, r_nan), (a_big, r_big) = runs["nan"], runs["big"]
    keys = sorted(k for k in r_nan if not k.startswith("_"))
    assert keys == sorted(runs["refs"]) and sorted(r_big) == sorted(r_nan)
    problems = []
    for tag, (arrays, report) in (("0xFF", runs["nan"]), ("0x4B", runs["big"])):
        if report["_red_zone_bytes_damaged"]:
            problems.append("[%s] %d red-zone bytes of the ABI buffers changed" % (tag, report["_red_zone_bytes_damaged"]))
        if report["_scratch"]["guard"] or report["_scratch"]["blocks"] < 0:
            problems.append("[%s] dcs_debug_check_guards: %s" % (tag, report["_scratch"]["guard"]))
        for k in keys:
            r = report[k]
            if r["red_zone_bytes_damaged"]:
                problems.append("%s [%s]: %d red-zone bytes of the ABI buffers changed" % (k, tag, r["red_zone_bytes_damaged"]))
            if r["scratch_guard"] or r["scratch_blocks"] < 0:
                problems.append("%s [%s]: dcs_debug_check_guards: %s" % (k, tag, r["scratch_guard"]))
            if not r.get("tail_kept", True):
                problems.append("%s [%s]: path rows behind n_path were written" % (k, tag))
            if not r["same_twice"]:
                problems.append("%s [%s]: two runs in one process differ" % (k, tag))
    for k in keys:
        if a_nan[k].tobytes() != a_big[k].tobytes():
            problems.append("%s: outputs differ between the two scratch poisons" % k)
        if k.startswith("dtw/") and r_nan[k]["cost"] != r_big[k]["cost"]:
            problems.append("%s: costs differ between the two scratch poisons" % k)
    assert not problems, "\n".join(problems)
    # the switch was honoured: the DTW's scratch is among the guarded blocks
    assert r_nan["dtw/exact_1x1"]["scratch_blocks"] >= 1, r_nan["dtw/exact_1x1"]


# ------------------------------------------------------------------------------------------------ end to end
def _stats(errors):
    return float(np.median(errors)), float(np.percentile(errors, 90))


@pytest.fixture(scope="module")
def aligned():
    """align_scores on the synthetic piece, without a band and with band 64"""
    import align_ref
    import deepconvsep_amd as dcs
    scores, audio = align_ref.piece()
    tt = dcs.transformFFT(frameSize=align_ref.FRAME, hopSize=align_ref.HOP, sampleRate=align_ref.RATE, precision='float32')
    out = {}
    for band in ('auto', 64):
        got, path, cost = dcs.align_scores(tt, audio, scores, band=band)
        out[band] = dict(scores=got, path=path, cost=cost, errors=align_ref.onset_errors([on for on, _, _ in got], scores))
    return out


@pytest.mark.parametrize("band", ['auto', 64])
def test_align_scores_on_the_synthetic_piece(aligned, band):
    """Device median and p90 onset error each <= the float64 oracle's recorded value + 1 frame (float32 features may move the
    path by a cell at near-ties); band 64 holds the optimum, so it must meet the same criterion."""
    import align_ref
    r = aligned[band]
    med, p90 = _stats(r["errors"])
    scores, _ = align_ref.piece()
    print("band %r: onset error median %.3f p90 %.3f max %.3f frames (oracle %.3f / %.3f), %d path points, cost %.4f"
          % (band, med, p90, r["errors"].max(), align_ref.ORACLE_MEDIAN, align_ref.ORACLE_P90, len(r["path"]), r["cost"]))
    assert med <= align_ref.ORACLE_MEDIAN + 1.0 and p90 <= align_ref.ORACLE_P90 + 1.0
    assert len(r["scores"]) == 4
    for (on, off, names), (on0, off0, names0) in zip(r["scores"], scores):
        assert names == list(names0) and on.shape == on0.shape and (np.diff(on) >= 0).all() and (off >= on).all()
    U = align_ref.score_frames(scores)
    assert tuple(r["path"][0]) == (0, 0) and r["path"][-1][1] == U - 1
    if band == 64:
        T = r["path"][-1][0] + 1
        assert align_ref.in_band(T, U, 64)[r["path"][:, 0], r["path"][:, 1]].all()
        m0, p0 = _stats(aligned['auto']["errors"])
        assert abs(med - m0) <= 1.0 and abs(p90 - p0) <= 1.0


def test_dtw_refuses_a_band_without_a_path():
    import align_ref
    from deepconvsep_amd import align
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    A, S = align_ref.unit_features(10, 100, seed=1)
    with pytest.raises(ValueError):
        align.dtw(ctx, ctx.to_device(A, np.float32), ctx.to_device(S, np.float32), band=2)
    path, cost = align.dtw(ctx, ctx.to_device(A, np.float32), ctx.to_device(S, np.float32), band=6)
    want_path, want_cost, D = align_ref.dtw(A, S, band=6)
    assert tuple(path[-1]) == (9, 99) and abs(cost - want_cost) <= 110 * EPS * (32 + float(np.abs(D[np.isfinite(D)]).max()))


# ------------------------------------------------------------------------------------------------ command lines
def _load(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("si_" + name[:-3], os.path.join(ROOT, "examples", "bach10_scoreinformed", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def piece_dir(tmp_path_factory):
    """the piece as a wav with its four score files at nominal tempo next to it"""
    import align_ref
    from deepconvsep_amd.score import write_score
    from deepconvsep_amd.separation import SI_SCORE_FILES, write_wav
    d = tmp_path_factory.mktemp("piece")
    scores, audio = align_ref.piece()
    write_wav(str(d / "mix.wav"), 0.5 * audio, 44100)
    for f, (on, off, names) in zip(SI_SCORE_FILES, scores):
        write_score(str(d / f), on, off, names)
    return d


def test_align_scores_script(piece_dir, tmp_path):
    """four files that read_score reads back, with the errors of ``align_scores`` on the samples the wav holds"""
    import align_ref
    import deepconvsep_amd as dcs
    from deepconvsep_amd.score import read_score
    from deepconvsep_amd.separation import SI_SCORE_FILES, read_wav
    out = tmp_path / "aligned"
    _load("align_scores.py").main(["-i", str(piece_dir / "mix.wav"), "-s", str(piece_dir), "-o", str(out)])
    scores, _ = align_ref.piece()
    got = [read_score(str(out / f)) for f in SI_SCORE_FILES]
    errors = align_ref.onset_errors([on for on, _, _ in got], scores)
    med, p90 = _stats(errors)
    print("script: onset error median %.3f p90 %.3f frames" % (med, p90))
    assert med <= align_ref.ORACLE_MEDIAN + 1.0 and p90 <= align_ref.ORACLE_P90 + 1.0
    _, audio = read_wav(str(piece_dir / "mix.wav"))
    tt = dcs.transformFFT(frameSize=2048, hopSize=512, precision='float32')
    want, _, _ = dcs.align_scores(tt, audio, scores)
    for (on, off, names), (on_w, off_w, names_w) in zip(got, want):
        assert names == names_w
        assert np.array_equal(on, on_w.astype(np.float32).astype(np.float64))
        assert np.array_equal(off, off_w.astype(np.float32).astype(np.float64))
    # a band that holds the optimum gives the same files
    out2 = tmp_path / "aligned_band"
    _load("align_scores.py").main(["-i", str(piece_dir / "mix.wav"), "-s", str(piece_dir), "-o", str(out2), "--band", "64"])
    banded = [read_score(str(out2 / f)) for f in SI_SCORE_FILES]
    m2, p2 = _stats(align_ref.onset_errors([on for on, _, _ in banded], scores))
    assert m2 <= align_ref.ORACLE_MEDIAN + 1.0 and p2 <= align_ref.ORACLE_P90 + 1.0


def test_separate_script_with_and_without_align(piece_dir, tmp_path):
    """``align=True`` (the script's ``--align``; tests/test_align_cpu.py checks that the flag arrives) writes the aligned score
    files into the output directory and separates with those; without it the script writes what it wrote before.  Both
    against ``Separator.separate_scoreinformed`` on the note tables of the two sets of files, truncated to int16.  A
    ``synth_params('bach10_si')`` model of 257 bins, handed over in memory: the script's own 2049 bins make 856 MB."""
    import scipy.io.wavfile
    import deepconvsep_amd as dcs
    from deepconvsep_amd.score import melody_table
    from deepconvsep_amd.separation import SI_SCORE_FILES, SI_SCORE_PARAMS, blackmanharris, output_paths, read_wav
    from deepconvsep_amd.synth import synth_params
    F, N, HOP = 257, 512, 256
    params = synth_params("bach10_si", 30, F, seed=6)
    wav = str(piece_dir / "mix.wav")
    cli = _load("separate_bach10.py")
    plain, with_align, by_hand = tmp_path / "plain", tmp_path / "align", tmp_path / "by_hand"
    for d in (plain, with_align):
        d.mkdir()
    cli.train_auto(wav, str(with_align), params, 0.3, 30, 25, 32, F, N, HOP, align=True)
    cli.train_auto(wav, str(plain), params, 0.3, 30, 25, 32, F, N, HOP)
    assert not [f for f in SI_SCORE_FILES if os.path.exists(str(plain / f))]
    _load("align_scores.py").main(["-i", wav, "-s", str(piece_dir), "-o", str(by_hand)])
    for f in SI_SCORE_FILES:
        assert open(str(with_align / f)).read() == open(str(by_hand / f)).read() != open(str(piece_dir / f)).read()

    _, audio = read_wav(wav)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, F, N, HOP, blackmanharris, tiler="library")
    nframes = int(np.ceil(len(audio) / float(HOP))) + 2
    stems = {}
    for out, score_dir in ((plain, piece_dir), (with_align, with_align)):
        melody = melody_table(SI_SCORE_FILES, str(score_dir), nframes, 44100, HOP, N, **SI_SCORE_PARAMS)
        pcm = sep.separate_scoreinformed(audio, melody)
        stems[str(out)] = []
        for p, want in zip(output_paths("bach10_si", wav, str(out)), pcm):
            rate, got = scipy.io.wavfile.read(p)
            assert rate == 44100 and np.array_equal(got, (want * 32767).astype(np.int16)), p
            stems[str(out)].append(got)
    assert any(not np.array_equal(a, b) for a, b in zip(stems[str(plain)], stems[str(with_align)]))


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
