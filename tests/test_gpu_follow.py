"""``dcs_follow_*`` (csrc/follow.hip) on the MI355X against the NumPy restatement of tests/follow_ref.py, and the causal
alignment it makes up: ``follow_scores`` on the seeded synthetic piece and ``align_scores.py --online``.

The kernel cases run through the C ABI in a child process started with ``DCS_WS_GUARD`` (the follower's one device block -- score,
row, window start, position -- between poisoned red zones, its payload poisoned too), on buffers carved out of an arena of this
file's own: a 64 KiB red zone on either side of every input and output, outputs poisoned.  Two children, poison 0xFF (float32
NaN) and 0x4B (1.3e7), run side by side.  Every case: W = 64, back = 16.
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

EPS = 2.0 ** -24
W, BACK, LAM = 64, 16, 1.0 / 16
# a window wider than the score, exactly the score, a moving window, a window clamped at U - W
SHAPES = ((1, 1), (1, 50), (2, 3), (70, 50), (63, 64), (130, 65), (150, 200), (200, 131), (90, 260))
STEPS = (1, 2, 4)
CUTS = (0, 1, 7, 64)                                     # 0: one block
BIG = dict(T=300, U=1500, W=1024, K=2, back=BACK)


def exact_cases():
    import align_ref
    cases = {}
    for i, (T, U) in enumerate(SHAPES):
        for K in STEPS:
            A, S = align_ref.dyadic_features(T, U, seed=300 + i)
            cases["exact_%dx%d_K%d" % (T, U, K)] = dict(A=A, S=S, K=K)
    return cases


def unit_cases():
    import align_ref
    cases = {}
    for i, (T, U) in enumerate(SHAPES):
        A, S = align_ref.unit_features(T, U, seed=400 + i)
        cases["unit_%dx%d" % (T, U)] = dict(A=A, S=S, K=2)
    return cases


def big_case():
    import align_ref
    A, S = align_ref.dyadic_features(BIG["T"], BIG["U"], seed=500)
    return dict(A=A, S=S)


def checkpoints(T):
    """frames pushed when the real-valued cases read the row: after pushes of 1, 7 and 64 frames, then the rest"""
    marks, t = [], 0
    for n in (1, 7, 64, T):
        t = min(T, t + n)
        if not marks or t > marks[-1]:
            marks.append(t)
    return marks


# ------------------------------------------------------------------------------------------------ the child process
def _child(poison, out_path):
    sys.path.insert(0, ROOT)
    import torch
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

    checked = [0]

    def red_zone_damage(everything=False):
        """damaged red-zone bytes of the blocks made since the last call (of every block: ``everything``)"""
        torch.cuda.synchronize()
        todo = blocks if everything else blocks[checked[0]:]
        checked[0] = len(blocks)
        return sum(int((raw[:G] != poison).sum().item()) + int((raw[G + n:] != poison).sum().item()) for raw, n in todo)

    def put(data):
        t = alloc(data.shape)
        t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
        return t

    def untouched(*ts):
        return all(bool((t.contiguous().view(torch.uint8) == poison).all().item()) for t in ts)

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:                                            # damaged red zone: reported, not raised
            return -1, str(exc)

    ctx = default_context()
    lib = ctx._lib
    vp = ctypes.c_void_p
    arrays, report = {}, {}

    def create(S, Wd=W, K=2, back=BACK, lam=LAM, max_frames=4096, U=None, null=False, h=None):
        S = np.ascontiguousarray(S, dtype=np.float32)
        out = vp(0xDEAD)
        rc = lib.dcs_follow_create(ctx._h if h is None else h, vp(None) if null else vp(S.ctypes.data), len(S) if U is None else U,
                                   Wd, K, back, lam, max_frames, ctypes.byref(out))
        return rc, out

    def state(f, Wd=W, guarded=True):
        """dcs_follow_row; ``guarded=False`` (the reads after every single frame): plain tensors, no red zones"""
        if guarded:
            row, w0, p = alloc((Wd,)), alloc((1,), torch.int64), alloc((1,), torch.int32)
        else:
            row = torch.empty((Wd,), dtype=torch.float32, device="cuda")
            w0, p = torch.empty((1,), dtype=torch.int64, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda")
        rc = lib.dcs_follow_row(f, vp(row.data_ptr()), vp(w0.data_ptr()), vp(p.data_ptr()))
        ctx.synchronize()
        assert rc == 0
        return row.cpu().numpy(), int(w0.item()), int(p.item())

    def run(f, A_t, T, cut, Wd=W, marks=(), guarded=True):
        """the frames in blocks of ``cut`` (0: one block); the state after ``marks`` frames and at the end"""
        pos = alloc((T,), torch.int32)
        seen, t = [], 0
        sizes = [T] if cut == 0 else [cut] * (T // cut) + ([T % cut] if T % cut else [])
        if marks:
            sizes = list(np.diff([0] + list(marks)))
        for n in sizes:
            rc = lib.dcs_follow_push(f, vp(A_t[t:].data_ptr()), int(n), vp(pos[t:].data_ptr()))
            assert rc == 0, rc
            t += int(n)
            if marks:
                seen.append(state(f, Wd, guarded))
        ctx.synchronize()
        assert t == T and lib.dcs_follow_frames(f) == T
        return pos.cpu().numpy(), state(f, Wd), seen

    def same(a, b):
        return bool(np.array_equal(a[0], b[0]) and a[1][0].tobytes() == b[1][0].tobytes() and a[1][1:] == b[1][1:])

    for name, c in exact_cases().items():
        T = len(c["A"])
        A_t = put(c["A"])
        rc, f = create(c["S"], K=c["K"])
        assert rc == 0, (name, rc)
        bytes0 = lib.dcs_follow_bytes(f)
        first = run(f, A_t, T, 0)
        lib.dcs_follow_reset(f)
        again = run(f, A_t, T, 0)
        n_ws, err = guards()
        report[name] = dict(same_after_reset=same(first, again), bytes_kept=bool(lib.dcs_follow_bytes(f) == bytes0), bytes=int(bytes0),
                            w0=first[1][1], p=first[1][2], scratch_blocks=n_ws, scratch_guard=err,
                            red_zone_bytes_damaged=red_zone_damage())
        arrays[name + "/pos"], arrays[name + "/row"] = first[0], first[1][0]
        lib.dcs_follow_destroy(f)

    for name, c in unit_cases().items():
        T = len(c["A"])
        A_t = put(c["A"])
        rc, f = create(c["S"], K=c["K"])
        assert rc == 0, (name, rc)
        # frame by frame, the row read after every frame: q is the lowest cell whose value is exactly zero
        one = run(f, A_t, T, 1, marks=range(1, T + 1), guarded=False)
        q = np.array([w0 + int(np.argmax(row == 0.0)) for row, w0, _ in one[2]], dtype=np.int64)
        assert all((row == 0.0).any() for row, _, _ in one[2])
        cuts = {}
        for cut in CUTS:
            lib.dcs_follow_reset(f)
            cuts[cut] = run(f, A_t, T, cut)
        lib.dcs_follow_reset(f)
        marks = checkpoints(T)
        marked = run(f, A_t, T, 0, marks=marks)
        n_ws, err = guards()
        report[name] = dict(cuts_same=bool(all(same(cuts[0], cuts[k]) for k in CUTS) and same(cuts[0], one) and same(cuts[0], marked)),
                            w0=[s[1] for s in marked[2]], p=[s[2] for s in marked[2]], marks=marks,
                            w0_each=[s[1] for s in one[2]], scratch_blocks=n_ws, scratch_guard=err,
                            red_zone_bytes_damaged=red_zone_damage())
        arrays[name + "/pos"], arrays[name + "/q"] = cuts[0][0], q
        arrays[name + "/rows"] = np.stack([s[0] for s in marked[2]])
        arrays[name + "/rows_each"] = np.stack([s[0] for s in one[2]])
        lib.dcs_follow_destroy(f)

    c = big_case()
    A_t = put(c["A"])
    rc, f = create(c["S"], Wd=BIG["W"], K=BIG["K"], back=BIG["back"])
    assert rc == 0
    big = run(f, A_t, BIG["T"], 0, Wd=BIG["W"])
    n_ws, err = guards()
    report["big"] = dict(w0=big[1][1], p=big[1][2], scratch_blocks=n_ws, scratch_guard=err, red_zone_bytes_damaged=red_zone_damage())
    arrays["big/pos"], arrays["big/row"] = big[0], big[1][0]
    lib.dcs_follow_destroy(f)

    # refusals: nothing written, the state as it was
    import align_ref
    A, S = align_ref.unit_features(20, 100, seed=1)
    args = {}
    for label, kw in {"W=32": dict(Wd=32), "W=96": dict(Wd=96), "W=2048": dict(Wd=2048), "K=0": dict(K=0), "K=5": dict(K=5),
                      "back=-1": dict(back=-1), "back=W": dict(back=W), "lambda<0": dict(lam=-1.0), "lambda=inf": dict(lam=float("inf")),
                      "lambda=nan": dict(lam=float("nan")), "U=0": dict(U=0), "max_frames=0": dict(max_frames=0),
                      "null score": dict(null=True), "null ctx": dict(h=vp(None))}.items():
        rc, out = create(S, **kw)
        args["create " + label] = dict(rc=rc, untouched=bool(out.value == 0xDEAD))
    rc = lib.dcs_follow_create(ctx._h, vp(S.ctypes.data), len(S), W, 2, BACK, LAM, 4096, None)
    args["create null out"] = dict(rc=rc, untouched=True)
    rc, f = create(S, max_frames=16)
    assert rc == 0
    A_t = put(A)
    pos = alloc((20,), torch.int32)
    assert lib.dcs_follow_push(f, vp(A_t.data_ptr()), 5, vp(pos.data_ptr())) == 0
    before = state(f)
    keep = alloc((20,), torch.int32)
    for label, a in {"n>max_frames": (f, A_t, 17, keep), "n<0": (f, A_t, -1, keep), "null chroma": (f, None, 4, keep),
                     "null handle": (vp(None), A_t, 4, keep)}.items():
        rc = lib.dcs_follow_push(a[0], vp(a[1].data_ptr()) if a[1] is not None else vp(None), a[2], vp(a[3].data_ptr()))
        ctx.synchronize()
        after = state(f)
        args["push " + label] = dict(rc=rc, untouched=bool(untouched(keep) and lib.dcs_follow_frames(f) == 5 and after[1:] == before[1:]
                                                          and after[0].tobytes() == before[0].tobytes()))
    rc = lib.dcs_follow_push(f, vp(A_t.data_ptr()), 4, vp(None))
    ctx.synchronize()
    after = state(f)
    args["push null pos"] = dict(rc=rc, untouched=bool(lib.dcs_follow_frames(f) == 5 and after[1:] == before[1:]
                                                     and after[0].tobytes() == before[0].tobytes()))
    rc = lib.dcs_follow_push(f, vp(A_t.data_ptr()), 0, vp(keep.data_ptr()))
    ctx.synchronize()
    args["push n=0"] = dict(rc=rc, untouched=bool(untouched(keep) and lib.dcs_follow_frames(f) == 5))
    row, w0, p = alloc((W,)), alloc((1,), torch.int64), alloc((1,), torch.int32)
    for label, ptr in {"row null row": (None, w0, p), "row null w0": (row, None, p), "row null p": (row, w0, None)}.items():
        rc = lib.dcs_follow_row(f, *[vp(t.data_ptr()) if t is not None else vp(None) for t in ptr])
        ctx.synchronize()
        args[label] = dict(rc=rc, untouched=untouched(row, w0, p))
    rc = lib.dcs_follow_row(vp(None), vp(row.data_ptr()), vp(w0.data_ptr()), vp(p.data_ptr()))
    ctx.synchronize()
    args["row null handle"] = dict(rc=rc, untouched=untouched(row, w0, p))
    # before the first frame and after a reset: all +inf, w0 = 0, p = 0
    lib.dcs_follow_reset(f)
    fresh = state(f)
    report["_fresh"] = dict(inf=bool(np.isposinf(fresh[0]).all()), w0=fresh[1], p=fresh[2], frames=int(lib.dcs_follow_frames(f)))
    lib.dcs_follow_destroy(f)
    report["_args"] = args
    report["_red_zone_bytes_damaged"] = red_zone_damage(everything=True)
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
    """both children, side by side; the restatement's results are computed while they run"""
    import follow_ref
    d = tmp_path_factory.mktemp("follow")
    f_nan, f_big = str(d / "nan.npz"), str(d / "big.npz")
    p_nan, p_big = _start(0xFF, f_nan), _start(0x4B, f_big)
    try:
        ec, uc, bc = exact_cases(), unit_cases(), big_case()
        refs = {k: follow_ref.follow(c["A"], c["S"], W, c["K"], BACK, LAM) for k, c in ec.items()}
        refs["big"] = follow_ref.follow(bc["A"], bc["S"], BIG["W"], BIG["K"], BIG["back"], LAM)
        nan_run, big_run = _finish(p_nan, f_nan), _finish(p_big, f_big)
    finally:
        for p in (p_nan, p_big):                        # whatever went wrong, no child outlives the fixture
            if p.poll() is None:
                p.kill()
                p.communicate()
    return dict(nan=nan_run, big=big_run, refs=refs, exact=ec, unit=uc)


@pytest.mark.parametrize("K", STEPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_follow_equals_the_restatement_on_dyadic_features(runs, shape, K):
    """every product and sum is exact in float32 and ties are everywhere: pos, the final row, w0 and p must EQUAL float64's"""
    import follow_ref
    name = "exact_%dx%d_K%d" % (shape + (K,))
    arrays, report = runs["nan"]
    want, r = runs["refs"][name], report[name]
    assert arrays[name + "/pos"].dtype == np.int32 and np.array_equal(arrays[name + "/pos"], want["pos"]), name
    assert (r["w0"], r["p"]) == (int(want["w0"][-1]), int(want["p"])), (name, r["w0"], r["p"])
    row = arrays[name + "/row"]
    assert row.dtype == np.float32 and np.array_equal(row.astype(np.float64), follow_ref.window(want["rows"][-1], r["w0"], W)), name
    assert r["same_after_reset"], name


def test_exact_cases_move_and_clamp_the_window(runs):
    """the case list does what it is there for: windows that never move, that move, and that end clamped at U - W"""
    w0 = {k: int(v["w0"][-1]) for k, v in runs["refs"].items() if k != "big"}
    assert w0["exact_70x50_K2"] == 0 and w0["exact_63x64_K4"] == 0
    assert w0["exact_150x200_K4"] == 200 - W and w0["exact_200x131_K2"] == 131 - W
    assert 0 < w0["exact_150x200_K1"] < 200 - W
    assert int(runs["refs"]["big"]["w0"][-1]) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_follow_on_unit_norm_rows(runs, shape):
    """The restatement in float64, forced to the device's decisions q: the +inf pattern and w0 must be equal, every finite
    cell of the rows read after pushes of 1, 7 and 64 frames and of the final row within T 2^-24 (32 + max|D|) -- dcs_dtw's
    form: a 13-term rounding per cell on values <= 2, the sum, the penalty and the subtraction of the minimum, per frame --
    and the forced cell within twice that of the restatement's own minimum."""
    import follow_ref
    name = "unit_%dx%d" % shape
    arrays, report = runs["nan"]
    c, r = runs["unit"][name], report[name]
    T = shape[0]
    q = arrays[name + "/q"]
    want = follow_ref.follow(c["A"], c["S"], W, c["K"], BACK, LAM, forced=q)
    finite = want["rows"][np.isfinite(want["rows"])]
    bound = T * EPS * (32 + float(np.abs(finite).max()))
    assert np.array_equal(arrays[name + "/pos"], want["pos"]), name
    assert r["w0_each"] == [int(x) for x in want["w0"]], name
    worst = 0.0
    for rows, frames in ((arrays[name + "/rows"], r["marks"]), (arrays[name + "/rows_each"], range(1, T + 1))):
        for row, t in zip(rows, frames):
            ref = follow_ref.window(want["rows"][t - 1], int(want["w0"][t - 1]), W)
            assert np.array_equal(np.isposinf(row), np.isposinf(ref)) and not np.isnan(row).any(), (name, t)
            live = np.isfinite(ref)
            worst = max(worst, float(np.abs(row[live] - ref[live]).max()))
    assert r["w0"] == [int(want["w0"][t - 1]) for t in r["marks"]] and r["p"] == [int(want["pos"][t - 1]) for t in r["marks"]]
    gap = float(want["gap"].max())
    print("%s: max |row - forced float64| = %.3g, max gap %.3g, bound %.3g" % (name, worst, gap, bound))
    assert worst <= bound and gap <= 2 * bound


def test_push_cuts_do_not_change_a_bit(runs):
    """one block, one frame at a time, blocks of 7 and of 64, and the cut of the checkpoints: the same pos and state"""
    for _, report in (runs["nan"], runs["big"]):
        for name in runs["unit"]:
            assert report[name]["cuts_same"], name


def test_widest_window(runs):
    """W = 1024 (sixteen waves), U = 1500, T = 300, dyadic features: equality with float64"""
    import follow_ref
    arrays, report = runs["nan"]
    want, r = runs["refs"]["big"], report["big"]
    assert np.array_equal(arrays["big/pos"], want["pos"]) and (r["w0"], r["p"]) == (int(want["w0"][-1]), int(want["p"]))
    assert np.array_equal(arrays["big/row"].astype(np.float64), follow_ref.window(want["rows"][-1], r["w0"], BIG["W"]))


def test_bad_arguments_are_refused_and_write_nothing(runs):
    from deepconvsep_amd import _lib
    for _, report in (runs["nan"], runs["big"]):
        args = dict(report["_args"])
        assert args.pop("push n=0") == dict(rc=_lib.DCS_OK, untouched=True)
        assert len(args) == 24
        for label, r in args.items():
            assert r == dict(rc=_lib.DCS_EINVAL, untouched=True), (label, r)
        assert report["_fresh"] == dict(inf=True, w0=0, p=0, frames=0)


def test_memory_and_determinism(runs):
    (a_nan, r_nan), (a_big, r_big) = runs["nan"], runs["big"]
    keys = sorted(k for k in r_nan if not k.startswith("_"))
    assert keys == sorted(list(runs["exact"]) + list(runs["unit"]) + ["big"]) and sorted(r_big) == sorted(r_nan)
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
            if not r.get("same_after_reset", True):
                problems.append("%s [%s]: the run after a reset differs from the first" % (k, tag))
            if not r.get("bytes_kept", True):
                problems.append("%s [%s]: dcs_follow_bytes changed with the frames pushed" % (k, tag))
    for k in sorted(a_nan):
        if a_nan[k].tobytes() != a_big[k].tobytes():
            problems.append("%s: outputs differ between the two poisons" % k)
    assert not problems, "\n".join(problems)
    # the switch was honoured (the follower's block is among the guarded ones) and the bytes are the shapes' alone
    assert r_nan["exact_1x1_K1"]["scratch_blocks"] >= 1, r_nan["exact_1x1_K1"]
    assert r_nan["exact_150x200_K1"]["bytes"] == r_nan["exact_150x200_K4"]["bytes"] > 200 * 12 * 4


# ------------------------------------------------------------------------------------------------ end to end
def _stats(errors):
    return float(np.median(errors)), float(np.percentile(errors, 90))


@pytest.fixture(scope="module")
def restated():
    """the follower's defaults in float64 on the oracle's float64 features of the synthetic piece"""
    import align_ref
    import follow_ref
    o = align_ref.oracle_run()
    scores, _ = align_ref.piece()
    r = follow_ref.follow(o["A"], o["S"], 512, 2, 128, 1.0 / 16)
    # (median, p90) of the position track's onset error, then of the onsets warped through its time map
    return _stats(follow_ref.onset_errors(r["pos"], scores, o["U"])) + _stats(follow_ref.warped_onset_errors(r["pos"], scores, o["U"]))


def test_follow_scores_on_the_synthetic_piece(restated):
    """Device median and p90 onset error each <= the float64 restatement's on the oracle's features + 1 frame (float32 chroma
    can move the minimum by a cell on a held chord: the margin of test_align_scores_on_the_synthetic_piece), and the median
    below a tenth of the unaligned one.  Restatement, float64: median 0.944, p90 3.861, max 10.5 frames; offline DTW 0.512 /
    2.347 / 14.2; unaligned median 61.6.  The onsets ``follow_scores`` writes go through ``warp_times``: they are held, in the
    same way, to the restatement's track warped in float64 + 1 frame."""
    import align_ref
    import follow_ref
    import deepconvsep_amd as dcs
    scores, audio = align_ref.piece()
    tt = dcs.transformFFT(frameSize=align_ref.FRAME, hopSize=align_ref.HOP, sampleRate=align_ref.RATE, precision='float32')
    got, pos = dcs.follow_scores(tt, audio, scores)
    U = align_ref.score_frames(scores)
    assert pos.dtype == np.int32 and pos.shape == (795,) and U == 688 and (np.diff(pos) >= 0).all() and 0 <= pos[0] and pos[-1] < U
    errors = align_ref.onset_errors([on for on, _, _ in got], scores)
    med, p90 = _stats(errors)
    track = follow_ref.onset_errors(pos, scores, U)
    med_t, p90_t = _stats(track)
    print("onset error of the device's position track: median %.3f p90 %.3f max %.3f frames (float64 restatement %.3f / %.3f); "
          "of the warped onsets: median %.3f p90 %.3f max %.3f (restatement %.3f / %.3f)"
          % (med_t, p90_t, track.max(), restated[0], restated[1], med, p90, errors.max(), restated[2], restated[3]))
    assert abs(restated[0] - 0.944) < 1e-3 and abs(restated[1] - 3.861) < 1e-3
    # the onset error of a position track (follow_ref.onset_errors), the device's against the restatement's
    assert med_t <= restated[0] + 1.0 and p90_t <= restated[1] + 1.0
    # the onsets the caller gets, against the restatement's track through the same interpolation in float64
    assert med <= restated[2] + 1.0 and p90 <= restated[3] + 1.0
    assert med_t < 0.1 * align_ref.ORACLE_UNALIGNED_MEDIAN and med < 0.1 * align_ref.ORACLE_UNALIGNED_MEDIAN
    # the warped onsets interpolate the time map between the score frames on either side of the onset (warp_times): on a held
    # chord the frame before the onset is reached well before the onset is, so they lie earlier than the first-frame rule
    tmap = follow_ref.time_map(pos, U)
    for (on, _, _), (on0, _, _) in zip(got, scores):
        x = np.asarray(on0, dtype=np.float64) * align_ref.FPS
        lo, hi = tmap[np.floor(x).astype(int)], tmap[np.minimum(np.ceil(x).astype(int), U - 1)]
        assert (on * align_ref.FPS >= lo - 1e-9).all() and (on * align_ref.FPS <= hi + 1e-9).all()
    for (on, off, names), (on0, off0, names0) in zip(got, scores):
        assert names == list(names0) and on.shape == on0.shape and (np.diff(on) >= 0).all() and (off >= on).all()
    # a narrower window and other cuts of the frames give the same track
    got2, pos2 = dcs.follow_scores(tt, audio, scores, window=256, max_frames=100)
    assert np.array_equal(pos, pos2)


def test_align_scores_script_online(tmp_path, restated):
    """``align_scores.py --online`` on the piece written to disk: four files that read_score reads back, within the same bounds"""
    import importlib.util
    import align_ref
    from deepconvsep_amd.score import read_score, write_score
    from deepconvsep_amd.separation import SI_SCORE_FILES, write_wav
    scores, audio = align_ref.piece()
    write_wav(str(tmp_path / "mix.wav"), 0.5 * audio, 44100)
    for f, (on, off, names) in zip(SI_SCORE_FILES, scores):
        write_score(str(tmp_path / f), on, off, names)
    spec = importlib.util.spec_from_file_location("si_align_scores_online",
                                                  os.path.join(ROOT, "examples", "bach10_scoreinformed", "align_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "followed"
    mod.main(["-i", str(tmp_path / "mix.wav"), "-s", str(tmp_path), "-o", str(out), "--online"])
    got = [read_score(str(out / f)) for f in SI_SCORE_FILES]
    med, p90 = _stats(align_ref.onset_errors([on for on, _, _ in got], scores))
    print("script --online: onset error median %.3f p90 %.3f frames (restatement, warped: %.3f / %.3f)" % ((med, p90) + restated[2:]))
    assert med <= restated[2] + 1.0 and p90 <= restated[3] + 1.0 and med < 0.1 * align_ref.ORACLE_UNALIGNED_MEDIAN
    # the files hold what follow_scores gives on the samples the wav holds
    import deepconvsep_amd as dcs
    from deepconvsep_amd.separation import read_wav
    _, wav_audio = read_wav(str(tmp_path / "mix.wav"))
    tt = dcs.transformFFT(frameSize=2048, hopSize=512, precision='float32')
    want, _ = dcs.follow_scores(tt, wav_audio, scores)
    for (on, off, names), (on_w, off_w, names_w) in zip(got, want):
        assert names == names_w
        assert np.array_equal(on, on_w.astype(np.float32).astype(np.float64))
        assert np.array_equal(off, off_w.astype(np.float32).astype(np.float64))


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
