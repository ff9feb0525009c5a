"""``dcs_mwf_f32`` on the MI355X against the NumPy oracle of tests/mwf_ref.py.

Every case runs through the C ABI in a child process started with ``DCS_WS_GUARD`` (libdcs's scratch -- v and the partial
sums over t -- between poisoned red zones, its payload poisoned too), on buffers carved out of an arena of this file's own: a
64 KiB red zone on either side of every input and output, outputs and the padding columns ``F .. ld-1`` poisoned.  Two
children, poison 0xFF (float32 NaN) and 0x4B (1.3e7), run side by side; each runs every case twice.

Parity: ``max |y_gpu - y_f64| / max |X|`` must stay within 4 x the error of the complex64 restatement of the same case and
iteration count (computed here, not a constant): the margin is for another summation order over t and the device's
sincos / atan2.  Where every Cx is singular up to eps (one source; one frame) the complex64 restatement breaks down -- it
is off by 8 x the peak with one source -- and its error bounds nothing, so no bound here exceeds ``CEILING``.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NITERS = (0, 1, 2, 5)
EPS = 1e-10
# The most any bound may be, from the number formats and not from a run: the outputs and v are float32 (2^-24 = 6e-8
# relative per rounding; a float32 phase near pi rounds by 1.2e-7 rad), v is rounded once per pass, and 1e-5 = 170 x 2^-24
# leaves room for those roundings to add up over five passes and to be amplified by a rank-1 Cx, where the float64 oracle is
# itself only good to a few 1e-7 (with one source it differs from the mixture by 3.3e-7).  Float32 algebra -- the complex64
# restatement -- is at 2e-6 .. 3e-3 after five iterations and at 8 with one source, so it fails where this ceiling applies.
CEILING = 1e-5


def _frames_per_block():
    from deepconvsep_amd import _lib
    return int(_lib.load().dcs_mwf_frames_per_block())


def build_cases():
    """name -> dict(mag, phase [2,T,F], A [2,J,T,F] as handed to the call, ld, pre_div); every case runs at each of its niters"""
    from mwf_ref import make_case
    B = _frames_per_block()
    cases = {}

    def add(name, J, T, F, ld, niters, seed=1, dual_mono=False, pre_div=1.0, eps=EPS, oracle=True):
        mag, phase, A, _ = make_case(J, T, F, seed=seed, dual_mono=dual_mono)
        cases[name] = dict(mag=mag, phase=phase, A=A, ld=ld, pre_div=pre_div, niters=niters, eps=eps, oracle=oracle)
        return cases[name]

    add("panned3", 3, 37, 70, 72, NITERS)
    add("chunks4", 4, 2 * B + 5, 65, 65, NITERS)              # three chunks of frames, the last one ragged
    add("dualmono3", 3, 37, 70, 72, NITERS, dual_mono=True)
    add("one_source", 1, 37, 70, 72, (2,), seed=2)
    add("five_sources", 5, 37, 70, 72, (2,), seed=9)          # the most sources whose middle pass runs 8 waves
    add("six_sources", 6, B + 5, 33, 33, (3,), seed=10)       # 4-wave middle passes, twice, over two chunks of frames
    add("seven_sources", 7, 37, 70, 72, (2,), seed=11)
    add("eight_sources", 8, 37, 70, 72, (2,), seed=8)         # the largest J
    add("one_frame", 3, 1, 70, 72, (2,), seed=3)
    add("one_bin", 3, 37, 1, 3, (2,), seed=4)
    add("pre_div", 3, 37, 70, 72, (2,), seed=5, pre_div=0.3)
    add("many_chunks", 2, 40 * B + 5, 2, 2, (2,), seed=7)     # more chunks than sets of sums (32): a workgroup takes several
    z = add("zeros", 3, 37, 70, 72, (0, 2), seed=6)
    z["mag"][:, 5:10] = 0                                       # frames where mixture and estimates are all zero ...
    z["phase"][:, 5:10] = 0
    z["A"][:, :, 5:10] = 0
    z["A"][:, 1] = 0                                            # ... and a source that is zero everywhere
    # the same with an eps whose square underflows: properties only (the oracle's generic inverse has no eps left to work with)
    cases["zeros_tiny_eps"] = dict(z, niters=(2,), eps=1e-200, oracle=False)
    return cases


# ------------------------------------------------------------------------------------------------ the child process
def _child(poison, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from deepconvsep_amd.runtime import default_context

    G = 1 << 16
    blocks = []

    def alloc(shape):
        """float32 [red zone | payload | red zone], all poisoned"""
        n = int(np.prod(shape)) * 4
        pay = (n + 255) // 256 * 256
        raw = torch.full((pay + 2 * G,), poison, dtype=torch.uint8, device="cuda")
        blocks.append((raw, n))
        return raw[G:G + n].view(torch.float32).view(tuple(shape))

    def red_zone_damage():
        torch.cuda.synchronize()
        return sum(int((raw[:G] != poison).sum().item()) + int((raw[G + n:] != poison).sum().item()) for raw, n in blocks)

    def put(data, ld):
        t = alloc(data.shape[:-1] + (ld,))
        t[..., :data.shape[-1]].copy_(torch.from_numpy(np.ascontiguousarray(data)))
        return t

    def untouched(t):
        return bool((t.contiguous().view(torch.uint8) == poison).all().item())

    ctx = default_context()
    lib = ctx._lib
    vp = ctypes.c_void_p

    def call(mag_t, ph_t, src_t, om, op, ld, T, F, J, niter, pre_div, eps, null=None, h=None):
        ptr = [vp(t.data_ptr()) for t in (mag_t, ph_t, src_t, om, op)]
        if null is not None:
            ptr[null] = vp(None)
        rc = lib.dcs_mwf_f32(ctx._h if h is None else h, ptr[0], ptr[1], T * ld, ptr[2], J * T * ld, T * ld, ld, T, F, J, niter,
                             pre_div, eps, ptr[3], ptr[4])
        ctx.synchronize()
        return rc

    arrays, report = {}, {}
    for name, c in build_cases().items():
        J, T, F = c["A"].shape[1:]
        ld = c["ld"]
        mag_t, ph_t, src_t = put(c["mag"], ld), put(c["phase"], ld), put(c["A"], ld)
        for niter in c["niters"]:
            outs = []
            for _ in range(2):
                om, op = alloc((2, J, T, ld)), alloc((2, J, T, ld))
                rc = call(mag_t, ph_t, src_t, om, op, ld, T, F, J, niter, c["pre_div"], c["eps"])
                outs.append((om, op, rc))
            (om, op, rc), (om2, op2, rc2) = outs
            key = "%s@%d" % (name, niter)
            try:
                n_ws, guard_err = ctx.check_guards(), ""
            except Exception as exc:                                        # damaged scratch red zone: reported, not raised
                n_ws, guard_err = -1, str(exc)
            report[key] = dict(
                rc=[rc, rc2],
                same_twice=bool(torch.equal(om[..., :F].view(torch.int32), om2[..., :F].view(torch.int32)) and
                                torch.equal(op[..., :F].view(torch.int32), op2[..., :F].view(torch.int32))),
                padding_kept=untouched(om[..., F:]) and untouched(op[..., F:]) if ld > F else True,
                scratch_blocks=n_ws, scratch_guard=guard_err, red_zone_bytes_damaged=red_zone_damage())
            arrays[key + "/mag"] = om[..., :F].cpu().numpy()
            arrays[key + "/phase"] = op[..., :F].cpu().numpy()

    # arguments: DCS_EINVAL, nothing written
    c = build_cases()["panned3"]
    J, T, F = c["A"].shape[1:]
    ld = c["ld"]
    mag_t, ph_t, src_t = put(c["mag"], ld), put(c["phase"], ld), put(c["A"], ld)
    om, op = alloc((2, J, T, ld)), alloc((2, J, T, ld))
    good = dict(ld=ld, T=T, F=F, J=J, niter=1, pre_div=1.0, eps=EPS)
    bad = {"J=0": dict(J=0), "J=9": dict(J=9), "niter=-1": dict(niter=-1), "niter=101": dict(niter=101), "F=0": dict(F=0),
           "ld<F": dict(ld=F - 1), "pre_div=0": dict(pre_div=0.0), "pre_div<0": dict(pre_div=-1.0), "eps=0": dict(eps=0.0),
           "eps<0": dict(eps=-1e-10), "eps subnormal": dict(eps=1e-320), "null ctx": dict(h=vp(None))}
    for i, what in enumerate(("mag", "phase", "src", "out_mag", "out_phase")):
        bad["null " + what] = dict(null=i)
    args = {}
    for label, change in bad.items():
        rc = call(mag_t, ph_t, src_t, om, op, **dict(good, **change))
        args[label] = dict(rc=rc, untouched=untouched(om) and untouched(op))
    rc = call(mag_t, ph_t, src_t, om, op, **dict(good, T=0))
    args["n_frames=0"] = dict(rc=rc, untouched=untouched(om) and untouched(op))
    report["_args"] = args
    report["_red_zone_bytes_damaged"] = red_zone_damage()

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
    d = tmp_path_factory.mktemp("mwf")
    f_nan, f_big = str(d / "nan.npz"), str(d / "big.npz")
    p_nan, p_big = _start(0xFF, f_nan), _start(0x4B, f_big)
    try:
        refs = _references()
        nan_run, big_run = _finish(p_nan, f_nan), _finish(p_big, f_big)
    finally:
        for p in (p_nan, p_big):                        # whatever went wrong, no child outlives the fixture
            if p.poll() is None:
                p.kill()
                p.communicate()
    return dict(nan=nan_run, big=big_run, refs=refs, cases=build_cases())


def _references():
    """key -> (y_f64 [2,J,T,F], min(4 x the complex64 restatement's error, CEILING), max |X|), None for a case without an
    oracle; computed once, never modified"""
    from mwf_ref import mixture, mwf_em
    refs = {}
    for name, c in build_cases().items():
        A = c["A"] / np.float32(c["pre_div"])                               # float32 division, as the call does it
        assert A.dtype == np.float32
        peak = float(np.abs(mixture(c["mag"], c["phase"])).max())
        for niter in c["niters"]:
            if not c["oracle"]:
                refs["%s@%d" % (name, niter)] = None
                continue
            y64 = mwf_em(c["mag"], c["phase"], A, niter, c["eps"])
            y32 = mwf_em(c["mag"], c["phase"], A, niter, c["eps"], precision="c64")
            c64 = 4.0 * float(np.abs(y32 - y64).max()) / peak
            bound = c64 if c64 < CEILING else CEILING           # also when the restatement is not finite
            y64.setflags(write=False)
            refs["%s@%d" % (name, niter)] = (y64, bound, peak)
    return refs


def _error(runs, key):
    from mwf_ref import polar
    arrays, report = runs["nan"]
    y64, bound, peak = runs["refs"][key]
    assert report[key]["rc"] == [0, 0], report[key]
    om, op = arrays[key + "/mag"], arrays[key + "/phase"]
    assert om.dtype == np.float32 and op.dtype == np.float32 and om.shape == y64.shape
    assert np.isfinite(om).all() and np.isfinite(op).all(), key
    err = float(np.abs(polar(om, op) - y64).max()) / peak
    print("%s: max |y_gpu - y_f64| / max |X| = %.3g, bound (4 x complex64 restatement, at most %g) = %.3g"
          % (key, err, CEILING, bound))
    return err, bound, om, op


@pytest.mark.parametrize("niter", NITERS)
@pytest.mark.parametrize("name", ["panned3", "chunks4", "dualmono3"])
def test_parity_with_the_float64_oracle(runs, name, niter):
    """Measured on the MI355X (DESIGN.md section 4o has the table): the kernel's error is 4e-8 .. 9e-8 of the mixture's peak
    at every iteration count from 1 on, the bound grows from 8e-7 (niter 1) to the ceiling of 1e-5 (niter 5; dual-mono from
    niter 2 on)."""
    key = "%s@%d" % (name, niter)
    err, bound, om, op = _error(runs, key)
    assert err <= bound, (key, err, bound)
    if niter == 0:
        c = runs["cases"][name]
        assert np.array_equal(om, c["A"] / np.float32(c["pre_div"]))
        assert np.array_equal(op, np.broadcast_to(c["phase"][:, None], op.shape))


@pytest.mark.parametrize("name", ["one_source", "five_sources", "six_sources", "seven_sources", "eight_sources", "one_frame",
                                  "one_bin", "pre_div", "many_chunks", "zeros"])
def test_edges(runs, name):
    """Measured on the MI355X: one_source 4.8e-7 from the oracle and 3.5e-7 from the mixture, one_frame 1.4e-7, both
    under the ceiling of 1e-5 (their complex64 bounds would be 32 and 3e-3)."""
    from mwf_ref import mixture, polar
    key = "%s@%d" % (name, runs["cases"][name]["niters"][-1])
    err, bound, om, op = _error(runs, key)
    assert err <= bound, (key, err, bound)
    c = runs["cases"][name]
    if name == "one_source":
        # one source takes the whole mixture: W = I - eps Cx^{-1}
        peak = runs["refs"][key][2]
        err_x = float(np.abs(polar(om, op)[:, 0] - mixture(c["mag"], c["phase"])).max()) / peak
        print("one_source: max |y - x| / max |X| = %.3g" % err_x)
        assert err_x <= bound
    if name == "zeros":
        for k in (key, name + "@0"):
            m, p = runs["nan"][0][k + "/mag"], runs["nan"][0][k + "/phase"]
            assert np.isfinite(m).all() and np.isfinite(p).all()
            assert not m[:, :, 5:10].any(), k
            assert not m[:, 1].any(), k
        assert not om[:, :, 5:10].any() and not op[:, :, 5:10].any()         # zero magnitude, phase 0
        assert not op[:, 1].any()
        assert om[:, 0].any() and om[:, 2].any()


def test_zero_rows_stay_zero_when_eps_squared_underflows(runs):
    arrays, report = runs["nan"]
    key = "zeros_tiny_eps@2"
    assert report[key]["rc"] == [0, 0]
    om, op = arrays[key + "/mag"], arrays[key + "/phase"]
    assert np.isfinite(om).all() and np.isfinite(op).all()
    assert not om[:, :, 5:10].any() and not op[:, :, 5:10].any()
    assert not om[:, 1].any() and not op[:, 1].any()
    assert om[:, 0].any() and om[:, 2].any()


def test_memory_and_determinism(runs):
    (a_nan, r_nan), (a_big, r_big) = runs["nan"], runs["big"]
    keys = sorted(k for k in r_nan if not k.startswith("_"))
    assert keys == sorted(runs["refs"]) and sorted(r_big) == sorted(r_nan)
    problems = []
    for tag, (arrays, report) in (("0xFF", runs["nan"]), ("0x4B", runs["big"])):
        if report["_red_zone_bytes_damaged"]:
            problems.append("[%s] %d red-zone bytes of the ABI buffers changed" % (tag, report["_red_zone_bytes_damaged"]))
        for k in keys:
            r = report[k]
            if r["red_zone_bytes_damaged"]:
                problems.append("%s [%s]: %d red-zone bytes of the ABI buffers changed" % (k, tag, r["red_zone_bytes_damaged"]))
            if r["scratch_guard"] or r["scratch_blocks"] < 0:
                problems.append("%s [%s]: dcs_debug_check_guards: %s" % (k, tag, r["scratch_guard"]))
            if not r["padding_kept"]:
                problems.append("%s [%s]: output columns F .. ld-1 were written" % (k, tag))
            if not r["same_twice"]:
                problems.append("%s [%s]: two runs in one process differ" % (k, tag))
            if not (np.isfinite(arrays[k + "/mag"]).all() and np.isfinite(arrays[k + "/phase"]).all()):
                problems.append("%s [%s]: non-finite output" % (k, tag))
    for k in keys:
        for part in ("/mag", "/phase"):
            if a_nan[k + part].tobytes() != a_big[k + part].tobytes():
                problems.append("%s%s: outputs differ between the two scratch poisons" % (k, part))
    assert not problems, "\n".join(problems)
    # the switch was honoured: the filter's scratch is among the guarded blocks once an iteration has run
    assert r_nan["panned3@1"]["scratch_blocks"] >= 1, r_nan["panned3@1"]


def test_bad_arguments_are_refused_and_write_nothing(runs):
    from deepconvsep_amd import _lib
    for _, report in (runs["nan"], runs["big"]):
        args = dict(report["_args"])
        noop = args.pop("n_frames=0")
        assert noop == dict(rc=_lib.DCS_OK, untouched=True), noop
        assert len(args) == 17
        for label, r in args.items():
            assert r == dict(rc=_lib.DCS_EINVAL, untouched=True), (label, r)


def test_separator_composes_the_four_stages():
    import deepconvsep_amd as dcs
    from deepconvsep_amd.arch import TILER_LIBRARY
    from deepconvsep_amd.synth import synth_audio, synth_params
    sep = dcs.Separator("dsd_ild", synth_params("dsd_ild", 30, 513, seed=7), 0.3, 30, 25, 32, 513, 1024, 512, np.hanning,
                        tiler="library")
    audio = synth_audio(2 * 44100 + 21, seed=12, channels=2)
    plain = sep.separate_stereo(audio)
    assert np.array_equal(sep.separate_stereo(audio, mwf_iters=0), plain)

    got = sep.separate_stereo(audio, mwf_iters=2)
    assert got.shape == plain.shape == (audio.shape[0], 4, 2) and np.isfinite(got).all()
    assert not np.array_equal(got, plain)
    ctx = sep.ctx
    a = ctx.to_device(np.ascontiguousarray(audio.T), np.float32)
    mag, ph = sep.plan.forward_clips(a, phase=True)
    _, spectra = sep.net.separate_stereo(sep.plan, a, 25, TILER_LIBRARY, 0.3, want_spectra=True)
    om, op = dcs.mwf(ctx, mag, ph, spectra, 2, pre_div=0.3)
    for c in range(2):
        for j in range(4):
            pcm = ctx.to_host(sep.plan.inverse(om[c, j], op[c, j], n_out=audio.shape[0]))
            assert np.array_equal(pcm.astype(np.float64), got[:, j, c]), (c, j)


def test_separate_script_writes_what_the_separator_returns(tmp_path):
    """examples/dsd100_2ch_ILD/separate_dsd_ild.py --mwf 1: one stereo wav per source, the int16 truncation of
    ``Separator.separate_stereo(audio, mwf_iters=1)`` on the samples the wav file holds."""
    import importlib.util
    import scipy.io.wavfile
    import deepconvsep_amd as dcs
    from deepconvsep_amd.separation import read_wav, save_model, write_wav
    from deepconvsep_amd.stereo_training import SOURCES
    from deepconvsep_amd.synth import synth_audio, synth_params
    spec = importlib.util.spec_from_file_location(
        "separate_dsd_ild", os.path.join(ROOT, "examples", "dsd100_2ch_ILD", "separate_dsd_ild.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    params = synth_params("dsd_ild", 30, 513, seed=7)
    model, wav, out = str(tmp_path / "model.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "out")
    save_model(model, params)
    write_wav(wav, 0.5 * synth_audio(44100 + 21, seed=13, channels=2), 44100)
    script.main(["-i", wav, "-o", out, "-m", model, "--mwf", "1"])
    _, audio = read_wav(wav)
    sep = dcs.Separator("dsd_ild", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning)
    want = sep.separate_stereo(audio, mwf_iters=1)
    for i, name in enumerate(SOURCES):
        rate, got = scipy.io.wavfile.read(os.path.join(out, name + ".wav"))
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (len(audio), 2)
        assert np.array_equal(got, (want[:, i, :] * 32767).astype(np.int16)), name


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
