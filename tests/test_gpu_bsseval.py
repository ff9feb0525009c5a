"""BSS Eval on the MI355X (csrc/bsseval.hip via deepconvsep_amd.evaluation) against the float64 restatement
tests/bsseval_ref.py: exact lag correlations, agreement in dB, closed forms, framewise structure, silence, determinism,
the guard-band harness and the three command lines of examples/evaluation."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io.wavfile
import scipy.signal

import bsseval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

T = 1 << 18


@pytest.fixture(scope="module")
def ev():
    from deepconvsep_amd import evaluation
    return evaluation


def _signals(kind, n, seed, length=T):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((n, length))
    if kind == "white":
        return w
    if kind.startswith("ar"):
        rho = float(kind[2:])
        return scipy.signal.lfilter([1.0], [1.0, -rho], w, axis=1)
    if kind == "sine":                              # sinusoids plus a -60 dB noise floor
        t = np.arange(length)
        f = rng.uniform(0.01, 0.2, n)
        return np.sin(2 * np.pi * f[:, None] * t[None, :] + rng.uniform(0, 6, n)[:, None]) + 1e-3 * w
    raise ValueError(kind)


def _estimates(s, seed):
    """each estimate: its source through a short filter, some of the next source, some noise"""
    rng = np.random.default_rng(seed)
    h = np.concatenate([[1.0], 0.3 * rng.standard_normal(7)])
    f = scipy.signal.lfilter(h, [1.0], s, axis=-1)
    return f + 0.25 * np.roll(s, 1, axis=0) + 0.05 * rng.standard_normal(s.shape) * s.std()


def _close(got, want, tol):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    m = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), m), (got, want)
    if m.any():
        err = np.max(np.abs(got[m] - want[m]))
        assert err <= tol, (err, got, want)


# ---------------------------------------------------------------------------------------------------- lag correlations
@pytest.mark.parametrize("n_ref,n_est,length,flen", [(4, 4, 1 << 16, 64), (1, 1, 1 << 17, 512)])
def test_lagcorr_is_bit_identical_to_int64(ev, n_ref, n_est, length, flen):
    rng = np.random.default_rng(7)
    r = rng.integers(-32768, 32768, (n_ref, length))
    e = rng.integers(-32768, 32768, (n_est, length))
    got = ev.lagcorr(r.astype(np.float64), e.astype(np.float64), flen)
    want = ref.lagcorr_int(r, e, flen)
    assert got.shape == want.shape
    assert np.array_equal(got, want.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- agreement
@pytest.mark.parametrize("kind,flen,nsrc", [("white", 512, 4), ("ar0.9", 64, 4), ("ar0.99", 512, 2), ("ar0.99", 64, 2),
                                            ("white", 64, 2), ("ar0.9", 512, 2)])
def test_sources_agree_with_the_restatement(ev, kind, flen, nsrc):
    s = _signals(kind, nsrc, 11)
    se = _estimates(s, 12)[::-1].copy()          # reversed: the permutation has work to do
    got = ev.bss_eval_sources(se, s, flen)
    want = ref.bss_eval_sources(se, s, flen)
    assert list(got[3]) == list(want[3])
    for g, w in zip(got[:3], want[:3]):
        _close(g, w, 1e-4)


@pytest.mark.parametrize("kind,flen,nsrc", [("white", 64, 4), ("ar0.9", 512, 2), ("ar0.99", 64, 2), ("white", 512, 2)])
def test_images_agree_with_the_restatement(ev, kind, flen, nsrc):
    s = _signals(kind, 2 * nsrc, 21).reshape(nsrc, 2, T).transpose(0, 2, 1)     # [nsrc, T, nchan]
    ie = _estimates(s.transpose(0, 2, 1), 22).transpose(0, 2, 1)
    ie = ie[np.roll(np.arange(nsrc), 1)].copy()
    got = ev.bss_eval_images(ie, s, flen)
    want = ref.bss_eval_images(ie, s, flen)
    assert list(got[4]) == list(want[4])
    for g, w in zip(got[:4], want[:4]):
        _close(g, w, 1e-4)


def test_sinusoids_with_a_minus_60_db_floor(ev):
    s = _signals("sine", 2, 31)
    se = _estimates(s, 32)
    got = ev.bss_eval_sources(se, s, 64)
    want = ref.bss_eval_sources(se, s, 64)
    assert list(got[3]) == list(want[3])
    for g, w in zip(got[:3], want[:3]):
        _close(g, w, 1e-3)


def test_framewise_agrees_and_equals_standalone_windows(ev):
    nsrc, nchan, win, ove, flen = 2, 2, 1 << 16, 1 << 15, 64
    n = T + 5000                                  # the last window MATLAB's formula counts would overrun
    s = _signals("ar0.9", nsrc * nchan, 41, n).reshape(nsrc, nchan, n).transpose(2, 1, 0)    # [T, nchan, nsrc]
    ie = _estimates(s.transpose(2, 1, 0), 42).transpose(2, 1, 0).copy()
    got = ev.bss_eval(ie, s, win, ove, flen)
    assert got[0].shape == (nsrc, ev.framewise_count(n, win, ove)) == (nsrc, 7)
    want = ref.bss_eval(ie, s, win, ove, flen)
    for g, w in zip(got, want):
        _close(g, w, 1e-4)
    for k in (0, 3, 6):
        sl = slice(k * ove, k * ove + win)
        one = ev.bss_eval_images(ie[sl].transpose(2, 0, 1), s[sl].transpose(2, 0, 1), flen)
        assert list(one[4]) == list(range(nsrc))
        for g, w in zip(got, one[:4]):
            _close(g[:, k], w, 1e-9)
    assert all(x.shape == (nsrc, 0) for x in ev.bss_eval(ie[:win - 1], s[:win - 1], win, ove, flen))


def test_shuffled_estimates_give_the_inverse_permutation(ev):
    s = _signals("white", 3, 51, 1 << 16)
    se = _estimates(s, 52)
    base = ev.bss_eval_sources(se, s, 64)
    assert list(base[3]) == [0, 1, 2]
    order = np.array([2, 0, 1])
    sh = ev.bss_eval_sources(se[order], s, 64)
    assert list(order[sh[3]]) == [0, 1, 2]
    for a, b in zip(base[:3], sh[:3]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- closed forms
def _tail_zero(n, seed, flen=64):
    s = np.random.default_rng(seed).standard_normal((n, 1 << 17))
    s[:, -flen:] = 0.0
    return s


def test_closed_forms_on_the_gpu(ev):
    s = _tail_zero(3, 61)
    for v in ev.bss_eval_sources(s, s, 64)[:3]:
        assert np.all(v >= 100.0), v
    for v in ev.bss_eval_images(s[:, :, None], s[:, :, None], 64)[:4]:
        assert np.all(v >= 100.0), v
    h = np.random.default_rng(62).standard_normal(48)
    e = np.array([np.convolve(x, h)[:s.shape[1]] for x in s])
    for v in ev.bss_eval_sources(e, s, 64)[:3]:
        assert np.all(v >= 100.0), v
    isr = ev.bss_eval_images(e[:, :, None], s[:, :, None], 64)[1]
    np.testing.assert_allclose(isr, [10 * np.log10((x @ x) / ((y - x) @ (y - x))) for x, y in zip(s, e)], rtol=0,
                               atol=1e-6)
    g = 0.1
    e = s.copy()
    e[0] = s[0] + g * s[1]
    assert abs(ev.bss_eval_sources(e, s, 64)[1][0] - 10 * np.log10((s[0] @ s[0]) / (g * g * (s[1] @ s[1])))) < 0.01
    noise = 0.05 * np.random.default_rng(63).standard_normal(s.shape[1])
    e = s.copy()
    e[2] = s[2] + noise
    assert abs(ev.bss_eval_sources(e, s, 64)[2][2] - 10 * np.log10((s[2] @ s[2]) / (noise @ noise))) < 0.05


# ---------------------------------------------------------------------------------------------------- silence, determinism
def test_a_reference_silent_in_one_window(ev):
    nsrc, nchan, win, ove, flen = 3, 2, 1 << 14, 1 << 13, 64
    n = 5 * ove
    s = _signals("white", nsrc * nchan, 71, n).reshape(nsrc, nchan, n).transpose(2, 1, 0).copy()
    s[ove:ove + win, :, 1] = 0.0                 # source 1 silent in window 1 exactly
    ie = _estimates(s.transpose(2, 1, 0), 72).transpose(2, 1, 0).copy()
    got = ev.bss_eval(ie, s, win, ove, flen)
    for v in got:
        assert np.isnan(v[1, 1]) and np.isfinite(np.delete(v.ravel(), [1 * v.shape[1] + 1])).all()
    want = ref.bss_eval(ie, s, win, ove, flen)    # the restatement drops the silent channels from the span
    for g, w in zip(got, want):
        _close(g, w, 1e-4)


def test_two_runs_are_bit_identical(ev):
    s = _signals("ar0.9", 4, 81).reshape(2, 2, T).transpose(0, 2, 1)
    ie = _estimates(s.transpose(0, 2, 1), 82).transpose(0, 2, 1)
    rows = lambda x: x.transpose(0, 2, 1).reshape(4, T)
    a = ev.energies(rows(s), rows(ie), 2, flen=512)
    b = ev.energies(rows(s), rows(ie), 2, flen=512)
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_bad_arguments_raise(ev):
    x = np.zeros((17, 1000))
    with pytest.raises(NotImplementedError):
        ev.energies(x, x[:1], 1, flen=64)
    with pytest.raises(ValueError):
        ev.energies(x[:2], x[:2], 1, flen=24)
    with pytest.raises(ValueError):
        ev.energies(x[:2], x[:2], 1, win=600, hop=500, nwin=2, flen=64)


# ---------------------------------------------------------------------------------------------------- guard harness
_CHILD = r'''
import hashlib, json, sys
ROOT, POISON, OUT = sys.argv[1], int(sys.argv[2]), sys.argv[3]
sys.path.insert(0, ROOT)
import numpy as np
import torch
from deepconvsep_amd import runtime
from deepconvsep_amd import evaluation as ev

G = 1 << 16
blocks = []


class GuardedTorch(object):
    """torch, with the device copies made by runtime.Context placed between poisoned red zones"""
    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, shape, dtype=None, device=None):
        shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full(((nbytes + 255) // 256 * 256 + 2 * G,), POISON, dtype=torch.uint8, device=device)
        blocks.append((raw, nbytes))
        return raw[G:G + nbytes].view(dtype).view(shape)

    def from_numpy(self, a):
        gt = self

        class _H(object):
            def to(self, device):
                t = torch.from_numpy(a)
                out = gt.empty(t.shape, t.dtype, device)
                out.copy_(t)
                return out
        return _H()


runtime._torch = lambda: GuardedTorch()
ctx = runtime.default_context()
res = {}
rng = np.random.default_rng(3)
cases = {
    "sources_512": (rng.standard_normal((4, 1 << 16)), 1, 1 << 16, 1 << 16, 1, 512, True, 4),
    "images_64": (rng.standard_normal((6, 50000)), 2, 50000, 50000, 1, 64, True, 6),
    "framewise_groups": (rng.standard_normal((4, 1 << 15)), 2, 1 << 13, 1 << 12, 7, 128, False, 4),
    "ragged_flen_48": (rng.standard_normal((3, 12345)), 1, 12345, 12345, 1, 48, True, 2),
}
for name, (r, nchan, win, hop, nwin, flen, pairs, n_est) in cases.items():
    e = r[:n_est] * 0.7 + 0.1 * rng.standard_normal((n_est, r.shape[1]))
    out = ev.energies(r, e, nchan, win=win, hop=hop, nwin=nwin, flen=flen, all_pairs=pairs, ctx=ctx)
    torch.cuda.synchronize()
    bad = sum(int((raw[:G] != POISON).sum().item()) + int((raw[G + n:] != POISON).sum().item()) for raw, n in blocks)
    try:
        n_ws, err = ctx.check_guards(), ""
    except Exception as exc:
        n_ws, err = -1, str(exc)
    res[name] = {"sha256": hashlib.sha256(out.tobytes()).hexdigest(), "finite": bool(np.isfinite(out).all()),
                 "abi_bad": bad, "scratch_guard": err, "scratch_blocks": n_ws}
lc = ev.lagcorr(rng.standard_normal((3, 9999)), rng.standard_normal((2, 9999)), 80, ctx=ctx)
res["lagcorr"] = {"sha256": hashlib.sha256(lc.tobytes()).hexdigest(), "finite": bool(np.isfinite(lc).all()),
                  "abi_bad": 0, "scratch_guard": "", "scratch_blocks": ctx.check_guards()}
json.dump(res, open(OUT, "w"))
'''


def test_guard_harness(tmp_path):
    runs = {}
    procs = []
    for poison in (0xFF, 0x4B):
        out = str(tmp_path / ("%d.json" % poison))
        env = dict(os.environ)
        env.update({"DCS_WS_GUARD": "65536", "DCS_WS_POISON": str(poison)})
        procs.append((poison, out, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(poison), out], env=env,
                                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for poison, out, p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (poison, so[-800:], se[-2500:])
        with open(out) as fh:
            runs[poison] = json.load(fh)
    a, b = runs[0xFF], runs[0x4B]
    assert sorted(a) == sorted(b) and len(a) == 5
    for name in a:
        for r in (a[name], b[name]):
            assert r["abi_bad"] == 0 and not r["scratch_guard"] and r["finite"] and r["scratch_blocks"] >= 1, (name, r)
        assert a[name]["sha256"] == b[name]["sha256"], name


# ---------------------------------------------------------------------------------------------------- command lines
def _wav(path, x, rate=8000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    scipy.io.wavfile.write(path, rate, np.clip(x * 12000, -32767, 32767).astype(np.int16))
    return scipy.io.wavfile.read(path)[1].astype(np.float64) / 32767.0


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "evaluation", script)] + list(args),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2500:])


def _val(x):
    return np.nan if x is None else float(x)


def test_cli_dsd100(tmp_path):
    rate, n = 8000, 8000 * 50
    rng = np.random.default_rng(91)
    names = ["bass", "drums", "other", "vocals"]
    song = "001 - Song"
    refs, ests = [], []
    for q, s in enumerate(names):
        x = 0.3 * rng.standard_normal((n, 2)) if q != 1 else 0.3 * rng.standard_normal(n)   # drums mono
        refs.append(_wav(str(tmp_path / "ds" / "Sources" / "Dev" / song / (s + ".wav")), x, rate))
        fname = s + ".wav" if q % 2 == 0 else "mixture_" + ("others" if s == "other" else s) + ".wav"
        y = 0.8 * x + 0.05 * rng.standard_normal(x.shape)
        ests.append(_wav(str(tmp_path / "est" / "Dev" / song / fname), y[: n - 100], rate))
    out = str(tmp_path / "r.json")
    _run("eval_dsd100.py", str(tmp_path / "ds"), str(tmp_path / "est"), "-o", out, "--flen", "64")
    got = json.load(open(out))["Dev"][song]
    st = lambda x: np.repeat(x[:, None], 2, axis=1) if x.ndim == 1 else x
    m = n - 100
    i = np.stack([st(x)[:m] for x in refs], axis=2)
    ie = np.stack([st(x)[:m] for x in ests], axis=2)
    want = ref.bss_eval(ie, i, 30 * rate, 15 * rate, 64)
    for q, s in enumerate(names):
        for k, key in enumerate(("SDR", "ISR", "SIR", "SAR")):
            _close([_val(v) for v in got[s][key]], want[k][q], 1e-4)
    acc = ref.bss_eval(np.stack([ie[:, :, 3], ie[:, :, :3].sum(2)], 2), np.stack([i[:, :, 3], i[:, :, :3].sum(2)], 2),
                       30 * rate, 15 * rate, 64)
    _close([_val(v) for v in got["accompaniment"]["SDR"]], acc[0][1], 1e-4)
    assert abs(got["vocals"]["median"]["SDR"] - np.nanmedian(want[0][3])) < 1e-4


def test_cli_ikala(tmp_path):
    rate, n = 8000, 8000 * 3
    rng = np.random.default_rng(92)
    mix = _wav(str(tmp_path / "Wavfile" / "10161_chorus.wav"), 0.3 * rng.standard_normal((n, 2)), rate)
    ev_ = _wav(str(tmp_path / "out" / "10161_chorus-voice.wav"), mix[:, 1] * 0.9 + 0.1 * mix[:, 0], rate)
    em = _wav(str(tmp_path / "out" / "10161_chorus-music.wav"), mix[:, 0] * 0.9 + 0.1 * mix[:, 1], rate)
    out = str(tmp_path / "r.json")
    _run("eval_ikala.py", str(tmp_path / "Wavfile"), str(tmp_path / "out"), "-o", out, "--flen", "64")
    got = json.load(open(out))["10161_chorus"]
    true = np.stack([mix[:, 1], mix[:, 0]])
    est = np.stack([ev_, em])
    tn = true / np.linalg.norm(true[0] + true[1])
    sdr, sir, sar, perm = ref.bss_eval_sources(est / np.linalg.norm(est[0] + est[1]), tn, 64)
    mx = np.stack([(true[0] + true[1]) / 2] * 2)
    msdr = ref.bss_eval_sources(mx / np.linalg.norm(mx[0] + mx[1]), tn, 64)[0]
    assert got["perm"] == list(perm)
    for q, s in enumerate(["voice", "music"]):
        assert abs(got[s]["SDR"][0] - sdr[q]) < 1e-4 and abs(got[s]["SIR"][0] - sir[q]) < 1e-4
        assert abs(got[s]["NSDR"][0] - (sdr[q] - msdr[q])) < 1e-4


def test_cli_bach10(tmp_path):
    rate, n = 8000, 8000 * 3
    rng = np.random.default_rng(93)
    inst = ["bassoon", "clarinet", "saxphone", "violin"]
    song = "01-AchGottundHerr"
    refs, ests = [], []
    for q, s in enumerate(inst):
        x = 0.3 * rng.standard_normal(n)
        refs.append(_wav(str(tmp_path / "ds" / "Sources" / song / ("%s-%s.wav" % (song, s))), x, rate))
    for q, s in enumerate(inst):                          # estimates written in a shuffled order
        y = 0.9 * refs[(q + 1) % 4] + 0.1 * refs[q]
        ests.append(_wav(str(tmp_path / "est" / ("%s-%s.wav" % (song, s))), y, rate))
    out = str(tmp_path / "r.json")
    _run("eval_bach10.py", str(tmp_path / "ds"), str(tmp_path / "est"), "-o", out, "--flen", "64")
    got = json.load(open(out))[song]
    sdr, sir, sar, perm = ref.bss_eval_sources(np.stack(ests), np.stack(refs), 64)
    assert got["perm"] == list(perm) == [3, 0, 1, 2]
    for q, s in enumerate(inst):
        for key, w in (("SDR", sdr), ("SIR", sir), ("SAR", sar)):
            assert abs(got[s][key][0] - w[q]) < 1e-4, (s, key)
