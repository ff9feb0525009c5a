"""``dcs_mask_fold_apply`` on the MI355X against the float64 reference of tests/chanmask_ref.py, on synthetic network outputs
(no network: nothing here is ill-conditioned).

The harness is that of tests/test_gpu_mwf.py: every case runs through the C ABI in a child process started with
``DCS_WS_GUARD``, on buffers carved out of an arena of this file's own -- a 64 KiB red zone on either side of every input and
output, outputs and the padding columns ``F .. ld-1`` poisoned.  Two children, poison 0xFF (float32 NaN) and 0x4B (1.3e7),
run side by side; each runs every case twice with both outputs, then once with the estimates alone and once with the masks alone.

Bound (chanmask_ref.bound): ``|est - est_ref| <= (S + 2 m + 4) 2^-23 mag[c, t, f]`` with ``m = ceil(ov / st) + 1`` the tiles
that can reach one frame -- twice the first-order float32 rounding count (S - 1 additions, the eps addition, one division, two
roundings per fold step, one product); the same with ``mag = 1`` for the masks.
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


# ------------------------------------------------------------------------------------------------ the child process
def _child(poison, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from chanmask_ref import CONVENTIONS, build_cases
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
        if data.size == 0:                      # no tiles: one poisoned float nobody may read (an empty tensor has no address)
            return alloc((1,))
        t = alloc(data.shape[:-1] + (ld,))
        t[..., :data.shape[-1]].copy_(torch.from_numpy(np.ascontiguousarray(data)))
        return t

    def untouched(t):
        return bool((t.contiguous().view(torch.uint8) == poison).all().item())

    def same(a, b):
        return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))

    ctx = default_context()
    lib = ctx._lib
    vp = ctypes.c_void_p

    def call(p_t, mag_t, est, mask, n, S, tc, ov, F, conv, C, T, ld, null=(), h=None, rise=True):
        ramp = np.ascontiguousarray(np.linspace(0.0, 1.0, num=max(ov, 0)), dtype=np.float64)
        ptr = dict(p=vp(p_t.data_ptr()), mag=vp(mag_t.data_ptr()), est=vp(est.data_ptr()) if est is not None else vp(None),
                   mask=vp(mask.data_ptr()) if mask is not None else vp(None))
        for k in null:
            ptr[k] = vp(None)
        rise_p = ramp.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if rise else None
        rc = lib.dcs_mask_fold_apply(ctx._h if h is None else h, ptr["p"], n * tc * max(F, 0), n, S, tc, ov, F, CONVENTIONS.index(conv),
                                     rise_p, ptr["mag"], T * ld, C, T, ld, ptr["est"], S * T * ld, T * ld, ptr["mask"], T * ld)
        ctx.synchronize()
        return rc

    arrays, report = {}, {}
    cases = build_cases()
    for name, c in cases.items():
        S, F, ld, tc, ov, T = c["S"], c["F"], c["ld"], c["tc"], c["ov"], c["n_frames"]
        n, C = c["p"].shape[1], c["mag"].shape[0]
        p_t, mag_t = put(c["p"], F), put(c["mag"], ld)
        args = (n, S, tc, ov, F, c["conv"], C, T, ld)
        outs = []
        for _ in range(2):
            est, mask = alloc((C, S, T, ld)), alloc((S, T, ld))
            outs.append((est, mask, call(p_t, mag_t, est, mask, *args)))
        (est, mask, rc), (est2, mask2, rc2) = outs
        est_only, mask_only = alloc((C, S, T, ld)), alloc((S, T, ld))
        rc3 = call(p_t, mag_t, est_only, None, *args)
        rc4 = call(p_t, mag_t, None, mask_only, *args)
        try:
            n_ws, guard_err = ctx.check_guards(), ""
        except Exception as exc:                                        # damaged red zone of a libdcs block: reported, not raised
            n_ws, guard_err = -1, str(exc)
        report[name] = dict(
            rc=[rc, rc2, rc3, rc4],
            same_twice=same(est[..., :F], est2[..., :F]) and same(mask[..., :F], mask2[..., :F]),
            alone_equal=same(est[..., :F], est_only[..., :F]) and same(mask[..., :F], mask_only[..., :F]),
            padding_kept=all(untouched(t[..., F:]) for t in (est, mask, est2, mask2, est_only, mask_only)) if ld > F else True,
            guarded_blocks=n_ws, guard=guard_err, red_zone_bytes_damaged=red_zone_damage())
        arrays[name + "/est"] = est[..., :F].cpu().numpy()
        arrays[name + "/mask"] = mask[..., :F].cpu().numpy()
        del blocks[:]                                                   # checked: the next case's arena starts empty

    # arguments: DCS_EINVAL, nothing written
    c = cases["tc30_ov25_n11_S4_C2_A_equal_F513"]
    S, F, ld, tc, ov, T = c["S"], c["F"], c["ld"], c["tc"], c["ov"], c["n_frames"]
    n, C = c["p"].shape[1], c["mag"].shape[0]
    p_t, mag_t = put(c["p"], F), put(c["mag"], ld)
    est, mask = alloc((C, S, T, ld)), alloc((S, T, ld))
    good = dict(n=n, S=S, tc=tc, ov=ov, F=F, conv=c["conv"], C=C, T=T, ld=ld)
    bad = {"S=0": dict(S=0), "S=9": dict(S=9), "C=0": dict(C=0), "C=9": dict(C=9), "overlap=0": dict(ov=0),
           "overlap=tc": dict(ov=tc), "F=0": dict(F=0), "ld<F": dict(ld=F - 1), "null p": dict(null=("p",)),
           "null mag": dict(null=("mag",)), "null rise": dict(rise=False), "both outputs null": dict(null=("est", "mask")),
           "null ctx": dict(h=vp(None))}
    res = {}
    for label, change in bad.items():
        rc = call(p_t, mag_t, est, mask, **dict(good, **change))
        res[label] = dict(rc=rc, untouched=untouched(est) and untouched(mask))
    report["_args"] = res
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


def _references(cases):
    """name -> (est_f64 [C, S, T, F], mask_f64 [S, T, F]); computed once, never modified"""
    from chanmask_ref import chanmask_ref
    refs = {}
    for name, c in cases.items():
        est, mask = chanmask_ref(c["p"][:c["S"]], c["mag"], c["ov"], c["conv"], c["n_frames"])
        est.setflags(write=False)
        mask.setflags(write=False)
        refs[name] = (est, mask)
    return refs


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """both children, side by side; the references are computed while they run"""
    from chanmask_ref import build_cases
    d = tmp_path_factory.mktemp("chanmask")
    f_nan, f_big = str(d / "nan.npz"), str(d / "big.npz")
    p_nan, p_big = _start(0xFF, f_nan), _start(0x4B, f_big)
    try:
        cases = build_cases()
        refs = _references(cases)
        nan_run, big_run = _finish(p_nan, f_nan), _finish(p_big, f_big)
    finally:
        for p in (p_nan, p_big):                        # whatever went wrong, no child outlives the fixture
            if p.poll() is None:
                p.kill()
                p.communicate()
    return dict(nan=nan_run, big=big_run, refs=refs, cases=cases)


def _case_names():
    for d in (ROOT, os.path.join(ROOT, "tests")):        # also when this file runs as the child process
        if d not in sys.path:
            sys.path.insert(0, d)
    from chanmask_ref import build_cases
    return sorted(build_cases())


@pytest.mark.parametrize("name", _case_names())
def test_estimates_and_masks_meet_the_rounding_bound(runs, name):
    """Measured on the MI355X: the worst case is at 0.13 of the bound (masks 1.5e-7, estimates 1.8e-7 of the magnitude), the
    figure a float32 NumPy restatement of the kernel gives on the same cases."""
    from chanmask_ref import bound
    c = runs["cases"][name]
    arrays, report = runs["nan"]
    est_ref, mask_ref = runs["refs"][name]
    assert report[name]["rc"] == [0, 0, 0, 0], report[name]
    est, mask = arrays[name + "/est"], arrays[name + "/mask"]
    assert est.dtype == np.float32 and est.shape == est_ref.shape and mask.shape == mask_ref.shape
    assert np.isfinite(est).all() and np.isfinite(mask).all()
    S, tc, ov = c["S"], c["tc"], c["ov"]
    mag = c["mag"].astype(np.float64)[:, None]
    unit = float(bound(S, tc, ov))
    if est.size:
        e_mask = float(np.abs(mask - mask_ref).max())
        ratio = np.abs(est - est_ref) / np.where(mag > 0, mag, 1.0)
        e_est = float(ratio.max())
        print("%s: max |mask - ref| = %.3g, max |est - ref| / mag = %.3g, bound %.3g" % (name, e_mask, e_est, unit))
        assert np.all(np.abs(mask - mask_ref) <= unit), (name, e_mask, unit)
        assert np.all(np.abs(est - est_ref) <= bound(S, tc, ov, mag)), (name, e_est, unit)
    # rows past the last tile are exactly zero
    n = c["p"].shape[1]
    covered = min(c["n_frames"], (n - 1) * (tc - ov) + tc) if n else 0
    assert not mask[:, covered:].any() and not est[:, :, covered:].any()
    if covered and c["conv"] == "A" and ov > 1:
        assert mask[:, :covered].any()
    # the planted column where every source is zero: 1 / S (A) or exactly 0 (B) wherever one tile alone covers the frame
    if n:
        first = mask[:, :tc - ov, 3]
        assert np.all(np.abs(first - 1.0 / S) <= unit) if c["conv"] == "A" else not first.any()


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
            if r["rc"] != [0, 0, 0, 0]:
                problems.append("%s [%s]: status %r" % (k, tag, r["rc"]))
            if r["red_zone_bytes_damaged"]:
                problems.append("%s [%s]: %d red-zone bytes of the ABI buffers changed" % (k, tag, r["red_zone_bytes_damaged"]))
            if r["guard"] or r["guarded_blocks"] < 0:
                problems.append("%s [%s]: dcs_debug_check_guards: %s" % (k, tag, r["guard"]))
            if not r["padding_kept"]:
                problems.append("%s [%s]: output columns F .. ld-1 were written" % (k, tag))
            if not r["same_twice"]:
                problems.append("%s [%s]: two runs in one process differ" % (k, tag))
            if not r["alone_equal"]:
                problems.append("%s [%s]: an output asked for alone differs from the same output asked for with the other" % (k, tag))
            if not (np.isfinite(arrays[k + "/est"]).all() and np.isfinite(arrays[k + "/mask"]).all()):
                problems.append("%s [%s]: non-finite output" % (k, tag))
    for k in keys:
        for part in ("/est", "/mask"):
            if a_nan[k + part].tobytes() != a_big[k + part].tobytes():
                problems.append("%s%s: outputs differ between the two poisons" % (k, part))
    assert not problems, "\n".join(problems)
    # the switch was honoured: the context's ramp is among the guarded blocks
    assert r_nan[keys[0]]["guarded_blocks"] >= 1, r_nan[keys[0]]


def test_bad_arguments_are_refused_and_write_nothing(runs):
    from deepconvsep_amd import _lib
    for _, report in (runs["nan"], runs["big"]):
        args = dict(report["_args"])
        assert len(args) == 13
        for label, r in args.items():
            assert r == dict(rc=_lib.DCS_EINVAL, untouched=True), (label, r)


if __name__ == "__main__":
    _child(int(sys.argv[1]), sys.argv[2])
