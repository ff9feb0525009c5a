"""The one-batch kernels of csrc/dsd_lat.hip that no other module launches alone -- ``lat_gemm_kernel<J, NA>`` in all ten
instances, ``lat_stft_kernel<9|10>`` on its whole-frame and its clamped path, ``lat_ifft_kernel<9|10, 4>`` and ``lat_ola_kernel<2|4>``
-- on the MI355X, one launch at a time, against float64.

The launches are reached through ``dcs_debug_lat_gemm`` / ``dcs_debug_lat_stft_forward_f32`` / ``dcs_debug_lat_stft_inverse_f32``
(the launchers net.hip calls, every address checked on the host first).  One child process under its own ``timeout -k 10``
(``CHILD_LIMIT``; a child that ends in a signal or at its limit ends the run), with ``DCS_WS_GUARD``.  Every launch runs on
buffers exactly as long as the aid's extents, carved out of one poisoned allocation with 64 KiB between and around them; every
data set of a case runs under the poisons 0xFF and 0x4B and a third time over its own output.  The child writes what the launches
wrote, the parent compares by the rules of tests/lat_ref.py.

Measured on the MI355X: the child 3.4 s, of which 0.7 s are the 771 launches; the module 5.7 s.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import lat_ref as lr
import stft_ref as sr
from gemm_ref import measure
from oracle import stft_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GB = 1 << 16
CHILD_LIMIT = 40                       # seconds; the child took 3.4 s on the MI355X, library load included
vp, i64 = ctypes.c_void_p, ctypes.c_int64
GEMM_CASES, FWD_CASES, INV_CASES = lr.gemm_cases(), lr.forward_cases(), lr.inverse_cases()
REFUSAL_BASES = ("conv2_nz4_parts4", "fc1x_M21_parts1")


def c_index(c):
    """[parts][M][n_store] float offsets into the C buffer"""
    z = np.arange(max(c["nz"], 1))[:, None, None] * c["c_part_stride"]
    return z + np.arange(c["M"])[None, :, None] * c["ldc"] + np.arange(c["n_store"])[None, None, :]


def a_flat(c, inp):
    flat = np.full(lr.extents(c)["A"], np.nan, dtype=np.float32)
    for p in range(c["a_parts"]):
        flat[p * c["a_part_stride"]:p * c["a_part_stride"] + c["n_A1"]] = inp["A"][p]
    return flat


# ------------------------------------------------------------------------------------------------ the child process
def child(out_path):
    import torch
    from deepconvsep_amd.runtime import StftPlan, default_context

    ctx = default_context()
    lib = ctx._lib
    arrays, report = {}, {}
    plans = {}

    def plan(N, hop):
        if (N, hop) not in plans:
            plans[(N, hop)] = StftPlan(ctx, N, hop, sr.window(N))
        return plans[(N, hop)]

    def arena(sizes, poison, skew=None):
        """sizes {name: bytes}; buffers 256-byte aligned plus skew[name] bytes, GB poisoned bytes between and around them"""
        place, off = {}, GB
        for name, nbytes in sizes.items():
            sk = (skew or {}).get(name, 0)
            place[name] = (off + sk, nbytes)
            off += (nbytes + sk + 255) // 256 * 256 + GB
        raw = torch.full((off,), poison, dtype=torch.uint8, device="cuda")
        assert raw.data_ptr() % 256 == 0
        return raw, place

    def put(raw, place, name, host):
        off, nbytes = place[name]
        b = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert b.size == nbytes, (name, b.size, nbytes)
        raw[off:off + nbytes].copy_(torch.from_numpy(b))

    def finish(raw, place, poison, owns):
        """owns {buffer: boolean byte mask of what the launch owns, or None for all of it}; returns (host copies of the outputs,
        whether every other byte of them is still poison, bytes changed outside every buffer)"""
        ctx.synchronize()
        host, untouched = {}, True
        for name, own in owns.items():
            off, nbytes = place[name]
            host[name] = raw[off:off + nbytes].cpu().numpy()
            if own is not None:
                untouched = untouched and bool(np.all(host[name][~own] == poison))
        total = int((raw != poison).sum().item())
        inside = sum(int((raw[o:o + b] != poison).sum().item()) for o, b in place.values())
        return host, untouched, total - inside

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:
            return -1, str(exc)

    def thrice(run):
        """run(poison, times) -> dict(rc, out {name: bytes}, owns, untouched, damage, extra): 0xFF once, 0x4B twice over itself"""
        r1, r2 = run(0xFF, 1), run(0x4B, 2)
        same = r1.get("extra") == r2.get("extra")
        for name, b in r1["out"].items():
            own = r1["owns"][name]
            same = same and bool(np.array_equal(b, r2["out"][name]) if own is None else np.array_equal(b[own], r2["out"][name][own]))
        return r1, dict(rc=r1["rc"] + r2["rc"], untouched=r1["untouched"] and r2["untouched"], damage=r1["damage"] + r2["damage"],
                        same=bool(same), extra=r1.get("extra"))

    # ---------------------------------------------------------------- lat_gemm
    def gemm_sizes(c):
        return {k: 4 * v for k, v in lr.extents(c).items()}

    def gemm_fill(c, inp, raw, place, names=("A", "Bp", "bias")):
        host = dict(A=a_flat(c, inp), Bp=lr.pack_b(lib, inp["B"], c["K"], c["n_cb"], c["slice_len"], c["n_slices"]), bias=inp["bias"])
        for k in names:
            put(raw, place, k, host[k])

    def c_owns(c):
        m = np.zeros(lr.extents(c)["C"], dtype=bool)
        m[c_index(c).reshape(-1)] = True
        return np.repeat(m, 4)

    def run_gemm(c, inp):
        def run(poison, times):
            raw, place = arena(gemm_sizes(c), poison)
            gemm_fill(c, inp, raw, place)
            a = lr.fill_args(c, inp["a_scale"], {k: raw.data_ptr() + place[k][0] for k in place})
            rc = [lib.dcs_debug_lat_gemm(ctx._h, ctypes.byref(a)) for _ in range(times)]
            owns = {"C": c_owns(c)}
            host, untouched, damage = finish(raw, place, poison, owns)
            return dict(rc=rc, out=host, owns=owns, untouched=untouched, damage=damage, extra=[a.J, a.NA, a.grid_x, a.grid_y, a.grid_z, a.block_x])
        return thrice(run)

    t_all = time.time()
    for c in GEMM_CASES:
        t0 = time.time()
        rep = dict(rc=[], untouched=True, damage=0, same=True, grid=None)
        for kind in lr.kinds_of(c):
            r1, r = run_gemm(c, lr.gemm_inputs(c, kind))
            rep["rc"] += r["rc"]
            rep["grid"] = r["extra"]
            rep["untouched"], rep["same"], rep["damage"] = rep["untouched"] and r["untouched"], rep["same"] and r["same"], rep["damage"] + r["damage"]
            arrays["gemm/%s/%s" % (c["name"], kind)] = r1["out"]["C"]
        rep["seconds"] = time.time() - t0
        report["gemm/" + c["name"]] = rep

    # the chain: the producer's four parts stay where the consumer reads them
    p, q = lr.chain_cases()
    ip, iq = lr.gemm_inputs(p, "signed"), lr.gemm_inputs(q, "signed")

    def run_chain(poison, times):
        sizes = {"A": 4 * lr.extents(p)["A"], "Bp": 4 * lr.extents(p)["Bp"], "bias": 4 * lr.extents(p)["bias"], "Z": 4 * lr.extents(p)["C"],
                 "Bp2": 4 * lr.extents(q)["Bp"], "bias2": 4 * lr.extents(q)["bias"], "C": 4 * lr.extents(q)["C"]}
        raw, place = arena(sizes, poison)
        gemm_fill(p, ip, raw, place)
        put(raw, place, "Bp2", lr.pack_b(lib, iq["B"], q["K"], q["n_cb"], q["slice_len"], q["n_slices"]))
        put(raw, place, "bias2", iq["bias"])
        at = lambda k: raw.data_ptr() + place[k][0]
        a1 = lr.fill_args(p, ip["a_scale"], dict(A=at("A"), Bp=at("Bp"), bias=at("bias"), C=at("Z")))
        a2 = lr.fill_args(q, iq["a_scale"], dict(A=at("Z"), Bp=at("Bp2"), bias=at("bias2"), C=at("C")))
        rc = []
        for _ in range(times):
            rc += [lib.dcs_debug_lat_gemm(ctx._h, ctypes.byref(a1)), lib.dcs_debug_lat_gemm(ctx._h, ctypes.byref(a2))]
        owns = {"Z": np.repeat(np.isin(np.arange(lr.extents(p)["C"]), c_index(p).reshape(-1)), 4), "C": c_owns(q)}
        host, untouched, damage = finish(raw, place, poison, owns)
        return dict(rc=rc, out=host, owns=owns, untouched=untouched, damage=damage, extra=[a2.J, a2.NA])
    r1, report["chain"] = thrice(run_chain)
    arrays["chain/Z"], arrays["chain/C"] = r1["out"]["Z"], r1["out"]["C"]
    report["_gemm_seconds"] = time.time() - t_all
    report["_guards_gemm"] = guards()

    # ---------------------------------------------------------------- forward STFT
    t_fwd = time.time()
    for c in FWD_CASES:
        N, hop, ld, n = c["N"], c["hop"], c["ld"], c["n_samples"]
        T = stft_np.frame_count(n, hop)
        rows = T + c["rows_extra"]
        audio = lr.forward_audio(c)

        def run(poison, times):
            sizes = {"audio": 4 * n, "mag": 4 * rows * ld, "unit": 8 * rows * ld}
            if c["phase"]:
                sizes["phase"] = 4 * rows * ld
            raw, place = arena(sizes, poison, skew={"audio": 4 * c["skew"]})
            put(raw, place, "audio", audio)
            at = lambda k: vp(raw.data_ptr() + place[k][0]) if k in place else vp(None)
            assert (raw.data_ptr() + place["audio"][0]) % 8 == 4 * c["skew"]
            rc = [lib.dcs_debug_lat_stft_forward_f32(plan(N, hop)._h, at("audio"), n, n, at("mag"), at("phase"), at("unit"), rows * ld, ld, rows)
                  for _ in range(times)]
            owns = {k: None for k in sizes if k != "audio"}
            host, untouched, damage = finish(raw, place, poison, owns)
            return dict(rc=rc, out=host, owns=owns, untouched=untouched, damage=damage)
        r1, rep = thrice(run)
        rep["rows"] = rows
        report["fwd/" + c["name"]] = rep
        for k, v in r1["out"].items():
            arrays["fwd/%s/%s" % (c["name"], k)] = v
    report["_fwd_seconds"] = time.time() - t_fwd

    # ---------------------------------------------------------------- inverse STFT
    t_inv = time.time()
    for c in INV_CASES:
        N, hop, ld, T, S, n_out, F = c["N"], c["hop"], c["ld"], c["T"], c["n_src"], c["n_out"], c["N"] // 2 + 1
        mag, unit = lr.inverse_inputs(c)
        e = lr.inverse_extents(c)
        mh = np.full((S, T, ld), np.nan, dtype=np.float32)
        mh[:, :, :F] = mag
        uh = np.full((T, ld, 2), np.nan, dtype=np.float32)
        uh[:, :F] = unit.view(np.float32).reshape(T, F, 2)

        def run(poison, times):
            sizes = {"mag": 4 * e["mag"], "unit": 8 * e["unit"], "audio": 4 * e["audio"], "frames": 4 * e["frames"]}
            raw, place = arena(sizes, poison)
            put(raw, place, "mag", mh.reshape(-1)[:e["mag"]])
            put(raw, place, "unit", uh.reshape(-1)[:2 * e["unit"]])
            at = lambda k: vp(raw.data_ptr() + place[k][0])
            rc = [lib.dcs_debug_lat_stft_inverse_f32(plan(N, hop)._h, at("mag"), e["mag"], T * ld, at("unit"), e["unit"], ld, T, S, sr.PRE_DIV,
                                                     at("audio"), e["audio"], n_out, at("frames"), 4 * e["frames"]) for _ in range(times)]
            owns = {"audio": None, "frames": None}
            host, untouched, damage = finish(raw, place, poison, owns)
            return dict(rc=rc, out=host, owns=owns, untouched=untouched, damage=damage)
        r1, report["inv/" + c["name"]] = thrice(run)
        arrays["inv/%s/audio" % c["name"]], arrays["inv/%s/frames" % c["name"]] = r1["out"]["audio"], r1["out"]["frames"]
    report["_inv_seconds"] = time.time() - t_inv
    report["_guards"] = guards()
    report["_args"] = _arguments(torch, ctx, lib, plan, arena, put)
    report["_seconds"] = time.time() - t_all
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _arguments(torch, ctx, lib, plan, arena, put):
    """per launch class one good call, then one call per class of refusal: the status, and the arena byte for byte as it was"""
    res = {}
    by_name = {c["name"]: c for c in GEMM_CASES}

    def record(label, rc, want, raw, before):
        ctx.synchronize()
        res[label] = dict(rc=rc, want=want, untouched=want == 0 or bool(torch.equal(raw, before)),
                          message=lib.dcs_last_error().decode("utf-8", "replace") if rc != 0 else "")

    for cname in REFUSAL_BASES:
        c = by_name[cname]
        inp = lr.gemm_inputs(c, "signed")
        # buffers far longer than any variant's extents, so that an aid that wrongly accepted would still stay inside them
        variants = [dict(c, **mods) for _, mods, _, _ in lr.gemm_refusals(c)]
        room = {k: 4 * max([lr.extents(c)[k]] + [abs(lr.extents(v)[k]) for v in variants]) + 4096 for k in ("A", "Bp", "bias", "C")}
        raw, place = arena(room, 0xFF)
        host = dict(A=a_flat(c, inp), Bp=lr.pack_b(lib, inp["B"], c["K"], c["n_cb"], c["slice_len"], c["n_slices"]), bias=inp["bias"])
        for k, v in host.items():
            off = place[k][0]
            raw[off:off + v.nbytes].copy_(torch.from_numpy(v.view(np.uint8).reshape(-1)))
        ptrs = {k: raw.data_ptr() + place[k][0] for k in place}
        before = raw.clone()
        a = lr.fill_args(c, inp["a_scale"], ptrs)
        record("%s: good" % cname, lib.dcs_debug_lat_gemm(ctx._h, ctypes.byref(a)), 0, raw, before)
        raw.copy_(before)
        for label, mods, counts, pmods in lr.gemm_refusals(c):
            v = dict(c, **mods)
            pp = dict(ptrs)
            for k, how in pmods.items():
                pp[k] = None if how == "null" else ptrs[k] + 4
            a = lr.fill_args(v, inp["a_scale"], pp, dict(lr.extents(c), **counts) if not mods else counts)
            record("%s: %s" % (cname, label), lib.dcs_debug_lat_gemm(ctx._h, ctypes.byref(a)), lr.EINVAL, raw, before)
    res["gemm: null arguments"] = dict(rc=lib.dcs_debug_lat_gemm(ctx._h, None), want=lr.EINVAL, untouched=True, message="")
    res["gemm: null context"] = dict(rc=lib.dcs_debug_lat_gemm(None, None), want=lr.EINVAL, untouched=True, message="")

    # forward: 3 hop + 5 samples of (1024, 512)
    N, hop, n = 1024, 512, 3 * 512 + 5
    T, F = stft_np.frame_count(n, hop), N // 2 + 1
    rows, ld = T + 1, F + 3
    raw, place = arena({"audio": 4 * n + 64, "mag": 4 * rows * ld + 64, "phase": 4 * rows * ld + 64, "unit": 8 * rows * ld + 64}, 0xFF)
    raw[place["audio"][0]:place["audio"][0] + 4 * n].copy_(torch.from_numpy(lr.forward_audio(dict(seed=1, n_samples=n, silence=False)).view(np.uint8)))
    before = raw.clone()
    at = lambda k, d=0: vp(raw.data_ptr() + place[k][0] + d)

    def fwd(label, want, pl=None, audio=None, n_audio=n, n_samples=n, mag=None, phase=None, unit=None, elems=rows * ld, ld_=ld, rows_=rows):
        raw.copy_(before)
        pick = lambda v, k: at(k) if v is None else v                        # (a null c_void_p is falsy: no `or` here)
        rc = lib.dcs_debug_lat_stft_forward_f32((pl or plan(N, hop))._h if pl != "null" else None, pick(audio, "audio"), n_audio, n_samples,
                                                pick(mag, "mag"), pick(phase, "phase"), pick(unit, "unit"), elems, ld_, rows_)
        record("forward: " + label, rc, want, raw, before)

    fwd("good", 0)
    fwd("good without phases, samples off 8 bytes", 0, audio=at("audio", 4), n_audio=n - 1, n_samples=n - 1, phase=vp(None))
    fwd("samples one short", lr.EINVAL, n_audio=n - 1)
    fwd("outputs one element short", lr.EINVAL, elems=rows * ld - 1)
    fwd("fewer rows than frames", lr.EINVAL, rows_=T - 1)
    fwd("ld below the bins", lr.EINVAL, ld_=F - 1)
    fwd("no sample", lr.EINVAL, n_samples=0)
    fwd("negative rows", lr.EINVAL, rows_=-1)
    fwd("null phasors", lr.EINVAL, unit=vp(None))
    fwd("null magnitudes", lr.EINVAL, mag=vp(None))
    fwd("phasors off 8 bytes", lr.EINVAL, unit=at("unit", 4))
    fwd("samples off 4 bytes", lr.EINVAL, audio=at("audio", 2))
    fwd("null plan", lr.EINVAL, pl="null")
    from deepconvsep_amd.runtime import StftPlan
    fwd("frameSize 4096", lr.EINVAL, pl=StftPlan(ctx, 4096, 1024, sr.window(4096)))
    fwd("frameSize / hop = 8", lr.EINVAL, pl=StftPlan(ctx, 1024, 128, sr.window(1024)))

    # inverse: 3 sources, 4 frames of (1024, 256)
    c = dict(N=1024, hop=256, T=4, n_src=3, n_out=700, ld=516, seed=2)
    e = lr.inverse_extents(c)
    mag, unit = lr.inverse_inputs(c)
    mh = np.zeros((3, 4, 516), dtype=np.float32)
    mh[:, :, :513] = mag
    uh = np.zeros((4, 516, 2), dtype=np.float32)
    uh[:, :513] = unit.view(np.float32).reshape(4, 513, 2)
    raw, place = arena({"mag": 4 * e["mag"] + 64, "unit": 8 * e["unit"] + 64, "audio": 4 * e["audio"] + 64, "frames": 4 * e["frames"] + 64}, 0xFF)
    for k, v in (("mag", mh.reshape(-1)[:e["mag"]]), ("unit", uh.reshape(-1)[:2 * e["unit"]])):
        raw[place[k][0]:place[k][0] + v.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(v).view(np.uint8)))
    before = raw.clone()

    def inv(label, want, pl=None, mag=None, n_mag=e["mag"], stride=4 * 516, unit=None, n_unit=e["unit"], ld_=516, T_=4, S_=3, pre=sr.PRE_DIV,
            audio=None, n_audio=e["audio"], n_out=700, frames=None, fbytes=4 * e["frames"]):
        raw.copy_(before)
        pick = lambda v, k: at(k) if v is None else v
        rc = lib.dcs_debug_lat_stft_inverse_f32((pl or plan(1024, 256))._h, pick(mag, "mag"), n_mag, stride, pick(unit, "unit"), n_unit, ld_, T_, S_,
                                                pre, pick(audio, "audio"), n_audio, n_out, pick(frames, "frames"), fbytes)
        record("inverse: " + label, rc, want, raw, before)

    inv("good", 0)
    inv("magnitudes one short", lr.EINVAL, n_mag=e["mag"] - 1)
    inv("phasors one short", lr.EINVAL, n_unit=e["unit"] - 1)
    inv("samples one short", lr.EINVAL, n_audio=e["audio"] - 1)
    inv("frames scratch one byte short", lr.EINVAL, fbytes=4 * e["frames"] - 1)
    inv("ld below the bins", lr.EINVAL, ld_=512)
    inv("sources closer than their rows", lr.EINVAL, stride=4 * 516 - 4)
    inv("pre_div 0", lr.EINVAL, pre=0.0)
    inv("no frame", lr.EINVAL, T_=0)
    inv("no source", lr.EINVAL, S_=0)
    inv("no sample", lr.EINVAL, n_out=0)
    inv("null frames scratch", lr.EINVAL, frames=vp(None))
    inv("frames scratch off 8 bytes", lr.EINVAL, frames=at("frames", 4), fbytes=4 * e["frames"])
    inv("phasors off 8 bytes", lr.EINVAL, unit=at("unit", 4))
    inv("frameSize 4096", lr.EINVAL, pl=StftPlan(ctx, 4096, 1024, sr.window(4096)))
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_lat_kernels as t; t.child(sys.argv[2])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(arrays, report) of the one child, under its own time limit; a child that ends in a signal or at its limit ends the run
    (nothing more is started on the device)"""
    out = str(tmp_path_factory.mktemp("lat_kernels") / "run.npz")
    env = dict(os.environ)
    env.update(DCS_WS_GUARD=str(GB))
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, "-c", _CHILD, ROOT, out], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print("child took %.1f s (limit %d), status %d" % (time.time() - t0, CHILD_LIMIT, p.returncode), flush=True)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        pytest.exit("the child ended with status %d; nothing more is started\n%s" % (p.returncode, p.stderr[-2000:]), 1)
    assert p.returncode == 0, (p.returncode, p.stdout[-400:], p.stderr[-2000:])
    z = np.load(out)
    return z, json.loads(bytes(z["_report"]).decode())


def _clean(r, calls):
    assert r["rc"] == [0] * calls, r["rc"]
    assert r["untouched"], "bytes of an output the launch does not own are no longer poison"
    assert r["damage"] == 0, "%d bytes changed outside every buffer" % r["damage"]
    assert r["same"], "the poisons 0xFF and 0x4B, or a launch over its own output, gave other bits"


_SIGNED = {}


def _signed(z, c):
    """(device, float64, restatement, S) of the signed data set, [parts][M][n_store]; computed once per case"""
    if c["name"] not in _SIGNED:
        inp = lr.gemm_inputs(c, "signed")
        got = z["gemm/%s/signed" % c["name"]].view(np.float32)[c_index(c)]
        _SIGNED[c["name"]] = (got, lr.reference(c, inp), lr.restatement(c, inp), lr.reference(c, inp, "abs"))
    return _SIGNED[c["name"]]


@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c["name"])
def test_gemm(run, c):
    z, report = run
    r = report["gemm/" + c["name"]]
    kinds = lr.kinds_of(c)
    _clean(r, 3 * len(kinds))
    assert r["grid"] == lr.grid(c), (r["grid"], lr.grid(c))
    assert r["seconds"] < 5, "the case took %.1f s in the child" % r["seconds"]
    for kind in kinds:
        if kind == "signed":
            continue
        inp = lr.gemm_inputs(c, kind)
        got = z["gemm/%s/%s" % (c["name"], kind)].view(np.float32)[c_index(c)]
        want = lr.reference(c, inp)
        bad = int((got.astype(np.float64) != want).sum())
        assert bad == 0, "%s %s: %d of %d elements differ from the float64 result" % (c["name"], kind, bad, got.size)
        if kind == "ties":
            j = np.arange(c["n_store"])
            assert not got[0][j % c["M"], j].any()
    got, want, rest, S = _signed(z, c)
    assert np.isfinite(got).all(), "%s: values that are not finite" % c["name"]
    assert not got[S == 0].any(), "%s: an output nothing but zeros goes into is not 0" % c["name"]
    d = np.abs(got.astype(np.float64) - want)
    cap = lr.roundings(c) * lr.U * S
    e, e32 = measure(got, want, S), measure(rest, want, S)
    print("\n%s (J %d, NA %d): E %.3g, restatement %.3g, E / E(restatement) %.2f, worst |err| / cap %.3g"
          % (c["name"], c["J"], c["a_parts"], e, e32, e / max(e32, 1e-300), float(np.max(d / (cap + 1e-300)))))
    assert np.all(d <= cap), "%s: outside %d 2^-24 S by a factor of %.3g" % (c["name"], lr.roundings(c), float(np.max(d / (cap + 1e-300))))


def test_gemm_yardstick_per_instantiation(run):
    z, report = run
    pooled = {}
    for c in GEMM_CASES:
        r = report["gemm/" + c["name"]]
        if not (r["rc"] and all(rc == 0 for rc in r["rc"]) and r["grid"] == lr.grid(c)):
            continue
        got, want, rest, S = _signed(z, c)
        p = pooled.setdefault((c["J"], c["a_parts"]), dict(n=0, e=0.0, e32=0.0))
        p["n"], p["e"], p["e32"] = p["n"] + got.size, max(p["e"], measure(got, want, S)), max(p["e32"], measure(rest, want, S))
    name = lambda k: "lat_gemm_kernel<%d, %d>" % k
    assert not set(lr.PRODUCTION) - set(pooled), "never launched: %r" % sorted(map(name, set(lr.PRODUCTION) - set(pooled)))
    assert not lr.AID_ONLY - set(pooled), "aid only, never launched: %r" % sorted(map(name, lr.AID_ONLY - set(pooled)))
    print("\nreached by production: %r\nreached by the aid only: %r" % (sorted((name(k), v) for k, v in lr.PRODUCTION.items()), sorted(map(name, lr.AID_ONLY))))
    for k in sorted(pooled):
        p = pooled[k]
        print("%s: %d outputs, E %.3g, restatement %.3g, E / E(restatement) %.2f" % (name(k), p["n"], p["e"], p["e32"], p["e"] / max(p["e32"], 1e-300)))
    for k, p in pooled.items():
        assert p["n"] >= lr.MIN_POOLED, (name(k), p["n"])
        assert p["e"] <= lr.FACTOR * p["e32"], "%s: device %.3g, restatement %.3g" % (name(k), p["e"], p["e32"])


def test_gemm_chain(run):
    z, report = run
    _clean(report["chain"], 6)
    p, q = lr.chain_cases()
    ip, iq = lr.gemm_inputs(p, "signed"), lr.gemm_inputs(q, "signed")
    want, bound = lr.chain_reference(p, q, ip, iq)
    got = z["chain/C"].view(np.float32)[c_index(q)][0]
    d = np.abs(got.astype(np.float64) - want)
    print("\nchain: worst |err| / bound %.3g" % float(np.max(d / (bound + 1e-300))))
    assert np.all(d <= bound)
    # and the parts the producer left are its own contract's
    parts = z["chain/Z"].view(np.float32)[c_index(p)]
    w1, S1 = lr.reference(p, ip), lr.reference(p, ip, "abs")
    assert np.all(np.abs(parts.astype(np.float64) - w1) <= lr.roundings(p) * lr.U * S1)


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c["name"])
def test_forward(run, c):
    z, report = run
    r = report["fwd/" + c["name"]]
    _clean(r, 3)
    N, hop, ld, rows, F = c["N"], c["hop"], c["ld"], r["rows"], c["N"] // 2 + 1
    audio = lr.forward_audio(c)
    X, X32 = sr.forward_ref64(audio, N, hop), sr.forward_ref32(audio, N, hop)
    T = X.shape[0]
    assert rows == T + c["rows_extra"]
    mag = z["fwd/%s/mag" % c["name"]].view(np.float32).reshape(rows, ld)
    u = z["fwd/%s/unit" % c["name"]].view(np.float32).reshape(rows, ld, 2)
    unit = u[..., 0] + 1j * u[..., 1]
    phase = z["fwd/%s/phase" % c["name"]].view(np.float32).reshape(rows, ld) if c["phase"] else None
    assert np.isfinite(mag).all() and np.isfinite(u).all()
    silent = np.array([not X[t].any() for t in range(T)])                    # frames of zeros only (exact: the inputs are)
    if c["silence"]:
        assert silent.any()
    quiet = np.concatenate([silent, np.ones(rows - T, dtype=bool)])          # and the rows past the last frame
    # silent frames, rows past T and the pad columns: magnitude exactly 0, phasor exactly (1, 0), angle 0
    assert not mag[quiet].any() and not mag[:, F:].any()
    assert np.all(unit[quiet] == 1.0) and np.all(unit[:, F:] == 1.0)
    m, un = mag[:T, :F], unit[:T, :F]
    fig = dict(mag=np.max(np.abs(m - np.abs(X))), mag32=np.max(np.abs(np.abs(X32) - np.abs(X))), cpx32=np.max(np.abs(X32 - X)),
               ph32=np.max(np.abs(np.abs(X32) * np.exp(1j * np.angle(X32).astype(np.float32).astype(np.float64)) - X)),
               unit=np.max(np.abs(m * un - X)), phase=0.0, norm=0.0)
    assert np.all(un[m == 0] == 1.0)
    live = m > 0
    if live.any():
        fig["norm"] = np.max(np.abs(np.abs(un[live].astype(np.complex128)) - 1))
    if phase is not None:
        assert np.isfinite(phase).all()
        assert not phase[quiet].any() and not phase[:, F:].any(), "angle of a silent frame, a row past T or a pad column: %r" % np.unique(phase[quiet])
        fig["phase"] = np.max(np.abs(m * np.exp(1j * phase[:T, :F].astype(np.float64)) - X))
    print("\n%s: %d of %d frames inside, |mag| %.3g (restatement %.3g), mag*unit %.3g (%.3g), mag*exp(j phase) %.3g (%.3g), ||unit|-1| %.3g"
          % (c["name"], lr.forward_inside(c) if not c["skew"] else 0, T, fig["mag"], fig["mag32"], fig["unit"], fig["cpx32"], fig["phase"],
             fig["ph32"], fig["norm"]))
    assert fig["mag"] <= sr.FACTOR * fig["mag32"] and fig["mag"] <= sr.BOUND_MAG
    assert fig["unit"] <= sr.FACTOR * fig["cpx32"] and fig["unit"] <= sr.BOUND_CPX
    assert fig["phase"] <= sr.FACTOR * fig["ph32"] and fig["phase"] <= sr.BOUND_CPX
    assert fig["norm"] <= sr.BOUND_UNIT


@pytest.mark.parametrize("c", INV_CASES, ids=lambda c: c["name"])
def test_inverse(run, c):
    z, report = run
    _clean(report["inv/" + c["name"]], 3)
    N, hop, T, S, n_out = c["N"], c["hop"], c["T"], c["n_src"], c["n_out"]
    mag, unit = lr.inverse_inputs(c)
    frames = z["inv/%s/frames" % c["name"]].view(np.float32).reshape(S, T, N)
    out = z["inv/%s/audio" % c["name"]].view(np.float32).reshape(S, n_out)
    assert np.isfinite(frames).all() and np.isfinite(out).all()
    # lat_ifft_kernel: every frame against float64 irfft(X_t) * w
    want, f32 = lr.frames_ref(c, mag, unit)
    d = np.max(np.abs(frames.astype(np.float64) - want), axis=2)
    d32 = np.max(np.abs(f32.astype(np.float64) - want), axis=2)
    print("\n%s: frames: worst device / restatement %.2f (device %.3g)" % (c["name"], float(np.max(d / np.where(d32 > 0, d32, 1e-300))) if d.max() > 0 else 0.0,
                                                                           float(d.max())))
    assert np.all(d <= sr.FACTOR * d32), "source, frame %r: device %r, restatement %r" % (np.argwhere(d > sr.FACTOR * d32)[0].tolist(), d.max(), d32.max())
    # lat_ola_kernel: the frames the device wrote, added in frame order and divided: bit for bit
    exp = lr.ola_ref(c, frames)
    diff = out.view(np.uint32) != np.ascontiguousarray(exp).view(np.uint32)
    assert not diff.any(), "%d of %d samples differ from the in-order float32 sum / float32 normaliser" % (int(diff.sum()), out.size)
    full = hop * (T - 1) + N // 2
    assert not out[:, full:].any(), "samples past the last frame's cover are not 0"
    # end to end, in the weighted measure
    worst = worst32 = 0.0
    for s in range(S):
        ref64, ref32 = sr.inverse_ref64(mag[s], unit, N, hop), sr.inverse_ref32(mag[s], unit, N, hop)
        norm = sr.inverse_norm(N, hop, T, ref64.size)
        n = min(n_out, full)
        e, e32 = sr.weighted_error(out[s, :n], ref64[:n], norm[:n]), sr.weighted_error(ref32, ref64, norm)
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= sr.FACTOR * e32 and e <= sr.BOUND_INV, "source %d: device %.3g, float32 restatement %.3g" % (s, e, e32)
    print("%s: weighted error %.3g (float32 restatement %.3g)" % (c["name"], worst, worst32))


def test_entries_refuse_bad_arguments(run):
    args = run[1]["_args"]
    assert len(args) > 80
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        assert r["untouched"], label


def test_guards_and_time(run):
    _, report = run
    for g in (report["_guards_gemm"], report["_guards"]):
        assert g[1] == "" and g[0] >= 0, g
    print("\nchild: %.2f s for the GEMM cases, %.2f s forward, %.2f s inverse, %.2f s in all; the slowest GEMM cases: %r" % (
        report["_gemm_seconds"], report["_fwd_seconds"], report["_inv_seconds"], report["_seconds"],
        sorted(((round(report["gemm/" + c["name"]]["seconds"], 3), c["name"]) for c in GEMM_CASES), reverse=True)[:3]))
    assert report["_seconds"] < CHILD_LIMIT / 2
