"""Every STFT / inverse-STFT kernel of csrc/fft.hip and csrc/fft_wave.hip on the MI355X, directly against float64.

The kernels are reached through ``dcs_debug_stft_forward_f32`` / ``dcs_debug_stft_inverse_unit_f32`` (the launchers
``dcs_separate*`` use, phasor input included) and through the public phase-input and float64 entries; after every launch
``dcs_debug_stft_last_kernel`` says which kernel ran and the test asserts that it is the one the case was written for.  One
child process per switch set (tests/stft_ref.py ``SWITCHES``; libdcs reads them once per process), four at a time, each with
``DCS_WS_GUARD=65536`` and each running all of its cases on buffers carved out of one poisoned allocation per case: 64 KiB
between and around the buffers, outputs, row padding, the rows past a clip's frames and the gap ``[n_out, out_stride)``
born as 0xFF bytes (float32 NaN).  The children write what they computed; the parent compares with the references.

Bounds (tests/stft_ref.py): a float32 kernel may be ``FACTOR`` = 4 x as far from float64 as the float32 restatement of the
same transform on the same inputs is -- for the inverse in the weighted measure, the restatement's figure taken over the
whole inverse length of the source so that a clip of one sample is not bounded by one sample's luck -- and never further
than the project's bounds (inverse 1e-5, magnitudes 2e-5, complex spectrum 4e-5); float64 kernels 1e-11.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import stft_ref as sr
from oracle import stft_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
POISON = 0xFF
G = 1 << 16
EINVAL, EUNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------------------ the child process
class _Arena(object):
    """one poisoned allocation; buffers 256-byte aligned (plus `skew` bytes) with G bytes around each"""

    def __init__(self, torch):
        self.torch, self.items, self.place, self.raw = torch, [], {}, None

    def add(self, name, nbytes, skew=0):
        self.items.append((name, int(nbytes), skew))

    def commit(self):
        off = G
        for name, n, skew in self.items:
            self.place[name] = (off + skew, n)
            off += (n + skew + 255) // 256 * 256 + G
        self.raw = self.torch.full((off,), POISON, dtype=self.torch.uint8, device="cuda")
        return self

    def u8(self, name):
        o, n = self.place[name]
        return self.raw[o:o + n]

    def f32(self, name):
        return self.u8(name).view(self.torch.float32)

    def ptr(self, name):
        return ctypes.c_void_p(self.u8(name).data_ptr()) if name in self.place else ctypes.c_void_p(None)

    def damage(self):
        """bytes outside the buffers that are no longer poison"""
        self.torch.cuda.synchronize()
        total = int((self.raw != POISON).sum().item())
        return total - sum(int((self.u8(name) != POISON).sum().item()) for name in self.place)


def _poisoned(t):
    """how many 4-byte words of a float32 / int32 tensor still hold the poison pattern"""
    import torch
    return int((t.contiguous().view(torch.int32) == -1).sum().item())


def child(switch, out_path):
    import torch
    from deepconvsep_amd.runtime import StftPlan, default_context

    ctx = default_context()
    lib = ctx._lib
    n_cu = int(torch.cuda.get_device_properties(ctx.device_index).multi_processor_count)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    plans = {}

    def plan(N, hop):
        if (N, hop) not in plans:
            plans[(N, hop)] = StftPlan(ctx, N, hop, sr.window(N))
        return plans[(N, hop)]

    def last(p):
        f, i, prm = ctypes.c_int(), ctypes.c_int(), i64()
        assert lib.dcs_debug_stft_last_kernel(p._h, ctypes.byref(f), ctypes.byref(i), ctypes.byref(prm)) == 0
        return f.value, i.value, prm.value

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:                                            # a damaged scratch red zone: reported, not raised
            return -1, str(exc)

    def put(dst, src):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    arrays, report = {}, {"_n_cu": n_cu}

    # ---------------------------------------------------------------- inverse
    def inverse_case(c):
        c = dict(c)
        N, hop, ld = c["N"], c["hop"], c["ld"]
        if c["cu_cap"]:
            c["n_out"] = sr.cap_n_out(n_cu)
            c["T"] = stft_np.frame_count(c["n_out"], hop)
            c["out_stride"], c["src_stride"], c["unit_clip_stride"] = c["n_out"], c["T"] * ld, c["T"] * ld
        T, bins, n_src, n_clips = c["T"], N // 2 + 1, c["n_src"], c["n_clips"]
        S, n_out, os_, ucs = n_src * n_clips, c["n_out"], c["out_stride"], c["unit_clip_stride"]
        mag, unit = sr.inverse_inputs(c)
        lengths = c["lengths"] or [n_out] * n_clips
        tab = sr.clip_table(lengths, hop, c["table"] == "compact") if c["table"] else None
        frames = [int(tab[k, 1]) for k in range(n_clips)] if tab is not None else [T] * n_clips
        ar = _Arena(torch)
        ar.add("mag", S * T * ld * 4 + 16, skew=4 * c["mag_off"])
        ar.add("unit", n_clips * ucs * 8)
        ar.add("out1", S * os_ * 4)
        ar.add("out2", S * os_ * 4)
        if tab is not None:
            ar.add("tab", tab.size * 8)
        if c["public"]:
            ar.add("phase", T * ld * 4)
            ar.add("out3", S * n_out * 4)
        ar.commit()
        magd = ar.f32("mag")[:S * T * ld].view(S, T, ld)
        unitd = ar.f32("unit")
        for k in range(n_clips):                                             # rows past a clip's frames stay poisoned
            Tk = frames[k]
            for s in range(n_src):
                put(magd[k * n_src + s, :Tk, :bins], mag[k * n_src + s, :Tk])
            r0 = int(tab[k, 3]) * ld if (tab is not None and tab[k, 3] >= 0) else k * ucs
            put(unitd[2 * r0:2 * (r0 + Tk * ld)].view(Tk, ld, 2)[:, :bins], unit[k, :Tk].view(np.float32).reshape(Tk, bins, 2))
        if tab is not None:
            put(ar.u8("tab").view(torch.int64), tab.reshape(-1))
        p = plan(N, hop)
        rcs = []
        for out in ("out1", "out2"):
            rcs.append(lib.dcs_debug_stft_inverse_unit_f32(p._h, ar.ptr("mag"), T * ld, ar.ptr("unit"), ucs, ld, T, n_src, n_clips,
                                                           sr.PRE_DIV, ar.ptr(out), n_out, ar.ptr("tab"),
                                                           os_ if c["out_pad"] else 0))
        ctx.synchronize()
        _, kern, param = last(p)
        o1, o2 = ar.f32("out1").view(S, os_), ar.f32("out2").view(S, os_)
        left = gap = 0
        same = True
        for k in range(n_clips):
            for s in range(k * n_src, (k + 1) * n_src):
                left += _poisoned(o1[s, :lengths[k]])
                gap += (os_ - lengths[k]) - _poisoned(o1[s, lengths[k]:])   # past the clip's samples nothing is written
                same = same and torch.equal(o1[s, :lengths[k]].view(torch.int32), o2[s, :lengths[k]].view(torch.int32))
        n_ws, guard_err = guards()
        r = dict(rc=rcs, kernel=kern, param=param, poison_left=left, gap_written=gap, same_twice=bool(same), n_out=n_out, T=T,
                 scratch_blocks=n_ws, scratch_guard=guard_err)
        arrays["inv/" + c["name"]] = o1.cpu().numpy()
        if c["public"]:
            ph = np.angle(unit[0]).astype(np.float32)
            put(ar.f32("phase").view(T, ld)[:, :bins], ph)
            r["public_rc"] = lib.dcs_stft_inverse_f32(p._h, ar.ptr("mag"), T * ld, ar.ptr("phase"), ld, T, n_src, sr.PRE_DIV,
                                                      ar.ptr("out3"), n_out)
            ctx.synchronize()
            _, r["public_kernel"], r["public_param"] = last(p)
            o3 = ar.f32("out3").view(S, n_out)
            r["public_poison_left"] = _poisoned(o3)
            arrays["inv_public/" + c["name"]] = o3.cpu().numpy()
        r["red_zone_bytes_damaged"] = ar.damage()
        report["inv/" + c["name"]] = r

    # ---------------------------------------------------------------- forward
    def forward_case(c):
        c = dict(c)
        N, hop, ld, n_clips = c["N"], c["hop"], c["ld"], c["n_clips"]
        if c["fpw4"]:
            c["n_samples"] = sr.fpw4_samples(n_cu, hop)
            c["audio_stride"] = c["n_samples"]
        n, stride, bins = c["n_samples"], c["audio_stride"], N // 2 + 1
        T = stft_np.frame_count(n, hop)
        rows = T + c["rows_extra"]
        audio = sr.forward_audio(c).astype(np.float32)
        lengths = c["lengths"] or [n] * n_clips
        tab = sr.clip_table(lengths, hop, c["table"] == "compact") if c["table"] else None
        ar = _Arena(torch)
        ar.add("audio", n_clips * stride * 4)
        ar.add("mag", n_clips * rows * ld * 4)
        if c["phase"]:
            ar.add("phase", n_clips * rows * ld * 4)
        if c["unit"]:
            ar.add("unit", n_clips * rows * ld * 8)
        if tab is not None:
            ar.add("tab", tab.size * 8)
        ar.commit()
        ad = ar.f32("audio").view(n_clips, stride)
        for k in range(n_clips):                                             # the stride's padding and a clip's tail stay poisoned
            put(ad[k, :lengths[k]], audio[k, :lengths[k]])
        if tab is not None:
            put(ar.u8("tab").view(torch.int64), tab.reshape(-1))
        p = plan(N, hop)
        rc = lib.dcs_debug_stft_forward_f32(p._h, ar.ptr("audio"), n, stride, n_clips, ar.ptr("mag"), ar.ptr("phase"),
                                            ar.ptr("unit"), ld, rows, 1 if c["interleave"] else 0, ar.ptr("tab"))
        ctx.synchronize()
        kern, _, _ = last(p)
        # rows that belong to somebody: all of them, or (compact table) the clips' own
        own = torch.ones(n_clips * rows, dtype=torch.bool, device="cuda")
        if c["table"] == "compact":
            own[:] = False
            for k in range(n_clips):
                own[int(tab[k, 3]):int(tab[k, 3] + tab[k, 5])] = True
        md = ar.f32("mag").view(n_clips * rows, ld)
        left = _poisoned(md[own])
        foreign = int(own.numel() - own.sum().item()) * ld - _poisoned(md[~own])
        pad_ok = bool((md[own][:, bins:] == 0).all().item())
        arrays["fwd/%s/mag" % c["name"]] = md[:, :bins].cpu().numpy()
        if c["phase"]:
            pd = ar.f32("phase").view(n_clips * rows, ld)
            left += _poisoned(pd[own])
            foreign += int(own.numel() - own.sum().item()) * ld - _poisoned(pd[~own])
            pad_ok = pad_ok and bool((pd[own][:, bins:] == 0).all().item())
            arrays["fwd/%s/phase" % c["name"]] = pd[:, :bins].cpu().numpy()
        if c["unit"]:
            ud = ar.f32("unit").view(n_clips * rows, ld, 2)
            left += _poisoned(ud[own])
            foreign += int(own.numel() - own.sum().item()) * ld * 2 - _poisoned(ud[~own])
            pad_ok = pad_ok and bool((ud[own][:, bins:, 0] == 1).all().item()) and bool((ud[own][:, bins:, 1] == 0).all().item())
            arrays["fwd/%s/unit" % c["name"]] = ud[:, :bins].cpu().numpy()
        n_ws, guard_err = guards()
        report["fwd/" + c["name"]] = dict(rc=rc, kernel=kern, poison_left=left, foreign_written=foreign, padding_ok=pad_ok,
                                          n_samples=n, rows=rows, scratch_blocks=n_ws, scratch_guard=guard_err,
                                          red_zone_bytes_damaged=ar.damage())

    for c in sr.inverse_cases():
        if c["switch"] == switch:
            inverse_case(c)
    for c in sr.forward_cases():
        if c["switch"] == switch:
            forward_case(c)
    if switch == "none":
        _float64_and_arguments(torch, ctx, lib, plan, last, put, arrays, report)
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _f64_inputs(N, hop):
    c = sr._inv("f64", "none", N, hop, nb=23, n_src=2, seed=N + hop)
    mag, unit = sr.inverse_inputs(c)
    return c, mag.astype(np.float64), np.angle(unit[0].astype(np.complex128))


def _f64_audio(N, hop):
    c = sr._fwd("f64", "none", N, hop, frames=14, seed=N + hop)
    return c, sr.forward_audio(c)[0]


def _float64_and_arguments(torch, ctx, lib, plan, last, put, arrays, report):
    vp = ctypes.c_void_p

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def ptr(t):
        return vp(t.data_ptr()) if t is not None else vp(None)

    f64 = {}
    for N, hop in sr.F64_INVERSE + [(8192, 8192)]:
        c, mag, ph = _f64_inputs(N, hop)
        S, T, bins = mag.shape
        out = torch.full((S, c["n_out"]), float("nan"), dtype=torch.float64, device="cuda")
        p = plan(N, hop)
        mag_d, ph_d = dev(mag), dev(ph)
        rc = lib.dcs_stft_inverse_f64(p._h, ptr(mag_d), T * bins, ptr(ph_d), bins, T, S, sr.PRE_DIV, ptr(out), c["n_out"])
        ctx.synchronize()
        f64["inv/%d_%d" % (N, hop)] = dict(rc=rc, kernel=last(p)[1], nan=int(torch.isnan(out).sum().item()))
        arrays["f64inv/%d_%d" % (N, hop)] = out.cpu().numpy()
    for N, hop in sr.F64_FORWARD:
        c, a = _f64_audio(N, hop)
        T, bins = stft_np.frame_count(a.size, hop), N // 2 + 1
        m = torch.full((T, bins), float("nan"), dtype=torch.float64, device="cuda")
        ph = torch.full((T, bins), float("nan"), dtype=torch.float64, device="cuda")
        p = plan(N, hop)
        a_d = dev(a)
        rc = lib.dcs_stft_forward_f64(p._h, ptr(a_d), a.size, ptr(m), ptr(ph), bins, T)
        ctx.synchronize()
        f64["fwd/%d_%d" % (N, hop)] = dict(rc=rc, kernel=last(p)[0])
        arrays["f64fwd/%d_%d/mag" % (N, hop)] = m.cpu().numpy()
        arrays["f64fwd/%d_%d/phase" % (N, hop)] = ph.cpu().numpy()
    report["_f64"] = f64

    # arguments: the status, and nothing written
    N, hop, T, S, nc = 1024, 512, 6, 2, 2
    bins = N // 2 + 1
    ld, n_out = bins, 2000
    p, p512 = plan(N, hop), plan(512, 200)
    mag = torch.zeros(S * nc * T * ld, device="cuda")
    unit = torch.ones(nc * T * ld * 2, device="cuda")
    out = torch.full((S * nc * (n_out + 3),), float("nan"), device="cuda")
    good_tab = sr.clip_table([n_out, 700], hop, False)

    def tabd(t):
        return dev(np.asarray(t, dtype=np.int64).reshape(-1))

    def inv(h=None, mag_=mag, unit_=unit, out_=out, src_stride=T * ld, ucs=T * ld, ld_=ld, T_=T, S_=S, nc_=nc, n_out_=n_out,
            tab=None, os_=0, pre_div=sr.PRE_DIV):
        t = tabd(tab) if tab is not None else None
        rc = lib.dcs_debug_stft_inverse_unit_f32(p._h if h is None else h, ptr(mag_), src_stride, ptr(unit_), ucs, ld_, T_, S_, nc_,
                                                 pre_div, ptr(out_), n_out_, ptr(t), os_)
        ctx.synchronize()
        return rc

    def edit(tab, row, col, val):
        t = np.array(tab)
        t[row, col] = val
        return t

    args = {}
    bad_inv = {
        "null plan": dict(h=vp(None)), "null mag": dict(mag_=None), "null unit": dict(unit_=None), "null audio": dict(out_=None),
        "n_frames<0": dict(T_=-1), "n_src<0": dict(S_=-1), "n_clips<0": dict(nc_=-1), "n_out<0": dict(n_out_=-5),
        "ld<bins": dict(ld_=bins - 1), "out_stride<n_out": dict(os_=n_out - 1), "out_stride<0": dict(os_=-1),
        "unit_clip_stride<T*ld": dict(ucs=T * ld - 1), "src_stride<T*ld": dict(src_stride=T * ld - 1),
        "pre_div=0": dict(pre_div=0.0), "n_out>inverse length": dict(n_out_=stft_np.inverse_length(T, hop, N) + 1),
        "table: samples>n_out": dict(tab=edit(good_tab, 1, 0, n_out + 1)), "table: frames>n_frames": dict(tab=edit(good_tab, 0, 1, T + 1)),
        "table: samples<0": dict(tab=edit(good_tab, 0, 0, -1)), "table: mixed layouts": dict(tab=edit(good_tab, 1, 3, 0)),
        "table: rows past the end": dict(tab=edit(edit(good_tab, 0, 3, 0), 1, 3, 2 * T - 2)),
    }
    for label, kw in bad_inv.items():
        args["inverse " + label] = dict(rc=inv(**kw), want=EINVAL, untouched=bool(torch.isnan(out).all().item()))
    args["inverse n_frames=0"] = dict(rc=inv(T_=0, n_out_=0), want=0, untouched=bool(torch.isnan(out).all().item()))
    args["inverse good table"] = dict(rc=inv(tab=good_tab, os_=n_out + 3), want=0, untouched=False)
    mag5 = torch.zeros(S * nc * T * 257, device="cuda")
    unit5 = torch.ones(nc * T * 257 * 2, device="cuda")
    out.fill_(float("nan"))
    tab5 = tabd(sr.clip_table([500, 100], 200, False))
    rc = lib.dcs_debug_stft_inverse_unit_f32(p512._h, ptr(mag5), T * 257, ptr(unit5), T * 257, 257, T, S, nc, sr.PRE_DIV, ptr(out), 500,
                                             ptr(tab5), 0)
    ctx.synchronize()
    args["inverse table at frameSize 512"] = dict(rc=rc, want=EUNSUPPORTED, untouched=bool(torch.isnan(out).all().item()))

    n = 2000
    Tf = stft_np.frame_count(n, hop)
    audio = torch.zeros(nc * (n + 17), device="cuda")
    fm = torch.full((nc * (Tf + 2) * ld,), float("nan"), device="cuda")
    fu = torch.full((nc * (Tf + 2) * ld * 2,), float("nan"), device="cuda")
    ftab = sr.clip_table([n, 700], hop, False)
    ctab = sr.clip_table([n, 700], hop, True)

    def fwd(h=None, audio_=audio, n_=n, stride=n + 17, nc_=nc, mag_=fm, unit_=fu, ld_=ld, rows=Tf + 2, il=0, tab=None, pl=None):
        t = tabd(tab) if tab is not None else None
        rc = lib.dcs_debug_stft_forward_f32((pl or p)._h if h is None else h, ptr(audio_), n_, stride, nc_, ptr(mag_), vp(None),
                                            ptr(unit_), ld_, rows, il, ptr(t))
        ctx.synchronize()
        return rc

    bad_fwd = {
        "null plan": dict(h=vp(None)), "null audio": dict(audio_=None), "null mag": dict(mag_=None), "n_samples<0": dict(n_=-1),
        "n_clips<0": dict(nc_=-1), "rows_out<0": dict(rows=-1), "rows_out<T": dict(rows=Tf - 1), "ld<bins": dict(ld_=bins - 1),
        "audio_stride<n_samples": dict(stride=n - 1), "table with interleave": dict(tab=ftab, il=1),
        "table: samples>n_samples": dict(tab=edit(ftab, 1, 0, n + 1)), "table: wrong frame count": dict(tab=edit(ftab, 1, 1, 5)),
        "table: mixed layouts": dict(tab=edit(ftab, 1, 3, 0)), "table: rows past the end": dict(tab=edit(ctab, 1, 3, 2 * (Tf + 2) - 3)),
        "table: rows<frames": dict(tab=edit(ctab, 1, 5, 2)),
    }
    for label, kw in bad_fwd.items():
        args["forward " + label] = dict(rc=fwd(**kw), want=EINVAL,
                                        untouched=bool(torch.isnan(fm).all().item() and torch.isnan(fu).all().item()))
    args["forward table at frameSize 512"] = dict(rc=fwd(tab=sr.clip_table([n, 700], 200, False), pl=p512, ld_=bins, rows=Tf + 20),
                                                  want=EUNSUPPORTED,
                                                  untouched=bool(torch.isnan(fm).all().item() and torch.isnan(fu).all().item()))
    args["forward good table"] = dict(rc=fwd(tab=ctab), want=0, untouched=False)
    report["_args"] = args


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_stft_kernels as t; t.child(sys.argv[2], sys.argv[3])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """switch set -> (arrays, report): eight children, four at a time"""
    from test_gpu_parity import _run_children
    d = tmp_path_factory.mktemp("stft_kernels")
    names = list(sr.SWITCHES)
    outs = [str(d / (name + ".npz")) for name in names]
    envs = [dict(sr.SWITCHES[name], DCS_WS_GUARD=str(G), DCS_WS_POISON=str(POISON)) for name in names]
    _run_children(_CHILD, [ROOT], envs, per_child_args=[(name, out) for name, out in zip(names, outs)])
    res = {}
    for name, out in zip(names, outs):
        z = np.load(out)
        res[name] = (z, json.loads(bytes(z["_report"]).decode()))
    return res


def _clean(r, name):
    assert r["scratch_guard"] == "" and r["scratch_blocks"] >= 0, (name, r["scratch_guard"])
    assert r["red_zone_bytes_damaged"] == 0, name


_REFS = {}


def _inverse_refs(key, mag, unit, N, hop, phase=None):
    """(float64 reference, float32 restatement), full inverse length; computed once per (case, source)"""
    if key not in _REFS:
        _REFS[key] = (sr.inverse_ref64(mag, unit, N, hop, phase=phase), sr.inverse_ref32(mag, unit, N, hop, phase=phase))
    return _REFS[key]


@pytest.mark.parametrize("case", sr.inverse_cases(), ids=lambda c: c["name"])
def test_inverse_kernel(runs, case):
    z, report = runs[case["switch"]]
    r = report["inv/" + case["name"]]
    n_cu = report["_n_cu"]
    c = dict(case, n_out=r["n_out"], T=r["T"])
    if case["cu_cap"]:
        c.update(out_stride=c["n_out"], src_stride=c["T"] * c["ld"], unit_clip_stride=c["T"] * c["ld"])
    N, hop, n_src, n_clips = c["N"], c["hop"], c["n_src"], c["n_clips"]
    assert r["rc"] == [0, 0], r
    kern, param = sr.expected_inverse(c, n_cu)
    assert r["kernel"] == kern, "ran kernel %d, the case is written for %d" % (r["kernel"], kern)
    if kern == sr.INV_BLOCK:
        param = sr.block_inverse_plan(N, hop, c["n_out"], n_src, n_cu)["C"]
    if param is not None:
        assert r["param"] == param, (r["param"], param)
    if case["cu_cap"]:
        assert r["param"] == 4 * (N // hop)
    assert r["poison_left"] == 0, "%d samples never written" % r["poison_left"]
    assert r["gap_written"] == 0, "%d samples written past a source's n_out" % r["gap_written"]
    assert r["same_twice"]
    _clean(r, case["name"])
    got = z["inv/" + case["name"]]
    mag, unit = sr.inverse_inputs(c)
    lengths = case["lengths"] or [c["n_out"]] * n_clips
    worst = worst32 = 0.0
    for k in range(n_clips):
        Tk = stft_np.frame_count(lengths[k], hop) if case["lengths"] else c["T"]
        for s in range(k * n_src, (k + 1) * n_src):
            want, want32 = _inverse_refs((case["name"], s), mag[s, :Tk], unit[k, :Tk], N, hop)
            norm = sr.inverse_norm(N, hop, Tk, want.size)
            e = sr.weighted_error(got[s, :lengths[k]], want[:lengths[k]], norm[:lengths[k]])
            e32 = sr.weighted_error(want32, want, norm)
            worst, worst32 = max(worst, e), max(worst32, e32)
            assert e <= sr.FACTOR * e32 and e <= sr.BOUND_INV, "source %d: device %.3g, float32 restatement %.3g" % (s, e, e32)
            if case["onehot"] is not None:                                   # nothing of the frame outside its own N samples
                lo, hi = max(0, case["onehot"] * hop - N // 2), case["onehot"] * hop + N // 2
                o = got[s, :lengths[k]]
                assert not o[:lo].any() and not o[hi:].any(), "the frame leaked outside [%d, %d)" % (lo, hi)
    print("\n%s: kernel %d param %d, weighted error %.3g (float32 restatement %.3g)" % (case["name"], r["kernel"], r["param"],
                                                                                      worst, worst32))
    if case["public"]:
        pk, pp = sr.expected_inverse(dict(c, phase_input=True), n_cu)
        assert r["public_rc"] == 0 and r["public_kernel"] == pk and r["public_poison_left"] == 0, r
        if pk == sr.INV_SEQ:
            assert r["public_param"] == pp
        gp = z["inv_public/" + case["name"]]
        ph = np.angle(unit[0]).astype(np.float32)
        pw = 0.0
        for s in range(n_src):
            want, want32 = _inverse_refs((case["name"], s, "phase"), mag[s], None, N, hop, phase=ph)
            norm = sr.inverse_norm(N, hop, c["T"], want.size)
            e, e32 = sr.weighted_error(gp[s], want[:c["n_out"]], norm[:c["n_out"]]), sr.weighted_error(want32, want, norm)
            pw = max(pw, e)
            assert e <= sr.FACTOR * e32 and e <= sr.BOUND_INV, "phase input, source %d: device %.3g, restatement %.3g" % (s, e, e32)
        print("%s through dcs_stft_inverse_f32: kernel %d, weighted error %.3g" % (case["name"], r["public_kernel"], pw))


@pytest.mark.parametrize("case", sr.forward_cases(), ids=lambda c: c["name"])
def test_forward_kernel(runs, case):
    z, report = runs[case["switch"]]
    r = report["fwd/" + case["name"]]
    c = dict(case, n_samples=r["n_samples"])
    N, hop, n_clips, rows, n = c["N"], c["hop"], c["n_clips"], r["rows"], r["n_samples"]
    bins = N // 2 + 1
    assert r["rc"] == 0, r
    assert r["kernel"] == sr.expected_forward(case), "ran kernel %d, the case is written for %d" % (r["kernel"], sr.expected_forward(case))
    assert r["poison_left"] == 0 and r["foreign_written"] == 0 and r["padding_ok"], r
    _clean(r, case["name"])
    audio = sr.forward_audio(c).astype(np.float32)
    lengths = case["lengths"] or [n] * n_clips
    tab = sr.clip_table(lengths, hop, case["table"] == "compact") if case["table"] else None
    mag = z["fwd/%s/mag" % case["name"]]
    phase = z["fwd/%s/phase" % case["name"]] if case["phase"] else None
    unit = z["fwd/%s/unit" % case["name"]] if case["unit"] else None
    if unit is not None:
        unit = unit[..., 0] + 1j * unit[..., 1]
    fig = dict(mag=0.0, mag32=0.0, unit=0.0, phase=0.0, cpx32=0.0, ph32=0.0, norm=0.0)
    for k in range(n_clips):
        a = audio[k, :lengths[k]]
        X, X32 = sr.forward_ref64(a, N, hop), sr.forward_ref32(a, N, hop)
        T = X.shape[0]
        if case["interleave"]:
            idx = np.arange(rows) * n_clips + k
        elif case["table"] == "compact":
            idx = int(tab[k, 3]) + np.arange(int(tab[k, 5]))
        else:
            idx = k * rows + np.arange(rows)
        m = mag[idx]
        silent = np.array([not X[t].any() for t in range(T)])                # frames of zeros only (exact: the inputs are)
        if "silence" in sr.forward_regimes(c) and not case["lengths"]:
            assert silent.any()
        quiet = np.concatenate([silent, np.ones(len(idx) - T, dtype=bool)])  # and the rows past the last frame
        assert not m[quiet].any()
        fig["mag"] = max(fig["mag"], np.max(np.abs(m[:T] - np.abs(X))))
        fig["mag32"] = max(fig["mag32"], np.max(np.abs(np.abs(X32) - np.abs(X))))
        fig["cpx32"] = max(fig["cpx32"], np.max(np.abs(X32 - X)))
        # the float32 restatement of (mag, phase): the angle rounded to float32
        fig["ph32"] = max(fig["ph32"], np.max(np.abs(np.abs(X32) * np.exp(1j * np.angle(X32).astype(np.float32).astype(np.float64)) - X)))
        if unit is not None:
            u = unit[idx]
            assert np.all(u[quiet] == 1.0)
            fig["unit"] = max(fig["unit"], np.max(np.abs(m[:T] * u[:T] - X)))
            live = m[:T] > 0
            if live.any():
                fig["norm"] = max(fig["norm"], np.max(np.abs(np.abs(u[:T][live].astype(np.complex128)) - 1)))
        if phase is not None:
            ph = phase[idx]
            assert not ph[quiet].any()
            fig["phase"] = max(fig["phase"], np.max(np.abs(m[:T] * np.exp(1j * ph[:T].astype(np.float64)) - X)))
    print("\n%s: kernel %d, |mag| %.3g (restatement %.3g), mag*unit %.3g (%.3g), mag*exp(j phase) %.3g (%.3g), ||unit|-1| %.3g"
          % (case["name"], r["kernel"], fig["mag"], fig["mag32"], fig["unit"], fig["cpx32"], fig["phase"], fig["ph32"], fig["norm"]))
    assert fig["mag"] <= sr.FACTOR * fig["mag32"] and fig["mag"] <= sr.BOUND_MAG
    assert fig["unit"] <= sr.FACTOR * fig["cpx32"] and fig["unit"] <= sr.BOUND_CPX
    assert fig["phase"] <= sr.FACTOR * fig["ph32"] and fig["phase"] <= sr.BOUND_CPX
    assert fig["norm"] <= sr.BOUND_UNIT


def test_float64_kernels(runs):
    z, report = runs["none"]
    f64 = report["_f64"]
    for N, hop in sr.F64_INVERSE:
        r = f64["inv/%d_%d" % (N, hop)]
        assert r["rc"] == 0 and r["kernel"] == sr.INV_BLOCK and r["nan"] == 0, r
        c, mag, ph = _f64_inputs(N, hop)
        got = z["f64inv/%d_%d" % (N, hop)]
        worst = 0.0
        for s in range(mag.shape[0]):
            want = sr.inverse_ref64(mag[s], None, N, hop, phase=ph)
            norm = sr.inverse_norm(N, hop, c["T"], want.size)
            worst = max(worst, sr.weighted_error(got[s], want[:c["n_out"]], norm[:c["n_out"]]))
        print("float64 inverse (%d, %d): weighted error %.3g" % (N, hop, worst))
        assert worst <= sr.BOUND_F64
    # frameSize 8192 at hop 8192 needs more LDS than a workgroup can have: refused, nothing launched
    r = f64["inv/8192_8192"]
    assert sr.block_inverse_plan(8192, 8192, 1000, 2, report["_n_cu"], size=8) is None
    assert r["rc"] == EUNSUPPORTED and np.isnan(z["f64inv/8192_8192"]).all(), r
    for N, hop in sr.F64_FORWARD:
        r = f64["fwd/%d_%d" % (N, hop)]
        assert r["rc"] == 0 and r["kernel"] == sr.FWD_BLOCK, r
        c, a = _f64_audio(N, hop)
        X = sr.forward_ref64(a, N, hop)
        m, ph = z["f64fwd/%d_%d/mag" % (N, hop)], z["f64fwd/%d_%d/phase" % (N, hop)]
        e_mag, e_cpx = np.max(np.abs(m - np.abs(X))), np.max(np.abs(m * np.exp(1j * ph) - X))
        print("float64 forward (%d, %d): |mag| %.3g, complex %.3g" % (N, hop, e_mag, e_cpx))
        assert e_mag <= sr.BOUND_F64 and e_cpx <= 2 * sr.BOUND_F64


def test_wrappers_refuse_bad_arguments(runs):
    args = runs["none"][1]["_args"]
    assert len(args) > 35
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        if r["want"] != 0:
            assert r["untouched"], label
