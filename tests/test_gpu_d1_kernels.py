"""Every kernel of the deep score-informed graph build_ca_1x1 on the MI355X, one launch at a time, against float64: the seven
modes of ``d1_igemm_kernel`` in every NT width the separator and the trainer launch, and the small kernels around them
(``d1_to_cl``, ``d1_mask``, ``code_apply``, ``codes_out``, both weight packers).

The launches are reached through ``dcs_debug_d1_conv`` / ``dcs_debug_d1_aux`` (the launch arguments filled by the helpers the
graph uses, every buffer checked first, the launch issued by the translation unit that issues it in production); the aid returns
the NT and the grid, which the test compares with the selection restated in tests/d1_ref.py.  Three child processes (forward
type, transposed type, small kernels), one after another, each under its own ``timeout -k 10`` (``CHILD_LIMIT``; the parent
stops at the first child that ends in a signal or at its limit), each with ``DCS_WS_GUARD``.  Every launch runs on buffers
carved out of one poisoned allocation, 64 KiB between and around them; every data set of a case runs under the poisons 0xFF and
0x4B and a second time over its own output.  The children write what the launches wrote, the parent compares by the rules of
tests/d1_ref.py, tests/gemm_ref.py and tests/conv_ref.py.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import conv_ref as cr
import d1_ref as d1
import maskcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GB = 1 << 16
CHILD_LIMIT = 120                      # seconds per child; the children take a few seconds each
GROUPS = ("fwd", "tr", "aux")
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class ConvArgs(ctypes.Structure):
    """dcs_debug_d1_args of include/dcs.h"""
    _fields_ = [("images", i32), ("Hi", i32), ("Wi", i32), ("Ci", i32), ("Ho", i32), ("Wo", i32), ("kh", i32), ("kw", i32), ("stride", i32),
                ("par", i32), ("N", i32), ("Co", i32), ("n_total", i64), ("k_first", i64), ("ch_off", i32), ("trainer_unit", i32),
                ("in_", vp), ("in_bytes", i64), ("code", vp), ("code_bytes", i64), ("B", vp), ("B_bytes", i64), ("b0", vp), ("b0_bytes", i64),
                ("b1", vp), ("b1_bytes", i64), ("out", vp), ("out_bytes", i64), ("code_out", vp), ("code_out_bytes", i64),
                ("nt", i32), ("grid_x", i32), ("grid_y", i32), ("K", i32), ("Kpad", i32), ("Wq", i32), ("M", i64)]


class AuxArgs(ctypes.Structure):
    """dcs_debug_d1_aux_args of include/dcs.h"""
    _fields_ = [("n", i64), ("plane", i64), ("n_total", i64), ("k_first", i64), ("rows", i64), ("per", i64), ("hw", i64),
                ("C", i32), ("Cp", i32), ("mode", i32), ("mix_n", i32), ("nsum", i32), ("Cin", i32), ("Cout", i32), ("kh", i32), ("kw", i32),
                ("in_", vp), ("in_bytes", i64), ("in2", vp), ("in2_bytes", i64), ("out", vp), ("out_bytes", i64), ("out2", vp),
                ("out2_bytes", i64), ("out3", vp), ("out3_bytes", i64)]


NAMES = {"in": "in_", "code": "code", "B": "B", "b0": "b0", "b1": "b1", "out": "out", "code_out": "code_out"}


def conv_buffers(c):
    """name -> bytes of every buffer of the launch; inputs come from d1.inputs"""
    g = d1.geom(c)
    sizes = {"out": int(np.prod(d1.out_shape(c))) * 4}
    if c["mode"] == d1.FWD:
        sizes["code_out"] = g["M"] * g["Co"]
    return sizes


def own_bytes(c, name):
    if name == "code_out":
        return np.ones(d1.geom(c)["M"] * d1.geom(c)["Co"], dtype=bool)
    m = np.zeros(d1.out_shape(c), dtype=bool)
    m[d1.owned(c)] = True
    return np.repeat(m.reshape(-1), 4)


# ------------------------------------------------------------------------------------------------ the child process
def child(group, out_path):
    import torch
    from deepconvsep_amd.runtime import default_context

    ctx = default_context()
    lib = ctx._lib
    arrays, report = {}, {}

    def arena(sizes, poison):
        place, off = {}, GB
        for name, nbytes in sizes.items():
            place[name] = (off, nbytes)
            off += (nbytes + 255) // 256 * 256 + GB
        return torch.full((off,), poison, dtype=torch.uint8, device="cuda"), place

    def put(raw, place, name, host):
        off, nbytes = place[name]
        b = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert b.size == nbytes, (name, b.size, nbytes)
        raw[off:off + nbytes].copy_(torch.from_numpy(b))

    def finish(raw, place, poison, outputs):
        """outputs: {buffer: boolean byte mask of what the launch owns}; every other byte of the arena that is not an input
        must still be poison.  Returns (host copies of the outputs, untouched, bytes changed outside every buffer)"""
        ctx.synchronize()
        host, untouched = {}, True
        for name, own in outputs.items():
            off, nbytes = place[name]
            host[name] = raw[off:off + nbytes].cpu().numpy()
            untouched = untouched and bool(np.all(host[name][~own] == poison))
        total = int((raw != poison).sum().item())
        inside = sum(int((raw[o:o + b] != poison).sum().item()) for o, b in place.values())
        return host, untouched, total - inside

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:
            return -1, str(exc)

    def run_conv(c, kind, poison, twice):
        g, inp = d1.geom(c), d1.inputs(c, kind)
        sizes = {k: v.nbytes for k, v in inp.items()}
        sizes.update(conv_buffers(c))
        raw, place = arena(sizes, poison)
        for k, v in inp.items():
            put(raw, place, k, v)
        a = ConvArgs()
        a.images, a.Hi, a.Wi, a.Ci, a.kh, a.kw, a.stride, a.par = c["images"], g["Hi"], g["Wi"], g["Ci"], c["kh"], c["kw"], g["stride"], c["par"]
        if c["mode"] not in d1.FORWARD_TYPE:
            a.Ho, a.Wo = g["Ho"], g["Wo"]
        a.N, a.Co, a.n_total, a.k_first, a.ch_off, a.trainer_unit = g["N"], g["Co"], c["n_total"], c["k_first"], c["ch_off"], c["unit"]
        for name, (off, nbytes) in place.items():
            setattr(a, NAMES[name], raw.data_ptr() + off)
            setattr(a, NAMES[name].rstrip("_") + "_bytes", nbytes)
        rc = [lib.dcs_debug_d1_conv(ctx._h, c["mode"], ctypes.byref(a)) for _ in range(2 if twice else 1)]
        host, untouched, damage = finish(raw, place, poison, {k: own_bytes(c, k) for k in conv_buffers(c)})
        sel = dict(nt=a.nt, grid=[a.grid_x, a.grid_y], K=a.K, Kpad=a.Kpad, Wq=a.Wq, M=a.M, Ho=a.Ho, Wo=a.Wo)
        return dict(rc=rc, out=host, untouched=untouched, damage=damage, sel=sel)

    if group in ("fwd", "tr"):
        for c in d1.cases():
            if c["group"] != group:
                continue
            t0 = time.time()
            rep = dict(rc=[], untouched=True, damage=0, same=True)
            for kind in d1.kinds_of(c):
                r1, r2 = run_conv(c, kind, 0xFF, False), run_conv(c, kind, 0x4B, True)
                rep["rc"] += r1["rc"] + r2["rc"]
                rep["sel"] = r1["sel"]
                rep["same"] = rep["same"] and r1["sel"] == r2["sel"]
                rep["untouched"] = rep["untouched"] and r1["untouched"] and r2["untouched"]
                rep["damage"] += r1["damage"] + r2["damage"]
                for name, b in r1["out"].items():                       # what the launch owns; the rest differs by the poison
                    own = own_bytes(c, name)
                    rep["same"] = rep["same"] and bool(np.array_equal(b[own], r2["out"][name][own]))
                    arrays["%s/%s/%s" % (c["name"], kind, name)] = b
            rep["scratch_blocks"], rep["scratch_guard"] = guards()
            rep["seconds"] = time.time() - t0
            report[c["name"]] = rep
    else:
        _aux(torch, ctx, lib, arena, put, finish, arrays, report)
        report["_guards"] = guards()
        report["_args"] = _arguments(torch, ctx, lib)
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _aux(torch, ctx, lib, arena, put, finish, arrays, report):
    def call(which, sizes, fill, outputs, **fields):
        """both poisons, the second one twice; fill {buffer: host array}, outputs {buffer: own mask or None (all)}"""
        runs = []
        for poison, times in ((0xFF, 1), (0x4B, 2)):
            raw, place = arena(sizes, poison)
            for k, v in fill.items():
                put(raw, place, k, v)
            a = AuxArgs()
            for k, v in fields.items():
                setattr(a, k, v)
            for name, (off, nbytes) in place.items():
                setattr(a, name, raw.data_ptr() + off)
                setattr(a, name.rstrip("_") + "_bytes", nbytes)
            rcs = []
            for t in range(times):
                if t and which == d1.AUX_CODE_APPLY:                    # in place: the second launch starts from the same data
                    put(raw, place, "out", fill["out"])
                rcs.append(lib.dcs_debug_d1_aux(ctx._h, which, ctypes.byref(a)))
            owns = {k: (np.ones(sizes[k], dtype=bool) if v is None else v) for k, v in outputs.items()}
            host, untouched, damage = finish(raw, place, poison, owns)
            runs.append(dict(rc=rcs, host=host, untouched=untouched, damage=damage, owns=owns))
        r1, r2 = runs
        same = all(np.array_equal(r1["host"][k][r1["owns"][k]], r2["host"][k][r1["owns"][k]]) for k in outputs)
        return r1["host"], dict(rc=r1["rc"] + r2["rc"], untouched=r1["untouched"] and r2["untouched"], damage=r1["damage"] + r2["damage"],
                                same=bool(same))

    # d1_to_cl: three tiles of 255 pixels: three workgroups, the last one partial
    n, plane = 3, 255
    x = d1._rs("to_cl").standard_normal((n, 4, plane)).astype(np.float32)
    host, report["to_cl"] = call(d1.AUX_TO_CL, dict(in_=x.nbytes, out=x.nbytes), dict(in_=x), dict(out=None), n=n, plane=plane)
    arrays["to_cl/out"] = host["out"]
    # codes_out
    n, hw, C, Cp = 2, 77, 30, 32
    code = d1._rs("codes_out").randint(0, 3, size=(n, hw, Cp)).astype(np.uint8)
    host, report["codes_out"] = call(d1.AUX_CODES_OUT, dict(in_=code.nbytes, out=n * C * hw * 4), dict(in_=code), dict(out=None), n=n, hw=hw, C=C, Cp=Cp)
    arrays["codes_out/out"] = host["out"]
    # code_apply, with and without partial sums
    for Cp, C in d1.CODE_APPLY_CHANNELS:
        for rows, per, nsum in d1.CODE_APPLY_ROWS:
            buf, code = d1.code_apply_inputs(Cp, C, rows)
            for sums in (1, 0):
                key = "code_apply/%d/%d/%d/%d" % (Cp, rows, nsum, sums)
                sizes = dict(in2=code.nbytes, out=buf.nbytes)
                outs = dict(out=None)
                if sums:
                    sizes["out2"] = nsum * C * 4
                    outs["out2"] = None
                host, report[key] = call(d1.AUX_CODE_APPLY, sizes, dict(in2=code, out=buf), outs, rows=rows, per=per, nsum=nsum, Cp=Cp, C=C)
                for k, v in host.items():
                    arrays[key + "/" + k] = v
    # the packers: the device packer writes live elements only, into operands that were zero
    for cin, cout, kh, kw in d1.PACK_LAYERS:
        W = d1.pack_weights(cin, cout, kh, kw)
        want = [d1.pack_B(W), d1.pack_Bt(W, 0)] + ([d1.pack_Bt(W, 1)] if kw > 1 else [])
        sizes = dict(in_=W.nbytes, out=want[0].nbytes, out2=want[1].nbytes)
        if kw > 1:
            sizes["out3"] = want[2].nbytes
        outs = {k: None for k in sizes if k != "in_"}
        for which, src, zero in ((d1.AUX_PACK_HOST, W, False), (d1.AUX_PACK_DEVICE, d1.internal_W(W), True)):
            fill = dict(in_=src)
            if zero:
                fill.update({k: np.zeros(sizes[k], dtype=np.uint8) for k in outs})
            key = "pack/%d/%d/%d/%d/%d" % (which, cin, cout, kh, kw)
            host, report[key] = call(which, sizes, fill, outs, Cin=cin, Cout=cout, kh=kh, kw=kw)
            for k, v in host.items():
                arrays[key + "/" + k] = v
    # d1_mask: two tiles written into the middle of four, both eps modes, both mixtures
    n, n_total, k_first, plane, C = 2, 4, 1, 301, 4
    own = np.zeros((4, n_total, plane, 4), dtype=bool)
    own[:, k_first:k_first + n] = True
    for kind in d1.MASK_KINDS:
        p, x = d1.mask_inputs(kind, n, plane, C)
        for mode in (0, 1):
            for mix_n in (1, C):
                key = "mask/%s/%d/%d" % (kind, mode, mix_n)
                host, report[key] = call(d1.AUX_MASK, dict(in_=p.nbytes, in2=x.nbytes, out=4 * n_total * plane * 4), dict(in_=p, in2=x),
                                         dict(out=own.reshape(-1)), n=n, n_total=n_total, k_first=k_first, plane=plane, C=C, mode=mode, mix_n=mix_n)
                arrays[key + "/out"] = host["out"]


def _arguments(torch, ctx, lib):
    """one case per class of refusal: the status, and nothing written"""
    res = {}
    cases = {c["name"]: c for c in d1.cases()}
    for cname in ("FWD 30->50 3x3x38", "TR 30<-50 3x2x6 par 1", "LAST 4<-30 1x1x6 par 0 tile 2 of 3 ch 4", "FWDC 4->30 3x2x37"):
        c = cases[cname]
        g, inp = d1.geom(c), d1.inputs(c, "signed")
        sizes = {k: v.nbytes for k, v in inp.items()}
        sizes.update(conv_buffers(c))
        bufs = {k: torch.full((v + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
        for k, v in inp.items():
            bufs[k][:v.nbytes].copy_(torch.from_numpy(v.view(np.uint8).reshape(-1)))

        def run(label, want, mode=c["mode"], **kw):
            for k in conv_buffers(c):
                bufs[k].fill_(0xFF)
            a = ConvArgs()
            a.images, a.Hi, a.Wi, a.Ci, a.kh, a.kw, a.stride, a.par = c["images"], g["Hi"], g["Wi"], g["Ci"], c["kh"], c["kw"], g["stride"], c["par"]
            a.Ho, a.Wo = g["Ho"], g["Wo"]
            a.N, a.Co, a.n_total, a.k_first, a.ch_off, a.trainer_unit = g["N"], g["Co"], c["n_total"], c["k_first"], c["ch_off"], c["unit"]
            for name in sizes:
                setattr(a, NAMES[name], bufs[name].data_ptr())
                setattr(a, NAMES[name].rstrip("_") + "_bytes", sizes[name])
            for k, v in kw.items():
                setattr(a, k, (bufs[v[0]].data_ptr() + v[1]) if isinstance(v, tuple) else v)
            rc = lib.dcs_debug_d1_conv(ctx._h, mode, ctypes.byref(a))
            ctx.synchronize()
            untouched = all(bool((bufs[k] == 0xFF).all().item()) for k in conv_buffers(c))
            res["%s: %s" % (cname, label)] = dict(rc=rc, want=want, untouched=untouched, message=lib.dcs_last_error().decode("utf-8", "replace"))

        run("good", 0)
        for name in sizes:
            f = NAMES[name]
            run("%s one byte short" % name, d1.EINVAL, **{f.rstrip("_") + "_bytes": sizes[name] - 1})
            run("%s misaligned" % name, d1.EINVAL, **{f: (name, 4)})
            run("null %s" % name, d1.EINVAL, **{f: None})
        run("no image (M == 0)", d1.EINVAL, images=0)
        run("input pitch not a multiple of 4", d1.EINVAL, Ci=g["Ci"] - 2)
        if c["mode"] != d1.LAST:
            run("output pitch not a multiple of 4", d1.EINVAL, Co=g["Co"] + 2)
            run("output pitch below N", d1.EINVAL, Co=g["Co"] - 4)
        run("filter taller than the image", d1.EINVAL, kh=c["kh"] + g["Hi"] + 64)
        if c["mode"] not in d1.FORWARD_TYPE:
            # D1Args: a tap holds at least 16 floats.  With 12 the kernel's K walk would start past the tap (found by this suite)
            run("a tap of 12 floats", d1.EINVAL, Ci=12)
        run("mode 7", d1.EINVAL, mode=7)
        run("no channel", d1.EINVAL, N=0)
        if c["mode"] == d1.LAST:
            run("tiles past n_total", d1.EINVAL, k_first=c["n_total"])
            run("a separator mode from the trainer's unit", d1.EINVAL, trainer_unit=1)
        if c["mode"] not in d1.FORWARD_TYPE:
            run("parity 2", d1.EINVAL, par=2)
            run("rows that are not the transpose's", d1.EINVAL, Ho=g["Ho"] + 1)
    res["null arguments"] = dict(rc=lib.dcs_debug_d1_conv(ctx._h, 0, None), want=d1.EINVAL, untouched=True, message="")
    res["null context"] = dict(rc=lib.dcs_debug_d1_aux(None, 0, None), want=d1.EINVAL, untouched=True, message="")
    # the small kernels: one of each class on d1_to_cl, and an unknown kernel
    n, plane = 2, 100
    bufs = {k: torch.full((n * plane * 16 + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k in ("in_", "out")}

    def aux(label, want, which=d1.AUX_TO_CL, **kw):
        bufs["out"].fill_(0xFF)
        a = AuxArgs()
        a.n, a.plane = n, plane
        for name in bufs:
            setattr(a, name, bufs[name].data_ptr())
            setattr(a, name.rstrip("_") + "_bytes", n * plane * 16)
        for k, v in kw.items():
            setattr(a, k, (bufs[v[0]].data_ptr() + v[1]) if isinstance(v, tuple) else v)
        rc = lib.dcs_debug_d1_aux(ctx._h, which, ctypes.byref(a))
        ctx.synchronize()
        res["aux: " + label] = dict(rc=rc, want=want, untouched=bool((bufs["out"] == 0xFF).all().item()), message=lib.dcs_last_error().decode("utf-8", "replace"))

    aux("good", 0)
    aux("output one byte short", d1.EINVAL, out_bytes=n * plane * 16 - 1)
    aux("input misaligned", d1.EINVAL, in_=("in_", 4))
    aux("null output", d1.EINVAL, out=None)
    aux("no tile", d1.EINVAL, n=0)
    aux("kernel 9", d1.EINVAL, which=9)
    aux("code_apply with a pitch above the workgroup", d1.EINVAL, which=d1.AUX_CODE_APPLY, rows=4, per=4, nsum=1, Cp=260, C=4)
    aux("packer with kw 3", d1.EINVAL, which=d1.AUX_PACK_DEVICE, Cin=4, Cout=4, kh=1, kw=3)
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_d1_kernels as t; t.child(sys.argv[2], sys.argv[3])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """group -> (arrays, report): one child after another, each under its own time limit; a child that ends in a signal or at
    its limit ends the run (nothing more is started on the device)"""
    d = tmp_path_factory.mktemp("d1_kernels")
    res = {}
    for name in GROUPS:
        out = str(d / (name + ".npz"))
        env = dict(os.environ)
        env.update(DCS_WS_GUARD=str(GB))
        t0 = time.time()
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, "-c", _CHILD, ROOT, name, out], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        print("group %s: child took %.1f s (limit %d), status %d" % (name, time.time() - t0, CHILD_LIMIT, p.returncode), flush=True)
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            pytest.exit("group %s: the child ended with status %d; no further child is started\n%s" % (name, p.returncode, p.stderr[-2000:]), 1)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-400:], p.stderr[-2000:])
        z = np.load(out)
        res[name] = (z, json.loads(bytes(z["_report"]).decode()))
    return res


WORST = {}
_REF = {}


def _ref(c, kind):
    """float64 result, S, the in-order float32 restatement, the live mask and the inputs, shared among the tests"""
    key = (c["name"], kind)
    if key not in _REF:
        inp = d1.inputs(c, kind)
        want = d1.launch_ref(c, inp)
        rest = d1.launch_ref(c, inp, d1.mul_chain)["out"].astype(np.float64) if kind == "signed" else None
        S = d1.launch_ref(c, inp, d1.mul_abs)
        _REF[key] = (want, S, rest, inp)
    return _REF[key]


@pytest.mark.parametrize("c", d1.cases(), ids=lambda c: c["name"])
def test_launch(runs, c):
    z, report = runs[c["group"]]
    r, g = report[c["name"]], d1.geom(c)
    mode, N, K = c["mode"], g["N"], g["K"]
    # 1. the launch is the one the restated selection predicts
    assert all(rc == 0 for rc in r["rc"]) and len(r["rc"]) == 3 * len(d1.kinds_of(c)), r["rc"]
    want_sel = dict(nt=g["nt"], grid=list(g["grid"]), K=K, Kpad=g["Kpad"], Wq=g["Wq"], M=g["M"], Ho=g["Ho"], Wo=g["Wo"])
    assert r["sel"] == want_sel, (r["sel"], want_sel)
    # 2. only owned bytes are written; 3. both poisons and a second launch give the same bits
    assert r["untouched"], "bytes outside what the launch writes are no longer poison"
    assert r["damage"] == 0 and r["scratch_guard"] == "" and r["scratch_blocks"] >= 0, r
    assert r["same"], "the poisons 0xFF and 0x4B, or a second launch over the first, gave other bits"
    assert r["seconds"] < 20, "the case took %.1f s in the child" % r["seconds"]
    for kind in d1.kinds_of(c):
        tag = "%s %s" % (c["name"], kind)
        want, S, rest, inp = _ref(c, kind)
        got = z["%s/%s/out" % (c["name"], kind)].view(np.float32).reshape(d1.out_shape(c))[d1.owned(c)].astype(np.float64)
        assert got.shape == want["out"].shape
        assert np.isfinite(got).all(), "%s: values that are not finite" % tag
        if mode in (d1.FWD, d1.TR, d1.FWDC, d1.B11):
            assert not got[..., N:].any(), "%s: channels N .. Co-1 are not 0" % tag
        code = None
        if mode == d1.FWD:
            code = z["%s/%s/code_out" % (c["name"], kind)].reshape(g["M"], g["Co"])
            assert not code[:, N:].any(), "%s: code bytes of channels N .. Co-1 are not 0" % tag
        if kind in ("int", "ties"):
            # 4. / 5. exact: every partial sum is an integer (or a half) below 2^24
            bad = int((got != want["out"]).sum())
            assert bad == 0, "%s: %d of %d elements differ from the float64 result" % (tag, bad, got.size)
            if code is not None:
                assert np.array_equal(code, want["code"]), "%s: %d code bytes differ" % (tag, int((code != want["code"]).sum()))
                if kind == "ties":
                    pre = want["pre"]
                    assert (pre == 0).any() and (pre > 0).any() and (pre < 0).any()
                    assert np.all(code[:, :N][pre == 0] == 1) and np.all(code[:, :N][pre > 0] == 2) and np.all(code[:, :N][pre < 0] == 0)
                    assert np.array_equal(got[:, :N], np.maximum(pre, 0) + inp["b1"].astype(np.float64)[None])
            continue
        # 6. signed random: the two f32-class conditions of gemm_ref.py / conv_ref.py
        So = S["out"]
        cap = (K + cr.cap_c(K, "f32")) * d1.U * So
        e, e32 = cr.measure(got, want["out"], So), cr.measure(rest, want["out"], So)
        ratio = float(np.max(np.abs(got - want["out"]) / (cap + 1e-300)))
        print("\n%s: E %.3g, restatement %.3g, ratio %.2f, worst |err| / cap %.3g" % (tag, e, e32, e / max(e32, 1e-300), ratio))
        key = d1.MODE_NAMES[mode]
        WORST[key] = max(WORST.get(key, 0.0), e / max(e32, 1e-300))
        assert np.isfinite(e), "%s: an output nothing but zeros goes into is not 0" % tag
        assert e <= d1.FACTOR * e32, "%s: device %.3g, restatement %.3g" % (tag, e, e32)
        assert ratio <= 1.0, "%s: outside the cap by a factor of %.3g" % (tag, ratio)
        if code is not None:
            # the code is the sign of the device's own pre-activation: the float64 sign wherever |pre| exceeds the cap of pre
            pre = want["pre"]
            sure = np.abs(pre) > (K + cr.cap_c(K, "f32")) * d1.U * S["pre"]
            assert np.array_equal(code[:, :N][sure], want["code"][:, :N][sure]), "%s: code bytes differ where the sign is certain" % tag
            # and everywhere, certain or not, the code agrees with the output next to it: y = max(pre, 0) + b1 is b1 itself
            # under the codes 0 and 1 and not below b1 under the code 2
            b1 = np.broadcast_to(inp["b1"].astype(np.float64)[None], pre.shape)
            flat = code[:, :N] < 2
            assert np.all(code <= 2) and np.array_equal(got[:, :N][flat], b1[flat]) and np.all(got[:, :N][~flat] >= b1[~flat]), tag
            assert sure.mean() > 0.5, "%s: the sign is certain on %.2f of the outputs only" % (tag, sure.mean())


def test_every_production_instance_is_reached(runs):
    reached = {(c["mode"], d1.geom(c)["nt"], c["unit"]) for c in d1.cases() if all(rc == 0 for rc in runs[c["group"]][1][c["name"]]["rc"])
               and runs[c["group"]][1][c["name"]]["sel"]["nt"] == d1.geom(c)["nt"]}
    missing = d1.PRODUCTION - reached
    assert not missing, "never launched: %r" % sorted((d1.MODE_NAMES[m], nt, "trainer" if u else "separator") for m, nt, u in missing)
    print("\nlargest E / E(restatement) per mode: %r" % sorted(WORST.items()))
    print("child seconds per case, the slowest: %r" % sorted(((round(r["seconds"], 2), k) for n in ("fwd", "tr") for k, r in runs[n][1].items()),
                                                             reverse=True)[:5])


def _aux_ok(report, key, calls=3):
    r = report[key]
    assert r["rc"] == [0] * calls, (key, r)
    assert r["untouched"] and r["damage"] == 0 and r["same"], (key, r)


def test_to_cl_and_codes_out(runs):
    z, report = runs["aux"]
    assert report["_guards"][1] == "" and report["_guards"][0] >= 0
    _aux_ok(report, "to_cl")
    x = d1._rs("to_cl").standard_normal((3, 4, 255)).astype(np.float32)
    assert np.array_equal(z["to_cl/out"].view(np.uint32), d1.to_cl(x).view(np.uint32).reshape(-1))
    _aux_ok(report, "codes_out")
    code = d1._rs("codes_out").randint(0, 3, size=(2, 77, 32)).astype(np.uint8)
    assert np.array_equal(z["codes_out/out"].view(np.uint32), d1.codes_out(code, 30).view(np.uint32).reshape(-1))


@pytest.mark.parametrize("Cp,C", d1.CODE_APPLY_CHANNELS)
def test_code_apply(runs, Cp, C):
    z, report = runs["aux"]
    for rows, per, nsum in d1.CODE_APPLY_ROWS:
        buf, code = d1.code_apply_inputs(Cp, C, rows)
        out, part = d1.code_apply(buf, code, C, per, nsum)
        for sums in (1, 0):
            key = "code_apply/%d/%d/%d/%d" % (Cp, rows, nsum, sums)
            _aux_ok(report, key)
            assert np.array_equal(z[key + "/out"].view(np.uint32), out.view(np.uint32).reshape(-1)), key
            if sums:
                got = z[key + "/out2"].view(np.float32).reshape(nsum, C)
                assert np.array_equal(got.view(np.uint32), part.view(np.uint32)), (key, float(np.max(np.abs(got - part))))
                # against float64 too: the restatement itself is a sum of at most `per` terms
                S = np.stack([np.abs(buf[w * per:(w + 1) * per, :C].astype(np.float64)).sum(axis=0) for w in range(nsum)])
                w64 = np.stack([buf[w * per:(w + 1) * per, :C].astype(np.float64).sum(axis=0) for w in range(nsum)])
                assert np.all(np.abs(got - w64) <= per * d1.U * S)


@pytest.mark.parametrize("layer", d1.PACK_LAYERS, ids=lambda l: "%d-%d-%dx%d" % l)
def test_packers(runs, layer):
    z, report = runs["aux"]
    cin, cout, kh, kw = layer
    W = d1.pack_weights(cin, cout, kh, kw)
    want = dict(out=d1.pack_B(W), out2=d1.pack_Bt(W, 0))
    if kw > 1:
        want["out3"] = d1.pack_Bt(W, 1)
    for which in (d1.AUX_PACK_HOST, d1.AUX_PACK_DEVICE):
        key = "pack/%d/%d/%d/%d/%d" % (which, cin, cout, kh, kw)
        _aux_ok(report, key)
        for k, w in want.items():
            got = z[key + "/" + k].view(np.uint32)
            assert np.array_equal(got, w.view(np.uint32).reshape(-1)), (key, k)          # pads included: still zero
    for k in want:
        assert np.array_equal(z["pack/%d/%d/%d/%d/%d/%s" % (d1.AUX_PACK_HOST, cin, cout, kh, kw, k)],
                              z["pack/%d/%d/%d/%d/%d/%s" % (d1.AUX_PACK_DEVICE, cin, cout, kh, kw, k)])


@pytest.mark.parametrize("kind", d1.MASK_KINDS)
def test_mask(runs, kind):
    z, report = runs["aux"]
    n, n_total, k_first, plane, C = 2, 4, 1, 301, 4
    p, x = d1.mask_inputs(kind, n, plane, C)
    for mode in (0, 1):
        for mix_n in (1, C):
            key = "mask/%s/%d/%d" % (kind, mode, mix_n)
            _aux_ok(report, key)
            got = z[key + "/out"].view(np.float32).reshape(4, n_total, plane)[:, k_first:k_first + n].astype(np.float64)
            want, mix = d1.mask_ref(p, x, mode, mix_n)
            p4 = p.astype(np.float64).transpose(1, 0, 2)[:, :, None, :]
            rec = maskcheck.check_masked(got[:, :, None, :], want[:, :, None, :], p4, p4.copy(), mix[:, None, :], 4, "AB"[mode], label=key, report=None)
            assert rec["within_conditioning_bound"] and rec["valid_magnitudes"] and rec["mask_consistent"], rec
            # the bound says something: all four sources are zero on 1 / 16 of the rand bins and on 0.8 of the sparse ones
            assert rec["conditioned_fraction"] >= dict(rand=0.8, pos=0.99, sparse=0.1, tiny=0.0)[kind], rec


def test_entries_refuse_bad_arguments(runs):
    args = runs["aux"][1]["_args"]
    assert len(args) > 60
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        if r["want"] != 0:
            assert r["untouched"], label
