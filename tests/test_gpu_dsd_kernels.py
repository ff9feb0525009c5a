"""Every decoder kernel of the DSD graphs on the MI355X -- transposed conv2, the split pass, transposed conv1 + bias + rectify +
soft mask + cross-fade fold, in their throughput, bf16 x 3 and one-batch forms -- directly against float64, one stage at a time.

The stages are reached through ``dcs_debug_dsd_stage`` (the launchers the separation paths call, with every buffer checked
first); after every launch ``dcs_debug_dsd_last_kernel`` says which kernel each role ran and with which launcher choices, and the
test asserts that they are what ``dsd_ref.expected`` derives from the launchers' arithmetic.  One child process per switch set
(``dsd_ref.SWITCHES``: the library reads them once per process), one after another, each under its own ``timeout -k 10``
(``CHILD_LIMIT``; the parent stops at the first child that ends in a signal or at its limit), each with ``DCS_WS_GUARD`` and each
running its cases on buffers carved out of one poisoned allocation per launch: 64 KiB between and around the buffers, everything
a stage does not write born as poison.  A case runs every data set under the poisons 0xFF and 0x4B and a second time over its
own output; the children write what the stages wrote, the parent compares by the rules of tests/dsd_ref.py.
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
import dsd_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GB = 1 << 16
CHILD_LIMIT = 60                       # seconds per child, about ten times the longest measured (4.8 s): DESIGN 4p4
vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
INT_SCALE, SCALE = 1.0, 0.3


class DsdArgs(ctypes.Structure):
    """dcs_debug_dsd_args of include/dcs.h"""
    _fields_ = [("family", i32), ("no_bq", i32), ("D", vp), ("D_bytes", i64), ("G", vp), ("G_bytes", i64), ("Gs", vp), ("Gs_bytes", i64),
                ("mix", vp), ("mix_bytes", i64), ("mix_ld", i64), ("out", vp), ("out_bytes", i64), ("out_ld", i64), ("out_src_stride", i64),
                ("n_items", i64), ("n", i64), ("rows", i64), ("ov", i32), ("fold", i32), ("mask_mode", i32), ("scale", f32),
                ("n_clips", i32), ("g_clip_tiles", i64), ("mix_clip_stride", i64), ("out_clip_stride", i64), ("clip_tab_h", vp)]


final_inputs = dr.inputs


def final_geometry(c):
    Fe, ld = dr.row_width(c["F"], c["C"])
    pitch = c["C"] * ld if c["ov"] is not None else Fe                  # the operator form: rows of F floats, F odd
    return Fe, pitch


def planes_reader(code):
    return code in (dr.K_FINAL_BF16X3, dr.K_FINAL_BF16X3 + 1, dr.K_LAT_FINAL, dr.K_LAT_FINAL + 1)


# ------------------------------------------------------------------------------------------------ the child process
def child(switch, out_path):
    import torch
    from deepconvsep_amd.runtime import Network, default_context

    ctx = default_context()
    lib = ctx._lib
    n_cu = int(torch.cuda.get_device_properties(ctx.device_index).multi_processor_count)
    arrays, report, nets = {}, {"_n_cu": n_cu}, {}

    def net(C, tc, F, kind):
        key = (C, tc, F, kind)
        if key not in nets:
            nets[key] = Network(ctx, "dsd" if C == 1 else "dsd_ild", dr.params(C, tc, F, kind), tc, F)
        return nets[key]

    def last(h):
        codes, prm = (i32 * 3)(), (i64 * 8)()
        assert lib.dcs_debug_dsd_last_kernel(h, codes, prm) == 0
        return {dr.ROLES[r]: codes[r] for r in range(3) if codes[r]}, list(prm)

    def arena(sizes, poison):
        place, off = {}, GB
        for name, nbytes in sizes.items():
            place[name] = (off, nbytes)
            off += (nbytes + 255) // 256 * 256 + GB
        return torch.full((off,), poison, dtype=torch.uint8, device="cuda"), place

    def finish(res, raw, place, poison, owned):
        """owned: {buffer: boolean byte mask (numpy) or None for an input}; everything else must still be poison"""
        ctx.synchronize()
        untouched = True
        for name, (off, nbytes) in place.items():
            if name in owned and owned[name] is None:
                continue
            host = raw[off:off + nbytes].cpu().numpy()
            keep = ~owned[name] if name in owned else np.ones(nbytes, dtype=bool)
            untouched = untouched and bool(np.all(host[keep] == poison))
            if name in owned:
                res["out"][name] = host
                res.setdefault("own", {})[name] = owned[name]
        total = int((raw != poison).sum().item())
        inside = sum(int((raw[o:o + b] != poison).sum().item()) for o, b in place.values())
        res["untouched"], res["damage"] = untouched, total - inside
        return res

    def run_deconv2(c, kind, poison, twice, exp):
        d, n = dr.dims(c["tc"]), c["n"]
        m = net(1, c["tc"], 65, kind)
        sizes = dict(D=n * d["h2"] * dr.CP * 4, G=n * dr.NGG * c["tc"] * 32, Gs=n * dr.NGG * c["tc"] * 48)
        raw, place = arena(sizes, poison)
        view = lambda name: raw[place[name][0]:place[name][0] + place[name][1]]
        Dp = np.zeros((n, d["h2"], dr.CP), dtype=np.float32)            # the pad filters 50, 51 are zero, as the dense layers leave them
        Dp[:, :, :dr.NF] = dr.dense(c["tc"], n, kind)
        view("D").copy_(torch.from_numpy(Dp.view(np.uint8).reshape(-1)))
        a = DsdArgs()
        a.family, a.no_bq, a.n_items = c["family"], c["no_bq"], n
        a.D, a.D_bytes = view("D").data_ptr(), sizes["D"]
        if c["g"]:
            a.G, a.G_bytes = view("G").data_ptr(), sizes["G"]
        if c["gs"]:
            a.Gs, a.Gs_bytes = view("Gs").data_ptr(), sizes["Gs"]
        res = dict(rc=[], out={})
        for _ in range(2 if twice else 1):
            res["rc"].append(lib.dcs_debug_dsd_stage(m._h, dr.STAGE_DECONV2, ctypes.byref(a)))
        res["kernels"], res["params"] = last(m._h)
        owned = dict(D=None)
        if exp["rc"] == 0:
            code = exp["kernels"]["deconv2"]
            if c["g"] and code in (dr.K_DECONV2, dr.K_STREAM, dr.K_LAT_DECONV2):
                owned["G"] = np.ones(sizes["G"], dtype=bool)
            if c["gs"] and code != dr.K_STREAM:
                owned["Gs"] = np.ones(sizes["Gs"], dtype=bool)
        return finish(res, raw, place, poison, owned)

    def run_final(c, kind, poison, twice, exp):
        tc, C, n, rows, nc = c["tc"], c["C"], c["n"], c["rows"], c["n_clips"]
        nbr = 3 if C == 1 else 4
        m = net(C, tc, c["F"], kind)
        clips, rows_all, tiles_all, tab = dr.clip_layout(c)
        Fe, pitch = final_geometry(c)
        G, mix = final_inputs(c, kind)
        sizes = dict(G=tiles_all * nbr * dr.NGG * tc * 32, Gs=tiles_all * nbr * dr.NGG * tc * 48, mix=rows_all * pitch * 4,
                     out=nc * 4 * rows * pitch * 4)
        raw, place = arena(sizes, poison)
        view = lambda name: raw[place[name][0]:place[name][0] + place[name][1]]
        put = lambda name, host: view(name).copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1)))
        items = G.reshape(tiles_all * nbr, dr.NF, tc)
        planes = exp["rc"] == 0 and planes_reader(exp["kernels"]["final"])
        if not planes:                                                  # a kernel that reads the planes finds poison in G
            put("G", dr.g_layout(items))
        if c["gs"]:
            put("Gs", dr.planes_layout(items))
        put("mix", mix[:, :pitch])
        a = DsdArgs()
        a.family, a.n, a.rows, a.mask_mode, a.scale = c["family"], n, rows, c["mode"], (INT_SCALE if kind == "int" else SCALE)
        a.fold, a.ov = (1, c["ov"]) if c["ov"] is not None else (0, 0)
        a.G, a.G_bytes = view("G").data_ptr(), sizes["G"]
        if c["gs"]:
            a.Gs, a.Gs_bytes = view("Gs").data_ptr(), sizes["Gs"]
        a.mix, a.mix_bytes, a.mix_ld = view("mix").data_ptr(), sizes["mix"], pitch
        a.out, a.out_bytes, a.out_ld, a.out_src_stride = view("out").data_ptr(), sizes["out"], pitch, rows * pitch
        a.n_clips, a.g_clip_tiles, a.mix_clip_stride, a.out_clip_stride = nc, n, rows * pitch, 4 * rows * pitch
        tab_c = None
        if tab:
            tab_c = (i64 * len(tab))(*tab)
            a.clip_tab_h = ctypes.cast(tab_c, vp)
        res = dict(rc=[], out={})
        for _ in range(2 if twice else 1):
            res["rc"].append(lib.dcs_debug_dsd_stage(m._h, dr.STAGE_FINAL, ctypes.byref(a)))
        res["kernels"], res["params"] = last(m._h)
        own = np.zeros((nc, 4, rows, pitch, 4), dtype=bool)
        if exp["rc"] == 0:
            for k, (fr, nt, r0, t0) in enumerate(clips):
                own[k, :, :fr, :Fe] = True
        return finish(res, raw, place, poison, dict(G=None, Gs=None, mix=None, out=own.reshape(-1)))

    def chain(poison):
        """deconv2, then the final stage on the device's own hand-over, under poison"""
        c = dr.CHAIN
        d, tc, n, F = dr.dims(c["tc"]), c["tc"], c["n"], c["F"]
        m = net(1, tc, F, "rand")
        sizes = dict(D=n * 3 * d["h2"] * dr.CP * 4, G=n * 3 * dr.NGG * tc * 32, mix=c["rows"] * 68 * 4, out=4 * c["rows"] * 68 * 4)
        raw, place = arena(sizes, poison)
        view = lambda name: raw[place[name][0]:place[name][0] + place[name][1]]
        Dp = np.zeros((n * 3, d["h2"], dr.CP), dtype=np.float32)
        Dp[:, :, :dr.NF] = np.float32(0.25) * dr.dense(tc, n * 3, "rand")
        view("D").copy_(torch.from_numpy(Dp.view(np.uint8).reshape(-1)))
        view("mix").copy_(torch.from_numpy(dr.mixture(c["rows"], F, 1, "rand").view(np.uint8).reshape(-1)))
        a = DsdArgs()
        a.n_items, a.D, a.D_bytes, a.G, a.G_bytes = n * 3, view("D").data_ptr(), sizes["D"], view("G").data_ptr(), sizes["G"]
        rc = [lib.dcs_debug_dsd_stage(m._h, dr.STAGE_DECONV2, ctypes.byref(a))]
        k1 = last(m._h)[0]
        a.n, a.rows, a.mask_mode, a.scale, a.fold, a.ov, a.n_clips = n, c["rows"], c["mode"], SCALE, 1, c["ov"], 1
        a.mix, a.mix_bytes, a.mix_ld = view("mix").data_ptr(), sizes["mix"], 68
        a.out, a.out_bytes, a.out_ld, a.out_src_stride = view("out").data_ptr(), sizes["out"], 68, c["rows"] * 68
        rc.append(lib.dcs_debug_dsd_stage(m._h, dr.STAGE_FINAL, ctypes.byref(a)))
        own = np.zeros((4, c["rows"], 68, 4), dtype=bool)
        own[:, :, :F] = True
        return finish(dict(rc=rc, out={}, kernels=[k1, last(m._h)[0]]), raw, place, poison, dict(D=None, mix=None, G=np.ones(sizes["G"], dtype=bool), out=own.reshape(-1)))

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:
            return -1, str(exc)

    for case in dr.cases(n_cu):
        if case["switch"] != switch:
            continue
        exp = dr.expected(case, n_cu)
        run = run_deconv2 if case["stage"] == dr.STAGE_DECONV2 else run_final
        kinds = ("rand", "int") if case["stage"] == dr.STAGE_DECONV2 else case["kinds"]
        t0 = time.time()
        rep = dict(rc=[], untouched=True, damage=0, same=True, kernels_same=True)
        for kind in kinds:
            r1 = run(case, kind, 0xFF, False, exp)
            r2 = run(case, kind, 0x4B, True, exp)
            rep["rc"] += r1["rc"] + r2["rc"]
            rep["kernels"], rep["params"] = r1["kernels"], r1["params"]
            rep["kernels_same"] = rep["kernels_same"] and r1["kernels"] == r2["kernels"] and r1["params"] == r2["params"]
            rep["untouched"] = rep["untouched"] and r1["untouched"] and r2["untouched"]
            rep["damage"] += r1["damage"] + r2["damage"]
            for name, b in r1["out"].items():                           # what the stage owns; the rest differs by the poison
                rep["same"] = rep["same"] and bool(np.array_equal(b[r1["own"][name]], r2["out"][name][r1["own"][name]]))
                arrays["%s/%s/%s" % (case["name"], kind, name)] = b
        rep["scratch_blocks"], rep["scratch_guard"] = guards()
        rep["seconds"] = time.time() - t0
        report[case["name"]] = rep
    if switch == "none":
        r1, r2 = chain(0xFF), chain(0x4B)
        report["_chain"] = dict(rc=r1["rc"] + r2["rc"], untouched=r1["untouched"] and r2["untouched"], damage=r1["damage"] + r2["damage"],
                                kernels=r1["kernels"], kernels_same=r1["kernels"] == r2["kernels"],
                                same=bool(np.array_equal(r1["out"]["G"], r2["out"]["G"]) and
                                          np.array_equal(r1["out"]["out"][r1["own"]["out"]], r2["out"]["out"][r1["own"]["out"]])))
        arrays["_chain/G"], arrays["_chain/out"], arrays["_chain/out2"] = r1["out"]["G"], r1["out"]["out"], r2["out"]["out"]
        report["_args"] = _arguments(torch, ctx, lib, net)
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _arguments(torch, ctx, lib, net):
    """every refusal of the entries: the status, and nothing written"""
    tc, F, n, rows = 30, 65, 4, 45
    m = net(1, tc, F, "rand")
    d = dr.dims(tc)
    sizes = dict(D=n * 3 * d["h2"] * dr.CP * 4, G=n * 3 * dr.NGG * tc * 32, Gs=n * 3 * dr.NGG * tc * 48, mix=((rows - 1) * 68 + F) * 4,
                 out=4 * rows * 68 * 4)                                 # the last mixture row ends with its last bin
    bufs = {k: torch.full((v + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    for k in ("D", "mix"):
        bufs[k].zero_()
    res = {}

    def run(label, want, stage, m_=m, zero_g=False, **kw):
        for k in ("G", "Gs", "out"):
            bufs[k].fill_(0xFF)
        if zero_g:
            bufs["G"].zero_()
        a = DsdArgs()
        a.n_items, a.n, a.rows, a.ov, a.fold, a.mask_mode, a.scale, a.n_clips = n * 3, n, rows, 25, 1, 0, 0.3, 1
        a.mix_ld, a.out_ld, a.out_src_stride = 68, 68, rows * 68
        for name in sizes:
            setattr(a, name, bufs[name].data_ptr())
            setattr(a, name + "_bytes", sizes[name])
        for k, v in kw.items():
            setattr(a, k, (bufs[v[0]].data_ptr() + v[1]) if isinstance(v, tuple) else v)
        rc = lib.dcs_debug_dsd_stage(m_._h if m_ is not None else None, stage, ctypes.byref(a))
        ctx.synchronize()
        untouched = all(bool((bufs[k] == 0xFF).all().item()) for k in ("G", "Gs", "out") if not (zero_g and k == "G"))
        res[label] = dict(rc=rc, want=want, untouched=untouched, message=lib.dcs_last_error().decode("utf-8", "replace"))

    run("deconv2 good", 0, 0)
    run("final good", 0, 1, zero_g=True)
    for stage, names in ((0, ("D", "G", "Gs")), (1, ("G", "mix", "out"))):
        for name in names:
            run("stage %d: %s one byte short" % (stage, name), dr.EINVAL, stage, zero_g=stage == 1, **{name + "_bytes": sizes[name] - 1})
            run("stage %d: %s misaligned" % (stage, name), dr.EINVAL, stage, zero_g=stage == 1, **{name: (name, 4)})
            if name != "Gs":
                run("stage %d: null %s" % (stage, name), dr.EINVAL, stage, zero_g=stage == 1, **{name: None})
    run("stage 2", dr.EINVAL, 2)
    run("family 2", dr.EINVAL, 0, family=2)
    run("no items", dr.EINVAL, 0, n_items=0)
    run("no tiles", dr.EINVAL, 1, zero_g=True, n=0)
    run("no rows", dr.EINVAL, 1, zero_g=True, rows=0)
    run("mask mode 4", dr.EINVAL, 1, zero_g=True, mask_mode=4)
    run("overlap 0", dr.EINVAL, 1, zero_g=True, ov=0)
    run("overlap tc", dr.EINVAL, 1, zero_g=True, ov=tc)
    run("unfolded rows that are not the tiles'", dr.EINVAL, 1, zero_g=True, fold=0)
    run("mixture pitch below the bins", dr.EINVAL, 1, zero_g=True, mix_ld=64)
    run("output pitch below the bins", dr.EINVAL, 1, zero_g=True, out_ld=64)
    run("sources that overlap", dr.EINVAL, 1, zero_g=True, out_src_stride=rows * 68 - 4)
    run("one tile more than G holds", dr.EINVAL, 1, zero_g=True, n=n + 1)
    run("two clips in buffers of one", dr.EINVAL, 1, zero_g=True, n_clips=2, g_clip_tiles=n, mix_clip_stride=rows * 68, out_clip_stride=4 * rows * 68)
    tab = (i64 * 6)(1, rows, n + 1, -1, 0, rows)
    run("a clip table with more tiles than n", dr.EINVAL, 1, zero_g=True, clip_tab_h=ctypes.cast(tab, vp))
    tab2 = (i64 * 6)(1, rows, n, 1, 0, rows)
    run("a clip table whose rows end past the mixture", dr.EINVAL, 1, zero_g=True, clip_tab_h=ctypes.cast(tab2, vp))
    run("null model", dr.EINVAL, 0, m_=None)
    res["null arguments"] = dict(rc=lib.dcs_debug_dsd_stage(m._h, 0, None), want=dr.EINVAL, untouched=True, message="")
    res["last_kernel without a model"] = dict(rc=lib.dcs_debug_dsd_last_kernel(None, None, None), want=dr.EINVAL, untouched=True, message="")
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_dsd_kernels as t; t.child(sys.argv[2], sys.argv[3])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """switch set -> (arrays, report): one child after another, each under its own time limit; a child that ends in a signal
    or at its limit ends the run (nothing more is started on the device)"""
    d = tmp_path_factory.mktemp("dsd_kernels")
    res = {}
    for name, env_add in dr.SWITCHES.items():
        out = str(d / (name + ".npz"))
        env = dict(os.environ)
        env.update(env_add)
        env.update(DCS_WS_GUARD=str(GB))
        t0 = time.time()
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, "-c", _CHILD, ROOT, name, out], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        print("switch set %s: child took %.1f s (limit %d), status %d" % (name, time.time() - t0, CHILD_LIMIT, p.returncode), flush=True)
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            pytest.exit("switch set %s: the child ended with status %d; no further child is started\n%s" % (name, p.returncode, p.stderr[-2000:]), 1)
        assert p.returncode == 0, (name, p.returncode, p.stdout[-400:], p.stderr[-2000:])
        z = np.load(out)
        res[name] = (z, json.loads(bytes(z["_report"]).decode()))
    return res


_CASES, WORST = {}, {}


def _cases_for(n_cu):
    if n_cu not in _CASES:
        _CASES[n_cu] = dr.cases(n_cu)
    return _CASES[n_cu]


def _note(code, what, value):
    key = (dr.code_name(code), what)
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _check_deconv2(tag, c, kind, code, G_dev, want, S, rest, sub):
    cls = dr.kernel_class(code)
    K = dr.NF * dr.dims(c["tc"])["kh"]
    got = np.asarray(G_dev, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: values that are not finite" % tag
    if kind == "int":
        bad = int((got != want).sum())
        assert bad == 0, "%s: integer probe: %d of %d elements differ from the float64 result" % (tag, bad, got.size)
        return
    e, e32 = cr.measure(got, want, S), cr.measure(rest, want[sub], S[sub])          # the device on every item, the yardstick on `sub`
    ratio = float(np.max(np.abs(got - want) / ((K + cr.cap_c(K, cls)) * dr.U * S + 1e-300)))
    print("\n%s: E %.3g, restatement %.3g, ratio %.2f, worst |err| / cap %.3g" % (tag, e, e32, e / e32, ratio))
    _note(code, "E / E(restatement)", e / e32)
    _note(code, "err / cap", ratio)
    assert e <= dr.FACTOR * e32, "%s: device %.3g, restatement %.3g" % (tag, e, e32)
    assert ratio <= 1.0, "%s: outside the cap by a factor of %.3g" % (tag, ratio)


_D2REF = {}


def _deconv2_ref(tc, n, kind, cls):
    key = (tc, n, kind)
    if key not in _D2REF:
        _, W2, _ = dr.weights(1, tc, 65, kind)
        D = dr.dense(tc, n, kind)
        _D2REF[key] = (D, W2, dr.deconv2(D, W2, tc), dr.deconv2(D, W2, tc, mul="abs"), np.unique(np.linspace(0, n - 1, min(n, 64)).astype(int)), {})
    D, W2, want, S, sub, rest = _D2REF[key]
    if cls not in rest:
        rest[cls] = dr.deconv2(D[sub], W2, tc, mul=dr.MUL[cls]).astype(np.float64)
    return want, S, sub, rest[cls]


def _common(r, exp, stage):
    assert all(rc == exp["rc"] for rc in r["rc"]), (r["rc"], exp["rc"])
    assert r["untouched"], "bytes outside what the stage writes are no longer poison"
    assert r["damage"] == 0 and r["scratch_guard"] == "" and r["scratch_blocks"] >= 0, r
    if exp["rc"] != 0:
        assert r["kernels"] == {}, "a refused call launched %r" % r["kernels"]
        return False
    assert r["kernels"] == exp["kernels"], "ran %r, the launchers' arithmetic says %r" % (
        {k: dr.code_name(v) for k, v in r["kernels"].items()}, {k: dr.code_name(v) for k, v in exp["kernels"].items()})
    half = slice(0, 4) if stage == dr.STAGE_DECONV2 else slice(4, 8)
    assert r["params"][half] == exp["params"][half], (r["params"], exp["params"])
    assert r["kernels_same"] and r["same"], "the poisons 0xFF and 0x4B, or a second launch over the first, gave other bits"
    assert r["seconds"] < 20, "the case took %.1f s in the child" % r["seconds"]
    return True


@pytest.mark.parametrize("case", [c for c in dr.cases() if c["stage"] == dr.STAGE_DECONV2], ids=lambda c: c["name"])
def test_deconv2_stage(runs, case):
    z, report = runs[case["switch"]]
    n_cu = report["_n_cu"]
    c = next(x for x in _cases_for(n_cu) if x["name"] == case["name"])          # the item counts follow the CU count
    r, exp = report[c["name"]], dr.expected(c, n_cu)
    if not _common(r, exp, dr.STAGE_DECONV2):
        return
    code, n, tc = exp["kernels"]["deconv2"], c["n"], c["tc"]
    for kind in ("rand", "int"):
        want, S, sub, rest = _deconv2_ref(tc, n, kind, dr.kernel_class(code))
        tag = "%s %s" % (c["name"], kind)
        key = "%s/%s/" % (c["name"], kind)
        g32 = None
        if key + "G" in z:
            g32, pad = dr.g_from_layout(z[key + "G"].view(np.float32), n, tc)
            assert not pad.any(), "%s: the pad channels 50 .. 55 of G are not zero" % tag
            _check_deconv2(tag + " G", c, kind, code, g32, want, S, rest, sub)
        if key + "Gs" in z:
            v, planes = dr.planes_value(z[key + "Gs"], n, tc)
            gv, pad = dr.g_from_layout(v, n, tc)
            assert np.isfinite(v).all() and not pad.any(), "%s: the pad channels 50 .. 55 of the planes are not zero" % tag
            # each plane is the truncation split of the value the planes sum to, bit for bit; where the f32 G exists too, of it
            src = np.ascontiguousarray(g32 if g32 is not None else gv)
            assert np.array_equal(dr.planes_layout(src), z[key + "Gs"].view(np.uint16).reshape(n, dr.NGG, tc, 3, dr.GCH)), \
                "%s: the planes are not the truncation split%s" % (tag, " of G" if g32 is not None else "")
            if g32 is None:
                _check_deconv2(tag + " Gs", c, kind, code, gv, want, S, rest, sub)
            elif "gsplit" in exp["kernels"]:
                _note(dr.K_GSPLIT, "err / cap", 0.0)
                _note(dr.K_GSPLIT, "E / E(restatement)", 0.0)


_FREF = {}


def _final_ref(c, kind, k, cls):
    """clip k of the case: float64 result, bound / cap, its scale and the restatement, shared among the switch sets"""
    key = (c["F"], c["C"], c["tc"], c["ov"], c["n"], c["rows"], c["mode"], c["n_clips"], c["table"], kind, k, cls)
    if key not in _FREF:
        G, mix = final_inputs(c, kind)
        fr, nt, r0, t0 = dr.clip_layout(c)[0][k]
        G, mix = G[t0:t0 + nt], mix[r0:r0 + fr]
        W1, _, b = dr.weights(c["C"], c["tc"], c["F"], kind)
        scale = INT_SCALE if kind == "int" else SCALE
        rows = fr if c["ov"] is not None else nt * c["tc"]
        want = dr.final(G, W1, b, c["F"], mix, scale, c["mode"], c["ov"], rows)
        rest = dr.final_f32(G, W1, b, c["F"], mix, scale, c["mode"], c["ov"], rows, cls)
        if c["mode"] == 2:
            St = dr.raw_tiles(G, W1, b, c["F"], mul="abs")
            Sout = (dr.fold(St.transpose(0, 2, 1, 3), c["ov"], rows).transpose(1, 0, 2) if c["ov"] is not None
                    else St.transpose(1, 0, 2, 3).reshape(4, rows, -1))
            bound = dr.raw_cap(Sout, cls, dr.mmax_of(c["tc"], c["ov"]) if c["ov"] is not None else 0)
        else:
            bound, Sout = dr.mask_bound(G, W1, b, c["F"], mix, scale, c["mode"], c["ov"], rows, cls, exact_raw=kind == "int")
        pow2 = dr.pow2_elements(G, W1, b, c["F"], c["mode"], c["ov"], rows) if kind == "int" and c["mode"] != 2 else None
        _FREF[key] = (want, rest, bound, Sout, float(mix.max()) * scale, pow2)
    return _FREF[key]


EXACT = {}


def _check_final(tag, c, kind, code, got, want, rest, bound, Sout, top, pow2=None):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: %d values are not finite" % (tag, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    exact_weights = c["ov"] is None or c["ov"] in (1, 2)
    if kind == "int" and c["mode"] == 2:
        if exact_weights:
            assert not err.any(), "%s: integer probe: %d elements differ from the float64 result" % (tag, int((err != 0).sum()))
        return
    if kind == "int":
        # the raw outputs are exact integers: what is left is the epilogue, whose reciprocal is documented to 1 ulp -- that is
        # what is asserted (the bound with eps = 0); whether a power-of-two denominator comes back exact is measured
        assert np.isfinite(bound).all() and np.all(err <= bound), "%s: integer probe outside the epilogue's roundings by a factor of %.3g" % (
            tag, float(np.max(err / (bound + 1e-300))))
        sel = np.broadcast_to(pow2[None], got.shape) & (want != 0)
        same = got[sel].astype(np.float32) == want[sel].astype(np.float32)
        k = dr.code_name(code)
        EXACT[k] = (EXACT.get(k, (0, 0))[0] + int(same.sum()), EXACT.get(k, (0, 0))[1] + int(sel.sum()))
        print("\n%s: %d of %d outputs with a power-of-two denominator and one covering tile equal the rounded float64 result" % (tag, int(same.sum()), int(sel.sum())))
        return
    fin = np.isfinite(bound)
    vac = float(np.mean(~(bound <= 1e-4 * top))) if c["mode"] != 2 else 0.0
    assert vac <= 0.01, "%s: %.2f %% of the bound is vacuous" % (tag, 100 * vac)
    ratio = float(np.max(err[fin] / (bound[fin] + 1e-300)))
    live = fin & (Sout > 0)
    assert not err[fin & ~live].any() or c["mode"] == 3, "%s: outputs that nothing but zeros went into are not the reference's" % tag
    e, e32 = float(np.max(err[live] / Sout[live])), float(np.max(np.abs(rest - want)[live] / Sout[live]))
    print("\n%s: E %.3g, restatement %.3g, ratio %.2f, worst |err| / bound %.3g, vacuous %.3f %%" % (tag, e, e32, e / max(e32, 1e-300), ratio, 100 * vac))
    _note(code, "E / E(restatement)", e / max(e32, 1e-300))
    _note(code, "err / bound", ratio)
    assert ratio <= 1.0, "%s: outside the bound by a factor of %.3g" % (tag, ratio)
    assert e <= dr.FACTOR * e32, "%s: device %.3g, restatement %.3g" % (tag, e, e32)


@pytest.mark.parametrize("case", [c for c in dr.cases() if c["stage"] == dr.STAGE_FINAL], ids=lambda c: c["name"])
def test_final_stage(runs, case):
    z, report = runs[case["switch"]]
    n_cu = report["_n_cu"]
    c = next(x for x in _cases_for(n_cu) if x["name"] == case["name"])
    r, exp = report[c["name"]], dr.expected(c, n_cu)
    if not _common(r, exp, dr.STAGE_FINAL):
        return
    code = exp["kernels"]["final"]
    Fe, pitch = final_geometry(c)
    clips = dr.clip_layout(c)[0]
    for kind in c["kinds"]:
        out = z["%s/%s/out" % (c["name"], kind)].view(np.float32).reshape(c["n_clips"], 4, c["rows"], pitch)
        for k, (fr, nt, r0, t0) in enumerate(clips):
            rows = fr if c["ov"] is not None else nt * c["tc"]
            want, rest, bound, Sout, top, pow2 = _final_ref(c, kind, k, dr.kernel_class(code))
            _check_final("%s %s clip %d" % (c["name"], kind, k), c, kind, code, out[k, :, :rows, :Fe], want, rest, bound, Sout, top, pow2)


def test_chained_stages(runs):
    """deconv2 and then the final stage on the device's own G, under both poisons: the same bits, and within the bound of the
    float64 final stage of that very G"""
    z, report = runs["none"]
    r, c = report["_chain"], dr.CHAIN
    assert r["rc"] == [0, 0, 0, 0] and r["untouched"] and r["damage"] == 0 and r["same"] and r["kernels_same"], r
    n_cu = report["_n_cu"]
    want_k = [dr.expected(dr._d("x", c["n"] * 3), n_cu)["kernels"], dr.expected(dr._f("x", c["F"], c["ov"], c["n"], c["rows"], c["mode"]), n_cu)["kernels"]]
    assert r["kernels"] == want_k, (r["kernels"], want_k)
    o1, o2 = z["_chain/out"].view(np.float32).reshape(4, c["rows"], 68)[:, :, :c["F"]], z["_chain/out2"].view(np.float32).reshape(4, c["rows"], 68)[:, :, :c["F"]]
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    G, pad = dr.g_from_layout(z["_chain/G"].view(np.float32), c["n"] * 3, c["tc"])
    assert not pad.any()
    G = G.reshape(c["n"], 3, dr.NF, c["tc"])
    W1, _, b = dr.weights(1, c["tc"], c["F"], "rand")
    mix = dr.mixture(c["rows"], c["F"], 1, "rand")
    want = dr.final(G, W1, b, c["F"], mix, SCALE, c["mode"], c["ov"], c["rows"])
    bound, Sout = dr.mask_bound(G, W1, b, c["F"], mix, SCALE, c["mode"], c["ov"], c["rows"], "f32")
    fin = np.isfinite(bound)
    err = np.abs(o1.astype(np.float64) - want)
    assert fin.mean() > 0.99 and np.all(err[fin] <= bound[fin])
    rest = dr.final_f32(G, W1, b, c["F"], mix, SCALE, c["mode"], c["ov"], c["rows"], "f32")
    live = fin & (Sout > 0)
    e, e32 = float(np.max(err[live] / Sout[live])), float(np.max(np.abs(rest - want)[live] / Sout[live]))
    print("\nchain: E %.3g, restatement %.3g" % (e, e32))
    assert e <= dr.FACTOR * e32


def test_every_kernel_code_is_reached(runs):
    seen = set()
    for name in runs:
        for key, r in runs[name][1].items():
            if not key.startswith("_"):
                seen |= set(r["kernels"].values())
    assert seen >= dr.ALL_CODES, "never launched: %r" % sorted(dr.code_name(k) for k in dr.ALL_CODES - seen)
    print("\nworst per kernel:")
    for (name, what), v in sorted(WORST.items()):
        print("  %-40s %-22s %.3g" % (name, what, v))
    print("integer probe, mask modes, power-of-two denominators (exact, of): %r" % sorted(EXACT.items()))
    print("child seconds per case, the slowest: %r" % sorted(((round(r["seconds"], 1), k) for n in runs for k, r in runs[n][1].items()
                                                              if not k.startswith("_")), reverse=True)[:5])


def test_entries_refuse_bad_arguments(runs):
    args = runs["none"][1]["_args"]
    assert len(args) > 30
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        if r["want"] != 0:
            assert r["untouched"], label
