"""The training GEMM ``train::gemm_kernel`` in all twelve instances (three tiles by four operand load orders) and its helper
kernels (``finish_kernel``, ``reduce_kernel``, every production instance of the conv1^T kernels) on the MI355X, one launch at a
time, against float64.

The launches are reached through ``dcs_debug_train_gemm`` / ``dcs_debug_train_aux`` (the Gemm built with the helpers the graph
files use, every address checked on the host first, the launch issued by ``dcs_trainer::launch`` / ``finish`` / ``reduce`` and
by the graph files' own conv1^T launch functions).  One child process under its own ``timeout -k 10`` (``CHILD_LIMIT``; a child
that ends in a signal or at its limit ends the run), with ``DCS_WS_GUARD``.  Every launch runs on buffers carved out of one
poisoned allocation, 64 KiB between and around them; every data set of a case runs under the poisons 0xFF and 0x4B and a second
time over its own output.  The child writes what the launches wrote, the parent compares by the rules of
tests/train_gemm_ref.py.

Measured on the MI355X: the child 3.1 s, of which 0.6 s are the 136 GEMM cases; the module 3.9 s.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import train_gemm_ref as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GB = 1 << 16
CHILD_LIMIT = 40                       # seconds; the child took 3.1 s on the MI355X, library load included
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class Mat(ctypes.Structure):
    """dcs_debug_train_mat of include/dcs.h"""
    _fields_ = [("p", vp), ("bytes", i64), ("off", i64), ("r", i64 * 5), ("c", i64 * 5)]


class GemmArgs(ctypes.Structure):
    """dcs_debug_train_gemm_args of include/dcs.h"""
    _fields_ = [("M", i32), ("N", i32), ("K", i32), ("tile", i32), ("ak", i32), ("bk", i32), ("A", Mat), ("B", Mat), ("C", Mat), ("X", Mat),
                ("ones_row", i32), ("ones_klim", i32), ("nbatch", i32), ("bias_cs", i32), ("boff", (i64 * 5) * 4), ("bias", vp), ("bias_bytes", i64),
                ("bias2", vp), ("bias2_bytes", i64), ("scale", vp), ("scale_bytes", i64), ("epi", i32), ("splits", i32), ("kchunk", i32),
                ("grid_x", i32), ("grid_y", i32), ("grid_z", i32), ("partial", vp), ("partial_bytes", i64)]


class AuxArgs(ctypes.Structure):
    """dcs_debug_train_aux_args of include/dcs.h"""
    _fields_ = [("B", i32), ("N", i32), ("splits", i32), ("epi", i32), ("count", i64 * 2), ("rsplits", i32 * 2), ("rN", i32 * 2), ("dup", i32 * 2),
                ("tc", i32), ("F", i32), ("w1", i32), ("pad_", i32), ("gslot", i64), ("in_", vp), ("in_bytes", i64), ("in2", vp), ("in2_bytes", i64),
                ("in3", vp), ("in3_bytes", i64), ("out", vp), ("out_bytes", i64), ("out2", vp), ("out2_bytes", i64)]


def buffers(c):
    """name -> floats of every buffer of the launch (inputs and outputs)"""
    names = [n for n in tg.OPERANDS if tg.used(c, n)]
    if c["partial"]:
        names.append("partial")
    else:
        names += [n for n in ("bias", "bias2") if c[n]]
    if c["scale"] is not None:
        names.append("scale")
    return {n: tg.floats(c, n) for n in names}


def outputs(c):
    """name -> boolean float mask of what the launch owns"""
    own = {}
    if c["partial"]:
        m = np.zeros(tg.floats(c, "partial"), dtype=bool)
        m[:m.size - tg.PARTIAL_TAIL] = True
        return {"partial": m}
    for name in ("C", "X"):
        if name == "C" or c["epi"] & tg.EPI_SAVEPRE:
            m = np.zeros(tg.floats(c, name), dtype=bool)
            for b in range(c["nbatch"]):
                m[tg.index(c, name, b).reshape(-1)] = True
            own[name] = m
    return own


def fill_args(c, place, base):
    """GemmArgs of case c on the buffers `place` {name: (byte offset, bytes)} of an allocation at `base`"""
    a = GemmArgs()
    for k in ("M", "N", "K", "tile", "ak", "bk", "ones_row", "ones_klim", "nbatch", "bias_cs", "epi", "splits", "kchunk"):
        setattr(a, k, c[k])
    for name in tg.OPERANDS:
        m = getattr(a, name)
        m.off = c[name]["off"]
        m.r, m.c = (i64 * 5)(*c[name]["r"]), (i64 * 5)(*c[name]["c"])
        if name in place:
            m.p, m.bytes = base + place[name][0], place[name][1]
    for b in range(4):
        for k in range(5):
            a.boff[b][k] = c["boff"][b][k]
    for name in ("bias", "bias2", "scale", "partial"):
        if name in place:
            setattr(a, name, base + place[name][0])
            setattr(a, name + "_bytes", place[name][1])
    return a


# ------------------------------------------------------------------------------------------------ the child process
def child(out_path):
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

    def finish(raw, place, poison, owns):
        """owns {buffer: boolean byte mask of what the launch owns}; returns (host copies of the outputs, whether every other
        byte of them is still poison, bytes changed outside every buffer)"""
        ctx.synchronize()
        host, untouched = {}, True
        for name, own in owns.items():
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

    def run_gemm(c, inp, poison, twice):
        sizes = {k: 4 * v for k, v in buffers(c).items()}
        raw, place = arena(sizes, poison)
        for k, v in inp.items():
            put(raw, place, k, v)
        a = fill_args(c, place, raw.data_ptr())
        rc = [lib.dcs_debug_train_gemm(ctx._h, ctypes.byref(a)) for _ in range(2 if twice else 1)]
        owns = {k: np.repeat(v, 4) for k, v in outputs(c).items()}
        host, untouched, damage = finish(raw, place, poison, owns)
        return dict(rc=rc, out=host, owns=owns, untouched=untouched, damage=damage, grid=[a.grid_x, a.grid_y, a.grid_z])

    t_all = time.time()
    for c in tg.cases():
        t0 = time.time()
        rep = dict(rc=[], untouched=True, damage=0, same=True, grid=None)
        for kind in tg.kinds_of(c):
            inp = tg.inputs(c, kind)
            r1, r2 = run_gemm(c, inp, 0xFF, False), run_gemm(c, inp, 0x4B, True)
            rep["rc"] += r1["rc"] + r2["rc"]
            rep["grid"] = r1["grid"]
            rep["same"] = rep["same"] and r1["grid"] == r2["grid"]
            rep["untouched"] = rep["untouched"] and r1["untouched"] and r2["untouched"]
            rep["damage"] += r1["damage"] + r2["damage"]
            for name, b in r1["out"].items():
                own = r1["owns"][name]
                rep["same"] = rep["same"] and bool(np.array_equal(b[own], r2["out"][name][own]))
                arrays["%s/%s/%s" % (c["name"], kind, name)] = b
        rep["seconds"] = time.time() - t0
        report[c["name"]] = rep
    report["_gemm_seconds"] = time.time() - t_all
    report["_guards_gemm"] = guards()
    _aux(torch, ctx, lib, arena, put, finish, arrays, report)
    report["_guards"] = guards()
    report["_args"] = _arguments(torch, ctx, lib)
    report["_seconds"] = time.time() - t_all
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _aux(torch, ctx, lib, arena, put, finish, arrays, report):
    def call(which, sizes, fill, owns, **fields):
        """both poisons, the second one twice; sizes in floats; fill {buffer: host array}; owns {buffer: float mask or None (all)}"""
        runs = []
        for poison, times in ((0xFF, 1), (0x4B, 2)):
            raw, place = arena({k: 4 * v for k, v in sizes.items()}, poison)
            for k, v in fill.items():
                put(raw, place, k, v)
            a = AuxArgs()
            for k, v in fields.items():
                if isinstance(v, (list, tuple)):
                    for i, x in enumerate(v):
                        getattr(a, k)[i] = x
                else:
                    setattr(a, k, v)
            for name, (off, nbytes) in place.items():
                setattr(a, name, raw.data_ptr() + off)
                setattr(a, name.rstrip("_") + "_bytes", nbytes)
            rcs = [lib.dcs_debug_train_aux(ctx._h, which, ctypes.byref(a)) for _ in range(times)]
            masks = {k: np.repeat(np.ones(sizes[k], dtype=bool) if v is None else v, 4) for k, v in owns.items()}
            host, untouched, damage = finish(raw, place, poison, masks)
            runs.append(dict(rc=rcs, host=host, untouched=untouched, damage=damage, masks=masks))
        r1, r2 = runs
        same = all(np.array_equal(r1["host"][k][r1["masks"][k]], r2["host"][k][r1["masks"][k]]) for k in owns)
        return r1["host"], dict(rc=r1["rc"] + r2["rc"], untouched=r1["untouched"] and r2["untouched"], damage=r1["damage"] + r2["damage"],
                                same=bool(same))

    for B, N, splits, epi, bias in tg.FINISH_ROWS:
        part, b, X = tg.finish_inputs(B, N, splits, epi, bias)
        key = "finish/%d/%d/%d/%d/%d" % (B, N, splits, epi, bias)
        sizes, fill, owns = dict(in_=part.size, out=B * N, out2=B * N), dict(in_=part), dict(out=None)
        if bias:
            sizes["in2"], fill["in2"] = N, b
        if epi & tg.EPI_DRELU:
            fill["out2"] = X
        else:
            owns["out2"] = None
        host, report[key] = call(tg.AUX_FINISH, sizes, fill, owns, B=B, N=N, splits=splits, epi=epi)
        for k, v in host.items():
            arrays[key + "/" + k] = v
    for ri, row in enumerate(tg.REDUCE_ROWS):
        for scale in (1.0, -1.0, 0.0):
            parts = tg.reduce_inputs(row, scale)
            key = "reduce/%d/%g" % (ri, scale)
            sizes, fill, owns = dict(in3=1), dict(in3=np.array([scale], dtype=np.float32)), {}
            for j, (name_in, name_out) in enumerate((("in_", "out"), ("in2", "out2"))):
                n, s, N, dup = row[j]
                if n == 0:
                    continue
                sizes[name_in], fill[name_in] = parts[j].size, parts[j]
                sizes[name_out] = n + N * dup + tg.REDUCE_TAIL
                m = np.zeros(sizes[name_out], dtype=bool)
                m[:n + N * dup] = True
                owns[name_out] = m
            host, report[key] = call(tg.AUX_REDUCE, sizes, fill, owns, count=[r[0] for r in row], rsplits=[r[1] for r in row],
                                     rN=[r[2] for r in row], dup=[r[3] for r in row])
            for k, v in host.items():
                arrays[key + "/" + k] = v
    for which in tg.DECONV1:
        for row in tg.DECONV1_ROWS:
            B, tc, F, pad = row
            d = tg.deconv1_geom(which, *row)
            g, W, bo = tg.deconv1_inputs(which, *row)
            key = "deconv1/%d/%d/%d/%d" % (which, B, tc, F)
            host, report[key] = call(which, dict(in_=g.size, in2=W.size, in3=bo.size, out=B * d["ns"] * tc * F), dict(in_=g, in2=W, in3=bo),
                                     dict(out=None), B=B, tc=tc, F=F, w1=d["w1"], gslot=d["gslot"])
            arrays[key + "/out"] = host["out"]


def _arguments(torch, ctx, lib):
    """one row per class of refusal: the status, and the outputs' poison intact"""
    res = {}
    by_name = {c["name"]: c for c in tg.cases()}
    for cname in tg.REFUSAL_CASES:
        c = by_name[cname]
        inp = tg.inputs(c, "signed")
        sizes = {k: 4 * v for k, v in buffers(c).items()}
        bufs = {k: torch.full((v + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
        outs = list(outputs(c))

        def run(label, want, mods):
            for k in outs:
                bufs[k].fill_(0xFF)
            for k, v in inp.items():
                if k not in outs:
                    bufs[k][:v.nbytes].copy_(torch.from_numpy(v.view(np.uint8).reshape(-1)))
            a = fill_args(c, {}, 0)
            for k in sizes:
                if k in tg.OPERANDS:
                    getattr(a, k).p, getattr(a, k).bytes = bufs[k].data_ptr(), sizes[k]
                else:
                    setattr(a, k, bufs[k].data_ptr())
                    setattr(a, k + "_bytes", sizes[k])
            for field, v in mods.items():
                obj, leaf = (getattr(a, field.split(".")[0]), field.split(".")[1]) if "." in field else (a, field)
                name = field.split(".")[0]
                if v == "null":
                    setattr(obj, leaf, None)
                elif v == "misaligned":
                    setattr(obj, leaf, bufs[name].data_ptr() + 4)
                elif isinstance(v, tuple):
                    setattr(obj, leaf, (i64 * 5)(*v))
                else:
                    setattr(obj, leaf, v)
            rc = lib.dcs_debug_train_gemm(ctx._h, ctypes.byref(a))
            ctx.synchronize()
            untouched = want == 0 or all(bool((bufs[k] == 0xFF).all().item()) for k in outs)
            res["%s: %s" % (cname, label)] = dict(rc=rc, want=want, untouched=untouched, message=lib.dcs_last_error().decode("utf-8", "replace"))

        run("good", 0, {})
        for label, mods in tg.refusals(c):
            run(label, tg.EINVAL, mods)
    res["null arguments"] = dict(rc=lib.dcs_debug_train_gemm(ctx._h, None), want=tg.EINVAL, untouched=True, message="")
    res["null context"] = dict(rc=lib.dcs_debug_train_aux(None, 0, None), want=tg.EINVAL, untouched=True, message="")
    # the helpers: one of each class on finish, reduce and conv1^T, and an unknown kernel
    B, N, splits = 3, 50, 2
    n = {"in_": splits * B * N, "in2": 80, "in3": 4, "out": B * N + 64, "out2": B * N + 64}
    bufs = {k: torch.full((4 * v + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k, v in n.items()}

    def aux(label, want, which=tg.AUX_FINISH, **kw):
        for k in ("out", "out2"):
            bufs[k].fill_(0xFF)
        a = AuxArgs()
        a.B, a.N, a.splits, a.epi = B, N, splits, tg.EPI_RELU | tg.EPI_SAVEPRE
        for name in bufs:
            setattr(a, name, bufs[name].data_ptr())
            setattr(a, name.rstrip("_") + "_bytes", 4 * n[name])
        for k, v in kw.items():
            if isinstance(v, list):
                for i, x in enumerate(v):
                    getattr(a, k)[i] = x
            else:
                setattr(a, k, (bufs[v[0]].data_ptr() + v[1]) if isinstance(v, tuple) else v)
        rc = lib.dcs_debug_train_aux(ctx._h, which, ctypes.byref(a))
        ctx.synchronize()
        untouched = want == 0 or all(bool((bufs[k] == 0xFF).all().item()) for k in ("out", "out2"))
        res["aux: " + label] = dict(rc=rc, want=want, untouched=untouched, message=lib.dcs_last_error().decode("utf-8", "replace"))

    aux("finish good", 0)
    aux("finish part one byte short", tg.EINVAL, in_bytes=4 * splits * B * N - 1)
    aux("finish good, bias of exactly N floats", 0, in2_bytes=4 * N)
    aux("finish bias short", tg.EINVAL, in2_bytes=4 * N - 1)
    aux("finish C misaligned", tg.EINVAL, out=("out", 4))
    aux("finish null X", tg.EINVAL, out2=None)
    aux("finish X short", tg.EINVAL, out2_bytes=4 * B * N - 1)
    aux("finish no row", tg.EINVAL, B=0)
    aux("finish SAVEPRE with DRELU", tg.EINVAL, epi=tg.EPI_SAVEPRE | tg.EPI_DRELU)
    red = dict(which=tg.AUX_REDUCE, count=[100, 40], rsplits=[3, 2], rN=[10, 10], dup=[1, 0])
    aux("reduce good", 0, **red)
    aux("reduce dst one byte short", tg.EINVAL, **dict(red, out_bytes=4 * 110 - 1))
    aux("reduce part short", tg.EINVAL, **dict(red, in2_bytes=4 * 80 - 1))
    aux("reduce null scale", tg.EINVAL, **dict(red, in3=None))
    aux("reduce dup wider than the job", tg.EINVAL, **dict(red, rN=[101, 10]))
    aux("reduce dst misaligned", tg.EINVAL, **dict(red, out2=("out2", 8)))
    # conv1^T of 1 x 1 x 30: g 30 floats, W 900 (the channels kernel 3600), bo 2 or 4, q 60 or 120
    dcv = dict(B=1, tc=1, F=30, w1=1, gslot=0)
    aux("conv1^T W short", tg.EINVAL, which=tg.AUX_DECONV1_IKALA, **dcv)                     # in2 holds 80 floats
    aux("conv1^T w1 not the graph's", tg.EINVAL, which=tg.AUX_DECONV1_BACH10, **dict(dcv, w1=2))
    aux("conv1^T F below the filter", tg.EINVAL, which=tg.AUX_DECONV1_BACH10SI, **dict(dcv, F=29))
    aux("kernel 9", tg.EINVAL, which=9)
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_train_kernels as t; t.child(sys.argv[2])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(arrays, report) of the one child, under its own time limit; a child that ends in a signal or at its limit ends the run
    (nothing more is started on the device)"""
    out = str(tmp_path_factory.mktemp("train_kernels") / "run.npz")
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


WORST = {}
REACHED = set()


def _gather(c, buf, name):
    """[nbatch][M][N] of the C or X buffer"""
    return np.stack([buf[tg.index(c, name, b)] for b in range(c["nbatch"])])


@pytest.mark.parametrize("c", tg.cases(), ids=lambda c: c["name"])
def test_launch(run, c):
    z, report = run
    r = report[c["name"]]
    kinds = tg.kinds_of(c)
    assert r["rc"] == [0] * (3 * len(kinds)), r["rc"]
    assert r["grid"] == tg.grid(c), (r["grid"], tg.grid(c))
    assert r["untouched"], "bytes of C, X or partial the launch does not own are no longer poison"
    assert r["damage"] == 0, "%d bytes changed outside every buffer" % r["damage"]
    assert r["same"], "the poisons 0xFF and 0x4B, or a second launch over the first, gave other bits"
    assert r["seconds"] < 5, "the case took %.1f s in the child" % r["seconds"]
    REACHED.add((c["tile"], c["ak"], c["bk"]))
    for kind in kinds:
        tag = "%s %s" % (c["name"], kind)
        inp = tg.inputs(c, kind)
        want, S = tg.reference(c, inp), tg.reference(c, inp, "abs")
        if c["partial"]:
            got = {"partial": z["%s/%s/partial" % (c["name"], kind)].view(np.float32)[:c["nbatch"] * c["splits"] * c["M"] * c["N"]]
                   .reshape(want["partial"].shape)}
        else:
            got = {"C": _gather(c, z["%s/%s/C" % (c["name"], kind)].view(np.float32), "C")}
            if c["epi"] & tg.EPI_SAVEPRE:
                got["pre"] = _gather(c, z["%s/%s/X" % (c["name"], kind)].view(np.float32), "X")
                # X is the pre-activation bit for bit next to C
                cw = np.maximum(got["pre"], np.float32(0)) if c["epi"] & tg.EPI_RELU else got["pre"]
                assert np.array_equal(cw.view(np.uint32), got["C"].view(np.uint32)), "%s: C is not the rectified X (or X itself)" % tag
        key = "partial" if c["partial"] else "C"
        for k in got:
            assert np.isfinite(got[k]).all(), "%s: %s holds values that are not finite" % (tag, k)
        if c["scale"] == 0.0 and not c["partial"]:
            # zeros before the bias: the output is the bias chain exactly
            rest = tg.reference(c, inp, "f32")
            assert np.array_equal(got["C"], rest["C"]), "%s: scale 0 does not give the biases alone" % tag
            if not (c["bias"] or c["bias2"]):
                assert not got["C"].any()
            continue
        if kind != "signed":
            for k in got:
                bad = int((got[k].astype(np.float64) != want[k]).sum())
                assert bad == 0, "%s: %d of %d elements of %s differ from the float64 result" % (tag, bad, got[k].size, k)
            if kind == "ties":
                assert (got["pre"] == 0).any()
            continue
        rest = tg.reference(c, inp, "f32")
        spans = [k1 - k0 for k0, k1 in tg.slices(c)] * c["nbatch"] if c["partial"] else [c["K"]] * c["nbatch"]
        for k in got:
            Sk = S[key]
            cap = np.stack([(n + tg.roundings(c)) * tg.U * Sk[i] for i, n in enumerate(spans)])
            d = np.abs(got[k].astype(np.float64) - want[k])
            assert not got[k][Sk == 0].any(), "%s: an output nothing but zeros goes into is not 0" % tag
            e = float(np.max(d / np.where(Sk > 0, Sk, 1.0)))
            e32 = float(np.max(np.abs(rest[k].astype(np.float64) - want[k]) / np.where(Sk > 0, Sk, 1.0)))
            ratio = float(np.max(d / (cap + 1e-300)))
            print("\n%s %s: E %.3g, restatement %.3g, E / E(restatement) %.2f, worst |err| / cap %.3g" % (tag, k, e, e32, e / max(e32, 1e-300), ratio))
            inst = "%s %s%s" % (tg.TILE_NAMES[c["tile"]], "K" if c["ak"] else "M", "K" if c["bk"] else "N")
            if e32 > 0:
                WORST[inst] = max(WORST.get(inst, 0.0), e / e32)
            assert e <= tg.FACTOR * e32, "%s %s: device %.3g, restatement %.3g" % (tag, k, e, e32)
            assert np.all(d <= cap), "%s %s: outside (K + c) 2^-24 S by a factor of %.3g" % (tag, k, ratio)


def test_every_production_instance_is_reached(run):
    _, report = run
    reached = {(c["tile"], c["ak"], c["bk"]) for c in tg.cases() if report[c["name"]]["rc"] and all(rc == 0 for rc in report[c["name"]]["rc"])
               and report[c["name"]]["grid"] == tg.grid(c)}
    names = lambda s: sorted("%s %s%s" % (tg.TILE_NAMES[t], "K" if a else "M", "K" if b else "N") for t, a, b in s)
    assert not tg.PRODUCTION - reached, "never launched: %r" % names(tg.PRODUCTION - reached)
    assert not tg.AID_ONLY - reached, "aid only, never launched: %r" % names(tg.AID_ONLY - reached)
    print("\nproduction instances reached: %r\naid only: %r" % (names(tg.PRODUCTION), names(tg.AID_ONLY)))
    print("largest E / E(restatement) per instance: %r" % sorted((k, round(v, 3)) for k, v in WORST.items()))
    print("child: %.1f s for the GEMM cases, %.1f s in all; the slowest cases: %r" % (
        report["_gemm_seconds"], report["_seconds"],
        sorted(((round(report[c["name"]]["seconds"], 3), c["name"]) for c in tg.cases()), reverse=True)[:3]))
    for g in (report["_guards_gemm"], report["_guards"]):
        assert g[1] == "" and g[0] >= 0, g


def _aux_ok(report, key, calls=3):
    r = report[key]
    assert r["rc"] == [0] * calls, (key, r)
    assert r["untouched"] and r["damage"] == 0 and r["same"], (key, r)


@pytest.mark.parametrize("row", tg.FINISH_ROWS, ids=lambda r: "%dx%d-%d-epi%d-bias%d" % r)
def test_finish(run, row):
    z, report = run
    B, N, splits, epi, bias = row
    key = "finish/%d/%d/%d/%d/%d" % row
    _aux_ok(report, key)
    part, b, X = tg.finish_inputs(*row)
    C, pre = tg.finish_ref(part, b, X, epi)
    assert np.array_equal(z[key + "/out"].view(np.uint32), C.view(np.uint32).reshape(-1)), key
    if pre is not None:
        assert np.array_equal(z[key + "/out2"].view(np.uint32), pre.view(np.uint32).reshape(-1)), key


@pytest.mark.parametrize("ri", range(len(tg.REDUCE_ROWS)))
def test_reduce(run, ri):
    z, report = run
    row = tg.REDUCE_ROWS[ri]
    for scale in (1.0, -1.0, 0.0):
        key = "reduce/%d/%g" % (ri, scale)
        _aux_ok(report, key)
        parts = tg.reduce_inputs(row, scale)
        for j, name in enumerate(("out", "out2")):
            n, s, N, dup = row[j]
            if n == 0:
                assert key + "/" + name not in z.files
                continue
            want = tg.reduce_ref(parts[j], scale, N, dup)
            got = z[key + "/" + name].view(np.float32)[:want.size]
            assert np.array_equal(got, want), (key, name)                    # -0 == +0 under the scale 0
            if scale != 0.0:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, name)
            if dup:
                assert np.array_equal(got[n:], got[n - N:n])


@pytest.mark.parametrize("which", sorted(tg.DECONV1))
def test_deconv1(run, which):
    z, report = run
    for row in tg.DECONV1_ROWS:
        B, tc, F, pad = row
        key = "deconv1/%d/%d/%d/%d" % (which, B, tc, F)
        _aux_ok(report, key)
        g, W, bo = tg.deconv1_inputs(which, *row)
        q64, taps = tg.deconv1_ref(which, *row, g, W, bo)
        q32, _ = tg.deconv1_ref(which, *row, g, W, bo, "f32")
        S, _ = tg.deconv1_ref(which, *row, g, W, bo, "abs")
        got = z[key + "/out"].view(np.float32).reshape(q64.shape)
        dead = taps == 0
        assert np.array_equal(got[..., dead], np.broadcast_to(bo[None, :, None, None], got.shape)[..., dead]), "%s: a column without a tap is not bo" % key
        d = np.abs(got.astype(np.float64) - q64)
        e, e32 = float(np.max(d / S)), float(np.max(np.abs(q32 - q64) / S))
        print("\n%s: E %.3g, restatement %.3g" % (key, e, e32))
        assert e <= tg.FACTOR * e32, (key, e, e32)
        assert np.all(d <= ((taps * tg.C1 + 1) * tg.U)[None, None, None, :] * S), key


def test_entries_refuse_bad_arguments(run):
    args = run[1]["_args"]
    assert len(args) > 100
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        assert r["untouched"], label
