"""Every convolution, transposed-convolution and pool / un-pool kernel of the generic graphs on the MI355X, directly against
float64, one stage of the forward pass at a time.

The stages are reached through ``dcs_debug_conv_stage`` (the functions the graphs call, with every buffer checked first);
after every launch ``dcs_debug_conv_last_kernel`` says which kernel each role ran and with which launcher parameters, and
the test asserts that they are what ``conv_ref.expected`` derives from the launchers' arithmetic.  One child process per switch
set (``conv_ref.SWITCHES``: the library reads them once per process), one after another, each under its own ``timeout -k 10``
(``CHILD_LIMIT``; the parent stops at the first child that ends in a signal or at its limit), each with ``DCS_WS_GUARD`` and
each running its cases on buffers carved out of one poisoned allocation per launch: 64 KiB between and around the buffers,
everything a stage does not write born as poison.  A case runs on random data under the poisons 0xFF and 0x4B and a second
time over its own output, and on the integer probe; the children write what the stages wrote, the parent compares by the
rules of tests/conv_ref.py.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
G = 1 << 16
EINVAL, EUNSUPPORTED = -1, -2
CHILD_LIMIT = 300                      # seconds per child: see DESIGN 4p3 for the measured times
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
BUFS = ("tiles", "a1b", "p1", "a2b", "D", "g2", "g1", "o")


class ConvArgs(ctypes.Structure):
    """dcs_debug_conv_args of include/dcs.h"""
    _fields_ = ([("n", i64), ("n_branch", i32), ("tie_mode", i32)] + [f for b in BUFS for f in ((b, vp), (b + "_bytes", i64))] +
                [("frames_src", vp), ("frames_bytes", i64), ("frames_rows", i32), ("frames_stride", i32), ("a1_layout", i32),
                 ("a1_rows", i32), ("d_layout", i32), ("fold2", i32), ("a2_f16", i32)])


def buffer_bytes(d, n, nb):
    """what the forward pass carves for n tiles and nb branches (include/dcs.h)"""
    p1, pp = d["tc"] * d["w1"], d["tc"] * d["wp"]
    return dict(tiles=n * d["C"] * d["tc"] * d["F"] * 4, a1b=n * cr.NF * p1 * 4, p1=n * cr.NF * pp * 4, a2b=n * d["flat_p"] * 4,
                D=max(n * nb * d["flat_p"] * 4, n * nb * d["n_out16"] * 2), g2=n * nb * cr.NF * pp * 4, g1=n * nb * cr.NF * p1 * 4,
                o=n * nb * d["C"] * d["tc"] * d["F"] * 4)


def dense_buffer(D, d, layout):
    """D [m][30][h2][w2] as the decoder finds it: rows of flat_p floats (the pad columns stay poison), or of n_out16 halves"""
    m = D.shape[0]
    if layout == cr.CL16:
        out = np.full((m, d["n_out16"]), np.nan, dtype=np.float16)
        out[:, :d["h2"] * d["w2"] * 32] = cr.to_layout(D, cr.CL16).reshape(m, -1)
        return out
    out = np.full((m, d["flat_p"]), np.nan, dtype=np.float32)
    out[:, :d["flat"]] = cr.to_layout(D, layout).reshape(m, -1)
    return out


# ------------------------------------------------------------------------------------------------ the child process
def child(switch, out_path):
    import torch
    from deepconvsep_amd.runtime import Network, default_context

    ctx = default_context()
    lib = ctx._lib
    n_cu = int(torch.cuda.get_device_properties(ctx.device_index).multi_processor_count)
    arrays, report, nets = {}, {"_n_cu": n_cu}, {}

    def net(graph, F, kind, f16):
        key = (graph, F, kind)
        if key not in nets:
            nets[key] = Network(ctx, graph, cr.params(graph, F, kind), cr.TC, F)
        assert lib.dcs_model_set_conv_precision(nets[key]._h, int(f16)) == 0
        return nets[key]

    def last(h):
        codes, prm = (i32 * 8)(), (i64 * 24)()
        assert lib.dcs_debug_conv_last_kernel(h, codes, prm) == 0
        return {cr.ROLES[r]: [codes[r]] + list(prm[3 * r:3 * r + 3]) for r in range(8) if codes[r]}

    def arena(sizes, poison):
        place, off = {}, G
        for name, nbytes in sizes.items():
            place[name] = (off, nbytes)
            off += (nbytes + 255) // 256 * 256 + G
        return torch.full((off,), poison, dtype=torch.uint8, device="cuda"), place

    def run(case, kind, poison, twice):
        """-> dict(rc, kernels, hand-over, outputs {name: bytes written region}, untouched ok, same twice, damage)"""
        c, d = case, cr.dims(case["graph"], case["F"])
        n, nb, stage = c["n"], c["nb"], c["stage"]
        m = net(c["graph"], c["F"], kind, c["f16"])
        sizes = buffer_bytes(d, n, nb)
        frames = c.get("frames")
        if frames:
            sizes["frames"] = d["C"] * frames[0] * d["F"] * 4
        raw, place = arena(sizes, poison)
        view = lambda name: raw[place[name][0]:place[name][0] + place[name][1]]

        def put(name, host):
            b = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
            view(name)[:b.size].copy_(torch.from_numpy(b))

        def args(**kw):
            a = ConvArgs()
            a.n, a.n_branch, a.tie_mode = n, nb, c["tie"]
            for name in BUFS:
                setattr(a, name, view(name).data_ptr())
                setattr(a, name + "_bytes", place[name][1])
            for key, v in kw.items():
                setattr(a, key, v)
            return a

        res = dict(rc=[], kernels={})
        pooled = bool(d["pool"])
        fused_pool = cr.model_flags(c["graph"], c["F"], switch)["pool_fused"]
        words = n * cr.NF * cr.TC * cr.pool_words(d["w1"]) * 4       # the routing words of the fused pool, where a1b would be
        if stage == cr.STAGE_CONV1 or (stage == cr.STAGE_DECODER and pooled):
            x, fr = cr.tiles(c["graph"], c["F"], n, kind, frames)
            put("tiles", x)
            a = args()
            if frames:
                put("frames", fr)
                a.frames_src, a.frames_bytes, a.frames_rows, a.frames_stride = view("frames").data_ptr(), place["frames"][1], frames[0], frames[1]
            for _ in range(2 if twice and stage == cr.STAGE_CONV1 else 1):
                res["rc"].append(lib.dcs_debug_conv_stage(m._h, cr.STAGE_CONV1, ctypes.byref(a)))
            if stage == cr.STAGE_CONV1:
                res["kernels"] = last(m._h)
                res.update(a1_layout=a.a1_layout, a1_rows=a.a1_rows, fold2=a.fold2, a2_f16=a.a2_f16)
        if stage == cr.STAGE_CONV2:
            mp = cr.a1_map(c["graph"], c["F"], n, kind, c["a1_rows"])
            src = mp[None] if c["a1_rows"] != cr.TC else cr.a1_tiles(mp, n, cr.TC)
            put("p1" if pooled else "a1b", cr.to_layout(src, c["a1_layout"]))
            a = args(a1_layout=c["a1_layout"], a1_rows=c["a1_rows"])
            for _ in range(2 if twice else 1):
                res["rc"].append(lib.dcs_debug_conv_stage(m._h, stage, ctypes.byref(a)))
            res["kernels"] = last(m._h) if res["rc"][-1] == 0 else {}
            res.update(a1_layout=a.a1_layout, a1_rows=a.a1_rows, fold2=a.fold2, a2_f16=a.a2_f16)
        if stage == cr.STAGE_DECODER:
            put("D", dense_buffer(cr.dense_out(c["graph"], c["F"], n, nb, kind), d, c["d_layout"]))
            a = args(d_layout=c["d_layout"])
            for _ in range(2 if twice else 1):
                res["rc"].append(lib.dcs_debug_conv_stage(m._h, stage, ctypes.byref(a)))
            res["kernels"] = last(m._h) if res["rc"][-1] == 0 else {}
        ctx.synchronize()
        # what the stage wrote: (buffer, leading bytes it owns); everything else must still be poison
        exp = cr.expected(c, n_cu)
        own = {}
        if all(rc == 0 for rc in res["rc"]):
            if stage == cr.STAGE_CONV1:
                rows = frames[0] if (frames and res["a1_layout"] != cr.CF) else n * cr.TC
                if pooled:
                    own["p1"] = sizes["p1"]
                    own["a1b"] = words if fused_pool else sizes["a1b"]
                else:
                    own["a1b"] = rows * d["w1"] * (64 if res["a1_layout"] == cr.CL16 else 120)
            elif stage == cr.STAGE_CONV2:
                own["a2b"] = 0 if res["fold2"] else n * (d["pitch16"] * 2 if res["a2_f16"] else d["flat_p"] * 4)
            else:
                own["o"] = sizes["o"]
                if pooled:
                    own["a1b"] = words if fused_pool else sizes["a1b"]          # conv1's, read by the un-pool
                    own["p1"] = sizes["p1"]
        inputs = {"tiles", "frames", "D"} | ({"p1" if pooled else "a1b"} if stage == cr.STAGE_CONV2 else set())
        # the two-kernel decoder writes all of g2 and, behind the separate un-pool, all of g1 (the buffers are exactly what
        # they hold: the red zones see what goes past); the one-kernel decoders and the fused un-pool leave them alone
        scratch = set()
        if stage == cr.STAGE_DECODER and "decoder" not in res["kernels"] and all(rc == 0 for rc in res["rc"]):
            scratch = {"g2"} | ({"g1"} if "unpool" in res["kernels"] else set())
        untouched = True
        for name in sizes:
            if name in inputs or name in scratch:
                continue
            tail = view(name)[own.get(name, 0):]
            untouched = untouched and bool((tail == poison).all().item())
        total = int((raw != poison).sum().item())
        inside = sum(int((view(name) != poison).sum().item()) for name in sizes)
        res["untouched"] = untouched
        res["red_zone_bytes_damaged"] = total - inside
        res["out"] = {name: view(name)[:nbytes].cpu().numpy().copy() for name, nbytes in own.items() if nbytes}
        if fused_pool and "a1b" in res["out"]:
            # routing words: a row's words past ceil(w1 / 32) are not written
            w = res["out"]["a1b"].view(np.uint32).reshape(-1, cr.pool_words(d["w1"]))
            res["words_tail_untouched"] = bool(np.all(w[:, cr.cdiv(d["w1"], 32):].view(np.uint8) == poison))
            w = w.copy()
            w[:, cr.cdiv(d["w1"], 32):] = 0
            res["out"]["a1b"] = w.view(np.uint8).reshape(-1)
        return res

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:
            return -1, str(exc)

    for case in cr.cases(n_cu):
        if case["switch"] != switch:
            continue
        r1 = run(case, "rand", 0xFF, False)
        r2 = run(case, "rand", 0x4B, True)
        ri = run(case, "int", 0x4B, False)
        same = lambda a, b: set(a["out"]) == set(b["out"]) and all(np.array_equal(a["out"][k], b["out"][k]) for k in a["out"])
        n_ws, guard_err = guards()
        report[case["name"]] = dict(
            rc=r1["rc"] + r2["rc"] + ri["rc"], kernels=r1["kernels"], kernels_same=r1["kernels"] == r2["kernels"] == ri["kernels"],
            handoff=[r1.get(k, 0) for k in ("a1_layout", "a1_rows", "fold2", "a2_f16")],
            untouched=r1["untouched"] and r2["untouched"] and ri["untouched"], same_poisons_and_twice=same(r1, r2),
            words_tail_untouched=all(r.get("words_tail_untouched", True) for r in (r1, r2, ri)),
            red_zone_bytes_damaged=r1["red_zone_bytes_damaged"] + r2["red_zone_bytes_damaged"] + ri["red_zone_bytes_damaged"],
            scratch_blocks=n_ws, scratch_guard=guard_err)
        for kind, r in (("rand", r1), ("int", ri)):
            for name, b in r["out"].items():
                arrays["%s/%s/%s" % (case["name"], kind, name)] = b
    if switch == "none":
        report["_args"] = _arguments(torch, ctx, lib, net)
        for F in cr.FOLD_SIZES:                               # fold_conv2_fc_kernel's weights, as the model made them
            m = Network(ctx, "ikala", cr.fold_params(F), cr.TC, F)
            rows, cols = i64(), i64()
            rc = [lib.dcs_debug_conv_fold_weights(m._h, None, 0, ctypes.byref(rows), ctypes.byref(cols))]
            out = np.full(rows.value * cols.value + 64, np.nan, dtype=np.float32)
            rc.append(lib.dcs_debug_conv_fold_weights(m._h, vp(out.ctypes.data), rows.value * cols.value, None, None))
            report["_fold%d" % F] = dict(rc=rc, rows=rows.value, cols=cols.value, past_untouched=bool(np.isnan(out[rows.value * cols.value:]).all()))
            arrays["_fold%d" % F] = out[:rows.value * cols.value]
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _arguments(torch, ctx, lib, net):
    """every refusal of the entries: the status, and nothing written"""
    graph, F, n, nb = "bach10", 93, 2, 4
    d = cr.dims(graph, F)
    m = net(graph, F, "rand", 0)
    sizes = buffer_bytes(d, n, nb)
    bufs = {k: torch.full((max(v, 2 << 20) + 64,), 0xFF, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    for k in ("tiles", "D"):
        bufs[k].zero_()
    res = {}

    def run(label, want, stage, m_=m, roomy=False, **kw):
        for k in ("a1b", "a2b", "o", "g2"):
            bufs[k].fill_(0xFF)
        a = ConvArgs()
        a.n, a.n_branch, a.tie_mode, a.a1_rows = n, nb, 0, cr.TC
        for name in BUFS:
            setattr(a, name, bufs[name].data_ptr())
            setattr(a, name + "_bytes", (2 << 20) if roomy else sizes[name])
        for k, v in kw.items():
            setattr(a, k, (bufs[v[0]].data_ptr() + v[1]) if isinstance(v, tuple) else v)
        rc = lib.dcs_debug_conv_stage(m_._h if m_ is not None else None, stage, ctypes.byref(a))
        ctx.synchronize()
        untouched = all(bool((bufs[k] == 0xFF).all().item()) for k in ("a1b", "a2b", "o", "g2"))
        res[label] = dict(rc=rc, want=want, untouched=untouched, message=lib.dcs_last_error().decode("utf-8", "replace"))

    run("conv1 good", 0, 0)
    bufs["a1b"].zero_()
    run("decoder good", 0, 2)
    for stage, name in ((0, "tiles"), (0, "a1b"), (1, "a1b"), (1, "a2b"), (2, "D"), (2, "g2"), (2, "o")):
        run("stage %d: null %s" % (stage, name), EINVAL, stage, **{name: None})
        run("stage %d: %s one byte short" % (stage, name), EINVAL, stage, **{name + "_bytes": sizes[name] - 1})
        run("stage %d: %s misaligned" % (stage, name), EINVAL, stage, **{name: (name, 4)})
    run("stage 3", EINVAL, 3)
    run("n = 0", EINVAL, 0, n=0)
    run("no branches", EINVAL, 2, n_branch=0)
    run("five branches", EINVAL, 2, n_branch=5)
    run("tie mode 2", EINVAL, 0, tie_mode=2)
    run("a1 layout 3", EINVAL, 1, a1_layout=3)
    run("D layout -1", EINVAL, 2, d_layout=-1)
    run("channel-first a1 with a row stride", EINVAL, 1, a1_rows=5)
    run("a1 rows 0", EINVAL, 1, a1_layout=1, a1_rows=0)
    run("frames that do not cover the tiles", EINVAL, 0, frames_src=("tiles", 0), frames_bytes=sizes["tiles"], frames_rows=40, frames_stride=5)
    run("frames at the tile length", EINVAL, 0, frames_src=("tiles", 0), frames_bytes=sizes["tiles"], frames_rows=60, frames_stride=30)
    run("frames one byte short", EINVAL, 0, frames_src=("tiles", 0), frames_bytes=35 * F * 4 - 1, frames_rows=35, frames_stride=5)
    run("null model", EINVAL, 0, m_=None)
    # layouts the plan cannot consume
    run("f16 a1 without the f16 switch", EUNSUPPORTED, 1, a1_layout=2)
    run("f16 D without the f16 switch", EUNSUPPORTED, 2, d_layout=2)
    mi = net("ikala", 267, "rand", 0)
    assert all(v <= (2 << 20) for v in buffer_bytes(cr.dims("ikala", 267), 1, 1).values())
    run("channels-last a1 in a graph with a pool", EUNSUPPORTED, 1, m_=mi, roomy=True, n=1, n_branch=1, a1_layout=1)
    run("channels-last D in a graph without a fused decoder", EUNSUPPORTED, 2, m_=mi, roomy=True, n=1, n_branch=1, d_layout=1)
    small = np.full(16, np.nan, dtype=np.float32)
    res["fold weights of a graph that does not fold"] = dict(rc=lib.dcs_debug_conv_fold_weights(m._h, vp(small.ctypes.data), 16, None, None),
                                                             want=EUNSUPPORTED, untouched=bool(np.isnan(small).all()), message="")
    res["fold weights into a short buffer"] = dict(rc=lib.dcs_debug_conv_fold_weights(mi._h, vp(small.ctypes.data), 16, None, None),
                                                   want=EINVAL, untouched=bool(np.isnan(small).all()), message="")
    res["fold weights without a model"] = dict(rc=lib.dcs_debug_conv_fold_weights(None, None, 0, None, None), want=EINVAL, untouched=True, message="")
    res["last_kernel without a model"] = dict(rc=lib.dcs_debug_conv_last_kernel(None, None, None), want=EINVAL, untouched=True, message="")
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_conv_kernels as t; t.child(sys.argv[2], sys.argv[3])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """switch set -> (arrays, report): one child after another, each under its own time limit; a child that ends in a signal
    or at its limit ends the run (nothing more is started on the device)"""
    d = tmp_path_factory.mktemp("conv_kernels")
    res = {}
    for name, spec in cr.SWITCHES.items():
        out = str(d / (name + ".npz"))
        env = dict(os.environ)
        env.update(spec["env"])
        env.update(DCS_WS_GUARD=str(G))
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


_REF, _CASES = {}, {}


def _cases_for(n_cu):
    if n_cu not in _CASES:
        _CASES[n_cu] = cr.cases(n_cu)
    return _CASES[n_cu]


def _conv1_ref(graph, F, n, kind, frames, cls, f16_out):
    """shared among the cases of one shape: the float64 result and the class's restatement"""
    key = ("conv1", graph, F, n, kind, frames, cls, f16_out)
    if key not in _REF:
        d = cr.dims(graph, F)
        W = cr.weights(graph, kind)
        x, fr = cr.tiles(graph, F, n, kind, frames)
        _REF[key] = cr.layer(cr.conv1, x, W[0], d, cls, bias=(W[1], W[2]), f16_out=f16_out)
    return _REF[key]


def _check(tag, got, want, S, extra, rest, sub, K, cls_c, exact):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), "%s: %d values are not finite" % (tag, int((~np.isfinite(got)).sum()))
    if exact:
        bad = int((got != want).sum())
        assert bad == 0, "%s: integer probe: %d of %d elements differ from the float64 result, worst by %g" % (
            tag, bad, got.size, float(np.abs(got - want).max()))
        return None
    e = cr.measure(got, want, S)
    e32 = cr.measure(rest, want[sub], S[sub])
    cap_ratio = float(np.max(np.abs(got - want) / ((K + cls_c) * cr.U * S + extra + 1e-300)))
    print("\n%s: E %.3g, restatement %.3g, ratio %.2f, worst |err| / cap %.3g" % (tag, e, e32, e / e32 if e32 else float("inf"), cap_ratio))
    assert e <= cr.gr.FACTOR * e32, "%s: device %.3g, float32 restatement %.3g" % (tag, e, e32)
    assert cr.inside_cap(got, want, S, extra, K, cls_c), "%s: outside the cap by a factor of %.3g" % (tag, cap_ratio)
    return e / e32 if e32 else 0.0


@pytest.mark.parametrize("case", cr.cases(), ids=lambda c: c["name"])
def test_conv_stage(runs, case):
    z, report = runs[case["switch"]]
    n_cu = report["_n_cu"]
    # the table depends on the CU count through the image counts of the second-round cases only: same names, resolved here
    case = next(c for c in _cases_for(n_cu) if c["name"] == case["name"])
    r = report[case["name"]]
    exp = cr.expected(case, n_cu)
    assert all(rc == exp["rc"] for rc in r["rc"]), (r["rc"], exp["rc"])
    assert r["untouched"], "bytes outside what the stage writes are no longer poison"
    assert r["red_zone_bytes_damaged"] == 0 and r["scratch_guard"] == "" and r["scratch_blocks"] >= 0, r
    if exp["rc"] != 0:
        return
    got_k = {k: tuple(v) for k, v in r["kernels"].items()}
    assert got_k == exp["kernels"], "ran %r, the launchers' arithmetic says %r" % (got_k, exp["kernels"])
    assert r["kernels_same"]
    graph, F, n, nb, stage = case["graph"], case["F"], case["n"], case["nb"], case["stage"]
    d = cr.dims(graph, F)
    if stage != cr.STAGE_DECODER:
        assert r["handoff"] == [exp["a1_layout"], exp["a1_rows"], exp["fold2"], exp["a2_f16"]], r["handoff"]
    assert r["same_poisons_and_twice"], "the poisons 0xFF and 0x4B, or a second launch over the first, gave other bits"
    assert r["words_tail_untouched"]
    pooled = bool(d["pool"])
    for kind in ("rand", "int"):
        exact = kind == "int"
        W = cr.weights(graph, kind)
        buf = lambda name: z["%s/%s/%s" % (case["name"], kind, name)]
        tag = "%s %s" % (case["name"], kind)
        if stage == cr.STAGE_CONV1:
            code = exp["kernels"]["conv1"][0]
            cls, lay = cr.CLASS[code], exp["a1_layout"]
            frames = case.get("frames") if lay != cr.CF else None
            want, S, extra, rest, sub = _conv1_ref(graph, F, n, kind, case.get("frames"), cls, lay == cr.CL16)
            K, c = cr.layer_K(graph, "conv1"), cr.cap_c(cr.layer_K(graph, "conv1"), cls)
            if frames:      # one map of the clip's frames: the reference tile k is rows k * stride .. of it
                dev = cr.from_layout(buf("a1b").view(np.float16 if lay == cr.CL16 else np.float32), lay, 1, frames[0], d["w1"])[0]
                _check(tag, np.stack([dev[:cr.NF, k * frames[1]:k * frames[1] + cr.TC] for k in range(n)]), want, S, extra, rest, sub, K, c, exact)
                if lay == cr.CL16:
                    assert not dev[cr.NF:].any(), "pad channels 30, 31 of the f16 hand-over are not zero"
                continue
            if pooled and code == cr.K_CONV1_REG3_POOL:
                p1 = buf("p1").view(np.float32).reshape(n, cr.NF, cr.TC, d["wp"])
                _check(tag + " pooled", p1, cr.pool(want), cr.pool(S), cr.pool(extra), cr.pool(rest), sub, K, c, exact)
                routes = cr.routes_from_words(buf("a1b").view(np.uint32).reshape(n, cr.NF, cr.TC, -1), d["w1"])[..., :4 * d["wp"]]
                per_window = routes.reshape(routes.shape[:-1] + (d["wp"], 4)).sum(axis=-1)
                assert per_window.min() >= 1 and (case["tie"] == cr.TIE_ALL or per_window.max() == 1), "a window routes to no / to several positions"
                if exact:
                    assert np.array_equal(routes, cr.pool_routes(want, case["tie"])[..., :4 * d["wp"]]), "routing words differ from the float64 routing"
                continue
            dev = cr.from_layout(buf("a1b").view(np.float16 if lay == cr.CL16 else np.float32), lay, n, cr.TC, d["w1"])
            _check(tag, dev[:, :cr.NF], want, S, extra, rest, sub, K, c, exact)
            if lay == cr.CL16:
                assert not dev[:, cr.NF:].any(), "pad channels 30, 31 of the f16 hand-over are not zero"
            if pooled:      # the separate pool kernel: exactly the window maxima of what conv1 wrote
                p1 = buf("p1").view(np.float32).reshape(n, cr.NF, cr.TC, d["wp"])
                assert np.array_equal(p1, cr.pool(np.ascontiguousarray(dev))), "pool_kernel: not the window maxima of its input"
        elif stage == cr.STAGE_CONV2:
            if exp["fold2"]:
                continue
            code = exp["kernels"]["conv2"][0]
            cls = cr.CLASS[code]
            mp = cr.a1_map(graph, F, n, kind, case["a1_rows"])
            x = cr.a1_tiles(mp, n, case["a1_rows"])
            if case["a1_layout"] == cr.CL16:
                x = cr._h(x)
            want, S, extra, rest, sub = cr.layer(cr.conv2, x, W[3], d, cls, bias=(W[4], W[5]), f16_out=bool(exp["a2_f16"]))
            if exp["a2_f16"]:
                rows = buf("a2b").view(np.float16).reshape(n, d["pitch16"])
            else:
                rows = buf("a2b").view(np.float32).reshape(n, d["flat_p"])
            assert not rows[:, d["flat"]:].any(), "the pad columns of conv2's map are not zero"
            K = cr.layer_K(graph, "conv2")
            _check(tag, rows[:, :d["flat"]].reshape(want.shape), want, S, extra, rest, sub, K, cr.cap_c(K, cls), exact)
        else:
            D = cr.dense_out(graph, F, n, nb, kind)
            if case["d_layout"] == cr.CL16:
                D = cr._h(D)
            routes = None
            if pooled:
                a1 = buf("a1b")
                if "unpool" in exp["kernels"]:
                    routes = cr.pool_routes(a1.view(np.float32).reshape(n, cr.NF, cr.TC, d["w1"]), case["tie"])
                else:
                    routes = cr.routes_from_words(a1.view(np.uint32).reshape(n, cr.NF, cr.TC, -1), d["w1"]).copy()
                    routes[..., 4 * d["wp"]:] = False
                if exact:
                    x, _ = cr.tiles(graph, F, n, kind)
                    a1w = cr.conv1(x, W[0], W[1], W[2], d)
                    assert np.array_equal(routes, cr.pool_routes(a1w, case["tie"])), "the routing differs from the float64 routing"
            if "decoder" in exp["kernels"]:
                code = exp["kernels"]["decoder"][0]
                cls2 = cls1 = cr.CLASS[code]
                mid16 = code in (cr.K_FUSED, cr.K_FUSED_CL, cr.K_FUSED_CL16)
            else:
                cls2, cls1, mid16 = cr.CLASS[exp["kernels"]["conv2t"][0]], cr.CLASS[exp["kernels"]["conv1t"][0]], False
            want, S, extra, rest, sub, K, c, _ = cr.decoder(D, W[0], W[3], d, graph, cls2, cls1, routes=routes, nb=nb, f16_mid=mid16)
            o = buf("o").view(np.float32).reshape(n * nb, d["C"], cr.TC, F)
            _check(tag, o, want, S, extra, rest, sub, K, c, exact)


@pytest.mark.parametrize("F", cr.FOLD_SIZES)
def test_folded_conv2_bottleneck_weights(runs, F):
    """fold_conv2_fc_kernel: every weight within one float32 ulp of the float64 fold rounded to float32 (both sides are
    float64 sums rounded once)"""
    z, report = runs["none"]
    r = report["_fold%d" % F]
    d = cr.dims("ikala", F)
    assert r["rc"] == [0, 0] and r["past_untouched"] and (r["rows"], r["cols"]) == (cr.NF * cr.TC * d["wp"], cr.HID), r
    p = cr.fold_params(F)
    want = cr.fold_want(p[3], p[6], d).astype(np.float32)
    got = z["_fold%d" % F].reshape(want.shape)
    assert np.isfinite(got).all() and np.count_nonzero(want) > want.size // 2
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    off = np.abs(got.astype(np.float64) - want.astype(np.float64)) > ulp
    print("\nF %d: %d x %d weights, %d differ from the rounded float64 fold (all by one ulp), largest |w| %.3g"
          % (F, want.shape[0], want.shape[1], int((got != want).sum()), float(np.abs(want).max())))
    assert not off.any(), "%d weights are more than one ulp from the float64 fold" % int(off.sum())


def test_every_kernel_code_is_reached(runs):
    seen = set()
    for name in runs:
        for key, r in runs[name][1].items():
            if not key.startswith("_"):
                seen |= {v[0] for v in r["kernels"].values()}
    assert seen >= cr.ALL_CODES, "never launched: %r" % sorted(cr.CODE_NAMES[k] for k in cr.ALL_CODES - seen)


def test_entries_refuse_bad_arguments(runs):
    args = runs["none"][1]["_args"]
    assert len(args) > 40
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        if r["want"] != 0:
            assert r["untouched"], label
