"""Every GEMM kernel and operand packer of csrc/gemm.hip, csrc/gemm_bf16x3.hip and csrc/gemm_f16.hip on the MI355X, directly
against float64.

The kernels are reached through ``dcs_debug_gemm`` / ``dcs_debug_gemm_f16_skinny`` / ``dcs_debug_gemm_f16_longk`` (the
launchers the graphs use, with every address checked first) and the packers through ``dcs_debug_gemm_pack``; after every
launch ``dcs_debug_gemm_last_kernel`` says which kernel ran and the test asserts that it is the one ``expected_kernel`` of
tests/gemm_ref.py names and the one the case was written for.  One child process per switch set (``gemm_ref.SWITCHES``:
libdcs reads them once per process), each with ``DCS_WS_GUARD=65536`` and each running its cases on buffers carved out of one
poisoned allocation per case: 64 KiB between and around the buffers; A's columns ``[K, lda)``, B's columns past ``n_cols``,
everything behind an operand's last element, C's rows nobody owns and its columns ``[n_store, ldc)`` born as 0xFF bytes
(float32 / f16 NaN).  A kernel that reads past an operand multiplies a NaN and shows it; one that writes outside C is counted.
Every case runs twice and the two outputs must be the same bits.  The children write what they computed; the parent compares
by the rules of tests/gemm_ref.py (the one-hot twins, whose expectation is a gather of rows of B, are compared bit for bit
in the child and only the count of differing elements travels).
"""
import ctypes
import json
import os

import numpy as np
import pytest

import gemm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
POISON = 0xFF
G = 1 << 16
EINVAL, EUNSUPPORTED = -1, -2
vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class GemmArgs(ctypes.Structure):
    """dcs_debug_gemm_args of include/dcs.h"""
    _fields_ = [("A", vp), ("n_A", i64), ("lda", i64), ("a_gdiv", i32), ("a_gmul", i64), ("a_scale", ctypes.c_float),
                ("a_rowmap", vp), ("n_rowmap", i64),
                ("B", vp), ("n_B", i64), ("ldb", i32),
                ("bias", vp), ("n_bias", i64),
                ("C", vp), ("n_C", i64), ("ldc", i64), ("c_gdiv", i32), ("c_gmul", i64),
                ("M", i64), ("n_cols", i32), ("n_store", i32), ("K", i32), ("relu", i32), ("a_vec", i32),
                ("Bq", vp), ("Bq_bytes", i64), ("bq_f32", i32),
                ("Aq", vp), ("Aq_bytes", i64), ("aq_rows", i32),
                ("Bfrag", vp), ("n_Bfrag", i64),
                ("n_br", i32), ("br_Bq", vp * 4), ("br_bias", vp * 4), ("br_C", vp * 4)]


# ------------------------------------------------------------------------------------------------ the child process
class _Arena(object):
    """one poisoned allocation; buffers 256-byte aligned with G bytes around each"""

    def __init__(self, torch):
        self.torch, self.items, self.place, self.raw = torch, [], {}, None

    def add(self, name, nbytes):
        self.items.append((name, int(nbytes)))

    def commit(self):
        off = G
        for name, n in self.items:
            self.place[name] = (off, n)
            off += (n + 255) // 256 * 256 + G
        self.raw = self.torch.full((off,), POISON, dtype=self.torch.uint8, device="cuda")
        return self

    def u8(self, name):
        o, n = self.place[name]
        return self.raw[o:o + n]

    def addr(self, name):
        return self.u8(name).data_ptr() if name in self.place else None

    def put(self, name, host):
        """host: a numpy array of exactly the buffer's bytes"""
        b = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert b.size == self.place[name][1], (name, b.size, self.place[name][1])
        self.u8(name).copy_(self.torch.from_numpy(b))

    def get(self, name, dtype):
        return self.u8(name).cpu().numpy().view(dtype)

    def damage(self):
        """bytes outside the buffers that are no longer poison"""
        self.torch.cuda.synchronize()
        total = int((self.raw != POISON).sum().item())
        return total - sum(int((self.u8(name) != POISON).sum().item()) for name in self.place)


def _poisoned_host(values, mask, dtype):
    """a buffer of mask.size elements: `values` where the mask is set, 0xFF bytes elsewhere"""
    out = np.full(mask.size * np.dtype(dtype).itemsize, POISON, dtype=np.uint8).view(dtype)
    out[mask] = values[mask]
    return out


def child(switch, out_path):
    import torch
    from deepconvsep_amd.runtime import default_context

    ctx = default_context()
    lib = ctx._lib
    n_cu = int(torch.cuda.get_device_properties(ctx.device_index).multi_processor_count)
    arrays, report = {}, {"_n_cu": n_cu}

    def last():
        code, prm = i32(), (i64 * 4)()
        assert lib.dcs_debug_gemm_last_kernel(ctx._h, ctypes.byref(code), prm) == 0
        return [code.value] + list(prm)

    def guards():
        try:
            return ctx.check_guards(), ""
        except Exception as exc:                                            # a damaged scratch red zone: reported, not raised
            return -1, str(exc)

    def pack(ar, kind, src_name, n_src, K, ld, n, p, dst_name):
        pp = (i64 * 4)(*(list(p) + [0] * (4 - len(p)))) if p is not None else None
        return lib.dcs_debug_gemm_pack(ctx._h, kind, vp(ar.addr(src_name)), n_src, K, ld, n, pp, vp(ar.addr(dst_name)),
                                       ar.place[dst_name][1])

    def gemm_case(case):
        c = gr.resolve(case, n_cu)
        inp = gr.inputs(c)
        M, K, n_cols, ns, ldb, ldc = c["M"], c["K"], c["n_cols"], c["n_store"], c["ldb"], c["ldc"]
        f16s, f16l = c["via"] == "f16_skinny", c["via"] == "f16_longk"
        nb = max(1, c["n_br"])
        crow = gr.c_rows(c)
        n_C = int(crow.max()) * ldc + ns
        csize = 2 if f16s else 4
        a_dt = np.float16 if c["a_f16"] else np.float32
        n_A, Kp = inp["A_flat"].size, gr.round_up(K, 128)
        packed_kind = gr.PACK_BH_PLAIN if (f16s or f16l) else (gr.PACK_B32 if c["bq"] == "b32" else gr.PACK_BQ)
        has_packed = f16s or f16l or bool(c["bq"])
        ar = _Arena(torch)
        ar.add("A", n_A * np.dtype(a_dt).itemsize)
        if c["rowmap"]:
            ar.add("map", M * 4)
        for b in range(nb):
            ar.add("B%d" % b, Kp * ldb * 4)
            if inp["bias"][b] is not None:
                ar.add("bias%d" % b, inp["bias"][b].size * 4)
            ar.add("C1_%d" % b, n_C * csize)
            ar.add("C2_%d" % b, n_C * csize)
            if has_packed:
                ar.add("Bq%d" % b, gr.pack_bytes(packed_kind, K, n_cols))
        if c["aq"]:
            ar.add("Aq", gr.pack_bytes(gr.PACK_SPLIT_A, K, c["aq_rows"]))
        if c["bfrag"]:
            ar.add("Bfrag", gr.pack_bytes(gr.PACK_BFRAG, K, n_cols))
        if f16s:
            ar.add("Ah", gr.pack_bytes(gr.PACK_SPLIT_A_F16, K, 128 if M <= 128 else 176))
        ar.commit()
        ar.put("A", _poisoned_host(inp["A_flat"], inp["A_mask"], a_dt))
        if c["rowmap"]:
            ar.put("map", inp["rowmap"])
        rcs = []
        for b in range(nb):
            Bh = inp["B"][b]
            ar.put("B%d" % b, _poisoned_host(Bh.reshape(-1), ~np.isnan(Bh.reshape(-1)), np.float32))
            if inp["bias"][b] is not None:
                ar.put("bias%d" % b, inp["bias"][b])
            if has_packed:
                rcs.append(pack(ar, packed_kind, "B%d" % b, Kp * ldb, K, ldb, n_cols, None, "Bq%d" % b))
        if c["aq"]:
            rcs.append(pack(ar, gr.PACK_SPLIT_A, "A", n_A, K, c["lda"], c["aq_rows"], (M,), "Aq"))
        if c["bfrag"]:
            fr = np.empty(gr.pack_bytes(gr.PACK_BFRAG, K, n_cols) // 4, dtype=np.float32)
            src = np.ascontiguousarray(np.nan_to_num(inp["B"][0]))
            rcs.append(lib.dcs_debug_gemm_pack(ctx._h, gr.PACK_BFRAG, vp(src.ctypes.data), src.size, K, ldb, n_cols, None,
                                               vp(fr.ctypes.data), fr.nbytes))
            ar.put("Bfrag", fr)

        def launch(which_c):
            if f16s:
                arr = lambda pre: (vp * 4)(*[ar.addr("%s%d" % (pre, b)) for b in range(nb)])
                return lib.dcs_debug_gemm_f16_skinny(ctx._h, vp(ar.addr("A")), n_A, c["lda"], M, K, n_cols, nb, arr("Bq"),
                                                     ar.place["Bq0"][1], arr("bias"), n_cols, arr(which_c + "_"), n_C, ldc,
                                                     vp(ar.addr("Ah")), ar.place["Ah"][1])
            if f16l:
                return lib.dcs_debug_gemm_f16_longk(ctx._h, vp(ar.addr("A")), n_A, c["lda"], M, K, n_cols, vp(ar.addr("Bq0")),
                                                    ar.place["Bq0"][1], int(c["a_f16"]), vp(ar.addr("bias0")), ns,
                                                    vp(ar.addr(which_c + "_0")), n_C, ldc, ns, c["relu"])
            a = GemmArgs()
            a.A, a.n_A, a.lda, a.a_gdiv, a.a_gmul, a.a_scale = ar.addr("A"), n_A, c["lda"], c["a_gdiv"], c["a_gmul"], c["a_scale"]
            a.a_rowmap, a.n_rowmap = ar.addr("map"), M if c["rowmap"] else 0
            a.B, a.n_B, a.ldb = ar.addr("B0"), Kp * ldb, ldb
            a.bias, a.n_bias = ar.addr("bias0"), ns
            a.C, a.n_C, a.ldc, a.c_gdiv, a.c_gmul = ar.addr(which_c + "_0"), n_C, ldc, c["c_gdiv"], c["c_gmul"]
            a.M, a.n_cols, a.n_store, a.K, a.relu, a.a_vec = M, n_cols, ns, K, c["relu"], c["a_vec"]
            if c["bq"]:
                a.Bq, a.Bq_bytes, a.bq_f32 = ar.addr("Bq0"), ar.place["Bq0"][1], int(c["bq"] == "b32")
            if c["aq"]:
                a.Aq, a.Aq_bytes, a.aq_rows = ar.addr("Aq"), ar.place["Aq"][1], c["aq_rows"]
            if c["bfrag"]:
                a.Bfrag, a.n_Bfrag = ar.addr("Bfrag"), ar.place["Bfrag"][1] // 4
            a.n_br = c["n_br"]
            for b in range(c["n_br"]):
                a.br_Bq[b], a.br_bias[b], a.br_C[b] = ar.addr("Bq%d" % b), ar.addr("bias%d" % b), ar.addr("%s_%d" % (which_c, b))
            return lib.dcs_debug_gemm(ctx._h, dict(rows=gr.VIA_ROWS, skinny=gr.VIA_SKINNY, longk=gr.VIA_LONGK)[c["via"]],
                                      ctypes.byref(a))

        rcs += [launch("C1"), launch("C2")]
        ctx.synchronize()
        kern = last()
        own = np.zeros(n_C, dtype=bool)
        own[(crow[:, None] * ldc + np.arange(ns)[None, :]).reshape(-1)] = True
        c_dt, c_u = (np.float16, np.uint16) if f16s else (np.float32, np.uint32)
        same, nan, foreign, mismatch = True, 0, 0, 0
        cls = gr.kernel_class(kern[0]) if kern[0] else None
        for b in range(nb):
            c1, c2 = ar.get("C1_%d" % b, c_u), ar.get("C2_%d" % b, c_u)
            same = same and bool(np.array_equal(c1, c2))
            foreign += int((c1[~own] != np.iinfo(c_u).max).sum())
            out = c1.view(c_dt)[crow[:, None] * ldc + np.arange(ns)[None, :]]
            nan += int(np.isnan(out).sum())
            if c["onehot"]:
                if cls:
                    want = gr.onehot_want(c, inp, b, cls)
                    mismatch += int((out.view(c_u) != np.ascontiguousarray(want).view(c_u)).sum())
            else:
                arrays["%s/%d" % (c["name"], b)] = out
        if f16s and not c["onehot"]:
            arrays[c["name"] + "/Ah"] = ar.get("Ah", np.uint16)
        n_ws, guard_err = guards()
        report[c["name"]] = dict(rc=rcs, kernel=kern, same_twice=same, nan=nan, foreign_written=foreign, onehot_mismatch=mismatch,
                                 scratch_blocks=n_ws, scratch_guard=guard_err, red_zone_bytes_damaged=ar.damage())

    for case in gr.cases():
        if case["switch"] == switch:
            gemm_case(case)
    if switch == "none":
        packs = {}
        for k, (name, kind, K, ld, n, p) in enumerate(gr.pack_cases()):
            src = gr.pack_source(kind, K, ld, n, p, 300 + k)
            nbytes = gr.pack_bytes(kind, K, n)
            if kind == gr.PACK_BFRAG:                                        # the host packer: NaN past the last byte it may write
                dst = np.full(nbytes // 4 + 64, np.nan, dtype=np.float32)
                rc = lib.dcs_debug_gemm_pack(ctx._h, kind, vp(src.ctypes.data), src.size, K, ld, n, None, vp(dst.ctypes.data), nbytes)
                packs[name] = dict(rc=rc, bytes=int(lib.dcs_debug_gemm_bytes(kind, K, n)), red_zone_bytes_damaged=int((~np.isnan(dst[nbytes // 4:])).sum()))
                arrays["pack/" + name] = dst[:nbytes // 4].view(np.uint8)
                continue
            ar = _Arena(torch)
            ar.add("src", src.size * 4)
            ar.add("dst", nbytes)
            ar.commit()
            flat = src.reshape(-1)
            ar.put("src", _poisoned_host(flat, ~np.isnan(flat), np.float32))
            rc = pack(ar, kind, "src", src.size, K, ld, n, p, "dst")
            ctx.synchronize()
            arrays["pack/" + name] = ar.get("dst", np.uint8)
            packs[name] = dict(rc=rc, bytes=int(lib.dcs_debug_gemm_bytes(kind, K, n)), red_zone_bytes_damaged=ar.damage())
        report["_packs"] = packs
        report["_args"] = _arguments(torch, ctx, lib)
    arrays["_report"] = np.frombuffer(json.dumps(report).encode(), dtype=np.uint8)
    np.savez(out_path, **arrays)


def _arguments(torch, ctx, lib):
    """every refusal of the entries: the status, and nothing written"""
    M, K, N = 20, 68, 64
    Kp = gr.round_up(K, 128)
    A = torch.zeros(M * K + 64, device="cuda")
    B = torch.zeros(Kp * N, device="cuda")
    bias = torch.zeros(N, device="cuda")
    C = torch.full((M * N,), float("nan"), device="cuda")
    rmap = torch.arange(M, dtype=torch.int32, device="cuda")
    bad_map = rmap.clone()
    bad_map[7] = M
    neg_map = rmap.clone()
    neg_map[3] = -1
    Bq = torch.zeros(gr.pack_bytes(gr.PACK_BQ, K, N), dtype=torch.uint8, device="cuda")
    Aq = torch.zeros(gr.pack_bytes(gr.PACK_SPLIT_A, K, 128), dtype=torch.uint8, device="cuda")
    Bfrag = torch.zeros(gr.pack_bytes(gr.PACK_BFRAG, K, N) // 4, device="cuda")

    def ptr(t, off=0):
        return t.data_ptr() + off if t is not None else None

    def args(**kw):
        a = GemmArgs()
        a.A, a.n_A, a.lda, a.a_gdiv, a.a_gmul, a.a_scale = ptr(A), M * K, K, gr.FLAT, 0, 1.0
        a.B, a.n_B, a.ldb, a.bias, a.n_bias = ptr(B), Kp * N, N, ptr(bias), N
        a.C, a.n_C, a.ldc, a.c_gdiv, a.c_gmul = ptr(C), M * N, N, gr.FLAT, 0
        a.M, a.n_cols, a.n_store, a.K, a.relu, a.a_vec = M, N, N, K, 0, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    res = {}

    def run(label, want, which=gr.VIA_ROWS, message=None, **kw):
        C.fill_(float("nan"))
        rc = lib.dcs_debug_gemm(ctx._h, which, ctypes.byref(args(**kw)))
        ctx.synchronize()
        msg = lib.dcs_last_error().decode("utf-8", "replace")
        res[label] = dict(rc=rc, want=want, untouched=bool(torch.isnan(C).all().item()),
                          message_ok=message is None or message in msg, message=msg)

    run("good", 0)
    bad = {
        "null A": dict(A=None), "null B": dict(B=None), "null C": dict(C=None), "M=0": dict(M=0), "K=0": dict(K=0), "n_cols=0": dict(n_cols=0),
        "n_store>n_cols": dict(n_store=N + 1), "n_store<0": dict(n_store=-1), "n_A short by one": dict(n_A=M * K - 1),
        "lda past A": dict(lda=K + 4), "lda<0": dict(lda=-4), "a_gdiv=0": dict(a_gdiv=0), "a_gmul<0": dict(a_gdiv=7, a_gmul=-1),
        "grouped rows past A": dict(a_gdiv=7, a_gmul=9), "n_B without the padding to 128 rows": dict(n_B=K * N),
        "ldb%64": dict(ldb=N + 4, n_B=Kp * (N + 4)), "ldb<n_cols": dict(n_cols=128, n_store=64, n_B=2 * Kp * N),
        "B misaligned": dict(B=ptr(B, 4), n_B=Kp * N - 1), "A misaligned on the vector path": dict(A=ptr(A, 4)),
        "n_C short by one": dict(n_C=M * N - 1), "ldc<n_store": dict(ldc=N - 1), "grouped C rows past C": dict(c_gdiv=7, c_gmul=9),
        "c_gdiv=0": dict(c_gdiv=0), "n_bias<n_store": dict(n_bias=N - 1),
        "row map shorter than M": dict(a_rowmap=ptr(rmap), n_rowmap=M - 1), "row map entry past A": dict(a_rowmap=ptr(bad_map), n_rowmap=M),
        "row map entry negative": dict(a_rowmap=ptr(neg_map), n_rowmap=M),
        "Bq one byte short": dict(Bq=ptr(Bq), Bq_bytes=Bq.numel() - 1), "Bq sized as f32 pieces, said to be planes": dict(Bq=ptr(Bq), Bq_bytes=gr.pack_bytes(gr.PACK_B32, K, N)),
        "Bq misaligned": dict(Bq=ptr(Bq, 8), Bq_bytes=Bq.numel()), "Aq one byte short": dict(Aq=ptr(Aq), Aq_bytes=Aq.numel() - 1, aq_rows=128),
        "Aq rows 0": dict(Aq=ptr(Aq), Aq_bytes=Aq.numel(), aq_rows=0), "Bfrag one float short": dict(Bfrag=ptr(Bfrag), n_Bfrag=Bfrag.numel() - 1),
        "branches with the rows launcher": dict(n_br=2), "n_br=5": dict(n_br=5), "a_scale NaN": dict(a_scale=float("nan")),
    }
    for label, kw in bad.items():
        run(label, EINVAL, **kw)
    run("which=3", EINVAL, which=3)
    run("row map with the skinny launcher", EINVAL, which=gr.VIA_SKINNY, a_rowmap=ptr(rmap), n_rowmap=M)
    run("n_cols%64 with the skinny launcher", EINVAL, which=gr.VIA_SKINNY, n_cols=32, n_store=32, ldb=64)
    run("branch with a null C", EINVAL, which=gr.VIA_SKINNY, n_br=1, Bq_bytes=Bq.numel(), br_Bq=(vp * 4)(ptr(Bq)), br_bias=(vp * 4)(ptr(bias)))
    # the launcher's own refusals
    run("gemm_rows: n_cols%64", EINVAL, message="gemm_rows: n_cols", n_cols=32, n_store=32)
    run("gemm_rows: vector path with K%4", EINVAL, message="gemm_rows: vector path", K=66)
    run("gemm_rows: vector path with lda%4", EINVAL, message="gemm_rows: vector path", lda=66, K=64)
    # launchers that do not take the shape
    run("skinny: 20 rows", EUNSUPPORTED, which=gr.VIA_SKINNY, Bq=ptr(Bq), Bq_bytes=Bq.numel())
    run("longk: short K", EUNSUPPORTED, which=gr.VIA_LONGK, Bq=ptr(Bq), Bq_bytes=Bq.numel())
    run("skinny: no planes", EUNSUPPORTED, which=gr.VIA_SKINNY)

    # the f16 entries
    M2, K2, N2 = 128, 32, 128
    Z = torch.zeros(150 * K2, device="cuda")
    Bh = torch.zeros(gr.pack_bytes(gr.PACK_BH, K2, N2), dtype=torch.uint8, device="cuda")
    bias2 = torch.zeros(N2, device="cuda")
    C16 = torch.full((150 * (N2 + 8),), float("nan"), dtype=torch.float16, device="cuda")
    C32 = torch.full((M2 * N2,), float("nan"), device="cuda")
    Ah = torch.zeros(gr.pack_bytes(gr.PACK_SPLIT_A_F16, K2, 128), dtype=torch.uint8, device="cuda")

    def f16s(label, want, **kw):
        d = dict(Z=ptr(Z), n_Z=M2 * K2, ldz=K2, M=M2, K=K2, n_cols=N2, n_br=1, Bh=(vp * 4)(ptr(Bh)), Bh_bytes=Bh.numel(),
                 bias=(vp * 4)(ptr(bias2)), n_bias=N2, C=(vp * 4)(ptr(C16)), n_C=M2 * N2, ldc=N2, Ah=ptr(Ah), Ah_bytes=Ah.numel())
        d.update(kw)
        C16.fill_(float("nan"))
        rc = lib.dcs_debug_gemm_f16_skinny(ctx._h, vp(d["Z"]), d["n_Z"], d["ldz"], d["M"], d["K"], d["n_cols"], d["n_br"], d["Bh"], d["Bh_bytes"],
                                           d["bias"], d["n_bias"], d["C"], d["n_C"], d["ldc"], vp(d["Ah"]), d["Ah_bytes"])
        ctx.synchronize()
        res["f16 skinny " + label] = dict(rc=rc, want=want, untouched=bool(torch.isnan(C16).all().item()), message_ok=True,
                                          message=lib.dcs_last_error().decode("utf-8", "replace"))

    f16s("good", 0)
    for label, kw in {"null Z": dict(Z=None), "n_Z short": dict(n_Z=M2 * K2 - 1), "n_C short": dict(n_C=M2 * N2 - 1), "ldc<n_cols": dict(ldc=N2 - 8),
                      "n_bias short": dict(n_bias=N2 - 1), "Bh short": dict(Bh_bytes=Bh.numel() - 1), "Ah short": dict(Ah_bytes=Ah.numel() - 1),
                      "Ah sized for 128 rows, M 150": dict(M=150, n_Z=150 * K2, n_C=150 * N2), "n_br=0": dict(n_br=0), "n_br=5": dict(n_br=5),
                      "null branch C": dict(C=(vp * 4)()), "M=0": dict(M=0)}.items():
        f16s(label, EINVAL, **kw)
    for label, kw in {"M=100": dict(M=100), "K%32": dict(K=28), "n_cols%128": dict(n_cols=64), "ldc%8": dict(n_cols=128, ldc=132, n_C=M2 * 132)}.items():
        f16s(label, EUNSUPPORTED, **kw)

    def f16l(label, want, **kw):
        d = dict(A=ptr(Z), n_A=M2 * K2, lda=K2, M=M2, K=K2, n_cols=N2, Bh=ptr(Bh), Bh_bytes=Bh.numel(), a_f16=0, bias=ptr(bias2), n_bias=N2,
                 C=ptr(C32), n_C=M2 * N2, ldc=N2, n_store=N2, relu=0)
        d.update(kw)
        C32.fill_(float("nan"))
        rc = lib.dcs_debug_gemm_f16_longk(ctx._h, vp(d["A"]), d["n_A"], d["lda"], d["M"], d["K"], d["n_cols"], vp(d["Bh"]), d["Bh_bytes"], d["a_f16"],
                                          vp(d["bias"]), d["n_bias"], vp(d["C"]), d["n_C"], d["ldc"], d["n_store"], d["relu"])
        ctx.synchronize()
        res["f16 longk " + label] = dict(rc=rc, want=want, untouched=bool(torch.isnan(C32).all().item()), message_ok=True,
                                         message=lib.dcs_last_error().decode("utf-8", "replace"))

    f16l("short K", EUNSUPPORTED)
    for label, kw in {"null A": dict(A=None), "n_A short": dict(n_A=M2 * K2 - 1), "n_C short": dict(n_C=M2 * N2 - 1), "n_store>n_cols": dict(n_store=N2 + 1),
                      "n_bias short": dict(n_bias=N2 - 1), "Bh short": dict(Bh_bytes=Bh.numel() - 1), "ldc<n_store": dict(ldc=N2 - 1), "K=0": dict(K=0)}.items():
        f16l(label, EINVAL, **kw)

    # the pack entry
    src = torch.zeros(K * N, device="cuda")
    dst = torch.full((gr.pack_bytes(gr.PACK_SPLIT_A, K, 128) // 4,), float("nan"), device="cuda")

    def pk(label, want, kind=gr.PACK_BQ, s=src, n_src=K * N, K_=K, ld=N, n=N, p=None, d=dst, nbytes=None):
        dst.fill_(float("nan"))
        pp = (i64 * 4)(*(list(p) + [0] * (4 - len(p)))) if p is not None else None
        rc = lib.dcs_debug_gemm_pack(ctx._h, kind, vp(ptr(s)), n_src, K_, ld, n, pp, vp(ptr(d)), dst.numel() * 4 if nbytes is None else nbytes)
        ctx.synchronize()
        res["pack " + label] = dict(rc=rc, want=want, untouched=bool(torch.isnan(dst).all().item()), message_ok=True,
                                    message=lib.dcs_last_error().decode("utf-8", "replace"))

    pk("good", 0)
    pk("null src", EINVAL, s=None)
    pk("null dst", EINVAL, d=None)
    pk("kind 9", EINVAL, kind=9)
    pk("src short", EINVAL, n_src=K * N - 1)
    pk("ld<n", EINVAL, ld=N - 1)
    pk("dst short", EINVAL, nbytes=gr.pack_bytes(gr.PACK_BQ, K, N) - 1)
    pk("permutation wider than B", EINVAL, p=(5, 13))
    pk("bh without parameters", EINVAL, kind=gr.PACK_BH)
    pk("bh source wider than ld", EINVAL, kind=gr.PACK_BH, p=(5, 13, 8))
    pk("bias_cl source short", EINVAL, kind=gr.PACK_BIAS_CL, p=(30, 200, 32))
    pk("split_a rows past the source", EINVAL, kind=gr.PACK_SPLIT_A, n=128, ld=K, n_src=K * N, p=(100,), nbytes=gr.pack_bytes(gr.PACK_SPLIT_A, K, 128))
    hs, hd = np.zeros(K * N, dtype=np.float32), np.full(8 * 1024, np.nan, dtype=np.float32)   # the host packer takes host pointers
    rc = lib.dcs_debug_gemm_pack(ctx._h, gr.PACK_BFRAG, vp(hs.ctypes.data), hs.size, K, N, 56, None, vp(hd.ctypes.data), hd.nbytes)
    res["pack bfrag n%16"] = dict(rc=rc, want=EINVAL, untouched=bool(np.isnan(hd).all()), message_ok=True, message="")
    res["bytes of an unknown kind"] = dict(rc=int(lib.dcs_debug_gemm_bytes(11, K, N)), want=-1, untouched=True, message_ok=True, message="")
    res["last_kernel without a context"] = dict(rc=lib.dcs_debug_gemm_last_kernel(None, None, None), want=EINVAL, untouched=True,
                                                message_ok=True, message="")
    return res


_CHILD = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests'); "
          "import test_gpu_gemm_kernels as t; t.child(sys.argv[2], sys.argv[3])")


# ------------------------------------------------------------------------------------------------ the parent
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """switch set -> (arrays, report): three children side by side"""
    from test_gpu_parity import _run_children
    d = tmp_path_factory.mktemp("gemm_kernels")
    names = list(gr.SWITCHES)
    outs = [str(d / (name + ".npz")) for name in names]
    envs = [dict(gr.SWITCHES[name], DCS_WS_GUARD=str(G), DCS_WS_POISON=str(POISON)) for name in names]
    _run_children(_CHILD, [ROOT], envs, per_child_args=[(name, out) for name, out in zip(names, outs)])
    res = {}
    for name, out in zip(names, outs):
        z = np.load(out)
        res[name] = (z, json.loads(bytes(z["_report"]).decode()))
    return res


@pytest.mark.parametrize("case", gr.cases(), ids=lambda c: c["name"])
def test_gemm_kernel(runs, case):
    z, report = runs[case["switch"]]
    n_cu = report["_n_cu"]
    c = gr.resolve(case, n_cu)
    r = report[c["name"]]
    assert all(rc == 0 for rc in r["rc"]), r
    exp = gr.expected_kernel(c, n_cu)
    assert exp is not None, "the launcher declines this case by its own arithmetic"
    assert tuple(r["kernel"]) == tuple(exp), "ran %r, the launcher's arithmetic says %r" % (r["kernel"], exp)
    assert exp[0] in (case["want"] if isinstance(case["want"], set) else {case["want"]}), "kernel %d: not what the case is written for" % exp[0]
    assert r["nan"] == 0, "%d NaN in C: an operand was read past its end" % r["nan"]
    assert r["foreign_written"] == 0, "%d elements of C written outside rows < M, columns < n_store" % r["foreign_written"]
    assert r["same_twice"], "two launches on the same operands differ"
    assert r["scratch_guard"] == "" and r["scratch_blocks"] >= 0, r["scratch_guard"]
    assert r["red_zone_bytes_damaged"] == 0
    cls = gr.kernel_class(exp[0])
    if c["onehot"]:
        assert r["onehot_mismatch"] == 0, "%d outputs are not the row of B the one-hot row of A selects" % r["onehot_mismatch"]
        return
    inp = gr.inputs(c)
    assert c["M"] * c["n_store"] >= 1024
    for b in range(max(1, c["n_br"])):
        got = z["%s/%d" % (c["name"], b)]
        want, S, extra = gr.reference(c, inp, b, cls)
        e = gr.measure(got, want, S)
        e32 = gr.measure(gr.restatement(c, inp, b, cls), want, S)
        print("\n%s branch %d: kernel %d (%s) params %r: E %.3g, restatement %.3g, ratio %.2f, cap %.3g"
              % (c["name"], b, exp[0], cls, r["kernel"][1:], e, e32, e / e32 if e32 else float("inf"), (c["K"] + gr.cap_c(c, cls)) * gr.U))
        assert e <= gr.FACTOR * e32, "device %.3g, float32 restatement %.3g" % (e, e32)
        assert gr.inside_cap(got, want, S, extra, c, cls)


def test_every_kernel_code_is_reached(runs):
    seen = set()
    for name in runs:
        for key, r in runs[name][1].items():
            if not key.startswith("_"):
                seen.add(r["kernel"][0])
    assert seen >= gr.ALL_CODES, "never launched: %r" % sorted(gr.ALL_CODES - seen)


def test_f16_row_planes(runs):
    """gemm_split_a_f16_kernel: what dcs_launch_gemm_f16_skinny leaves in Ah_scratch, byte for byte"""
    z, report = runs["none"]
    n = 0
    for case in gr.cases():
        if case["via"] == "f16_skinny" and not case["onehot"]:
            c = gr.resolve(case, report["_n_cu"])
            want = gr.pack_split_a_f16(gr.inputs(c)["A"], c["M"], c["K"], 128 if c["M"] <= 128 else 176)
            assert np.array_equal(z[c["name"] + "/Ah"], want.view(np.uint16).reshape(-1)), c["name"]
            n += 1
    assert n >= 4


@pytest.mark.parametrize("pc", gr.pack_cases(), ids=lambda p: p[0])
def test_packer(runs, pc):
    name, kind, K, ld, n, p = pc
    z, report = runs["none"]
    r = report["_packs"][name]
    assert r["rc"] == 0 and r["red_zone_bytes_damaged"] == 0, r
    assert r["bytes"] == gr.pack_bytes(kind, K, n)
    k = [q[0] for q in gr.pack_cases()].index(name)
    want = gr.pack_want(kind, gr.pack_source(kind, K, ld, n, p, 300 + k), K, n, p)
    got = z["pack/" + name]
    assert got.size == want.nbytes
    assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint8).reshape(-1)), "%d bytes differ" % int(
        (got != np.ascontiguousarray(want).view(np.uint8).reshape(-1)).sum())


def test_entries_refuse_bad_arguments(runs):
    args = runs["none"][1]["_args"]
    assert len(args) > 80
    for label, r in args.items():
        assert r["rc"] == r["want"], (label, r)
        assert r["message_ok"], (label, r["message"])
        if r["want"] != 0:
            assert r["untouched"], label
