"""tests/gemm_ref.py checked on the CPU: what tests/test_gpu_gemm_kernels.py holds the GEMM kernels to must itself be right.

* the float64 reference is ``A @ B`` on plain operands and the gather of grouped, mapped and overlapping rows otherwise;
* every float32 restatement -- the yardstick -- is further than 0 from float64 (a yardstick of 0 would demand bit equality)
  and inside the a-priori cap of its class, on every case, over at least 1024 outputs;
* the packer restatements invert: unpacking recovers B (its f16 rounding for the f16 plane);
* ``expected_kernel`` sends every case to the kernel it was written for at 64, 104, 256 and 304 CUs, and the case tables
  between them name every ``DCS_GEMM_K_*`` code of include/dcs.h;
* the one-hot probe is exact in every restatement.
"""
import os
import re

import numpy as np
import pytest

import gemm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = (64, 104, 256, 304)


def _wanted(case):
    return case["want"] if isinstance(case["want"], set) else {case["want"]}


def test_codes_match_the_header():
    with open(os.path.join(ROOT, "include", "dcs.h")) as fh:
        text = fh.read()
    codes = {name: int(val) for name, val in re.findall(r"#define DCS_GEMM_K_(\w+) (\d+)", text)}
    assert len(codes) == 32 and set(codes.values()) == gr.ALL_CODES
    for name, val in codes.items():
        assert getattr(gr, "K_" + name) == val, name
    for name in ("VIA_ROWS", "VIA_SKINNY", "VIA_LONGK"):
        assert int(re.search(r"#define DCS_GEMM_%s (\d+)" % name, text).group(1)) == getattr(gr, name)
    for name, val in re.findall(r"#define DCS_GEMM_PACK_(\w+) (\d+)", text):
        assert getattr(gr, "PACK_" + name) == int(val), name


@pytest.mark.parametrize("n_cu", N_CUS)
def test_expected_kernel_sends_every_case_to_its_kernel(n_cu):
    for case in gr.cases():
        c = gr.resolve(case, n_cu)
        exp = gr.expected_kernel(c, n_cu)
        assert exp is not None, c["name"]
        assert exp[0] in _wanted(case), (c["name"], n_cu, exp)
        assert c["n_cols"] % 64 == 0 and c["ldb"] % 64 == 0 and 0 < c["n_store"] <= c["n_cols"] <= c["ldb"] and c["ldc"] >= c["n_store"]
        if not c["onehot"]:
            assert c["M"] * c["n_store"] >= 1024, c["name"]


@pytest.mark.parametrize("n_cu", N_CUS)
def test_case_tables_name_every_kernel_code(n_cu):
    seen = {sw: set() for sw in gr.SWITCHES}
    for case in gr.cases():
        seen[case["switch"]].add(gr.expected_kernel(gr.resolve(case, n_cu), n_cu)[0])
    assert seen["none"] == gr.ALL_CODES, sorted(gr.ALL_CODES - seen["none"])
    # with the bf16 pipe off, or the f32 K-split forced, the bf16 shapes fall to the f32 kernels
    assert seen["bf16_0"] and all(gr.kernel_class(k) == "f32" for k in seen["bf16_0"] | seen["ksplit3"])
    assert seen["ksplit3"] == {gr.K_KSPLIT_16, gr.K_KSPLIT_64}


def test_k_split_slices_at_256_cus():
    """the slice counts the issue's cases were chosen for"""
    by = {c["name"]: c for c in gr.cases()}
    assert gr.expected_kernel(gr.resolve(by["ksplit16"], 256), 256)[:3] == (gr.K_KSPLIT_16, 33, 512)       # 33 slices, the last 4 long
    assert gr.expected_kernel(gr.resolve(by["ksplit64_M52"], 256), 256)[:3] == (gr.K_KSPLIT_64, 33, 512)   # 33 (slice, tile) pairs
    assert gr.expected_kernel(gr.resolve(by["ksplit64_M100"], 256), 256)[1] * 4 % 8 != 0
    assert gr.expected_kernel(gr.resolve(by["ksplit3_M52"], 256), 256)[:3] == (gr.K_KSPLIT_64, 3, 5632)
    assert gr.resolve(by["bf16x3_2_K36"], 256)["M"] == 1035 and gr.resolve(by["bf16x3_4_K36"], 256)["M"] == 4107
    assert gr.bfrag_chunks(1560) == 100 and gr.bfrag_chunks(68) == 8 and gr.bfrag_chunks(64) == 4


def test_reference_is_the_contract():
    rng = np.random.RandomState(0)
    by = {c["name"]: c for c in gr.cases()}
    # plain operands: A @ B + bias
    c = gr.resolve(by["splitk_ldb"], 256)
    inp = gr.inputs(c)
    want, S, extra = gr.reference(c, inp, 0, "f32")
    A = np.stack([inp["A_flat"][r * c["lda"]:r * c["lda"] + c["K"]] for r in range(c["M"])]).astype(np.float64)
    plain = A @ inp["B"][0][:c["K"], :c["n_cols"]].astype(np.float64) + inp["bias"][0].astype(np.float64)
    assert np.array_equal(want, np.maximum(plain, 0) if c["relu"] else plain)
    assert not extra.any() and S.shape == want.shape and np.all(S >= np.abs(want))
    # grouped, mapped and overlapping rows: element by element
    for name in ("splitk_M20_N128_K1560", "splitk_rowmap", "splitk_overlap", "rows_1_128_K5"):
        c = gr.resolve(by[name], 256)
        inp = gr.inputs(c)
        want, S, _ = gr.reference(c, inp, 0, "f32")
        rows = gr.a_rows(c)
        if c["rowmap"]:
            assert np.array_equal(rows, inp["rowmap"]) and len(set(rows)) < c["M"] and np.all(np.diff(rows) <= 0)
        for r in rng.choice(c["M"], 5, replace=False):
            a = inp["A_flat"][rows[r] * c["lda"]:rows[r] * c["lda"] + c["K"]].astype(np.float64) * np.float64(np.float32(c["a_scale"]))
            v = a @ inp["B"][0][:c["K"], :c["n_store"]].astype(np.float64)
            if inp["bias"][0] is not None:
                v = v + inp["bias"][0]
            assert np.all(np.abs(want[r] - (np.maximum(v, 0) if c["relu"] else v)) <= 1e-13 * S[r])
        assert inp["A_mask"].all() == (c["lda"] <= c["K"] and c["a_gdiv"] >= c["M"])   # poison only where nobody reads
    # the f16 reference multiplies by the weights as the packer rounds them
    c = gr.resolve(by["f16_skinny_M150_K256_N128_br1"], 256)
    inp = gr.inputs(c)
    w = gr.weights64(c, inp["B"][0], "f16")
    assert np.array_equal(w, inp["B"][0][:c["K"], :c["n_cols"]].astype(np.float16).astype(np.float64)) and not np.array_equal(
        w, inp["B"][0][:c["K"], :c["n_cols"]])
    # inputs: zero rows and columns in B, zero rows in A, zero padding, scales over 2^-4 .. 2^4
    B = inp["B"][0]
    assert not B[c["K"]:].any() and not B[7].any() and not B[:, 3].any() and not inp["A"][5].any()
    sd = inp["A"].std(axis=1)
    assert sd[sd > 0].max() / sd[sd > 0].min() > 30


def _figures(case):
    c = gr.resolve(case, 256)
    cls = gr.kernel_class(gr.expected_kernel(c, 256)[0])
    inp = gr.inputs(c)
    out = []
    for b in range(max(1, c["n_br"])):
        want, S, extra = gr.reference(c, inp, b, cls)
        rest = gr.restatement(c, inp, b, cls)
        out.append((c, cls, want, S, extra, rest))
    return out


@pytest.mark.parametrize("case", [c for c in gr.cases() if not c["onehot"]], ids=lambda c: c["name"])
def test_restatement_is_a_yardstick(case):
    for c, cls, want, S, extra, rest in _figures(case):
        assert want.size >= 1024 and np.isfinite(rest).all() and np.isfinite(want).all()
        e = gr.measure(rest, want, S)
        assert 0 < e < np.inf, e
        assert gr.inside_cap(rest, want, S, extra, c, cls), (e, (c["K"] + gr.cap_c(c, cls)) * gr.U)
        if cls != "f16":
            assert e <= (c["K"] + gr.cap_c(c, cls)) * gr.U
        # and a reference with one k dropped is far outside what the restatement allows
        k = c["K"] // 2
        a = np.abs(gr.inputs(c)["A"][:, k].astype(np.float64) * c["a_scale"])[:, None] * np.abs(gr.weights64(c, gr.inputs(c)["B"][0], cls)[k])[None, :]
        if a.any() and not c["relu"]:
            assert np.max(a[S > 0] / S[S > 0]) > 100 * gr.FACTOR * e


@pytest.mark.parametrize("case", [c for c in gr.cases() if c["onehot"]], ids=lambda c: c["name"])
def test_one_hot_probe_is_exact_in_the_restatement(case):
    c = gr.resolve(case, 256)
    if c["M"] * c["n_store"] * c["K"] > 1 << 27:
        c = dict(c, M=min(c["M"], 180), n_store=min(c["n_store"], 256))       # the same arithmetic on a corner of the case
    cls = gr.kernel_class(gr.expected_kernel(gr.resolve(case, 256), 256)[0])
    inp = gr.inputs(c)
    for b in range(max(1, c["n_br"])):
        want = gr.onehot_want(c, inp, b, cls)
        rest = gr.restatement(c, inp, b, cls)
        assert np.array_equal(rest.astype(want.dtype).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
        assert np.count_nonzero(want) > want.size // 3                      # (the f16 all-rows kernel rectifies)


def test_split_is_exact_and_truncating():
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(4096) * 2.0 ** rng.uniform(-20, 20, 4096)).astype(np.float32)
    hi, mid, lo = gr.split3(x)
    assert np.array_equal((lo + mid) + hi, x)
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & 0xffff).any()
    assert np.all(np.abs(hi) <= np.abs(x)) and np.all(np.abs(x - hi) < np.abs(x) * 2.0 ** -7 + 1e-45)


@pytest.mark.parametrize("pc", gr.pack_cases(), ids=lambda p: p[0])
def test_packer_restatements_invert(pc):
    name, kind, K, ld, n, p = pc
    src = gr.pack_source(kind, K, ld, n, p, 7)
    out = gr.pack_want(kind, src, K, n, p)
    assert out.nbytes == gr.pack_bytes(kind, K, n)
    assert not np.isnan(out.view(np.float16 if kind in (gr.PACK_BH, gr.PACK_BH_PLAIN) else np.float32) if kind not in (gr.PACK_BQ, gr.PACK_SPLIT_A)
                        else gr.unpack_bq(out, K, n)[0]).any(), "the restatement read a column nobody may read"
    if kind in (gr.PACK_BQ, gr.PACK_B32):
        perm = gr._perm(n, *(p or (0, 0)))
        assert sorted(perm) == list(range(n))
        B = src[:K, :n][:, perm]
        if kind == gr.PACK_BQ:
            back, parts = gr.unpack_bq(out, K, n)
            assert np.array_equal(back, B)
            assert np.array_equal(parts[0].view(np.uint32), B.view(np.uint32) & 0xffff0000)           # truncation
            if K % 32:
                assert not out[-1, :, :, (K % 32 + 7) // 8:].any()                                    # zero past K
        else:
            assert np.array_equal(gr.unpack_b32(out, K, n), B)
    elif kind in (gr.PACK_BH, gr.PACK_BH_PLAIN):
        nch, npos, chpad = p or (1, n, 1)
        back = gr.unpack_bh(out, K, n)
        for ch in range(nch):
            for pos in range(0, min(npos, n // chpad), 3):
                assert np.array_equal(back[:, pos * chpad + ch], src[:K, ch * npos + pos].astype(np.float16))
        pad = [(j // chpad >= npos) or (j % chpad >= nch) for j in range(n)]
        assert not back[:, pad].any()
    elif kind == gr.PACK_BIAS_CL:
        nch, npos, chpad = p
        for j in range(n):
            pos, ch = j // chpad, j % chpad
            assert out[j] == (src[ch * npos + pos] if pos < npos and ch < nch else 0)
    elif kind == gr.PACK_SPLIT_A:
        back, _ = gr.unpack_bq(out, K, n)                                                            # [K][rows_pad]
        assert np.array_equal(back[:, :p[0]].T, src[:p[0], :K]) and not back[:, p[0]:].any()
    else:
        assert out.shape == (n // 16, gr.bfrag_chunks(K), 64, 4)
        assert np.array_equal(gr.unpack_bfrag(out, K, n), src[:K, :n])
        assert not out.reshape(n // 16, -1, 4, 16, 4)[:, K // 16 + 1:].any()                         # chunks past K zero
        # lane (kq, fi) of column block t and chunk c holds B[16 c + 4 kq + e][16 t + fi]
        assert out[1, 2, 37, 3] == src[16 * 2 + 4 * 2 + 3, 16 + 5]


def test_f16_row_planes_restatement():
    rng = np.random.RandomState(5)
    A = (rng.standard_normal((150, 64)) * 2.0 ** rng.uniform(-4, 4, (150, 1))).astype(np.float32)
    P = gr.pack_split_a_f16(A, 150, 64, 176)
    assert P.shape == (2, 2, 176, 4, 8) and P.nbytes == gr.pack_bytes(gr.PACK_SPLIT_A_F16, 64, 176)
    hi = P[:, 0].transpose(0, 2, 3, 1).reshape(64, 176).astype(np.float32)
    lo = P[:, 1].transpose(0, 2, 3, 1).reshape(64, 176).astype(np.float32)
    assert not hi[:, 150:].any() and not lo[:, 150:].any()
    assert np.all(np.abs((hi + lo)[:, :150].T - A) <= np.abs(A) * 2.0 ** -22 + 2.0 ** -25)
