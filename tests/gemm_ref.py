"""Shared by tests/test_gemm_ref_cpu.py and tests/test_gpu_gemm_kernels.py (test infrastructure): the GEMM kernels and operand
packers of csrc/gemm.hip, csrc/gemm_bf16x3.hip and csrc/gemm_f16.hip held directly to float64.

The contract (csrc/dcs_internal.h): ``C[crow(r)][0..n_store) = act(a_scale * A[arow(r)][0..K) . B + bias)``.

* ``reference`` -- the contract in float64 (for the f16 kernels with the weights as ``gemm_pack_bh_kernel`` rounds them: a
  ``(_Float16)`` conversion, round to nearest even, which is numpy's ``astype(float16)``);
* ``restatement`` -- the same in float32, per kernel class, the yardstick of the device's distance from float64:
  ``f32`` k ascending; ``bf16x3`` three truncated bf16 terms per operand, the six products above 2^-24 of a 32-wide k tile
  added to a float32 accumulator, smallest first; ``f16`` A as two f16 terms (one when the rows arrive as f16), B in f16,
  float32 accumulation per k tile, and for the all-rows kernel one rounding of the result to f16;
* the measure ``E = max_ij |got - want| / S_ij`` with ``S_ij = sum_k |a_scale a_ik b_kj| + |bias_j|`` in float64.  A kernel
  passes when ``E <= FACTOR * E(restatement)`` (over the whole output of the case, never fewer than 1024 elements) and when
  every element is inside the a-priori cap ``|got - want| <= (K + c) 2^-24 S_ij + extra_ij``:

  - ``f32`` (``v_mfma_f32_16x16x4_f32`` is an fmaf chain, k ascending): a term passes through at most K roundings of the
    chain -- with K slices, at most kchunk of its slice's chain and one per slice added behind it, kchunk + ksplit <= K for
    K >= 16384 -- plus one for ``a_scale * a``, one for the bias, one for ``acc0 + acc1`` and three for the four waves'
    partial sums of the few-rows kernel, one for the product that numpy rounds and the chain does not: c = 8, plus
    ``ceil(K^2 2^-24)`` for the second-order term of ``(1 + u)^K``;
  - ``bf16x3``: the documented ``3 * 2^-24`` for the three dropped products; the matrix instruction adds 32 products and the
    accumulator in an order that is not specified -- at most 33 roundings inside the instruction a term enters with, then 6
    accumulations per later k tile, 6 K / 32 + 6 + 33 <= K + 39: c = 8 + 3 + 39 = 50 (plus the second-order term).  Only the yardstick is sharp here;
  - ``f16``: a = hi + lo to 22 bits drops at most 2^-22 |a|, 4 more, and the matrix instruction's 39 as above: c = 8 + 4 +
    39 = 51.  Where lo falls below f16's normal range it is rounded to a multiple of 2^-24: ``extra_ij = 2^-25 sum_k
    |b_kj|`` (not when the rows arrive as f16).  An f16 output adds one f16 rounding of ``|want_ij|``: ``2^-11 |want_ij| +
    2^-25``.

* exact probes: one-hot rows (``A[r][(7 r + 3) mod K] = 1``, and ``A[r][(K - 1 - 7 r) mod K] = 1`` for the end of K: the
  output row is a row of B, bit for bit), every case twice
  with identical bits, the packers byte for byte against ``pack_*`` below;
* ``expected_kernel`` -- the launchers' selection arithmetic (``dcs_launch_gemm_rows``, ``dcs_launch_gemm_bf16x3*``,
  ``dcs_launch_gemm_f16_*``), K-split slice counts included;
* the case tables, as functions of the CU count.
"""
import numpy as np

FACTOR = 4.0                          # a reordered float32 sum against the in-order one (tests/stft_ref.py, tests/test_gpu_mwf.py)
U = 2.0 ** -24

# kernel codes of include/dcs.h (dcs_debug_gemm_last_kernel)
K_ROWS_1_128, K_ROWS_1_128_VEC, K_ROWS_1_32, K_ROWS_1_32_VEC, K_ROWS_2_32, K_ROWS_2_32_VEC, K_ROWS_4_32, K_ROWS_4_32_VEC = range(1, 9)
K_SPLITK, K_SPLITK_BFRAG, K_KSPLIT_16, K_KSPLIT_64, K_BF16X3_2, K_BF16X3_4 = range(9, 15)
K_SKINNY_8, K_SKINNY_8_AQ, K_SKINNY_8_B32, K_SKINNY_8_AQ_B32, K_SKINNY_11, K_SKINNY_11_AQ, K_SKINNY_11_B32, K_SKINNY_11_AQ_B32 = range(15, 23)
K_LONGK_8, K_LONGK_8_B32, K_LONGK_11, K_LONGK_11_B32 = range(23, 27)
K_F16_SKINNY_8, K_F16_SKINNY_11, K_F16_LONGK_8, K_F16_LONGK_8_A16, K_F16_LONGK_11, K_F16_LONGK_11_A16 = range(27, 33)
ALL_CODES = set(range(1, 33))
VIA_ROWS, VIA_SKINNY, VIA_LONGK = 0, 1, 2
PACK_BQ, PACK_B32, PACK_BH, PACK_BH_PLAIN, PACK_BIAS_CL, PACK_SPLIT_A, PACK_BFRAG, PACK_SPLIT_A_F16 = range(8)

SWITCHES = {"none": {}, "bf16_0": {"DCS_GEMM_BF16": "0"}, "ksplit3": {"DCS_GEMM_KSPLIT": "3"}}
FLAT = 1 << 30                        # a_gdiv / c_gdiv of an operand with one group


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


def kernel_class(code):
    if code <= K_KSPLIT_64:
        return "f32"
    return "bf16x3" if code <= K_LONGK_11_B32 else "f16"


# ------------------------------------------------------------------------------------------------ selection arithmetic
def _skinny(c):
    if c["switch"] == "bf16_0" or not c["bq"] or not c["a_vec"] or c["K"] % 4 or c["lda"] % 4:
        return None
    if c["M"] < 128 or c["M"] > 176 or c["n_cols"] < 8192 or c["ldc"] % 4:
        return None
    rbt = 8 if c["M"] <= 128 else 11
    aq = bool(c["aq"]) and c["aq_rows"] == rbt * 16 and c["a_scale"] == 1.0 and c["a_gdiv"] >= c["M"]
    return ((K_SKINNY_8 if rbt == 8 else K_SKINNY_11) + int(aq) + 2 * int(c["bq"] == "b32"), 0, 0, rbt, int(aq))


def _longk_slices(M, K, n_cols, n_cu):
    if M < 128 or M > 176 or n_cols % 128 or n_cols > 1024 or K < 16384 or K % 4:
        return 0, 0
    col_wgs, nkt = n_cols // 128, cdiv(K, 32)
    ksplit = min(cdiv(2 * n_cu, col_wgs), nkt)
    kts = cdiv(nkt, ksplit)
    ksplit = cdiv(nkt, kts)
    return (ksplit, kts) if ksplit >= 2 else (0, 0)


def _longk(c, n_cu):
    if c["switch"] == "bf16_0" or not c["bq"] or not c["a_vec"] or c["rowmap"] or c["K"] % 4 or c["lda"] % 4:
        return None
    ksplit, kts = _longk_slices(c["M"], c["K"], c["n_cols"], n_cu)
    if not ksplit:
        return None
    rbt = 8 if c["M"] <= 128 else 11
    return ((K_LONGK_8 if rbt == 8 else K_LONGK_11) + int(c["bq"] == "b32"), ksplit, kts * 32, rbt, 0)


def _bf16x3(c, n_cu):
    if c["switch"] == "bf16_0" or not c["bq"] or not c["a_vec"] or c["K"] % 4 or c["lda"] % 4:
        return None
    if c["bq"] == "b32":
        return _skinny(c)
    groups16, col_groups = cdiv(c["M"], 16), c["n_cols"] // 64
    if groups16 * col_groups <= 4 * n_cu or c["n_cols"] < 1024 or c["M"] < 128:
        return None
    s = _skinny(c)
    if s:
        return s
    return (K_BF16X3_2, 0, 0, 2, 0) if groups16 * col_groups <= 16 * n_cu else (K_BF16X3_4, 0, 0, 4, 0)


def expected_kernel(c, n_cu):
    """(code, ksplit, kchunk, row blocks of 16, Aq used) of a resolved case; None where the launcher declines"""
    M, K, n_cols = c["M"], c["K"], c["n_cols"]
    if c["via"] == "skinny":
        return _skinny(c)
    if c["via"] == "longk":
        return _longk(c, n_cu)
    if c["via"] == "f16_skinny":
        if M < 128 or M > 176 or n_cols % 128 or K < 32 or K % 32 or c["ldc"] % 8:
            return None
        return (K_F16_SKINNY_8 if M <= 128 else K_F16_SKINNY_11, 0, 0, 8 if M <= 128 else 11, 0)
    if c["via"] == "f16_longk":
        ksplit, kts = _longk_slices(M, K, n_cols, n_cu)
        if not ksplit or (c["a_f16"] and (c["lda"] % 32 or K != c["lda"])) or (not c["a_f16"] and c["lda"] % 4):
            return None
        return ((K_F16_LONGK_8 if M <= 128 else K_F16_LONGK_11) + int(c["a_f16"]), ksplit, kts * 32, 8 if M <= 128 else 11, 0)
    assert c["via"] == "rows"
    if not c["rowmap"]:
        b = _bf16x3(c, n_cu)
        if b:
            return b
    groups16, col_groups = cdiv(M, 16), n_cols // 64
    ks_env = 3 if c["switch"] == "ksplit3" else -1
    tiles16 = groups16 * (n_cols // 16)
    if c["a_vec"] and K >= 16384 and tiles16 < 4 * n_cu:
        if ks_env < 0:
            lk = _longk(c, n_cu)
            if lk:
                return lk
        tiled = M >= 48
        units = cdiv(M, 64) * col_groups if tiled else tiles16
        ksplit = ks_env if ks_env > 0 else cdiv((3 if tiled else 8) * n_cu, units)
        ksplit = min(ksplit, 64)
        kchunk = round_up(cdiv(K, ksplit), 256)
        ksplit = cdiv(K, kchunk)
        if ksplit > 1:
            return (K_KSPLIT_64 if tiled else K_KSPLIT_16, ksplit, kchunk, 4 if tiled else 1, 0)
    v = int(bool(c["a_vec"]))
    if c["a_vec"] and groups16 * col_groups <= n_cu // 2:
        return (K_SPLITK_BFRAG if c["bfrag"] else K_SPLITK, 0, 0, 1, 0)
    if groups16 * col_groups <= 2 * n_cu:
        return (K_ROWS_1_128 + v, 0, 0, 1, 0)
    if groups16 * col_groups <= 4 * n_cu:
        return (K_ROWS_1_32 + v, 0, 0, 1, 0)
    if groups16 * col_groups <= 16 * n_cu:
        return (K_ROWS_2_32 + v, 0, 0, 2, 0)
    return (K_ROWS_4_32 + v, 0, 0, 4, 0)


def bfrag_chunks(K):
    return ((K + 63) >> 6) * 4


# ------------------------------------------------------------------------------------------------ case tables
def _case(name, want, via="rows", switch="none", M=20, K=68, n_cols=64, n_store=None, lda=None, ldc=None, ldb=None, a_vec=1, relu=0,
          bias=True, a_scale=1.0, a_gdiv=FLAT, a_gmul=0, c_gdiv=FLAT, c_gmul=0, rowmap=False, bq=None, aq=False, aq_rows=None,
          bfrag=False, n_br=0, a_f16=False, seed=0):
    """M and n_cols may be functions of the CU count.  want: the kernel code(s) the case is written for (a set: the code
    differs with the CU count only in the row-block count named by the case)"""
    return dict(name=name, want=want, via=via, switch=switch, M=M, K=K, n_cols=n_cols, n_store=n_store, lda=lda, ldc=ldc, ldb=ldb,
                a_vec=a_vec, relu=relu, bias=bias, a_scale=a_scale, a_gdiv=a_gdiv, a_gmul=a_gmul, c_gdiv=c_gdiv, c_gmul=c_gmul,
                rowmap=rowmap, bq=bq, aq=aq, aq_rows=aq_rows, bfrag=bfrag, n_br=n_br, a_f16=a_f16, seed=seed, onehot=False)


def _past(mult, div, col_groups):
    """rows of the first 16-row group count whose launch has more than mult * n_cu / div workgroup columns, minus 5"""
    return lambda n_cu: 16 * (mult * n_cu // div // col_groups + 1) - 5


def _fill_cols(n_cu):
    """the narrowest B of at least 8256 columns with which 128 rows pass the bf16 launcher's fill test"""
    return max(8256, 64 * (4 * n_cu // 8 + 1))


def base_cases():
    G = dict(a_gdiv=7, a_gmul=9)
    GC = dict(c_gdiv=7, c_gmul=9)
    c = []
    # few rows: one 16 x 16 tile per workgroup, K dealt to four waves
    for i, (M, n_cols, K) in enumerate([(1, 1024, 4), (20, 64, 68), (33, 128, 324), (20, 128, 1560), (33, 64, 1560)]):
        c.append(_case("splitk_M%d_N%d_K%d" % (M, n_cols, K), K_SPLITK, M=M, n_cols=n_cols, K=K, relu=i & 1, bias=i != 1,
                       a_scale=0.3 if i == 2 else 1.0, seed=10 + i, lda=K + 4 * (i % 3), **(G if i == 3 else {})))
    c.append(_case("splitk_rowmap", K_SPLITK, M=33, n_cols=64, K=324, rowmap=True, n_store=41, seed=16, **GC))
    c.append(_case("splitk_overlap", K_SPLITK, M=20, n_cols=64, K=324, lda=12, relu=1, seed=17))
    c.append(_case("splitk_ldb", K_SPLITK, M=20, n_cols=64, K=68, ldb=128, ldc=70, seed=18))
    for i, K in enumerate((68, 1560)):
        c.append(_case("splitk_bfrag_K%d" % K, K_SPLITK_BFRAG, M=33, n_cols=128, K=K, bfrag=True, relu=i, a_scale=(1.0, 0.3)[i],
                       seed=20 + i))
    # a_vec = 0
    c.append(_case("rows_1_128_K131", K_ROWS_1_128, M=20, K=131, lda=133, a_vec=0, n_store=53, seed=30, relu=1))
    c.append(_case("rows_1_128_K5", K_ROWS_1_128, M=20, K=5, lda=7, a_vec=0, n_cols=128, seed=31, a_scale=0.3, **G))
    c.append(_case("rows_1_128_rowmap", K_ROWS_1_128, M=20, K=131, lda=131, a_vec=0, rowmap=True, bias=False, seed=32))
    c.append(_case("rows_1_32_novec", K_ROWS_1_32, M=_past(2, 1, 1), K=35, lda=37, a_vec=0, seed=33))
    c.append(_case("rows_2_32_novec", K_ROWS_2_32, M=_past(4, 1, 2), K=35, lda=35, n_cols=128, a_vec=0, relu=1, seed=34))
    c.append(_case("rows_4_32_novec", K_ROWS_4_32, M=_past(16, 1, 4), K=33, lda=33, n_cols=256, a_vec=0, bias=False, seed=35))
    # the thresholds of the vector path
    c.append(_case("rows_1_128_vec", K_ROWS_1_128_VEC, M=_past(1, 2, 1), K=132, lda=136, relu=1, seed=40, **GC))
    c.append(_case("rows_1_128_vec_overlap", K_ROWS_1_128_VEC, M=_past(1, 2, 1), K=132, lda=4, a_scale=0.3, seed=41))
    c.append(_case("rows_1_32_vec", K_ROWS_1_32_VEC, M=_past(2, 1, 1), K=36, n_store=27, seed=42, **G))
    c.append(_case("rows_2_32_vec", K_ROWS_2_32_VEC, M=_past(4, 1, 2), K=36, n_cols=128, rowmap=True, relu=1, seed=43))
    c.append(_case("rows_4_32_vec", K_ROWS_4_32_VEC, M=_past(16, 1, 4), K=36, n_cols=256, a_scale=0.3, bias=False, seed=44))
    # K split over workgroups, two passes
    c.append(_case("ksplit16", K_KSPLIT_16, M=20, n_cols=64, K=16388, relu=1, seed=50, **G))
    c.append(_case("ksplit16_rowmap", K_KSPLIT_16, M=33, n_cols=64, K=16388, rowmap=True, n_store=50, a_scale=0.3, seed=51))
    c.append(_case("ksplit64_M52", K_KSPLIT_64, M=52, n_cols=64, K=16388, seed=52, bias=False, **GC))
    c.append(_case("ksplit64_M100", K_KSPLIT_64, M=100, n_cols=128, K=16388, relu=1, n_store=100, seed=53))
    c.append(_case("ksplit3_M52", K_KSPLIT_64, switch="ksplit3", M=52, n_cols=64, K=16388, relu=1, seed=54))
    c.append(_case("ksplit3_M20", K_KSPLIT_16, switch="ksplit3", M=20, n_cols=64, K=16388, a_scale=0.3, seed=55))
    c.append(_case("ksplit3_longk_shape", K_KSPLIT_64, switch="ksplit3", M=130, n_cols=128, K=16388, bq="bq", seed=56))
    # bf16 x 3, 64-column tiles
    for i, K in enumerate((36, 100, 68)):
        c.append(_case("bf16x3_2_K%d" % K, K_BF16X3_2, M=_past(1, 4, 1), n_cols=1024, K=K, bq="bq", relu=i & 1, bias=i != 2,
                       a_scale=0.3 if i == 1 else 1.0, n_store=1024 - 37 * (i == 0), seed=60 + i, lda=K + 4 * i, **(G if i == 2 else {})))
    c.append(_case("bf16x3_4_K36", K_BF16X3_4, M=_past(1, 1, 1), n_cols=1024, K=36, bq="bq", relu=1, seed=64, **GC))
    c.append(_case("bf16x3_4_K100", K_BF16X3_4, M=_past(1, 1, 1), n_cols=1024, K=100, bq="bq", a_scale=0.3, lda=20, seed=65))
    c.append(_case("bf16_0_tiles2", {K_ROWS_2_32_VEC}, switch="bf16_0", M=_past(1, 4, 1), n_cols=1024, K=68, bq="bq", seed=66))
    c.append(_case("bf16_0_tiles4", {K_ROWS_4_32_VEC}, switch="bf16_0", M=_past(1, 1, 1), n_cols=1024, K=36, bq="bq", relu=1, seed=67))
    # all rows in one workgroup
    sk = [
        # M, n_cols, K, n_br, aq, bq, extra
        (128, _fill_cols, 36, 0, False, "bq", dict(relu=1)),
        (128, 8192, 256, 0, True, "bq", dict()),
        (128, 8192, 36, 4, True, "b32", dict(relu=1, lda=40)),
        (128, 8256, 36, 1, False, "b32", dict(a_scale=0.3, aq=True)),          # a_scale != 1 switches Aq off
        (129, 8256, 36, 0, False, "bq", dict(bias=False, **G)),
        (150, 8192, 256, 0, True, "bq", dict(relu=1)),
        (150, 8192, 36, 0, False, "b32", dict(lda=20, **GC)),
        (176, 8256, 36, 4, False, "bq", dict(a_scale=0.3)),
        (176, 8192, 36, 1, True, "b32", dict()),
        (176, 8256, 256, 0, False, "b32", dict(relu=1, lda=260)),
        (150, 8256, 36, 0, True, "bq", dict(aq_rows=128)),                     # planes made for another row tiling: not used
    ]
    for i, (M, n_cols, K, n_br, aq, bq, extra) in enumerate(sk):
        rbt = 8 if M <= 128 else 11
        kw = dict(M=M, n_cols=n_cols, K=K, n_br=n_br, aq=aq, bq=bq, seed=70 + i)
        kw.update(extra)
        used = kw["aq"] and kw.get("aq_rows", rbt * 16) == rbt * 16 and kw.get("a_scale", 1.0) == 1.0 and "a_gdiv" not in kw
        code = (K_SKINNY_8 if rbt == 8 else K_SKINNY_11) + int(used) + 2 * int(bq == "b32")
        via = "rows" if (n_br == 0 and i in (0, 5, 6)) else "skinny"
        nn = n_cols if callable(n_cols) else (lambda n_cu, n=n_cols: n)
        kw["n_cols"] = nn
        kw["n_store"] = lambda n_cu, nn=nn: nn(n_cu) - 37
        c.append(_case("skinny_%d_M%d_K%d_br%d_%s%s_%s" % (i, M, K, n_br, bq, "_aq" if kw["aq"] else "", via), code, via=via, **kw))
    # 128 rows against exactly 8192 columns: the fill test of the bf16 launcher declines, the f32 tiles take it
    # (with fewer than 256 CUs 8 x 128 workgroup columns fill the chip and the all-rows kernel runs)
    c.append(_case("skinny_declined_M128", {K_ROWS_1_32_VEC, K_SKINNY_8}, M=128, n_cols=lambda n_cu: max(8192, 64 * (4 * n_cu // 8)), K=36,
                   bq="bq", seed=85))
    c.append(_case("bf16_0_skinny_shape", {K_ROWS_2_32_VEC, K_ROWS_4_32_VEC}, switch="bf16_0", M=150, n_cols=8192, K=36, bq="bq", seed=86))
    # long K on the bf16 pipe
    c.append(_case("longk_M130_bq", K_LONGK_11, via="longk", M=130, n_cols=128, K=16388, bq="bq", relu=1, seed=90))
    c.append(_case("longk_M176_b32", K_LONGK_11_B32, via="rows", M=176, n_cols=128, K=16388, bq="b32", n_store=91, a_scale=0.3, seed=91, **GC))
    c.append(_case("longk_M128_bq", K_LONGK_8, via="rows", M=128, n_cols=128, K=16388, bq="bq", bias=False, seed=92))
    c.append(_case("longk_M128_b32", K_LONGK_8_B32, via="longk", M=128, n_cols=256, K=16388, bq="b32", relu=1, seed=93, **G))
    c.append(_case("bf16_0_longk_shape", K_KSPLIT_64, switch="bf16_0", M=130, n_cols=128, K=16388, bq="b32", relu=1, seed=94))
    # f16
    f16 = [(128, 32, 128, 1), (128, 256, 384, 4), (150, 256, 128, 1), (176, 32, 384, 4), (150, 32, 128, 1)]
    for i, (M, K, n_cols, n_br) in enumerate(f16):
        c.append(_case("f16_skinny_M%d_K%d_N%d_br%d" % (M, K, n_cols, n_br), K_F16_SKINNY_8 if M <= 128 else K_F16_SKINNY_11,
                       via="f16_skinny", M=M, K=K, n_cols=n_cols, n_br=n_br, relu=1, lda=K + 8 * (i & 1), ldc=n_cols + 8 * (i & 1), seed=100 + i))
    c.append(_case("f16_longk_M130_a16", K_F16_LONGK_11_A16, via="f16_longk", M=130, n_cols=128, K=16416, a_f16=True, relu=1, seed=110))
    c.append(_case("f16_longk_M128_a16", K_F16_LONGK_8_A16, via="f16_longk", M=128, n_cols=128, K=16416, a_f16=True, n_store=100, seed=111))
    c.append(_case("f16_longk_M130_f32", K_F16_LONGK_11, via="f16_longk", M=130, n_cols=128, K=16388, relu=1, lda=16392, bias=False, seed=112))
    c.append(_case("f16_longk_M128_f32", K_F16_LONGK_8, via="f16_longk", M=128, n_cols=256, K=16388, n_store=200, seed=113))
    return c


def cases():
    """every case, and behind each its one-hot twins: plain rows (no map, no overlap), a_scale = 1, no bias, no rectifier.
    "head": A[r][(7 r + 3) mod K] = 1; "tail": A[r][(K - 1 - 7 r) mod K] = 1 -- with few rows the first probes only the first
    7 M of K, the second the last k tile, chunk and slice, where the tails are."""
    out = []
    for c in base_cases():
        out.append(c)
        t = dict(c, name=c["name"] + "_onehot", onehot="head", a_scale=1.0, bias=False, relu=0, rowmap=False)
        if c["lda"] is not None and c["lda"] < c["K"]:
            t["lda"] = None
        if c["via"] == "f16_skinny":
            t["relu"] = 1                                                    # that kernel always rectifies
        if c["a_scale"] != 1.0 and c["aq"] and c["aq_rows"] is None:        # the twin's Aq planes are taken
            t["want"] = c["want"] + 1
        out.append(t)
        out.append(dict(t, name=c["name"] + "_onehot_tail", onehot="tail"))
    return out


def resolve(c, n_cu):
    """the case with every CU-dependent figure and every default filled in"""
    c = dict(c)
    for k in ("M", "n_cols", "n_store"):
        if callable(c[k]):
            c[k] = c[k](n_cu)
    if c["n_store"] is None:
        c["n_store"] = c["n_cols"]
    if c["lda"] is None:
        c["lda"] = c["K"]
    if c["ldb"] is None:
        c["ldb"] = c["n_cols"]
    if c["ldc"] is None:
        c["ldc"] = c["n_cols"] if c["n_store"] == c["n_cols"] else c["n_store"] + 3 + (-(c["n_store"] + 3)) % 4
    if c["aq_rows"] is None:
        c["aq_rows"] = 128 if c["M"] <= 128 else 176
    return c


# ------------------------------------------------------------------------------------------------ inputs
def row_index(M, gdiv, gmul):
    r = np.arange(M, dtype=np.int64)
    return r if gdiv >= M else (r // gdiv) * gmul + r % gdiv


def onehot_k(c):
    """the column of A's one in every row of a one-hot twin"""
    r = np.arange(c["M"])
    return (7 * r + 3) % c["K"] if c["onehot"] == "head" else (c["K"] - 1 - 7 * r) % c["K"]


def a_rows(c):
    """storage row of every logical row of A"""
    if c["rowmap"]:
        return (c["M"] - 1 - np.arange(c["M"], dtype=np.int64)) // 2        # descending, every row twice
    return row_index(c["M"], c["a_gdiv"], c["a_gmul"])


def inputs(c):
    """A resolved case's operands.  A: flat storage (float32, or float16 for the f16 rows) and the mask of the elements that are
    data (the rest stays poison); B [round_up(K, 128)][ldb] with zero padding rows and NaN in the columns past n_cols; bias per
    branch; the logical A [M][K]."""
    rng = np.random.RandomState(1000 + c["seed"] + (500 if c["onehot"] else 0))
    M, K, lda, n_cols = c["M"], c["K"], c["lda"], c["n_cols"]
    rows = a_rows(c)
    n_A = int(rows.max()) * lda + K
    idx = rows[:, None] * lda + np.arange(K)[None, :]
    mask = np.zeros(n_A, dtype=bool)
    mask[idx.reshape(-1)] = True
    blk = np.arange(n_A) // max(lda, 1)
    scale = 2.0 ** rng.uniform(-4, 4, size=int(blk.max()) + 1)
    scale[5::11] = 0.0                                                       # some rows all zero
    if c["onehot"]:
        flat = np.zeros(n_A, dtype=np.float32)
        flat[rows * lda + onehot_k(c)] = 1.0
    else:
        flat = (rng.standard_normal(n_A) * scale[blk] + 0.0).astype(np.float32)
    if c["a_f16"]:
        flat = flat.astype(np.float16)
    nb = max(1, c["n_br"])
    Kp = round_up(K, 128)
    Bs, biases = [], []
    for b in range(nb):
        B = np.zeros((Kp, c["ldb"]), dtype=np.float32)
        cs = 2.0 ** rng.uniform(-4, 4, size=n_cols)
        cs[3::17] = 0.0
        body = rng.standard_normal((K, n_cols)) * cs[None, :] + 0.0          # (+ 0: the zero columns hold +0, not -0)
        body[7::13] = 0.0
        B[:K, :n_cols] = body
        B[:, n_cols:] = np.nan
        Bs.append(B)
        if c["via"] == "f16_skinny":                                         # that kernel has no null bias
            biases.append(np.zeros(n_cols, dtype=np.float32) if not c["bias"] else (rng.standard_normal(n_cols) * cs).astype(np.float32))
        else:
            biases.append((rng.standard_normal(c["n_store"]) * cs[:c["n_store"]]).astype(np.float32) if c["bias"] else None)
    return dict(A_flat=flat, A_mask=mask, A=flat[idx], rowmap=rows.astype(np.int32) if c["rowmap"] else None, B=Bs, bias=biases)


def c_rows(c):
    return row_index(c["M"], c["c_gdiv"], c["c_gmul"])


# ------------------------------------------------------------------------------------------------ references
def _act(c, v):
    return np.maximum(v, 0) if c["relu"] else v


def weights64(c, B, cls):
    Bk = B[:c["K"], :c["n_store"]]
    return (Bk.astype(np.float16) if cls == "f16" else Bk).astype(np.float64)


def reference(c, inp, b, cls):
    """(want, S, extra): the contract in float64, the measure's denominator and the absolute term of the cap"""
    A = inp["A"].astype(np.float64) * np.float64(np.float32(c["a_scale"]))
    W = weights64(c, inp["B"][b], cls)
    bias = inp["bias"][b]
    bias = np.zeros(c["n_store"]) if bias is None else bias[:c["n_store"]].astype(np.float64)
    want = _act(c, A @ W + bias[None, :])
    S = np.abs(A) @ np.abs(W) + np.abs(bias)[None, :]
    extra = np.zeros_like(S)
    if cls == "f16":
        if not c["a_f16"]:
            extra += 2.0 ** -25 * np.abs(W).sum(axis=0)[None, :]
        if c["via"] == "f16_skinny":
            extra += 2.0 ** -11 * np.abs(want) + 2.0 ** -25
    return want, S, extra


def cap_c(c, cls):
    base = 8 + int(np.ceil(c["K"] ** 2 * U))
    return base if cls == "f32" else base + 3 + 39 if cls == "bf16x3" else base + 4 + 39


def split3(x):
    """x (float32) = hi + mid + lo, each a bf16 value (truncation), exactly"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    m = np.uint32(0xffff0000)
    hi = (x.view(np.uint32) & m).view(np.float32)
    r1 = x - hi
    mid = (r1.view(np.uint32) & m).view(np.float32)
    r2 = r1 - mid
    lo = (r2.view(np.uint32) & m).view(np.float32)
    return hi, mid, lo


def restatement(c, inp, b, cls):
    """the kernel class's arithmetic in float32 (see the module docstring)"""
    K, ns = c["K"], c["n_store"]
    B = np.ascontiguousarray(inp["B"][b][:K, :ns])
    acc = np.zeros((c["M"], ns), dtype=np.float32)
    if cls == "f32":
        A = (inp["A"].astype(np.float32) * np.float32(c["a_scale"])).astype(np.float32)
        At = np.ascontiguousarray(A.T)
        for k in range(K):
            acc += At[k][:, None] * B[k][None, :]
    elif cls == "bf16x3":
        A = (inp["A"].astype(np.float32) * np.float32(c["a_scale"])).astype(np.float32)
        a0, a1, a2 = split3(A)
        b0, b1, b2 = split3(B)
        for k0 in range(0, K, 32):
            s = slice(k0, min(K, k0 + 32))
            for x, y in ((a2, b0), (a0, b2), (a1, b1), (a1, b0), (a0, b1), (a0, b0)):
                acc += x[:, s] @ y[s]
    else:
        A = inp["A"].astype(np.float32)
        hi = A.astype(np.float16).astype(np.float32)
        lo = (A - hi).astype(np.float16).astype(np.float32)
        Bh = B.astype(np.float16).astype(np.float32)
        for k0 in range(0, K, 32):
            s = slice(k0, min(K, k0 + 32))
            if not c["a_f16"]:
                acc += lo[:, s] @ Bh[s]
            acc += hi[:, s] @ Bh[s]
    bias = inp["bias"][b]
    if bias is not None:
        acc = acc + bias[:ns][None, :]
    acc = _act(c, acc)
    if c["via"] == "f16_skinny":
        acc = acc.astype(np.float16)
    return acc.astype(np.float64)


def measure(got, want, S):
    """E = max |got - want| / S; where S is 0 (nothing but zeros went in) the output must be the reference exactly"""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    live = S > 0
    if not np.all(d[~live] == 0):
        return np.inf
    return float(np.max(d[live] / S[live])) if live.any() else 0.0


def inside_cap(got, want, S, extra, c, cls):
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return bool(np.all(d <= (c["K"] + cap_c(c, cls)) * U * S + extra))


def onehot_want(c, inp, b, cls):
    """rows onehot_k of B (as the class stores it), bit for bit"""
    B = inp["B"][b][:c["K"], :c["n_store"]]
    k = onehot_k(c)
    if cls == "f16":
        w = B.astype(np.float16)[k] + np.float16(0)                          # (a weight that underflows to -0 adds up to +0)
        return np.maximum(w, np.float16(0)) if c["relu"] else (w if c["via"] == "f16_skinny" else w.astype(np.float32))
    return B[k]


# ------------------------------------------------------------------------------------------------ packers
def _tiles(B, K, n):
    """[kt][n][4][8]: the 8 consecutive k of piece (kt, column, kq), zero past K"""
    kt = cdiv(K, 32)
    P = np.zeros((kt * 32, n), dtype=np.float32)
    P[:K] = B[:K, :n]
    return np.ascontiguousarray(P.reshape(kt, 4, 8, n).transpose(0, 3, 1, 2))


def _perm(n, perm_c, perm_p):
    j = np.arange(n)
    return np.where(j < perm_c * perm_p, (j % perm_c) * perm_p + j // perm_c, j) if perm_c > 0 else j


def _bf16_bits(x):
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def pack_b32(B, K, n, perm_c=0, perm_p=0):
    return _tiles(B[:, _perm(n, perm_c, perm_p)], K, n)


def pack_bq(B, K, n, perm_c=0, perm_p=0):
    """uint16 [kt][3 planes][n][4][8]"""
    t = pack_b32(B, K, n, perm_c, perm_p)
    return np.ascontiguousarray(np.stack([_bf16_bits(p) for p in split3(t)], axis=1))


def unpack_bq(Q, K, n):
    f = (Q.astype(np.uint32) << np.uint32(16)).view(np.float32)
    parts = [f[:, p].transpose(0, 2, 3, 1).reshape(-1, n)[:K] for p in range(3)]
    return (parts[2] + parts[1]) + parts[0], parts


def unpack_b32(P, K, n):
    return P.transpose(0, 2, 3, 1).reshape(-1, n)[:K]


def pack_split_a(A, M, K, rows_pad):
    """uint16 [kt][3][rows_pad][4][8]; rows >= M and k >= K zero"""
    Ap = np.zeros((K, rows_pad), dtype=np.float32)
    Ap[:, :min(M, rows_pad)] = A[:min(M, rows_pad), :K].T
    return pack_bq(Ap, K, rows_pad)


def pack_split_a_f16(A, M, K, rows_pad):
    """float16 [kt][2][rows_pad][4][8]"""
    Ap = np.zeros((K, rows_pad), dtype=np.float32)
    Ap[:, :M] = A[:M, :K].T
    t = _tiles(Ap, K, rows_pad)
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return np.ascontiguousarray(np.stack([hi, lo], axis=1))


def pack_bh(B, K, n_out, nch, npos, chpad):
    """float16 [kt][n_out][4][8]: output column pos * chpad + ch is source column ch * npos + pos"""
    j = np.arange(n_out)
    pos, ch = j // chpad, j % chpad
    real = (pos < npos) & (ch < nch)
    src = np.where(real, ch * npos + pos, 0)
    Bp = np.where(real[None, :], B[:K][:, src], np.float32(0)).astype(np.float32)
    return _tiles(Bp, K, n_out).astype(np.float16)


def unpack_bh(P, K, n):
    return P.transpose(0, 2, 3, 1).reshape(-1, n)[:K]


def pack_bias_cl(bias, n_out, nch, npos, chpad):
    j = np.arange(n_out)
    pos, ch = j // chpad, j % chpad
    real = (pos < npos) & (ch < nch)
    return np.where(real, bias[np.where(real, ch * npos + pos, 0)], np.float32(0)).astype(np.float32)


def pack_bfrag(B, K, n_cols):
    """float32 [n_cols / 16][bfrag_chunks(K)][64 lanes][4]: lane (kq, fi) of chunk c holds B[16 c + 4 kq + e][16 t + fi]"""
    kc = bfrag_chunks(K)
    P = np.zeros((kc * 16, n_cols), dtype=np.float32)
    P[:K] = B[:K, :n_cols]
    # [c][kq][e][t][fi] -> [t][c][kq][fi][e]
    return np.ascontiguousarray(P.reshape(kc, 4, 4, n_cols // 16, 16).transpose(3, 0, 1, 4, 2)).reshape(n_cols // 16, kc, 64, 4)


def unpack_bfrag(P, K, n_cols):
    kc = P.shape[1]
    return P.reshape(n_cols // 16, kc, 4, 16, 4).transpose(1, 2, 4, 0, 3).reshape(kc * 16, n_cols)[:K]


def pack_cases():
    """(name, kind, K, ld, n, p): the packers at sizes that leave a last k tile short, with and without the permutation"""
    return [
        ("bq", PACK_BQ, 36, 128, 128, None), ("bq_perm", PACK_BQ, 100, 192, 128, (5, 24)), ("bq_K128", PACK_BQ, 128, 64, 64, (4, 16)),
        ("b32", PACK_B32, 36, 128, 128, None), ("b32_perm", PACK_B32, 68, 64, 64, (3, 20)),
        ("bh", PACK_BH, 36, 200, 128, (3, 37, 4)), ("bh_K64", PACK_BH, 64, 96, 128, (30, 3, 32)), ("bh_plain", PACK_BH_PLAIN, 68, 128, 128, None),
        ("bias_cl", PACK_BIAS_CL, 1, 0, 300, (30, 9, 32)),
        ("split_a_128", PACK_SPLIT_A, 36, 40, 128, (100,)), ("split_a_176", PACK_SPLIT_A, 256, 256, 176, (150,)),
        ("bfrag_K68", PACK_BFRAG, 68, 128, 128, None), ("bfrag_K1560", PACK_BFRAG, 1560, 256, 256, None),
        ("bfrag_K64", PACK_BFRAG, 64, 64, 64, None),
    ]


def pack_source(kind, K, ld, n, p, seed):
    """(source array as the packer reads it, element count): rows of ld floats, NaN in the columns nobody may read"""
    rng = np.random.RandomState(seed)
    if kind == PACK_BIAS_CL:
        return rng.standard_normal(p[0] * p[1]).astype(np.float32)
    rows = p[0] if kind == PACK_SPLIT_A else K
    width = K if kind == PACK_SPLIT_A else (p[0] * p[1] if kind == PACK_BH else n)
    src = np.full((rows, ld), np.nan, dtype=np.float32)
    src[:, :width] = rng.standard_normal((rows, width)) * 2.0 ** rng.uniform(-4, 4, size=(1, width))
    src[::5, 1:width:3] = 0.0
    return src


def pack_want(kind, src, K, n, p):
    if kind == PACK_BQ:
        return pack_bq(src, K, n, *(p or (0, 0)))
    if kind == PACK_B32:
        return pack_b32(src, K, n, *(p or (0, 0)))
    if kind == PACK_BH:
        return pack_bh(src, K, n, *p)
    if kind == PACK_BH_PLAIN:
        return pack_bh(src, K, n, 1, n, 1)
    if kind == PACK_BIAS_CL:
        return pack_bias_cl(src, n, *p)
    if kind == PACK_SPLIT_A:
        return pack_split_a(src, p[0], K, n)
    return pack_bfrag(src, K, n)


def pack_bytes(kind, K, n):
    kt = cdiv(K, 32)
    return {PACK_BQ: kt * 3 * n * 64, PACK_B32: kt * n * 128, PACK_BH: kt * n * 64, PACK_BH_PLAIN: kt * n * 64, PACK_BIAS_CL: n * 4,
            PACK_SPLIT_A: kt * 3 * n * 64, PACK_BFRAG: (n // 16) * bfrag_chunks(K) * 1024, PACK_SPLIT_A_F16: kt * 2 * n * 64}[kind]
