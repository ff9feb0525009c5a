"""float64 references of the training GEMM (``train::gemm_kernel`` of csrc/train_core.hip) and of its helper kernels
(``finish_kernel``, ``reduce_kernel``, the conv1^T kernels), the case table of tests/test_gpu_train_kernels.py and a restatement
of the host-side extent computation of ``dcs_debug_train_gemm``.  Pure NumPy; tests/test_train_gemm_ref_cpu.py checks it alone.

An operand axis is ``(d0, d1, s0, s1, s2)``: index i is at ``(i % d0) s0 + (i / d0 % d1) s1 + (i / (d0 d1)) s2``, ``d0 d1``
clipped at 2^30 (``train::Ax``).  A case is a dict: the GEMM's fields by the names of ``train::Gemm``; an operand is
``dict(off, r, c)``; ``bias`` / ``bias2`` are flags, ``scale`` is None or the value the device scalar holds; ``partial`` is a
flag.  Buffers are exactly as long as the descriptor reaches (``extent``), so a read one element past an operand is a read of
poison.  Three data sets: ``signed`` (standard normal), ``int`` (A in -3 .. 3, B in -2 .. 2, integer biases: every partial sum
is an integer far below 2^24 and the result is exact in any order) and, for the rows that keep pre-activations, ``ties`` (the
integer set with ``bias`` minus an attained sum, so that pre-activations of exactly 0 occur).

The rule for the signed sets is the one of tests/gemm_ref.py and tests/d1_ref.py for MFMA sums: with S = sum |a||b| + |bias| +
|bias2| per output, E = max |got - f64| / S is at most ``FACTOR`` times the E of the in-order float32 chain, and every element
lies within ``(K + c) 2^-24 S``, c the count of epilogue roundings of the case (scale, bias, bias2, r'); K is the slice length
for ``partial``.  (K roundings: a product and K - 1 additions for the first term, fewer for the others.)
"""
import zlib

import numpy as np

import gemm_ref as gr

U = gr.U
FACTOR = gr.FACTOR
EINVAL = -1
KT = 32
BIG = 1 << 30
EPI_RELU, EPI_SAVEPRE, EPI_DRELU = 1, 2, 4
T128, T64, T32 = 0, 1, 2
TILE_NAMES = ("T128x32", "T64x64", "T32x32")
BLOCK = {T128: (128, 32), T64: (64, 64), T32: (32, 32)}
AUX_FINISH, AUX_REDUCE, AUX_DECONV1_IKALA, AUX_DECONV1_BACH10, AUX_DECONV1_BACH10SI = range(5)

# (tile, ak, bk) of every launch of a graph file: train_ca.hip:95, 104, 164, 180 (T128x32, K, N), :112 (T32x32, K, N), :131
# (rows_tile(B), K, N: T32x32 below 64 rows, T64x64 from 64), :144, 205 (T128x32, K, K), :188 (T32x32, K, K), :197 (rows_tile(B),
# K, K), :215 (T32x32, M, N), :224 (T128x32, M, N), :234, 249 (T64x64, M, N); train_dsd.hip:104 (every form T64x64, K, N);
# train_dsdild.hip:293-301 (kn, kk, mn on T64x64; T32x32 K, N and K, K; rows_tile(B) K, N and K, K)
PRODUCTION = {(T128, 1, 0), (T128, 1, 1), (T128, 0, 0), (T64, 1, 0), (T64, 1, 1), (T64, 0, 0), (T32, 1, 0), (T32, 1, 1), (T32, 0, 0)}
AID_ONLY = {(T128, 0, 1), (T64, 0, 1), (T32, 0, 1)}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ Ax
def ax3(d0, d1, s0, s1, s2):
    return (int(d0), int(d1), int(s0), int(s1), int(s2))


def ax2(d0, s0, s1):
    return ax3(d0, BIG, s0, s1, 0)


def ax1(s0):
    return ax3(BIG, 1, s0, 0, 0)


def ax_off(ax, i):
    d0, d1, s0, s1, s2 = ax
    i = np.asarray(i, dtype=np.int64)
    d01 = min(d0 * d1, BIG)
    return (i % d0) * s0 + (i // d0 % d1) * s1 + (i // d01) * s2


def _top2(ax, n):
    d0, _, s0, s1, _ = ax
    if n <= d0:
        return (n - 1) * s0
    q, r = divmod(n - 1, d0)
    return max((d0 - 1) * s0 + (q - 1) * s1, r * s0 + q * s1)


def ax_top(ax, n):
    """the aid's host-side computation (csrc/train_debug.hip top()): the largest offset over the indices 0 .. n - 1"""
    d01 = min(ax[0] * ax[1], BIG)
    q2 = (n - 1) // d01
    best = q2 * ax[4] + _top2(ax, n - q2 * d01)
    if q2 > 0:
        best = max(best, (q2 - 1) * ax[4] + _top2(ax, d01))
    return best


# ------------------------------------------------------------------------------------------------ a case's geometry
OPERANDS = ("A", "B", "C", "X")


def dims(c, name):
    """index ranges (rows, columns) of an operand; A's synthetic rows are not addressed"""
    if name == "A":
        return min(c["M"], c["ones_row"]), c["K"]
    return (c["K"], c["N"]) if name == "B" else (c["M"], c["N"])


def used(c, name):
    if name == "A":
        return dims(c, "A")[0] > 0
    if name == "C":
        return not c["partial"]
    if name == "X":
        return not c["partial"] and bool(c["epi"] & (EPI_SAVEPRE | EPI_DRELU))
    return True


def extent(c, name):
    """(lowest, highest) element of the operand's buffer the launch can address, as the aid computes it"""
    nr, nc = dims(c, name)
    m, w = c[name], OPERANDS.index(name)
    span = ax_top(m["r"], nr) + ax_top(m["c"], nc)
    los = [m["off"] + c["boff"][b][w] for b in range(c["nbatch"])]
    return min(los), max(los) + span


def index(c, name, b):
    """[rows][columns] element offsets of batch b"""
    nr, nc = dims(c, name)
    m, w = c[name], OPERANDS.index(name)
    return m["off"] + c["boff"][b][w] + ax_off(m["r"], np.arange(nr))[:, None] + ax_off(m["c"], np.arange(nc))[None, :]


def floats(c, name):
    """length of the operand's buffer: exactly what the descriptor reaches"""
    if name in OPERANDS:
        return extent(c, name)[1] + 1
    if name in ("bias", "bias2"):
        return max(c["boff"][b][4] for b in range(c["nbatch"])) + (c["N"] - 1) * c["bias_cs"] + 1
    if name == "partial":
        return c["nbatch"] * c["splits"] * c["M"] * c["N"] + PARTIAL_TAIL
    return 1                                                               # scale


PARTIAL_TAIL = 37                                                          # floats behind [nbatch splits][M][N] that stay poison


def slices(c):
    kc = c["kchunk"] if c["splits"] > 1 else c["K"]
    return [(s * kc, min(c["K"], (s + 1) * kc)) for s in range(c["splits"])]


def grid(c):
    bm, bn = BLOCK[c["tile"]]
    return [cdiv(c["M"], bm), cdiv(c["N"], bn), c["nbatch"] * c["splits"]]


def roundings(c):
    """epilogue roundings of the case: scale, bias, bias2, r'"""
    if c["partial"]:
        return 0
    return (c["scale"] is not None) + c["bias"] + c["bias2"] + bool(c["epi"] & EPI_DRELU)


def kinds_of(c):
    return ("signed", "int", "ties") if (c["epi"] & EPI_SAVEPRE and c["bias"]) else ("signed", "int")


# ------------------------------------------------------------------------------------------------ data
def _rs(*parts):
    return np.random.RandomState(zlib.crc32(repr(parts).encode()) & 0x7fffffff)


def relu_d(x):
    return np.where(x > 0, 1.0, np.where(x == 0, 0.5, 0.0))


def inputs(c, kind):
    rs = _rs(c["name"], kind)
    integer = kind != "signed"

    def draw(n, lim):
        if not integer:
            return rs.standard_normal(n).astype(np.float32)
        v = rs.randint(1, lim + 1, size=n) * (2 * rs.randint(0, 2, size=n) - 1)          # no zero: S > 0 on every output
        return v.astype(np.float32)

    inp = {}
    if used(c, "A"):
        inp["A"] = draw(floats(c, "A"), 3)
    inp["B"] = draw(floats(c, "B"), 2)
    if not c["partial"]:
        if c["bias"]:
            inp["bias"] = draw(floats(c, "bias"), 5)
        if c["bias2"]:
            inp["bias2"] = draw(floats(c, "bias2"), 5)
        if c["epi"] & EPI_DRELU:
            x = draw(floats(c, "X"), 2)
            x[rs.rand(x.size) < 0.25] = 0.0                                # negative, positive and exactly zero
            inp["X"] = x
    if c["scale"] is not None:
        inp["scale"] = np.array([c["scale"]], dtype=np.float32)
    if kind == "ties":
        # bias = -(scale * an attained sum) - bias2: the pre-activation of (row n % M, column n) of each batch is exactly 0
        sums = _sums(c, inp, np.float64)
        sc = 1.0 if c["scale"] is None else float(c["scale"])
        for b in range(c["nbatch"]):
            for n in range(c["N"]):
                at = c["boff"][b][4] + n * c["bias_cs"]
                b2 = float(inp["bias2"][at]) if c["bias2"] else 0.0
                inp["bias"][at] = -(sc * sums[b * c["splits"]][n % c["M"], n]) - b2
    return inp


def matrices(c, inp, b, ty):
    """A [M][K] with the ones rows, B [K][N] of batch b"""
    M, K = c["M"], c["K"]
    A = np.zeros((M, K), dtype=ty)
    ar = dims(c, "A")[0]
    if ar:
        A[:ar] = inp["A"][index(c, "A", b)]
    A[ar:] = (np.arange(K) < c["ones_klim"]).astype(ty)[None, :]
    return A, inp["B"][index(c, "B", b)].astype(ty)


def chain(A, B):
    """A . B, one float32 product and one float32 addition per k, k ascending"""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc += A[:, k, None] * B[k][None, :]
    return acc


def _sums(c, inp, ty, absolute=False):
    """[nbatch splits][M][N] raw slice sums"""
    out = []
    for b in range(c["nbatch"]):
        A, B = matrices(c, inp, b, ty)
        if absolute:
            A, B = np.abs(A), np.abs(B)
        for k0, k1 in slices(c):
            out.append(chain(A[:, k0:k1], B[k0:k1]) if ty == np.float32 else A[:, k0:k1] @ B[k0:k1])
    return np.stack(out)


def reference(c, inp, mode="f64"):
    """mode f64: the float64 result; f32: the in-order float32 chain with the kernel's epilogue order; abs: S.
    partial: {"partial": [nbatch splits][M][N]}; else {"C": [nbatch][M][N], "pre": likewise with EPI_SAVEPRE}"""
    ty = np.float32 if mode == "f32" else np.float64
    sums = _sums(c, inp, ty, absolute=mode == "abs")
    if c["partial"]:
        return {"partial": sums}
    out = {"C": [], "pre": []}
    for b in range(c["nbatch"]):
        v = sums[b]
        at = c["boff"][b][4] + np.arange(c["N"]) * c["bias_cs"]
        if mode == "abs":
            for name in ("bias", "bias2"):
                if c[name]:
                    v = v + np.abs(inp[name][at].astype(ty))[None, :]
            out["C"].append(v)
            continue
        if c["scale"] is not None:
            v = v * ty(inp["scale"][0])
        for name in ("bias", "bias2"):
            if c[name]:
                v = v + inp[name][at].astype(ty)[None, :]
        if c["epi"] & EPI_SAVEPRE:
            out["pre"].append(v.copy())
        elif c["epi"] & EPI_DRELU:
            v = v * relu_d(inp["X"][index(c, "X", b)]).astype(ty)
        if c["epi"] & EPI_RELU:
            v = np.maximum(v, ty(0))
        out["C"].append(v)
    res = {"C": np.stack(out["C"])}
    if out["pre"]:
        res["pre"] = np.stack(out["pre"])
    return res


def max_partial(c, inp):
    """the largest |partial sum| any order of summation can meet, per slice: sum |a||b| (+ the biases)"""
    S = reference(c, inp, "abs")
    return float(max(np.max(v) for v in S.values()))


# ------------------------------------------------------------------------------------------------ the case table
def _mat(off, r, c):
    return dict(off=int(off), r=r, c=c)


def _case(name, tile, ak, bk, M, N, K, A=None, B=None, C=None, X=None, ones_row=BIG, ones_klim=0, nbatch=1, boff=None, bias=False,
          bias_cs=1, bias2=False, scale=None, epi=0, partial=False, splits=1, kchunk=None, cite=""):
    # the plain operands: each contiguous the way it is loaded
    A = A or (_mat(0, ax1(K), ax1(1)) if ak else _mat(0, ax1(1), ax1(M)))
    B = B or (_mat(0, ax1(1), ax1(K)) if bk else _mat(0, ax1(N), ax1(1)))
    C = C or _mat(0, ax1(N), ax1(1))
    X = X or _mat(0, ax1(N), ax1(1))
    boff = [list(r) for r in (boff or [[0] * 5] * nbatch)] + [[0] * 5] * (4 - nbatch)
    return dict(name="%s %s%s %s" % (TILE_NAMES[tile], "K" if ak else "M", "K" if bk else "N", name), tile=tile, ak=ak, bk=bk, M=M, N=N,
                K=K, A=A, B=B, C=C, X=X, ones_row=ones_row, ones_klim=ones_klim, nbatch=nbatch, boff=boff, bias=bias, bias_cs=bias_cs,
                bias2=bias2, scale=scale, epi=epi, partial=partial, splits=splits, kchunk=kchunk or K, cite=cite)


KS = (1, 3, 31, 32, 33, 64, 95, 34, 2)            # the issue's seven, and 34 and 2 for K % 4 == 2
_EPIS = (dict(), dict(bias=True), dict(bias=True, bias2=True, scale=-1.0), dict(bias=True, epi=EPI_RELU | EPI_SAVEPRE), dict(epi=EPI_DRELU))


def _tail_rows():
    """every instance on the tails of its block: each M and N value once, the two corners together; K and the epilogue rotate"""
    rows, j = [], 0
    for tile in (T128, T64, T32):
        bm, bn = BLOCK[tile]
        ms = (1, bm - 1, bm, bm + 1, 2 * bm + 1)
        ns = (1, bn + 1, bn, bn - 1, 2 * bn + 1)
        for ak in (1, 0):
            for bk in (0, 1):
                for i in range(5):
                    K = KS[(i + 5 * j) % len(KS)]
                    rows.append(_case("tails %dx%dx%d" % (ms[i], ns[i], K), tile, ak, bk, ms[i], ns[i], K, **_EPIS[(i + j) % 5]))
                j += 1
    return rows


def _split_rows():
    rows = []
    for tile, ak, bk, cite in ((T32, 1, 0, "F3 train_ca.hip:108-112"), (T32, 1, 1, "B3 train_ca.hip:184-188"),
                               (T128, 0, 0, "dW2 train_ca.hip:219-224")):
        # (kchunk, splits, K): last slice of 1, of 31, a whole chunk
        for kc, s, K in ((32, 2, 33), (32, 3, 95), (64, 2, 128), (32, 5, 160), (64, 3, 129)):
            rows.append(_case("split %d x %d of %d" % (s, kc, K), tile, ak, bk, 33, 35, K, partial=True, splits=s, kchunk=kc, cite=cite))
    # two batches of three slices: blockIdx.z decodes both; the batches' operands follow each other
    M, N, K = 33, 30, 65
    rows.append(_case("split 3 x 32 of 65, two batches", T32, 0, 0, M, N, K, partial=True, splits=3, kchunk=32, nbatch=2,
                      boff=[[0] * 5, [M * K, K * N, 0, 0, 0]], cite="dW1 train_ca.hip:210-215"))
    rows.append(_case("split 3 x 32 of 65, two batches", T64, 1, 0, M, N, K, partial=True, splits=3, kchunk=32, nbatch=2,
                      boff=[[0] * 5, [M * K, K * N, 0, 0, 0]], cite="train_dsd_graph.hip G_F3"))
    # partial with one slice: raw sums, no epilogue although one is asked for
    rows.append(_case("partial, one slice", T32, 1, 0, 20, 33, 33, partial=True, bias=True, scale=-1.0, epi=EPI_RELU,
                      cite="train_ca.hip:111 with splits3 == 1"))
    return rows


def _ones_rows():
    rows = []
    # dW1 form: the ones row is the only row of the last tile; ones_klim inside the second slice
    rows.append(_case("ones row alone in its tile, klim 40 of 95 across slices", T32, 0, 0, 33, 30, 95, ones_row=32, ones_klim=40,
                      partial=True, splits=3, kchunk=32, cite="dW1 train_ca.hip:210-215"))
    rows.append(_case("ones row alone in its tile, klim on the slice boundary", T128, 0, 0, 129, 30, 95, ones_row=128, ones_klim=64,
                      partial=True, splits=3, kchunk=32, cite="dW2 train_ca.hip:219-224"))
    # dWfc form: ones row in the middle of a tile, klim = K, times sign(E)
    rows.append(_case("ones row mid tile, klim K", T64, 0, 0, 20, 65, 33, ones_row=19, ones_klim=33, scale=-1.0, cite="dWfc train_ca.hip:228-234"))
    rows.append(_case("ones row alone in its tile, klim 20 of 33", T64, 0, 0, 65, 33, 33, ones_row=64, ones_klim=20, scale=1.0,
                      cite="dW_k train_ca.hip:238-249"))
    # the other A load order
    rows.append(_case("ones row alone in its tile, klim K", T32, 1, 0, 33, 30, 34, ones_row=32, ones_klim=34))
    rows.append(_case("ones row mid tile, klim 5 of 34", T32, 1, 1, 20, 30, 34, ones_row=19, ones_klim=5))
    return rows


def _descriptor_rows():
    rows = []
    # conv1 windows, train_ca.hip:73-74, 90-95 (F1): x [B][NCH][tc][F], rows (b, t, w) at ax3(w1, tc, S1, F, NCH plane), K =
    # (channel, tap) at ax2(K1, 1, plane); S1 < K1: the windows overlap.  d0 = 7 (K1) and w1 = 4.
    Bn, NCH, tc, F, K1, S1, C1 = 2, 2, 3, 16, 7, 3, 30
    w1, plane = (F - K1) // S1 + 1, tc * F
    R1, KW = Bn * tc * w1, NCH * K1
    c1rows, c1k = ax3(w1, tc, S1, F, NCH * plane), ax2(K1, 1, plane)
    rows.append(_case("conv1 windows", T128, 1, 0, R1, C1, KW, A=_mat(0, c1rows, c1k), bias=True, bias2=True, cite="F1 train_ca.hip:90-95"))
    # B1, train_ca.hip:155-164: the same with two batches, slots of xy and U
    rows.append(_case("conv1 windows, two batches", T128, 1, 0, R1, C1, KW, A=_mat(0, c1rows, c1k), nbatch=2,
                      boff=[[NCH * Bn * plane, 0, R1 * C1, 0, 0], [2 * NCH * Bn * plane, 0, 2 * R1 * C1, 0, 0]], cite="B1 train_ca.hip:155-164"))
    # dW1, train_ca.hip:210-215: A transposed (c1k rows, c1rows columns) over two slots, ones row over the first slot
    rows.append(_case("conv1 windows transposed, ones row", T32, 0, 0, KW + 1, C1, 2 * R1, A=_mat(0, c1k, c1rows), ones_row=KW, ones_klim=R1,
                      partial=True, splits=2, kchunk=32, cite="dW1 train_ca.hip:210-215"))
    # the same with tc = 1: d1 = 1
    rows.append(_case("conv1 windows, tc 1 (d1 = 1)", T128, 1, 0, Bn * w1, C1, KW, A=_mat(0, ax3(w1, 1, S1, F, NCH * F), ax2(K1, 1, F)),
                      cite="F1 train_ca.hip:73"))
    # conv2 on the channels-last map, train_ca.hip:75, 77, 99-104 (F2): U [B][tc][w1][C], rows (b, h, w) at ax3(w2, h2, C, row1,
    # img1), K (dh, (dw, c)) at ax2(kw C, 1, row1).  kw C = 30 = d0.
    C, tc, w1, kh, kw = 10, 4, 5, 2, 3
    h2, w2, row1 = tc - kh + 1, w1 - kw + 1, w1 * C
    img1, Rh, K2 = tc * row1, 2 * h2 * w2, kh * kw * C
    map1, win1 = ax3(w2, h2, C, row1, img1), ax2(kw * C, 1, row1)
    rows.append(_case("map positions", T128, 1, 0, Rh, 30, K2, A=_mat(0, map1, win1), bias=True, bias2=True, cite="F2 train_ca.hip:99-104"))
    rows.append(_case("map positions, r'", T128, 1, 0, Rh, 30, K2, A=_mat(0, map1, win1), epi=EPI_DRELU, nbatch=2,
                      boff=[[2 * img1, 0, 0, 0, 0], [4 * img1, 0, Rh * 30, Rh * 30, 0]], cite="B2 train_ca.hip:168-180"))
    # dW2, train_ca.hip:219-224: A (win1, map1), B the map positions of V with unit columns, ones row
    mapp = ax3(w2, h2, 30, (w2 + 2) * 30, (h2 + 2) * (w2 + 2) * 30)
    rows.append(_case("windows by map positions, ones row", T128, 0, 0, K2 + 1, 30, Rh, A=_mat(0, win1, map1), B=_mat(64, mapp, ax1(1)),
                      ones_row=K2, ones_klim=h2 * w2, partial=True, cite="dW2 train_ca.hip:219-224"))
    # a map one column wide: d0 = 1
    rows.append(_case("map positions, w2 1 (d0 = 1)", T128, 1, 1, 2 * h2, 30, K2, A=_mat(0, ax3(1, h2, C, row1, img1), win1), cite="F2 train_ca.hip:77"))
    # B3, train_ca.hip:184-188: K concatenated over the branches, A columns ax2(flat, 1, Bflat), B rows ax2(flat, 1, wstep)
    Bn, flat, hid = 5, 161, 33
    rows.append(_case("K concatenation, d0 161", T32, 1, 1, Bn, hid, 2 * flat, A=_mat(0, ax1(flat), ax2(flat, 1, Bn * flat)),
                      B=_mat(0, ax2(flat, 1, hid * flat + flat), ax1(flat)), partial=True, splits=6, kchunk=64, cite="B3 train_ca.hip:184-188"))
    flat = 64
    rows.append(_case("K concatenation, d0 64", T32, 1, 1, Bn, hid, 3 * flat, A=_mat(0, ax1(flat), ax2(flat, 1, Bn * flat)),
                      B=_mat(0, ax2(flat, 1, hid * flat + flat), ax1(flat)), partial=True, splits=3, kchunk=64, cite="B3 train_ca.hip:184-188"))
    # F4, train_ca.hip:117-131: C into the padded map V (rows ax1(imgp), columns ax2(w2 C2, 1, rowp)) behind padoff, X row-major,
    # a bias section per batch, RELU | SAVEPRE; both tiles rows_tile gives
    C2, h2, w2 = 6, 3, 4
    rowp, flat = (w2 + 2) * C2, h2 * w2 * C2
    imgp, padoff = (h2 + 2) * rowp, rowp + C2
    for tile, Bn in ((T32, 5), (T64, 65)):
        Vslot, wstep = Bn * imgp, hid * flat + flat
        rows.append(_case("padded map out, %d rows" % Bn, tile, 1, 0, Bn, flat, hid, C=_mat(padoff, ax1(imgp), ax2(w2 * C2, 1, rowp)),
                          X=_mat(0, ax1(flat), ax1(1)), bias=True, epi=EPI_RELU | EPI_SAVEPRE, nbatch=2,
                          boff=[[0, 0, Vslot, 0, 0], [0, wstep, 2 * Vslot, Bn * flat, wstep]], cite="F4 train_ca.hip:117-131"))
        # B4, train_ca.hip:193-197: B transposed (ax1(1), ax1(K)), C the padded map
        rows.append(_case("padded map out, B transposed, %d rows" % Bn, tile, 1, 1, Bn, flat, hid, C=_mat(padoff, ax1(imgp), ax2(w2 * C2, 1, rowp)),
                          cite="B4 train_ca.hip:193-197"))
    # one bias value per batch, four batches (the output bias of one channel)
    rows.append(_case("bias_cs 0, four batches", T64, 1, 1, 33, 35, 34, bias=True, bias_cs=0, nbatch=4,
                      boff=[[b * 33 * 34, 0, b * 33 * 35, 0, b] for b in range(4)], cite="F6 train_dsd_graph.hip"))
    rows.append(_case("bias_cs 0, four batches, ties", T64, 1, 0, 33, 35, 34, bias=True, bias_cs=0, nbatch=4, epi=EPI_RELU | EPI_SAVEPRE,
                      boff=[[b * 33 * 34, 0, b * 33 * 35, b * 33 * 35, b] for b in range(4)], cite="F6 train_dsd_graph.hip"))
    # a non-zero offset on every operand
    for tile, ak, bk in sorted(PRODUCTION):
        M, N, K = 33, 34, 35
        rows.append(_case("offsets on A, B, C, X", tile, ak, bk, M, N, K, A=_mat(12, ax1(K), ax1(1)) if ak else _mat(12, ax1(1), ax1(M)),
                          B=_mat(20, ax1(1), ax1(K)) if bk else _mat(20, ax1(N), ax1(1)), C=_mat(8, ax1(N + 3), ax1(1)),
                          X=_mat(4, ax1(N + 1), ax1(1)), bias=True, epi=EPI_RELU | EPI_SAVEPRE))
    return rows


def _epilogue_rows():
    rows = []
    for tile, ak, bk in ((T128, 1, 0), (T64, 0, 0), (T32, 1, 1)):
        for sc in (1.0, -1.0, 0.0):
            rows.append(_case("scale %+g" % sc, tile, ak, bk, 33, 34, 35, scale=sc))
            rows.append(_case("scale %+g, bias, bias2" % sc, tile, ak, bk, 33, 34, 35, scale=sc, bias=True, bias2=True))
        rows.append(_case("relu, pre kept", tile, ak, bk, 33, 34, 35, bias=True, bias2=True, epi=EPI_RELU | EPI_SAVEPRE))
        rows.append(_case("r', bias", tile, ak, bk, 33, 34, 35, bias=True, scale=-1.0, epi=EPI_DRELU))
        rows.append(_case("relu alone", tile, ak, bk, 33, 34, 35, epi=EPI_RELU))
    return rows


_CASES = []


def cases():
    if not _CASES:
        _CASES.extend(_tail_rows() + _split_rows() + _ones_rows() + _descriptor_rows() + _epilogue_rows())
        names = [c["name"] for c in _CASES]
        assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return _CASES


def refusals(c):
    """(label, {field: value}) rows the aid must refuse with DCS_EINVAL; fields are named as the test sets them: 'A.bytes',
    'A.p' ('null' or 'misaligned'), 'A.r' (an axis), or a scalar field.  The byte counts are one byte short of the extent."""
    rows = []
    for name in OPERANDS:
        if used(c, name):
            rows += [("%s one byte short" % name, {name + ".bytes": 4 * (extent(c, name)[1] + 1) - 1}),
                     ("%s misaligned" % name, {name + ".p": "misaligned"}), ("null %s" % name, {name + ".p": "null"})]
    for name in ("bias", "bias2", "partial"):
        if c[name]:
            need = floats(c, name) - (PARTIAL_TAIL if name == "partial" else 0)
            rows += [("%s one byte short" % name, {name + "_bytes": 4 * need - 1}), ("%s misaligned" % name, {name: "misaligned"})]
    if c["scale"] is not None:
        rows += [("scale short", {"scale_bytes": 3}), ("scale misaligned", {"scale": "misaligned"})]
    neg = list(c["B"]["r"])
    neg[2] = -1
    rows += [("M 0", dict(M=0)), ("N 0", dict(N=0)), ("K 0", dict(K=0)), ("M 2^30", dict(M=BIG)), ("K 2^30", dict(K=BIG)), ("nbatch 0", dict(nbatch=0)),
             ("nbatch 5", dict(nbatch=5)), ("SAVEPRE with DRELU", dict(epi=EPI_SAVEPRE | EPI_DRELU)), ("tile 3", dict(tile=3)),
             ("a negative stride", {"B.r": tuple(neg)}), ("d0 0", {"B.r": (0,) + tuple(c["B"]["r"][1:])})]
    if not c["partial"]:
        rows += [("two slices without partial", dict(splits=2, kchunk=32))]
    else:
        rows += [("kchunk 48 with two slices", dict(splits=2, kchunk=48)), ("kchunk 0 with two slices", dict(splits=2, kchunk=0))]
    return rows


REFUSAL_CASES = ("T128x32 KN conv1 windows", "T32x32 KN padded map out, 5 rows", "T32x32 KK K concatenation, d0 161",
                 "T64x64 MN scale -1, bias, bias2", "T128x32 KN map positions, r'")


# ------------------------------------------------------------------------------------------------ the helper kernels
def finish_ref(part, bias, X, epi):
    """finish_kernel in float32: slices ascending, + bias[n], SAVEPRE -> X, DRELU * r'(X), RELU.  part [splits][B][N]; returns
    (C, X written or None)"""
    s = np.zeros(part.shape[1:], dtype=np.float32)
    for z in range(part.shape[0]):
        s = s + part[z]
    if bias is not None:
        s = s + bias[None, :]
    pre = s.copy() if epi & EPI_SAVEPRE else None
    if epi & EPI_DRELU:
        s = s * relu_d(X).astype(np.float32)
    if epi & EPI_RELU:
        s = np.maximum(s, np.float32(0))
    return s, pre


FINISH_ROWS = [(B, N, splits, epi, bias) for (B, N) in ((5, 53), (3, 256)) for splits in (1, 2, 7)
               for epi, bias in ((EPI_RELU | EPI_SAVEPRE, True), (EPI_RELU | EPI_SAVEPRE, False), (EPI_DRELU, False), (EPI_DRELU, True))]
# production: train_ca.hip:113 (RELU | SAVEPRE with bias) and :189 (DRELU without)


def finish_inputs(B, N, splits, epi, bias, kind="signed"):
    rs = _rs("finish", B, N, splits, epi, bias, kind)
    part = rs.standard_normal((splits, B, N)).astype(np.float32)
    b = rs.standard_normal(N).astype(np.float32) if bias else None
    X = rs.randint(-1, 2, size=(B, N)).astype(np.float32) * rs.rand(B, N).astype(np.float32) if epi & EPI_DRELU else None
    if X is not None:
        X[0, ::3] = 0.0
    return part, b, X


def reduce_ref(part, scale, N, dup):
    """reduce_kernel in float32: slices ascending, times the scale; dup: the last N values once more right behind.  part
    [splits][count]; returns count (+ N) floats"""
    s = np.zeros(part.shape[1], dtype=np.float32)
    for z in range(part.shape[0]):
        s = s + part[z]
    s = s * np.float32(scale)
    return np.concatenate([s, s[s.size - N:]]) if dup else s


# (count, splits, N, dup) of the two jobs; count[1] == 0: one job.  Production: train_ca.hip:252-259, both jobs dup with N = 30
REDUCE_ROWS = [((31 * 30, 3, 30, 1), (301, 5, 30, 1)), ((257, 1, 30, 0), (1000, 2, 7, 1)), ((777, 4, 30, 1), (0, 0, 0, 0))]
REDUCE_TAIL = 64                                       # floats of dst behind count (+ N) that stay poison


def reduce_inputs(row, scale):
    rs = _rs("reduce", row, scale)
    return [rs.standard_normal((s, n)).astype(np.float32) if n else None for n, s, _, _ in row]


DECONV1 = {AUX_DECONV1_IKALA: dict(S1=3, ns=2, channels=False), AUX_DECONV1_BACH10: dict(S1=4, ns=4, channels=False),
           AUX_DECONV1_BACH10SI: dict(S1=4, ns=4, channels=True)}
K1, C1 = 30, 30
# (B, tc, F, gslot pad): F = K1 (w1 = 1); an F whose last columns have no tap; tc 2; B 1 and 3
DECONV1_ROWS = [(1, 2, 30, 0), (3, 2, 37, 64), (1, 3, 44, 4)]


def deconv1_geom(which, B, tc, F, pad):
    d = DECONV1[which]
    w1 = (F - K1) // d["S1"] + 1
    gslot = B * tc * w1 * C1 + pad
    return dict(d, w1=w1, gslot=gslot, gfloats=(B * tc * w1 * C1 if d["channels"] else (d["ns"] - 1) * gslot + B * tc * w1 * C1))


def deconv1_inputs(which, B, tc, F, pad):
    g = deconv1_geom(which, B, tc, F, pad)
    rs = _rs("deconv1", which, B, tc, F, pad)
    return (rs.standard_normal(g["gfloats"]).astype(np.float32), rs.standard_normal(((g["ns"] if g["channels"] else 1), K1, C1)).astype(np.float32),
            (rs.standard_normal(g["ns"]) + 3.0 * np.arange(g["ns"])).astype(np.float32))


def deconv1_ref(which, B, tc, F, pad, g, W, bo, mode="f64"):
    """train_core.h: q[b][k][t][f] = bo[k] + sum over the taps S1 w + j = f of sum_c g_k[b][t][w][c] W[j][c], w then c ascending;
    columns without a tap hold bo alone.  mode f64, f32 (the in-order chain) or abs (S).  Returns (q, taps per column)"""
    d = deconv1_geom(which, B, tc, F, pad)
    ty = np.float32 if mode == "f32" else np.float64
    q = np.zeros((B, d["ns"], tc, F), dtype=ty)
    taps = np.zeros(F, dtype=np.int64)
    for k in range(d["ns"]):
        gk = (g if d["channels"] else g[k * d["gslot"]:])[:B * tc * d["w1"] * C1].reshape(B, tc, d["w1"], C1).astype(ty)
        Wk = W[k if d["channels"] else 0].astype(ty)
        if mode == "abs":
            gk, Wk = np.abs(gk), np.abs(Wk)
        for f in range(F):
            acc = np.zeros((B, tc), dtype=ty)
            n = 0
            for w in range(d["w1"]):
                j = f - d["S1"] * w
                if 0 <= j < K1:
                    n += 1
                    if mode == "f32":
                        for c in range(C1):
                            acc = acc + gk[:, :, w, c] * Wk[j, c]
                    else:
                        acc = acc + gk[:, :, w, :] @ Wk[j]
            taps[f] = n
            q[:, k, :, f] = acc + (abs(ty(bo[k])) if mode == "abs" else ty(bo[k]))
    return q, taps
