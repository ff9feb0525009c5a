"""Shared by tests/test_conv_ref_cpu.py and tests/test_gpu_conv_kernels.py (test infrastructure): the convolution, transposed
convolution and pool / un-pool kernels of the generic graphs (csrc/generic.hip, slabconv_ps.hip, colconv_fwd_x3.hip,
colconv_wreg.hip, colconv_x3.hip, conv1_mfma.hip, deconv1_mfma.hip) held directly to float64, one stage of the forward pass at
a time (``dcs_debug_conv_stage``).

* the operations in float64, from the contracts in the kernel headers (``conv1``, ``pool``, ``pool_routes``, ``unpool``,
  ``conv2``, ``conv2_t``, ``conv1_t``, ``routing_words``, the three hand-over layouts ``to_layout`` / ``from_layout``).  Every
  convolution is one routine, ``corr``: a correlation of a zero-padded (and, for conv1^T, zero-stuffed) image as a matrix
  product of its windows with the filter matrix, K ordered (tap row, tap column, channel);
* ``layer`` / ``decoder`` restate the same product in float32 per kernel class, the yardstick: ``f32`` one multiply-add
  per k, k ascending; ``bf16x3`` three truncated bf16 terms per operand (``gemm_ref.split3``), the six products above 2^-24
  of a 32-wide k tile added to a float32 accumulator, smallest first; ``f16`` both operands rounded to f16 (the weights
  when they are packed, the activations where the kernel loads them), float32 accumulation.  Inside a k tile the matrix
  instruction adds its products and the accumulator in an order and with an intermediate precision that are not specified
  (tests/gemm_ref.py allows it 33 roundings per instruction in its cap); the yardstick takes the same stand and adds the
  products of the leading terms one float32 multiply-add at a time, k ascending, like the ``f32`` class -- not through a BLAS
  product, whose blocked order is neither defined nor the instruction's (the five small product groups of ``bf16x3``, 2^-8
  and less of the leading one, are matrix products: their rounding is 2^-8 of the leading group's).  The
  f16 fused decoder rounds the map between its two layers to f16; conv1's f16 hand-over and the f16 conv2 map are one f16
  rounding of the float32 result.  The yardstick is computed on the first and the last image of a case;
* the measure ``E = max |got - want| / S``, ``S = sum |x| |w| + |bias|`` in float64 (for the two-layer decoder the sum over
  both layers: ``sum |w1| (sum |D| |w2|)``), over EVERY element the stage writes.  A case passes when ``E <= gemm_ref.FACTOR *
  E(restatement)`` and every element is inside the cap ``|got - want| <= (K + c) 2^-24 S + extra`` of ``gemm_ref.cap_c``'s form,
  K = taps x channels of the layer (both layers added for the decoder, c likewise).  For the f16 class ``want`` is the float64
  result on the operands as the kernel rounds them, so that the measure sees the arithmetic and not the format; ``extra`` is
  what a rounding the reference does not make can move: ``2^-11 |want| + 2^-25`` for an f16 output, ``2^-11 sum |w1| |G| +
  2^-25 sum |w1|`` for the f16 map G between the decoder's layers;
* the integer probe (``kind='int'``): tiles in 0 .. 3, conv1 weights and biases in -2 .. 2, conv2 inputs in -1 .. 2 and
  weights in -1 .. 1, dense outputs in 0 .. 2 -- every partial sum in any order is an integer below 2^24, and at most 2^11
  where a value is stored as f16 (``int_ranges``), so every class's restatement IS the float64 result and the device must
  return it bit for bit.  Ties are plentiful (zero rows and bands tie all four), so the pool, both tie routings and the routing
  words are checked exactly;
* ``expected`` -- the launchers' selection arithmetic restated: kernel code and launcher parameters per role as a function
  of the CU count and the switches; ``cases`` -- the case tables.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import gemm_ref as gr

U = gr.U
TC = 30
STAGE_CONV1, STAGE_CONV2, STAGE_DECODER = 0, 1, 2
CF, CL32, CL16 = 0, 1, 2                                    # DCS_CONV_LAYOUT_*
TIE_ALL, TIE_FIRST = 0, 1
ROLES = ("conv1", "pool", "conv2", "conv2t", "unpool", "conv1t", "decoder", "pad")

# DCS_CONV_K_* of include/dcs.h
(K_CONV1, K_CONV1_REG4, K_CONV1_REG3, K_CONV1_REG3_POOL, K_CONV1_MFMA_1, K_CONV1_MFMA_1_CL, K_CONV1_MFMA_1_CL16, K_CONV1_MFMA_4,
 K_CONV1_MFMA_4_CL, K_POOL, K_UNPOOL, K_IGEMM, K_IGEMM_T, K_IGEMM_F16, K_SLAB_MX_0, K_SLAB_MX_1, K_SLAB_PS_0, K_SLAB_PS_1,
 K_SLAB_PS_STRIP_0, K_SLAB_PS_STRIP_1, K_SLAB_PS_COL_0, K_COLCONV, K_COLCONV_T, K_COLCONV_F16, K_COLCONV_FWD_X3, K_WREG_SCATTER,
 K_WREG_SCATTER_I16, K_WREG_SCATTER_O16, K_WREG_SCATTER_I16_O16, K_WREG_GATHER, K_DECONV1, K_DECONV1_REG3, K_DECONV1_REG3_POOL,
 K_DECONV1_REG4, K_DECONV1_MFMA_1, K_DECONV1_MFMA_4, K_FUSED, K_FUSED_CL, K_FUSED_CL16, K_FUSED_X3_1, K_FUSED_X3_4,
 K_ZERO_PAD) = range(1, 43)
ALL_CODES = set(range(1, 43))
CODE_NAMES = {v: k for k, v in list(globals().items()) if k.startswith("K_")}
K_UNLISTED = 255                                            # an instance no graph reaches (csrc/slabconv_ps.hip)

CLASS = {}
for _c in (K_CONV1, K_CONV1_REG4, K_CONV1_REG3, K_CONV1_REG3_POOL, K_IGEMM, K_IGEMM_T, K_COLCONV, K_COLCONV_T, K_DECONV1, K_DECONV1_REG3,
           K_DECONV1_REG3_POOL, K_DECONV1_REG4):
    CLASS[_c] = "f32"
for _c in (K_CONV1_MFMA_1, K_CONV1_MFMA_1_CL, K_CONV1_MFMA_1_CL16, K_CONV1_MFMA_4, K_CONV1_MFMA_4_CL, K_SLAB_MX_0, K_SLAB_PS_0,
           K_SLAB_PS_STRIP_0, K_SLAB_PS_COL_0, K_COLCONV_FWD_X3, K_DECONV1_MFMA_1, K_DECONV1_MFMA_4, K_FUSED_X3_1, K_FUSED_X3_4):
    CLASS[_c] = "bf16x3"
for _c in (K_IGEMM_F16, K_SLAB_MX_1, K_SLAB_PS_1, K_SLAB_PS_STRIP_1, K_COLCONV_F16, K_WREG_SCATTER, K_WREG_SCATTER_I16,
           K_WREG_SCATTER_O16, K_WREG_SCATTER_I16_O16, K_WREG_GATHER, K_FUSED, K_FUSED_CL, K_FUSED_CL16):
    CLASS[_c] = "f16"

GRAPHS = {   # name: (input channels, conv1 stride, pool width, conv2 filter rows, columns, decoder branches)
    "bach10": (1, 4, 0, 20, 1, 4), "bach10_si1": (4, 4, 0, 20, 1, 1), "ikala": (1, 3, 4, 10, 20, 2), "ikala_nopool": (1, 3, 0, 10, 20, 2)}
NF, KW1, HID = 30, 30, 256

# the switch sets, one child process each (the library reads them once per process); `f16`: the settings of
# dcs_model_set_conv_precision the set is run with; `graphs` / `stages`: what the switch can change
SWITCHES = {
    "none": dict(env={}, f16=(0, 1), graphs=None, stages=(0, 1, 2)),
    "conv1_mfma0": dict(env={"DCS_CONV1_MFMA": "0"}, f16=(0,), graphs=("bach10", "bach10_si1"), stages=(0,)),
    "conv1_mfma0_reg0": dict(env={"DCS_CONV1_MFMA": "0", "DCS_CONV1_REG": "0"}, f16=(0,), graphs=None, stages=(0, 2)),
    "deconv1_mfma0": dict(env={"DCS_DECONV1_MFMA": "0"}, f16=(0,), graphs=("bach10", "bach10_si1"), stages=(2,)),
    "deconv1_mfma0_reg0": dict(env={"DCS_DECONV1_MFMA": "0", "DCS_DECONV1_REG": "0"}, f16=(0,), graphs=None, stages=(0, 2)),
    "colconv0": dict(env={"DCS_COLCONV": "0"}, f16=(0, 1), graphs=("bach10", "bach10_si1"), stages=(0, 1, 2)),
    "colconv_wreg0": dict(env={"DCS_COLCONV_WREG": "0"}, f16=(1,), graphs=("bach10", "bach10_si1"), stages=(0, 1, 2)),
    "decoder_fused0": dict(env={"DCS_DECODER_FUSED": "0"}, f16=(0, 1), graphs=("bach10", "bach10_si1"), stages=(2,)),
    "decoder_x30": dict(env={"DCS_DECODER_X3": "0"}, f16=(0,), graphs=("bach10", "bach10_si1"), stages=(2,)),
    "decoder_cl0": dict(env={"DCS_DECODER_CL": "0"}, f16=(1,), graphs=("bach10",), stages=(0, 1, 2)),
    "slabconv0": dict(env={"DCS_SLABCONV": "0", "DCS_FOLD_CONV2": "0"}, f16=(0, 1), graphs=("ikala", "ikala_nopool"), stages=(1, 2)),
    "slabconv_ps0": dict(env={"DCS_SLABCONV_PS": "0", "DCS_FOLD_CONV2": "0"}, f16=(0, 1), graphs=None, stages=(1, 2)),
    "pool_fused0": dict(env={"DCS_POOL_FUSED": "0"}, f16=(0,), graphs=("ikala",), stages=(0, 2)),
    "fold_conv20": dict(env={"DCS_FOLD_CONV2": "0"}, f16=(0, 1), graphs=("ikala", "ikala_nopool"), stages=(1,)),
}


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


def dims(graph, F, tc=TC):
    C, sw, pool, kh, kw, nb = GRAPHS[graph]
    w1 = (F - KW1) // sw + 1
    wp = w1 // pool if pool else w1
    h2, w2 = tc - kh + 1, wp - kw + 1
    flat = NF * h2 * w2
    return dict(C=C, sw=sw, pool=pool, kh=kh, kw=kw, n_branch=nb, w1=w1, wp=wp, h2=h2, w2=w2, flat=flat, flat_p=round_up(flat, 4),
                pitch16=round_up(flat, 32), n_out16=round_up(h2 * w2 * 32, 128), tc=tc, F=F)


def param_shapes(graph, F):
    d = dims(graph, F)
    s = [(NF, d["C"], 1, KW1), (NF,), (NF,), (NF, NF, d["kh"], d["kw"]), (NF,), (NF,), (d["flat"], HID), (HID,)]
    for _ in range(d["n_branch"]):
        s += [(HID, d["flat"]), (d["flat"],)]
    return s + [(d["n_branch"] * d["C"],)]


# ------------------------------------------------------------------------------------------------ data
def _seed(*parts):
    h = 2166136261
    for p in parts:
        for ch in str(p):
            h = ((h ^ ord(ch)) * 16777619) & 0xffffffff
    return h


def weights(graph, kind):
    """conv1.W, conv1.b, conv1b.b, conv2.W, conv2.b, conv2b.b (float32; the dense layers take no part and are zeros)"""
    C, sw, pool, kh, kw, nb = GRAPHS[graph]
    rs = np.random.RandomState(_seed("w", graph, kind))
    if kind == "int":
        return [rs.randint(-2, 3, (NF, C, 1, KW1)).astype(np.float32), rs.randint(-1, 2, NF).astype(np.float32),
                rs.randint(-1, 2, NF).astype(np.float32), rs.randint(-1, 2, (NF, NF, kh, kw)).astype(np.float32),
                rs.randint(-2, 3, NF).astype(np.float32), rs.randint(-2, 3, NF).astype(np.float32)]
    return [rs.uniform(-0.25, 0.25, (NF, C, 1, KW1)).astype(np.float32), rs.uniform(-0.1, 0.1, NF).astype(np.float32),
            rs.uniform(-0.1, 0.1, NF).astype(np.float32), rs.uniform(-0.25, 0.25, (NF, NF, kh, kw)).astype(np.float32),
            rs.uniform(-0.1, 0.1, NF).astype(np.float32), rs.uniform(-0.1, 0.1, NF).astype(np.float32)]


def params(graph, F, kind):
    shapes = param_shapes(graph, F)
    return weights(graph, kind) + [np.zeros(s, dtype=np.float32) for s in shapes[6:]]


FOLD_SIZES = (267, 306, 513)     # w2 = 1 (one output column); the pool drops a column; a size at which the model itself folds


def fold_params(F):
    """the iKala graph with a bottleneck layer that is not zero: random conv2 filters and biases, fc.W uniform in +-0.05"""
    p = params("ikala", F, "rand")
    rs = np.random.RandomState(_seed("fold", F))
    p[6] = rs.uniform(-0.05, 0.05, p[6].shape).astype(np.float32)
    p[7] = rs.uniform(-0.05, 0.05, p[7].shape).astype(np.float32)
    return p


def fold_want(W2, Wfc, d):
    """conv2 + bottleneck layer as one map of conv2's input, float64 [30 tc wp][hidden]:
    W2fc[(ci, r, x)][h] = sum_{co, u, v} Wc[co][ci][u][v] Wfc[(co, r - u, x - v)][h], Wc the flipped W2 (column h is the VJP
    of conv2 applied to column h of fc.W read as a [30][h2][w2] map), summed tap by tap"""
    cols = np.ascontiguousarray(Wfc.T, dtype=np.float64).reshape(Wfc.shape[1], NF, d["h2"], d["w2"])
    Wc = np.asarray(_flip(W2), dtype=np.float64)
    out = np.zeros((NF, Wfc.shape[1], d["tc"], d["wp"]))                    # [ci][h][r][x]
    for u in range(d["kh"]):
        for v in range(d["kw"]):                                            # tap (u, v) sends (r - u, x - v) to (r, x)
            out[:, :, u:u + d["h2"], v:v + d["w2"]] += np.tensordot(Wc[:, :, u, v], cols, axes=(0, 1))
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)).reshape(-1, Wfc.shape[1])


def tiles(graph, F, n, kind, frames=None):
    """[n][C][tc][F]; with frames = (rows, stride) the tiles are windows of one clip [C][rows][F], which is returned too.
    Rows 3 and 17 of every second tile and a band of columns are zero: every pool window over them ties four ways"""
    C = GRAPHS[graph][0]
    rs = np.random.RandomState(_seed("x", graph, F, n, kind, frames))
    rows = frames[0] if frames else n * TC
    x = rs.randint(0, 4, (C, rows, F)).astype(np.float32) if kind == "int" else rs.uniform(0.0, 1.0, (C, rows, F)).astype(np.float32)
    x[:, 3::2 * TC] = 0
    x[:, 17::2 * TC] = 0
    x[:, :, F // 3:F // 3 + 40] = 0
    if frames:
        t = np.stack([x[:, k * frames[1]:k * frames[1] + TC] for k in range(n)])
        return np.ascontiguousarray(t), x
    return np.ascontiguousarray(x.reshape(C, n, TC, F).transpose(1, 0, 2, 3)), None


def a1_map(graph, F, n, kind, rows=TC):
    """conv2's input [n][30][tc][wp]; rows < tc: tile k is rows k * rows .. + tc of one map (the per-frame hand-over)"""
    d = dims(graph, F)
    rs = np.random.RandomState(_seed("a1", graph, F, n, kind, rows))
    R = (n - 1) * rows + TC
    m = rs.randint(-1, 3, (NF, R, d["wp"])).astype(np.float32) if kind == "int" else rs.uniform(-1.0, 1.0, (NF, R, d["wp"])).astype(np.float32)
    return m                                                  # [30][R][wp]: the frames; a1_tiles cuts the windows


def a1_tiles(m, n, rows):
    return np.ascontiguousarray(np.stack([m[:, k * rows:k * rows + TC] for k in range(n)]))


def dense_out(graph, F, n, nb, kind):
    """the per-source dense layers' output [n * nb][30][h2][w2]: rectified, so about a third of it zero"""
    d = dims(graph, F)
    rs = np.random.RandomState(_seed("D", graph, F, n, nb, kind))
    shp = (n * nb, NF, d["h2"], d["w2"])
    if kind == "int":
        return rs.randint(0, 3, shp).astype(np.float32)
    return np.maximum(rs.uniform(-0.5, 1.0, shp), 0).astype(np.float32)


def int_ranges(graph):
    """largest magnitude any partial sum of the integer probe can have: (conv1, conv2, conv2^T, conv1^T)"""
    C, sw, pool, kh, kw, nb = GRAPHS[graph]
    c1 = 3 * 2 * KW1 * C + 2
    c2 = 2 * 1 * NF * kh * kw + 4
    g2 = 2 * 1 * NF * kh * kw
    o = g2 * 2 * NF * cdiv(KW1, sw)
    return c1, c2, g2, o


# ------------------------------------------------------------------------------------------------ the operations, float64
def _windows(xp, kh, kw, sw):
    """xp [ci][H][W] -> [Ho][Wo][kh * kw * ci], K ordered (u, v, ci)"""
    w = sliding_window_view(xp, (kh, kw), axis=(1, 2))[:, :, ::sw]             # [ci][Ho][Wo][kh][kw]
    Ho, Wo = w.shape[1], w.shape[2]
    return np.ascontiguousarray(w.transpose(1, 2, 3, 4, 0)).reshape(Ho, Wo, -1)


def _wmat(Wc):
    """Wc [co][ci][kh][kw] (correlation filter) -> [(u, v, ci)][co]"""
    return np.ascontiguousarray(Wc.transpose(2, 3, 1, 0)).reshape(-1, Wc.shape[0])


def _corr_taps(x, Wc, sw, pad):
    """the float64 correlation tap by tap: a matrix product over the channels per (u, v)"""
    xp = np.pad(x, ((0, 0), (0, 0), (pad[0], pad[1]), (pad[2], pad[3])))
    co, ci, kh, kw = Wc.shape
    n, _, H, W = xp.shape
    Ho, Wo = H - kh + 1, (W - kw) // sw + 1
    out = np.zeros((co, n, Ho, Wo))
    for u in range(kh):
        for v in range(kw):
            out += np.tensordot(Wc[:, :, u, v], xp[:, :, u:u + Ho, v:v + sw * (Wo - 1) + 1:sw], axes=(1, 1))
    return np.ascontiguousarray(out.transpose(1, 0, 2, 3))


def corr(x, Wc, sw=1, pad=(0, 0, 0, 0), stuff=1, mul=None, images=None):
    """out[n][co][y][x] = sum Wc[co][ci][u][v] xp[n][ci][y + u][sw x + v], xp = x zero-stuffed along W (a value every `stuff`
    columns) and zero-padded (top, bottom, left, right).  mul: None = float64, "abs" = float64 on the magnitudes (the S of the
    measure), else a function (A, Wm) of the window matrix [M][K] and the filter matrix [K][co] (the restatements)"""
    n, ci, H, W = x.shape
    kh, kw = Wc.shape[2], Wc.shape[3]
    if mul is None or mul == "abs":
        x, Wc = x.astype(np.float64), np.asarray(Wc, dtype=np.float64)
        if mul == "abs":
            x, Wc = np.abs(x), np.abs(Wc)
        if images is not None:
            x = x[images]
        if stuff > 1:
            z = np.zeros(x.shape[:3] + (stuff * (W - 1) + 1,))
            z[..., ::stuff] = x
            x = z
        return _corr_taps(x, Wc, sw, pad)
    Wm = _wmat(Wc)
    out = []
    for i in (range(n) if images is None else images):
        xi = x[i]
        if stuff > 1:
            z = np.zeros((ci, H, stuff * (W - 1) + 1), dtype=x.dtype)
            z[:, :, ::stuff] = xi
            xi = z
        xp = np.pad(xi, ((0, 0), (pad[0], pad[1]), (pad[2], pad[3])))
        A = _windows(xp, kh, kw, sw)
        Ho, Wo = A.shape[0], A.shape[1]
        r = mul(A.reshape(Ho * Wo, -1), Wm)
        out.append(r.reshape(Ho, Wo, -1).transpose(2, 0, 1))
    return np.stack(out)


def _flip(W):
    return W[:, :, ::-1, ::-1]


def _conv1_args(d):
    return dict(sw=d["sw"])


def conv1(x, W1, b1, b1b, d, **kw):
    """[n][C][tc][F] -> [n][30][tc][w1]: Conv2DLayer (a true convolution: the filter flipped) with a frequency stride, plus
    both biases"""
    r = corr(x, _flip(W1), sw=d["sw"], **kw)
    return r if kw.get("mul") else r + (b1.astype(np.float64) + b1b.astype(np.float64))[None, :, None, None]


def conv2(a, W2, b2, b2b, d, **kw):
    r = corr(a, _flip(W2), **kw)
    return r if kw.get("mul") else r + (b2.astype(np.float64) + b2b.astype(np.float64))[None, :, None, None]


def conv2_t(D, W2, d, **kw):
    """InverseLayer(conv2): the VJP of conv2 = the 'full' correlation of D with W2[co][ci] read as [ci][co]"""
    kh, kwd = W2.shape[2], W2.shape[3]
    return corr(D, W2.transpose(1, 0, 2, 3), pad=(kh - 1, kh - 1, kwd - 1, kwd - 1), **kw)


def conv1_t(g, W1, d, **kw):
    """InverseLayer(conv1): [m][30][tc][w1] -> [m][C][tc][F]; out[c][t][f] = sum_{o, sw j + u = f} g[o][t][j] Wc[o][c][u], Wc
    the flipped W1 -- the 'full' correlation of g zero-stuffed by the stride with W1 unflipped, columns up to F zero"""
    full = d["sw"] * (d["w1"] - 1) + KW1
    mul = kw.get("mul")
    if mul is None or mul == "abs":
        g = g.astype(np.float64) if kw.get("images") is None else g[kw["images"]].astype(np.float64)
        Wc = _flip(W1)[:, :, 0, :].astype(np.float64)                       # [o][c][u]
        if mul == "abs":
            g, Wc = np.abs(g), np.abs(Wc)
        out = np.zeros((Wc.shape[1], g.shape[0], g.shape[2], d["F"]))
        for u in range(KW1):
            out[..., u:u + d["sw"] * (d["w1"] - 1) + 1:d["sw"]] += np.tensordot(Wc[:, :, u], g, axes=(0, 1))
        return np.ascontiguousarray(out.transpose(1, 0, 2, 3))
    return corr(g, W1.transpose(1, 0, 2, 3), pad=(0, 0, KW1 - 1, KW1 - 1 + d["F"] - full), stuff=d["sw"], **kw)


def pool(a, pw=4):
    wp = a.shape[-1] // pw
    return a[..., :wp * pw].reshape(a.shape[:-1] + (wp, pw)).max(axis=-1)


def pool_routes(a, tie_mode, pw=4):
    """bool [..., w1]: the positions the VJP of the pool sends a window's value to -- every position equal to the window
    maximum (Theano's CPU MaxPoolGrad) or the first of them; columns past wp * pw get nothing"""
    w1 = a.shape[-1]
    wp = w1 // pw
    win = a[..., :wp * pw].reshape(a.shape[:-1] + (wp, pw))
    eq = win == win.max(axis=-1, keepdims=True)
    if tie_mode == TIE_FIRST:
        first = np.argmax(eq, axis=-1)
        eq = np.arange(pw) == first[..., None]
    out = np.zeros(a.shape, dtype=bool)
    out[..., :wp * pw] = eq.reshape(a.shape[:-1] + (wp * pw,))
    return out


def unpool(g, routes, nb, pw=4):
    """g [n * nb][30][tc][wp], routes [n][30][tc][w1] -> [n * nb][30][tc][w1]"""
    r = np.repeat(routes, nb, axis=0)
    return np.where(r, _spread(g, r.shape[-1], pw), 0.0)


def _spread(g, w1, pw):
    out = np.zeros(g.shape[:-1] + (w1,), dtype=g.dtype)
    wp = g.shape[-1]
    out[..., :wp * pw] = np.repeat(g, pw, axis=-1)
    return out


def routing_words(routes):
    """conv1_reg_kernel<30, 3, true>: 4 bits per window, 8 windows per 32-bit word -- bit j % 32 of word j / 32 of a row is
    position j's route.  [rows][ceil(w1 / 32)] uint32"""
    w1 = routes.shape[-1]
    nw = cdiv(w1, 32)
    r = np.zeros(routes.shape[:-1] + (nw * 32,), dtype=np.uint64)
    r[..., :w1] = routes
    r = r.reshape(routes.shape[:-1] + (nw, 32))
    return (r << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def routes_from_words(words, w1):
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(words.shape[:-1] + (-1,))[..., :w1].astype(bool)


def pool_words(w1):
    return cdiv(w1, 64) * 2


def to_layout(m, layout):
    """[n][30][rows][w] channel-first float32 -> the flat buffer of a hand-over layout (CL16: 32 halves per position, two zeros)"""
    if layout == CF:
        return np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    cl = np.ascontiguousarray(m.transpose(0, 2, 3, 1))
    if layout == CL32:
        return cl.astype(np.float32).reshape(-1)
    out = np.zeros(cl.shape[:-1] + (32,), dtype=np.float16)
    out[..., :cl.shape[-1]] = cl.astype(np.float16)
    return out.reshape(-1)


def from_layout(buf, layout, n, rows, w):
    if layout == CF:
        return buf.reshape(n, NF, rows, w)
    if layout == CL32:
        return buf.reshape(n, rows, w, NF).transpose(0, 3, 1, 2)
    return buf.reshape(n, rows, w, 32).transpose(0, 3, 1, 2)          # 32 channels: 30 and 31 are the pad


# ------------------------------------------------------------------------------------------------ float32 restatements
def _h(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def _chain(acc, A, B):
    """acc += A . B, one float32 multiply-add per k, k ascending"""
    At = np.ascontiguousarray(A.T)
    for k in np.flatnonzero(np.any(At != 0, axis=1)):                   # a zero column (zero-stuffing, padding) adds nothing
        acc += At[k][:, None] * B[k][None, :]
    return acc


def _mul_f32(A, B):
    A, B = A.astype(np.float32), B.astype(np.float32)
    return _chain(np.zeros((A.shape[0], B.shape[1]), dtype=np.float32), A, B)


def _mul_bf16x3(A, B):
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    a0, a1, a2 = gr.split3(A)
    b0, b1, b2 = gr.split3(B)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for k0 in range(0, A.shape[1], 32):
        s = slice(k0, k0 + 32)
        if not np.any(A[:, s]):
            continue
        for x, y in ((a2, b0), (a0, b2), (a1, b1), (a1, b0), (a0, b1)):
            acc += x[:, s] @ y[s]
        _chain(acc, a0[:, s], b0[s])
    return acc


def _mul_f16(A, B):
    A, B = _h(A), _h(B)
    return _chain(np.zeros((A.shape[0], B.shape[1]), dtype=np.float32), A, B)


MUL = {"f32": _mul_f32, "bf16x3": _mul_bf16x3, "f16": _mul_f16}


def _bias32(b, bb):
    return (b.astype(np.float32) + bb.astype(np.float32)).astype(np.float32)           # as dcs_generic_create adds them


def ends(n):
    return [0] if n == 1 else [0, n - 1]


def layer(op, x, W, d, cls, bias=None, f16_out=False):
    """one layer: (want, S, extra) over every image, and the class's restatement on the first and last image.
    f16 class: x and W as the kernel rounds them"""
    if cls == "f16":
        x, W = _h(x), _h(W)
    want = op(x, W, d) if bias is None else op(x, W, *bias, d)
    S = op(x, W, d, mul="abs") if bias is None else op(x, W, *bias, d, mul="abs")
    sub = ends(x.shape[0])
    rest = (op(x, W, d, mul=MUL[cls], images=sub) if bias is None else op(x, W, *bias, d, mul=MUL[cls], images=sub)).astype(np.float32)
    if bias is not None:
        S = S + np.abs(bias[0].astype(np.float64) + bias[1].astype(np.float64))[None, :, None, None]
        rest = rest + _bias32(*bias)[None, :, None, None]
    extra = np.zeros_like(want)
    if f16_out:
        rest = rest.astype(np.float16).astype(np.float32)
        extra = 2.0 ** -11 * np.abs(want) + 2.0 ** -25
    return want, S, extra, rest.astype(np.float64), sub


def layer_K(graph, which):
    C, sw, pool_w, kh, kw, nb = GRAPHS[graph]
    return {"conv1": KW1 * C, "conv2": NF * kh * kw, "conv2t": NF * kh * kw, "conv1t": NF * cdiv(KW1, sw)}[which]


def cap_c(K, cls):
    return gr.cap_c(dict(K=K), cls)


def measure(got, want, S):
    return gr.measure(got, want, S)


def inside_cap(got, want, S, extra, K, c):
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - want) <= (K + c) * U * S + extra))


def decoder(D, W1, W2, d, graph, cls2, cls1, routes=None, nb=1, f16_mid=False):
    """both InverseLayers (and the un-pool between them, by `routes`): (want, S, extra, restatement, images of it, K, c)"""
    pw = d["pool"]
    if cls2 == "f16":
        D, W2 = _h(D), _h(W2)
    if cls1 == "f16":
        W1 = _h(W1)
    g = conv2_t(D, W2, d)
    Sg = conv2_t(D, W2, d, mul="abs")
    m = D.shape[0]
    sub = ends(m)
    gr_ = conv2_t(D, W2, d, mul=MUL[cls2], images=sub).astype(np.float32)
    if f16_mid:
        gr_ = gr_.astype(np.float16).astype(np.float32)
    if pw:
        r = np.repeat(routes, nb, axis=0)
        g, Sg = np.where(r, _spread(g, d["w1"], pw), 0.0), np.where(r, _spread(Sg, d["w1"], pw), 0.0)
        gr_ = np.where(r[sub], _spread(gr_, d["w1"], pw), np.float32(0))
    want = conv1_t(g, W1, d)
    S = conv1_t(Sg, W1, d, mul="abs")
    rest = conv1_t(gr_, W1, d, mul=MUL[cls1]).astype(np.float64)
    extra = np.zeros_like(want)
    if f16_mid:
        extra = 2.0 ** -11 * conv1_t(np.abs(g), W1, d, mul="abs") + 2.0 ** -25 * np.abs(W1).astype(np.float64).sum()
    K = layer_K(graph, "conv2t") + layer_K(graph, "conv1t")
    c = cap_c(layer_K(graph, "conv2t"), cls2) + cap_c(layer_K(graph, "conv1t"), cls1)
    return want, S, extra, rest, sub, K, c, (g, Sg)


# ------------------------------------------------------------------------------------------------ selection arithmetic
def _on(sw, name):
    return SWITCHES[sw]["env"].get(name, "1") != "0"


def model_flags(graph, F, sw):
    C, s1, pool_w, kh, kw, nb = GRAPHS[graph]
    d = dims(graph, F)
    f = dict(d)
    f["slab"] = kw > 1 and _on(sw, "DCS_SLABCONV")
    f["col"] = kw == 1 and _on(sw, "DCS_COLCONV")
    f["W1m"] = s1 == 4 and C in (1, 4)
    f["W1dq"] = f["W1m"]
    Kf = NF * TC * d["wp"]
    conv2_flop = 2.0 * NF * NF * kh * kw * d["h2"] * d["w2"]
    more = 2.0 * (Kf - d["flat"]) * HID
    f["fold"] = _on(sw, "DCS_FOLD_CONV2") and kw > 1 and Kf % 4 == 0 and conv2_flop >= 4.0 * more
    f["Wfx3"] = f["col"] and kh % 2 == 0 and not pool_w
    f["W1q"] = f["col"] and s1 == 4 and not pool_w
    f["Wx3"] = f["W1q"] and kh % 2 == 0
    f["pool_fused"] = (_on(sw, "DCS_POOL_FUSED") and _on(sw, "DCS_CONV1_REG") and _on(sw, "DCS_DECONV1_REG") and pool_w == 4 and s1 == 3
                       and not f["W1m"] and pool_words(d["w1"]) + 1 <= d["w1"] and d["wp"] * 4 <= d["w1"])
    return f


def _fwd_x3_ok(kh, ph, H, Ho, W):
    return kh == 20 and ph == 0 and H == 30 and Ho == 11 and W >= 16


def _scatter_ok(sw, kh, ph, H, Ho, W):
    return _on(sw, "DCS_COLCONV_WREG") and kh == 20 and W >= 16 and ph == 0 and H == 30 and Ho == 11


def _fused_ok(sw, f):
    return (_on(sw, "DCS_DECODER_FUSED") and f["kh"] == 20 and f["h2"] == 11 and f["tc"] == 30 and f["w2"] >= 16
            and 4 * f["w2"] + 26 <= f["F"] <= 4 * f["w2"] + 32)


def _plans(sw, f, f16):
    """(fuse_planned, fuse_x3) of plans_channels_last"""
    if not (f["col"] and f["W1q"] and (True if f16 else f["Wx3"])):
        return False, False
    planned = (f["C"] == 1 and _fused_ok(sw, f)) if f16 else (_on(sw, "DCS_DECODER_X3") and _fused_ok(sw, f))
    return planned, planned and not f16


def decoder_fuses(sw, f, f16, d_cl):
    if not f["col"]:
        return False
    if f16:
        return f["C"] == 1 and f["W1q"] and _fused_ok(sw, f)
    return _plans(sw, f, f16)[1] and d_cl


def _slab_ps(sw, n_cu, n_images, mode, H, W, Ho, Wo, kh, kw, ph, pw):
    """dcs_launch_slabconv_ps: (code, band, xt, pstage) or None"""
    if not _on(sw, "DCS_SLABCONV_PS"):
        return None
    pu = kw == 1
    np_ = 3 if mode == 0 else 1
    nvp = (kw + 1) // 2
    nxb_all = cdiv(Wo, 16)
    rec = np_ * 2 * 16
    fast = (not pu) and nvp <= 32
    nw, slots = 16, 32
    band, xt, ps_best, best = 0, 0, 1, 0.0
    cxt = 1 if pu else nxb_all
    while cxt <= nxb_all and cxt <= slots:
        n_xt = cdiv(nxb_all, cxt)
        swd = min(cxt * 16 + (0 if pu else 2 * nvp - 1), W)
        cand = 1
        while cand <= Ho and cand * cxt <= slots:
            rows = min(cand + kh - 1, H)
            ps = 5
            while ps >= 1 and 2 * ps * np_ * 128 * 16 + (rows * swd + 1) * rec > 160 * 1024:
                ps -= 1
            if ps < 1:
                break
            n_wg = n_images * cdiv(Ho, cand) * n_xt
            rounds = cdiv(cand * cxt, nw)
            eff = float(n_images) * Ho * nxb_all / (float(n_wg) * nw * rounds)
            if n_wg < n_cu:
                eff *= float(n_wg) / n_cu
            eff /= 1.0 + 0.6 / ps
            tie = eff > best - 1e-9
            if eff > best + 1e-9 or (tie and (ps > ps_best or (ps == ps_best and cand * cxt >= band * (xt // 16)))):
                best, band, xt, ps_best = eff, cand, cxt * 16, ps
            cand += 1
        cxt += 1
    strips = False
    if fast and pw > 0 and Ho <= slots and nxb_all >= 2:
        rows = min(Ho + kh - 1, H)
        swd = min(16 + 2 * nvp - 1, W)
        for ps in range(5, 0, -1):
            if 2 * ps * np_ * 128 * 16 + (rows * swd + 1) * rec <= 160 * 1024:
                band, xt, ps_best, strips = Ho, 16, ps, True
                break
    if band < 1 or band * (xt // 16) < 8:
        return None
    code = K_SLAB_PS_COL_0 if pu else (K_SLAB_PS_STRIP_0 if strips else K_SLAB_PS_0) + (1 if mode else 0)
    return (code, band, xt, ps_best)


def _slab_mx(n_cu, n_images, mode, W, Ho, Wo, kh, kw):
    """launch_slabconv's own kernel: (code, band, 0, tstage) or None"""
    nxb = cdiv(Wo, 16)
    np_ = 3 if mode == 0 else 1
    tstage = min(kw, 2)
    w_bytes = 2 * tstage * np_ * 32 * 5 * 16
    row_bytes = W * 36 * 4
    band = 32 // nxb
    if band < 1:
        return None
    band = min(band, Ho)
    while band > 1 and n_images * cdiv(Ho, band) < n_cu:
        band -= 1
    band = cdiv(Ho, cdiv(Ho, band))
    while True:
        if band < 1:
            return None
        if w_bytes + row_bytes * (band + kh - 1) <= 160 * 1024:
            break
        band -= 1
    return (K_SLAB_MX_0 + (1 if mode else 0), band, 0, tstage)


def _per_wg(n_cu, n_images, n_xb):
    per = 8
    while per > 1 and n_images * cdiv(n_xb, per) < 4 * n_cu:
        per >>= 1
    return per


def _colconv(sw, n_cu, f, n_images, f16, transposed, in_f16=False, out_f16=False):
    """launch_colconv: (role, (code, p0, p1, p2))"""
    role = "conv2t" if transposed else "conv2"
    W = f["w2"] if transposed else f["wp"]
    n_xb = cdiv(W, 16)
    if f16 and _on(sw, "DCS_COLCONV_WREG") and f["kh"] == 20 and W >= 16:
        grid = min(cdiv(n_images * n_xb, 4), n_cu)
        if transposed:
            return role, (K_WREG_GATHER, 0, 0, grid)
        return role, (K_WREG_SCATTER + int(in_f16) + 2 * int(out_f16), 0, 0, grid)
    assert not (in_f16 or out_f16)
    if not f16 and not transposed:
        ps = _slab_ps(sw, n_cu, n_images, 0, TC, W, f["h2"], W, f["kh"], 1, 0, 0)
        if ps:
            return role, ps
    per = _per_wg(n_cu, n_images, n_xb)
    code = K_COLCONV_F16 if f16 else (K_COLCONV_T if transposed else K_COLCONV)
    return role, (code, per, 0, n_images * cdiv(n_xb, per))


def _conv2_general(sw, n_cu, f, n_images, f16, transposed):
    role = "conv2t" if transposed else "conv2"
    H, W, Ho, Wo = (f["h2"], f["w2"], TC, f["wp"]) if transposed else (TC, f["wp"], f["h2"], f["w2"])
    M = n_images * Ho * Wo
    if f16 and not f["slab"]:
        return role, (K_IGEMM_F16, 0, 0, cdiv(M, 128))
    if f["slab"]:
        ph, pw = (f["kh"] - 1, f["kw"] - 1) if transposed else (0, 0)
        r = _slab_ps(sw, n_cu, n_images, int(f16), H, W, Ho, Wo, f["kh"], f["kw"], ph, pw) or _slab_mx(n_cu, n_images, int(f16), W, Ho, Wo, f["kh"], f["kw"])
        if r:
            return role, r
    return role, (K_IGEMM_T if transposed else K_IGEMM, 0, 0, cdiv(M, 128))


def _best_rpi(n_images, n_xb, workers):
    best, best_cost = 1, -1
    for rpi in range(1, n_xb + 1):
        length = cdiv(n_xb, rpi) + (1 if rpi > 1 else 0)
        cost = cdiv(n_images * rpi, workers) * length
        if best_cost < 0 or cost < best_cost:
            best_cost, best = cost, rpi
    return best


def expected(case, n_cu):
    """what dcs_debug_conv_stage does with the case: dict(rc, kernels {role: (code, p0, p1, p2)}, a1_layout, a1_rows, fold2,
    a2_f16).  rc -2: refused (a layout the plan cannot consume)"""
    sw, graph, F, n, f16 = case["switch"], case["graph"], case["F"], case["n"], case["f16"]
    f = model_flags(graph, F, sw)
    C, tc, w1, wp = f["C"], TC, f["w1"], f["wp"]
    k, out = {}, dict(rc=0, a1_layout=CF, a1_rows=tc, fold2=0, a2_f16=0)
    if case["stage"] == STAGE_CONV1:
        frames = case.get("frames")
        want_cl = (not f16 and f["col"] and f["Wfx3"] and f["W1m"] and not f["pool"] and _fwd_x3_ok(f["kh"], 0, tc, f["h2"], w1))
        want_16 = (_on(sw, "DCS_DECODER_CL") and f16 and C == 1 and f["col"] and f["W1m"] and not f["pool"]
                   and _scatter_ok(sw, f["kh"], 0, tc, f["h2"], w1))
        mfma = _on(sw, "DCS_CONV1_MFMA") and f["W1m"]
        grid1 = cdiv(w1, 256) * n * tc
        gm = lambda rows: rows * cdiv(w1, 256)
        if f["pool_fused"]:
            k["conv1"] = (K_CONV1_REG3_POOL, 0, 0, grid1)
        elif frames and want_16 and mfma:
            k["conv1"] = (K_CONV1_MFMA_1_CL16, 0, 0, gm(frames[0]))
            out.update(a1_layout=CL16, a1_rows=frames[1])
        elif frames and want_cl and mfma:
            k["conv1"] = ((K_CONV1_MFMA_1_CL if C == 1 else K_CONV1_MFMA_4_CL), 0, 0, gm(frames[0]))
            out.update(a1_layout=CL32, a1_rows=frames[1])
        elif want_16 and mfma:
            k["conv1"] = (K_CONV1_MFMA_1_CL16, 0, 0, gm(n * tc))
            out.update(a1_layout=CL16)
        elif mfma:
            k["conv1"] = ((K_CONV1_MFMA_1 if C == 1 else K_CONV1_MFMA_4) + int(want_cl), 0, 0, gm(n * tc))
            if want_cl:
                out.update(a1_layout=CL32)
        elif _on(sw, "DCS_CONV1_REG") and f["sw"] == 4:
            k["conv1"] = (K_CONV1_REG4, 0, 0, grid1)
        elif _on(sw, "DCS_CONV1_REG") and f["sw"] == 3:
            k["conv1"] = (K_CONV1_REG3, 0, 0, grid1)
        else:
            k["conv1"] = (K_CONV1, 0, 0, grid1)
        if f["pool"] and not f["pool_fused"]:
            k["pool"] = (K_POOL, 0, 0, cdiv(n * NF * tc * wp, 256))
    elif case["stage"] == STAGE_CONV2:
        lay, rows = case["a1_layout"], case["a1_rows"]
        out.update(a1_layout=lay, a1_rows=rows)
        if lay != CF:
            ok = f["col"] and not f["pool"] and (
                (not f16 and f["Wfx3"] and _fwd_x3_ok(f["kh"], 0, tc, f["h2"], w1) and (rows * w1 * NF) % 2 == 0) if lay == CL32
                else (f16 and C == 1 and _scatter_ok(sw, f["kh"], 0, tc, f["h2"], w1)))
            if not ok:
                return dict(rc=-2, kernels={})
        a2_f16 = False
        if f16:
            ks16 = gr._longk_slices(n, f["pitch16"], HID, n_cu)[0]
            if ks16 >= 2 and f["col"] and not f["pool"] and f["flat"] % 2 == 0:
                a2_f16 = _scatter_ok(sw, f["kh"], 0, tc, f["h2"], wp)
        out["a2_f16"] = int(a2_f16)
        if f["fold"] and not f16 and lay == CF:
            out["fold2"] = 1
        else:
            if a2_f16:
                if f["pitch16"] != f["flat"]:
                    k["pad"] = (K_ZERO_PAD, 0, 0, cdiv(n * ((f["pitch16"] - f["flat"]) // 2), 256))
            elif f["flat_p"] != f["flat"]:
                k["pad"] = (K_ZERO_PAD, 0, 0, cdiv(n * (f["flat_p"] - f["flat"]), 256))
            if f["col"]:
                if lay == CL32:
                    items = n * cdiv(w1, 16)
                    k["conv2"] = (K_COLCONV_FWD_X3, 0, 0, cdiv(items, cdiv(items, 2 * n_cu)))
                else:
                    role, v = _colconv(sw, n_cu, f, n, f16, False, in_f16=lay == CL16, out_f16=a2_f16)
                    k[role] = v
            else:
                role, v = _conv2_general(sw, n_cu, f, n, f16, False)
                k[role] = v
    else:
        nb, lay = case["nb"], case["d_layout"]
        m = n * nb
        d_cl = lay != CF
        if d_cl and (not decoder_fuses(sw, f, f16, True) or (lay == CL16 and not f16)):
            return dict(rc=-2, kernels={})
        n_xb = cdiv(f["w2"], 16)
        if decoder_fuses(sw, f, f16, d_cl):
            if f16:
                rpi = _best_rpi(m, n_xb, 4 * n_cu)
                k["decoder"] = (K_FUSED_CL16 if lay == CL16 else K_FUSED_CL if lay == CL32 else K_FUSED, 0, rpi, min(cdiv(m * rpi, 4), n_cu))
            else:
                rpi = _best_rpi(m, n_xb, 2 * n_cu)
                k["decoder"] = (K_FUSED_X3_4 if C == 4 else K_FUSED_X3_1, 0, rpi, min(m * rpi, 2 * n_cu))
        else:
            role, v = _colconv(sw, n_cu, f, m, f16, True) if f["col"] else _conv2_general(sw, n_cu, f, m, f16, True)
            k[role] = v
            if f["pool"] and not f["pool_fused"]:
                k["unpool"] = (K_UNPOOL, 0, 0, cdiv(m * NF * tc, 4))
            if f["pool_fused"]:
                k["conv1t"] = (K_DECONV1_REG3_POOL, 0, 0, cdiv(tc * cdiv(F, 12), 256) * m)
            elif f["W1dq"] and _on(sw, "DCS_DECONV1_MFMA") and w1 >= 16:
                k["conv1t"] = (K_DECONV1_MFMA_1 if C == 1 else K_DECONV1_MFMA_4, 0, 0, min(cdiv(m * ((tc + 1) // 2), 4), 3 * n_cu))
            elif _on(sw, "DCS_DECONV1_REG") and f["sw"] == 3:
                k["conv1t"] = (K_DECONV1_REG3, 0, 0, cdiv(tc * cdiv(F, 12), 256) * m)
            elif _on(sw, "DCS_DECONV1_REG") and f["sw"] == 4:
                k["conv1t"] = (K_DECONV1_REG4, 0, 0, cdiv(tc * cdiv(F, 16), 256) * m)
            else:
                k["conv1t"] = (K_DECONV1, 0, 0, cdiv(F, 256) * m * tc)
    out["kernels"] = k
    return out


def branches(case, n_cu):
    """the named branches of the launchers a case enters (tests/test_conv_ref_cpu.py asserts that the table reaches each)"""
    e = expected(case, n_cu)
    f = dims(case["graph"], case["F"])
    b = set()
    for role, (code, p0, p1, p2) in e.get("kernels", {}).items():
        if code in (K_WREG_SCATTER, K_WREG_SCATTER_I16, K_WREG_SCATTER_O16, K_WREG_SCATTER_I16_O16):
            if case["n"] * cdiv(f["wp"], 16) > 4 * p2:
                b.add("wreg_scatter second unit")
        if code == K_WREG_GATHER and case["n"] * case["nb"] * cdiv(f["w2"], 16) > 4 * p2:
            b.add("wreg_gather second unit")
        if code in (K_FUSED, K_FUSED_CL, K_FUSED_CL16):
            b.add("fused rpi>1" if p1 > 1 else "fused rpi==1")
            if case["n"] * case["nb"] * p1 > 4 * p2:
                b.add("fused second run")
        if code in (K_FUSED_X3_1, K_FUSED_X3_4):
            b.add("x3 rpi>1" if p1 > 1 else "x3 rpi==1")
            if case["n"] * case["nb"] * p1 > p2:
                b.add("x3 second run")
        if code == K_COLCONV_FWD_X3 and case["n"] * cdiv(f["w1"], 16) > p2:
            b.add("fwd_x3 second item")
        if code in (K_DECONV1_MFMA_1, K_DECONV1_MFMA_4) and case["n"] * case["nb"] * 15 > 4 * p2:
            b.add("deconv1_mfma second unit")
        if code in (K_SLAB_PS_0, K_SLAB_PS_1, K_SLAB_PS_STRIP_0, K_SLAB_PS_STRIP_1, K_SLAB_PS_COL_0):
            Ho, Wo = (TC, f["wp"]) if role == "conv2t" else (f["h2"], f["w2"])
            if p2 < 5:
                b.add("pstage<5")
            if code in (K_SLAB_PS_STRIP_0, K_SLAB_PS_STRIP_1):
                b.add("column strips")
            if Ho % p0:
                b.add("short last band")
            if cdiv(Wo, 16) * 16 > p1:
                b.add("n_xt>1")
        if code in (K_COLCONV, K_COLCONV_T, K_COLCONV_F16):
            b.add("xb_per_wg=%d" % p0)
        if code in (K_CONV1_MFMA_1, K_CONV1_MFMA_1_CL, K_CONV1_MFMA_1_CL16, K_CONV1_MFMA_4, K_CONV1_MFMA_4_CL, K_CONV1_REG4, K_CONV1) and f["w1"] > 256:
            b.add("conv1 second workgroup along x")
    return b


BRANCHES = {"wreg_scatter second unit", "wreg_gather second unit", "fused rpi>1", "fused rpi==1", "fused second run", "x3 rpi>1", "x3 rpi==1",
            "x3 second run", "fwd_x3 second item", "deconv1_mfma second unit", "pstage<5", "column strips", "short last band", "n_xt>1",
            "xb_per_wg=1", "xb_per_wg=8", "conv1 second workgroup along x"}


# ------------------------------------------------------------------------------------------------ case tables
def _second_round(n_cu, per_image, mult):
    """the smallest image count with more than mult * n_cu units of per_image each"""
    return mult * n_cu // per_image + 1


def _shape_cases(n_cu):
    """(graph, F, stage, n, ...) before the switches: the smallest shapes that still have the tails.  `lean`: also run under
    the switch sets (the others only without switches)"""
    c = []
    for graph in ("bach10", "bach10_si1"):
        nb_all = GRAPHS[graph][5]
        for F in (90, 92, 93, 94, 96, 158):                  # w1 = 16, 16, 16, 17, 17, 33
            lean = F in (93, 158)
            for n in (1, 3):
                c.append(dict(graph=graph, F=F, stage=STAGE_CONV1, n=n, lean=lean))
            for lay in (CF, CL32, CL16):
                if F in (90, 94, 158):                       # conv2 sees F through w1 alone
                    for n in (1, 3):
                        c.append(dict(graph=graph, F=F, stage=STAGE_CONV2, n=n, a1_layout=lay, a1_rows=TC, lean=F == 158 and n == 3))
                c.append(dict(graph=graph, F=F, stage=STAGE_DECODER, n=1, nb=nb_all, d_layout=lay, lean=lean))
                if lean:
                    c.append(dict(graph=graph, F=F, stage=STAGE_DECODER, n=3, nb=1, d_layout=lay, lean=False))
        # per-frame conv1 (3 tiles at a stride of 5) and conv2 on its hand-over
        c.append(dict(graph=graph, F=94, stage=STAGE_CONV1, n=3, frames=(2 * 5 + TC, 5), lean=False))
        for lay in (CL32, CL16):
            c.append(dict(graph=graph, F=94, stage=STAGE_CONV2, n=3, a1_layout=lay, a1_rows=5, lean=False))
        # a second round of every persistent kernel: more than 4 n_cu images of one column block (F = 90) and of three (F = 158, conv2)
        m2 = 4 * n_cu + 4
        for lay in (CF, CL32, CL16):
            c.append(dict(graph=graph, F=158, stage=STAGE_CONV2, n=_second_round(n_cu, 3, 4), ntag="round2", a1_layout=lay, a1_rows=TC, lean=False))
            c.append(dict(graph=graph, F=90, stage=STAGE_DECODER, n=m2 // nb_all, ntag="round2", nb=nb_all, d_layout=lay, lean=False))
        # the second workgroup along x of the conv1 kernels; conv1^T at that width
        c.append(dict(graph=graph, F=1054, stage=STAGE_CONV1, n=1, lean=True))
        c.append(dict(graph=graph, F=1054, stage=STAGE_DECODER, n=1, nb=1, d_layout=CF, lean=True))
    # conv2 writing f16 for the long-K f16 bottleneck layer (128 tiles, K >= 16 384)
    for lay in (CF, CL16):
        c.append(dict(graph="bach10", F=226, stage=STAGE_CONV2, n=128, a1_layout=lay, a1_rows=TC, lean=True))
    for graph, Fs in (("ikala", (267, 306, 513)), ("ikala_nopool", (120,))):
        for F in Fs:
            lean = F in (306, 120)
            for n in (1, 3):
                for tie in (TIE_ALL, TIE_FIRST):
                    if tie == TIE_FIRST and not GRAPHS[graph][2]:
                        continue
                    c.append(dict(graph=graph, F=F, stage=STAGE_CONV1, n=n, tie=tie, lean=lean))
                    c.append(dict(graph=graph, F=F, stage=STAGE_DECODER, n=n, nb=2 if n == 1 else 1, d_layout=CF, tie=tie, lean=lean or n == 1))
                c.append(dict(graph=graph, F=F, stage=STAGE_CONV2, n=n, a1_layout=CF, a1_rows=TC, lean=True))
    # F = 1025: six column strips, w1 = 332, and a weight stage shorter than five pairs from 37 images on (256 CUs)
    c.append(dict(graph="ikala", F=1025, stage=STAGE_CONV2, n=ikala_1025_images(n_cu), ntag="short_stage", a1_layout=CF, a1_rows=TC, lean=True))
    c.append(dict(graph="ikala", F=1025, stage=STAGE_CONV1, n=1, tie=TIE_ALL, lean=False))
    c.append(dict(graph="ikala", F=1025, stage=STAGE_DECODER, n=1, nb=2, d_layout=CF, tie=TIE_FIRST, lean=True))
    return c


def ikala_1025_images(n_cu):
    """the smallest image count at which the forward conv2 of the iKala graph at F = 1025 stages fewer than five tap pairs"""
    return next(n for n in range(1, 4000) if (_slab_ps("none", n_cu, n, 0, TC, 83, 21, 64, 10, 20, 0, 0) or (0, 0, 0, 5))[3] < 5)


def cases(n_cu=256):
    out = []
    for sw, spec in SWITCHES.items():
        for base in _shape_cases(n_cu):
            if spec["graphs"] is not None and base["graph"] not in spec["graphs"]:
                continue
            if base["stage"] not in spec["stages"] or (sw != "none" and not base["lean"]):
                continue
            for f16 in spec["f16"]:
                if f16 and base["stage"] == STAGE_CONV1 and base["graph"] not in ("bach10", "bach10_si1"):
                    continue                                              # the precision switch changes conv1 of these graphs only
                c = dict(base, switch=sw, f16=f16)
                c.setdefault("tie", TIE_ALL)
                c.setdefault("nb", 1)
                c["name"] = "%s-%s-F%d-%s-n%s-f16_%d" % (sw, c["graph"], c["F"], ("conv1", "conv2", "decoder")[c["stage"]], c.get("ntag", c["n"]), f16)
                if c["stage"] == STAGE_CONV1 and c.get("frames"):
                    c["name"] += "-frames"
                if c["stage"] == STAGE_CONV2:
                    c["name"] += "-a1_%d_%d" % (c["a1_layout"], c["a1_rows"])
                if c["stage"] == STAGE_DECODER:
                    c["name"] += "-nb%d-D%d" % (c["nb"], c["d_layout"])
                if GRAPHS[c["graph"]][2]:
                    c["name"] += "-tie%d" % c["tie"]
                e = expected(c, n_cu)
                # a switch set runs the cases it changes: another kernel, other parameters or another hand-over than without
                # it (refusals are checked once, without switches)
                if sw != "none" and (e["rc"] != 0 or e == expected(dict(c, switch="none"), n_cu)):
                    continue
                out.append(c)
    return out
