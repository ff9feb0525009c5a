"""Float64 references, float32 restatements, the launchers' selection and the case table for the decoder kernels of the DSD
graphs (csrc/dsd.hip, dsd_bf16x3.hip, dsd_lat.hip), one stage at a time (``dcs_debug_dsd_stage``).

Stages
  deconv2   D [items][h2][50] -> G[item][ci][t] = sum_dt sum_co D[item][t - dt][co] W2[co, ci, kh - 1 - dt]   (0 <= t - dt < h2)
            device layouts: G f32 [item][7][tc][8] (channel ci = 8 g + c; channels 50 .. 55 zero) and the three bf16 truncation
            planes [item][7][tc][3][8]
  final     x_b = G_b . Bfin + bias_b (Bfin[c][f] = W1[c, ch, 0, F - 1 - f]); with three branches the fourth source is
            x_1 + (b_3 - b_1); p = max(x, floor) (floor = eps r = 5e-19 for convention A, else 0); masks
              A: p_i / sum_j p_j      B: p_i / (sum_j p_j + 5e-19)      stereo trainer: p_i / (sum_j p_j + 1e-13), + 1e-13 after the fold
            times mixture times scale; raw: p itself.  Fold: the sequential cross-fade of util.overlapadd_multi.

Measures (tests/gemm_ref.py, tests/conv_ref.py): E = max |got - want| / S with S the sum of the |products|;
E(device) <= FACTOR x E(restatement) and every element inside (K + cap_c(K, class)) U S.  The folded raw output adds
FOLD_ROUNDINGS roundings per covering tile to K (table value of up and of down, the product, the fma).  For the mask modes
the caps of the raw outputs are pushed through the mask and the fold in float64 (``mask_bound``) and the epilogue's own
roundings are added, EPILOGUE_ROUNDINGS per covering tile, counted from final_kernel's source:
    den: 3 adds (4 with the eps of conventions B / stereo)    4
    v_rcp_f32 at its documented 1 ulp = 2 U                   2
    mixv = scale * mix (once), mu = mixv * up, w = rcp * mu   3
    s_i * w, the fma into res                                 2
    the table values of up and down                           2      -> 13
"""
import numpy as np

import conv_ref as cr
import gemm_ref as gr

U, FACTOR = gr.U, gr.FACTOR
NF, CP, GCH, NGG = 50, 52, 8, 7
EPS_A, EPS_ILD = float(np.float32(5e-19)), float(np.float32(1e-13))      # the kernels' float32 constants
STAGE_DECONV2, STAGE_FINAL = 0, 1
THROUGHPUT, ONE_BATCH = 0, 1
EINVAL, EUNSUPPORTED = -1, -2
FOLD_ROUNDINGS, EPILOGUE_ROUNDINGS = 4, 13
LAT_MAX_COVERS = 6

K_DECONV2, K_STREAM, K_STREAM_SPLIT, K_BF16_4, K_BF16_16, K_GSPLIT, K_LAT_DECONV2 = 1, 2, 3, 4, 5, 6, 7
K_FINAL, K_FINAL4, K_FINAL_BF16X3, K_LAT_FINAL = 8, 20, 24, 26
ALL_CODES = set(range(1, 28))
ROLES = ("deconv2", "gsplit", "final")


def code_name(k):
    if k < K_FINAL:
        return ("", "deconv2_kernel<13>", "deconv2_stream_kernel<false>", "deconv2_stream_kernel<true>", "deconv2_stream_bf16_kernel<4>",
                "deconv2_stream_bf16_kernel<16>", "g_split_kernel", "lat_deconv2_kernel")[k]
    if k < K_FINAL4:
        v = k - K_FINAL
        return "final_kernel<%s, %d, %d, 3>" % ("true" if v // 6 else "false", v // 2 % 3, v % 2 + 1)
    if k < K_FINAL_BF16X3:
        v = k - K_FINAL4
        return "final_kernel<%s, %d, 1, 4>" % ("true" if v // 2 else "false", v % 2 + 2)
    return ("final_bf16x3_kernel<%d>" if k < K_LAT_FINAL else "lat_final_kernel<%d>") % ((k - K_FINAL_BF16X3) % 2)


def kernel_class(k):
    return "bf16x3" if k in (K_BF16_4, K_BF16_16, K_FINAL_BF16X3, K_FINAL_BF16X3 + 1, K_LAT_FINAL, K_LAT_FINAL + 1) else "f32"


# instances no public entry point reaches (the separation paths take conventions A / B only, the operator API refuses the stereo
# model): reached through dcs_debug_dsd_stage alone
NO_CALLER = {K_FINAL + (3 + 2) * 2, K_FINAL + (3 + 2) * 2 + 1, K_FINAL4, K_FINAL4 + 1, K_FINAL4 + 2}

SWITCHES = {"none": {}, "deconv2_1": {"DCS_DECONV2": "1"}, "deconv2_2": {"DCS_DECONV2": "2"}, "cbw_1": {"DCS_FINAL_CBW": "1"},
            "cbw_2": {"DCS_FINAL_CBW": "2"}}
cdiv, round_up = gr.cdiv, gr.round_up


def dims(tc):
    kh = tc // 2
    return dict(tc=tc, kh=kh, h2=tc - kh + 1)


def row_width(F, C):
    ld = round_up(F, 4)
    return (C - 1) * ld + F, ld


# ------------------------------------------------------------------------------------------------ synthetic weights and data
def _rng(*parts):
    return np.random.default_rng(cr._seed("dsd", *parts))


def weights(C, tc, F, kind):
    """W1 [50][C][1][F], W2 [50][50][kh][1], output bias [4 C].  sparse, tiny: see below.  rand: signed (with gdata's quarter-size G and the bias 1 of the
    first source the mask bound stays meaningful: tests/test_dsd_ref_cpu.py); pos: non-negative with positive biases (the
    well-conditioned half); int: the integer probe (W2 in -1 .. 1, W1 in -2 .. 2, integer biases)"""
    r, kh = _rng("w", C, tc, F, kind), tc // 2
    if kind == "int":
        return (r.integers(-2, 3, (NF, C, 1, F)).astype(np.float32), r.integers(-1, 2, (NF, NF, kh, 1)).astype(np.float32),
                r.integers(-3, 4, 4 * C).astype(np.float32))
    W1 = (r.standard_normal((NF, C, 1, F)) / np.sqrt(NF)).astype(np.float32)
    W2 = (r.standard_normal((NF, NF, kh, 1)) / np.sqrt(NF * kh)).astype(np.float32)
    b = (0.1 * r.standard_normal(4 * C)).astype(np.float32)
    b[:C] = 1.0                   # the first source keeps the denominators away from zero; the rectifier works on the others
    if kind == "pos":
        W1, W2, b = np.abs(W1), np.abs(W2), np.abs(b) + np.float32(0.05)
    if kind in ("sparse", "tiny"):
        # the hard sets, after oracle/cases.py.  The raw outputs before the bias are about N(0, 1/4) (gdata); a bias of -0.35 is
        # their 92 % quantile, so most outputs are cut and in most elements all four sources are: the denominator is then
        # nothing but the eps of the convention.  tiny: the first source gets a bias of the order of that eps instead (2 eps of
        # A / B, 2 eps of the stereo mask), which it IS on the frames whose G is zero (inputs): there the mask depends on the
        # value of eps itself, 0.4 under A and 2 / 3 under B.
        b = (-0.35 + 0.01 * r.standard_normal(4 * C)).astype(np.float32)
        if kind == "tiny":
            b[:C] = 1e-18 if C == 1 else 2e-13
    return W1, W2, b


def params(C, tc, F, kind):
    """the model's whole parameter list; only W1, W2 and the output bias reach the decoder stages"""
    d, hidden, n_fc = dims(tc), (128 if C == 1 else 256), (3 if C == 1 else 4)
    W1, W2, b = weights(C, tc, F, kind)
    flat = NF * d["h2"]
    z = lambda *s: np.zeros(s, dtype=np.float32)
    p = [W1, z(NF), z(NF), W2, z(NF), z(NF), z(flat, hidden), z(hidden)]
    for _ in range(n_fc):
        p += [z(hidden, flat), z(flat)]
    return p + [b]


def dense(tc, n, kind):
    """D [n][h2][50]: the rectified outputs of the per-source dense layers (int: 0 .. 2)"""
    r, h2 = _rng("D", tc, n, kind), dims(tc)["h2"]
    if kind == "int":
        return r.integers(0, 3, (n, h2, NF)).astype(np.float32)
    return np.maximum(r.standard_normal((n, h2, NF)), -0.5).astype(np.float32)       # signed: the sums cancel


def gdata(n, nbr, tc, kind):
    """G [tile][branch][50][tc] (int: -1 .. 2; pos: non-negative)"""
    r = _rng("G", n, nbr, tc, kind)
    if kind == "int":
        return r.integers(-1, 3, (n, nbr, NF, tc)).astype(np.float32)
    g = r.standard_normal((n, nbr, NF, tc)).astype(np.float32)                     # sparse and tiny: as rand
    return np.abs(g) if kind == "pos" else (np.float32(0.25) * g).astype(np.float32)


def mixture(rows, F, C, kind):
    """mixture rows [rows][C ld] (the pad columns of a channel zero, as the STFT leaves them); some bins are zero"""
    Fe, ld = row_width(F, C)
    r = _rng("mix", rows, F, C, kind)
    m = r.integers(0, 4, (rows, C * ld)).astype(np.float32) if kind == "int" else np.abs(r.standard_normal((rows, C * ld))).astype(np.float32)
    m[r.random((rows, C * ld)) < 0.02] = 0
    for ch in range(C):
        m[:, ch * ld + F:(ch + 1) * ld] = 0
    return m


ZERO_EVERY, ZERO_AT = 11, 3


def inputs(c, kind):
    """a final case's G of every tile [tiles][branches][50][tc] and the mixture rows of every clip, back to back.  In the
    sparse and tiny sets G is zero wherever a tile covers a frame f with f % 11 == 3: those frames' raw outputs ARE the biases"""
    clips, rows_all, tiles_all, tab = clip_layout(c)
    G, mix = gdata(tiles_all, 3 if c["C"] == 1 else 4, c["tc"], kind), mixture(rows_all, c["F"], c["C"], kind)
    if kind in ("sparse", "tiny"):
        st = c["tc"] - c["ov"] if c["ov"] is not None else c["tc"]
        for fr, nt, r0, t0 in clips:
            for k in range(nt):
                for j in range(c["tc"]):
                    if (k * st + j) % ZERO_EVERY == ZERO_AT:
                        G[t0 + k, :, :, j] = 0
    return G, mix


def int_ranges():
    """the largest integers of the probe stay far below 2^24: every float32 operation on them is exact"""
    return dict(deconv2=2 * 1 * NF * 20, final=2 * 2 * NF + 3 + 6)


# ------------------------------------------------------------------------------------------------ float64 references
def deconv2(D, W2, tc, mul=None):
    """-> G [n][50][tc].  mul: None float64, "abs" the sum of the |products|, or a restatement's product function"""
    n, h2, kh = D.shape[0], D.shape[1], W2.shape[2]
    if mul is None or mul == "abs":
        A, B = D.astype(np.float64).reshape(n * h2, NF), W2[:, :, ::-1, 0].astype(np.float64)        # B[co][ci][dt]
        if mul == "abs":
            A, B = np.abs(A), np.abs(B)
        P = (A @ B.reshape(NF, NF * kh)).reshape(n, h2, NF, kh)
        G = np.zeros((n, NF, tc))
        for dt in range(kh):
            G[:, :, dt:dt + h2] += P[:, :, :, dt].transpose(0, 2, 1)
        return G
    P = mul(np.ascontiguousarray(D.reshape(n * h2, NF)), np.ascontiguousarray(W2[:, :, ::-1, 0].reshape(NF, NF * kh))).reshape(n, h2, NF, kh)
    G = np.zeros((n, NF, tc), dtype=np.float32)
    for dt in range(kh):                        # the col2im sum in tap order (deconv2_kernel; the skewed row sums of the others)
        G[:, :, dt:dt + h2] += P[:, :, :, dt].transpose(0, 2, 1)
    return G


def mul_bf16x3(A, B):
    """the six products above 2^-24 of the truncation planes, K padded to two blocks of 32, float32 accumulation, in the
    order of deconv2_stream_bf16_kernel (term, then K block)"""
    a, b = gr.split3(A), gr.split3(B)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=np.float32)
    for pa, pb in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        for k0 in range(0, A.shape[1], 32):
            acc += a[pa][:, k0:k0 + 32] @ b[pb][k0:k0 + 32]
    return acc


MUL = {"f32": cr._mul_f32, "bf16x3": mul_bf16x3}


def g_layout(G):
    """G [n][50][tc] -> the kernels' [n][7][tc][8], channels 50 .. 55 zero"""
    n, _, tc = G.shape
    out = np.zeros((n, NGG * GCH, tc), dtype=G.dtype)
    out[:, :NF] = G
    return np.ascontiguousarray(out.reshape(n, NGG, GCH, tc).transpose(0, 1, 3, 2))


def g_from_layout(buf, n, tc):
    """-> (G [n][50][tc], pad channels [n][6][tc])"""
    g = np.asarray(buf).reshape(n, NGG, tc, GCH).transpose(0, 1, 3, 2).reshape(n, NGG * GCH, tc)
    return g[:, :NF], g[:, NF:]


def planes_layout(G32):
    """float32 G [n][50][tc] -> uint16 [n][7][tc][3][8]: the truncation split, bit for bit"""
    g = g_layout(np.ascontiguousarray(G32, dtype=np.float32))
    return np.stack([(p.view(np.uint32) >> 16).astype(np.uint16) for p in gr.split3(g)], axis=3)


def planes_value(buf, n, tc):
    """uint16 planes -> (float32 sum hi + mid + lo [n][7][tc][8] in the G layout, the planes as float32 [3][...])"""
    p = np.asarray(buf).view(np.uint16).reshape(n, NGG, tc, 3, GCH)
    f = [(p[:, :, :, i].astype(np.uint32) << 16).view(np.float32) for i in range(3)]
    return (f[0] + f[1]) + f[2], f


def bfin(W1, F):
    """[50][Fe]: Bfin[c][ch ld + f] = W1[c, ch, 0, F - 1 - f], the pad columns between the channels zero"""
    C = W1.shape[1]
    Fe, ld = row_width(F, C)
    B = np.zeros((NF, Fe), dtype=W1.dtype)
    for ch in range(C):
        B[:, ch * ld:ch * ld + F] = W1[:, ch, 0, ::-1]
    return B


def bias_rows(b, F, C):
    """[4][Fe]: the output bias of source s at every bin (per input channel in the stereo model)"""
    Fe, ld = row_width(F, C)
    out = np.zeros((4, Fe), dtype=b.dtype)
    for s in range(4):
        for ch in range(C):
            out[s, ch * ld:] = b[s * C + ch]
    return out


def rise_table(ov):
    """ensure_rise of csrc/net.hip: np.linspace(0, 1, ov) rounded to float32"""
    return np.linspace(0.0, 1.0, num=ov).astype(np.float32) if ov > 1 else np.zeros(1, dtype=np.float32)


def fold(tiles, ov, rows, rise=None, dtype=np.float64):
    """the sequential cross-fade of util.overlapadd_multi on tiles [n][tc][...] -> [rows][...]; frames no tile covers are zero.
    float32: one fused multiply-add per blend, down * old + (new * up) with the product rounded first, as the kernels do"""
    n, tc = tiles.shape[:2]
    st = tc - ov
    rise = np.linspace(0.0, 1.0, num=ov) if rise is None else rise
    up = rise.reshape((-1,) + (1,) * (tiles.ndim - 2))
    down = up[::-1]
    sep = np.zeros((max(rows, (n - 1) * st + tc),) + tiles.shape[2:], dtype=dtype)
    for k in range(n):
        s = k * st
        if k == 0:
            sep[:tc] = tiles[0]
        else:
            sep[s + ov:s + tc] = tiles[k, ov:]
            if dtype == np.float32:
                prod = (tiles[k, :ov] * up).astype(np.float32)
                sep[s:s + ov] = (down.astype(np.float64) * sep[s:s + ov] + prod).astype(np.float32)
            else:
                sep[s:s + ov] = down * sep[s:s + ov] + up * tiles[k, :ov]
    return sep[:rows]


def raw_tiles(G, W1, b, F, mul=None):
    """x [n][4][tc][Fe] before the rectifier, the fourth source of a three-branch graph as x_1 + (b_3 - b_1).
    mul None: float64; "abs": S; else a restatement (bias as the initial accumulator value)"""
    n, nbr, _, tc = G.shape
    C = W1.shape[1]
    B, bias = bfin(W1, F), bias_rows(b, F, C)
    A = np.ascontiguousarray(G.transpose(0, 1, 3, 2).reshape(n * nbr * tc, NF))
    if mul is None or mul == "abs":
        A, B, bias = A.astype(np.float64), B.astype(np.float64), bias.astype(np.float64)
        x = ((np.abs(A) @ np.abs(B)) if mul == "abs" else A @ B).reshape(n, nbr, tc, -1)
        if mul == "abs":
            x = x + np.abs(bias[:nbr])[None, :, None, :]
            return x if nbr == 4 else np.concatenate([x, x[:, 1:2] + np.abs(bias[3] - bias[1])[None, None, None, :]], axis=1)
        x = x + bias[:nbr][None, :, None, :]
        return x if nbr == 4 else np.concatenate([x, x[:, 1:2] + (bias[3] - bias[1])[None, None, None, :]], axis=1)
    raise ValueError(mul)


def raw_tiles_f32(G, W1, b, F, cls):
    """the class's restatement of raw_tiles: the bias is the accumulator's initial value"""
    n, nbr, _, tc = G.shape
    C = W1.shape[1]
    B, bias = np.ascontiguousarray(bfin(W1, F)), bias_rows(b, F, C)
    A = np.ascontiguousarray(G.transpose(0, 1, 3, 2).reshape(n * nbr * tc, NF))
    acc = np.ascontiguousarray(np.broadcast_to(bias[:nbr][None, :, None, :], (n, nbr, tc, B.shape[1])).reshape(A.shape[0], -1), dtype=np.float32)
    if cls == "f32":
        acc = cr._chain(acc, A, B)
    else:
        a3, b3 = gr.split3(A), gr.split3(B)
        for group in (((2, 0), (0, 2), (1, 1)), ((1, 0), (0, 1)), ((0, 0),)):       # final_bf16x3_kernel: K blocks inside a group
            for k0 in (0, 32):
                for pa, pb in group:
                    acc = acc + a3[pa][:, k0:k0 + 32] @ b3[pb][k0:k0 + 32]
    x = acc.reshape(n, nbr, tc, -1)
    if nbr == 4:
        return x
    d31 = (bias[3] - bias[1]).astype(np.float32)
    return np.concatenate([x, (x[:, 1:2] + d31[None, None, None, :]).astype(np.float32)], axis=1)


def _floor(mode):
    return EPS_A if mode == 0 else 0.0


def _den_eps(mode):
    return {0: 0.0, 1: EPS_A, 3: EPS_ILD}[mode]


def final(G, W1, b, F, mix, scale, mode, ov, rows):
    """float64: out [4][rows][Fe].  ov None: no fold (rows = n tc)"""
    x = raw_tiles(G, W1, b, F)
    n, _, tc, Fe = x.shape
    p = np.maximum(x, _floor(mode))
    if ov is None:
        mixt = mix[:, :Fe].astype(np.float64).reshape(n, 1, tc, Fe) * scale
        o = p if mode == 2 else p / (p.sum(axis=1, keepdims=True) + _den_eps(mode)) * mixt
        if mode == 3:
            o = o + EPS_ILD
        return o.transpose(1, 0, 2, 3).reshape(4, n * tc, Fe)
    m = p if mode == 2 else p / (p.sum(axis=1, keepdims=True) + _den_eps(mode))
    out = fold(m.transpose(0, 2, 1, 3), ov, rows).transpose(1, 0, 2)          # the mixture of a frame is the same in every tile
    if mode != 2:
        out = out * (mix[:rows, :Fe].astype(np.float64) * scale)[None]
    return out + EPS_ILD if mode == 3 else out


def final_f32(G, W1, b, F, mix, scale, mode, ov, rows, cls):
    """the restatement: the class's products, then the epilogue of final_kernel in float32 (den left to right, the reciprocal
    rounded once, w = rcp * (mixv * up), res = fma(down, res, s * w))"""
    f32 = np.float32
    x = raw_tiles_f32(G, W1, b, F, cls)
    n, _, tc, Fe = x.shape
    p = np.maximum(x, f32(_floor(mode)))
    if mode == 2:
        w = None
    else:
        den = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
        if mode != 0:
            den = den + f32(_den_eps(mode))
        with np.errstate(divide="ignore"):
            w = (f32(1) / den).astype(f32)
    if ov is None:
        mixv = (f32(scale) * mix[:, :Fe]).astype(f32).reshape(n, tc, Fe)
        o = p if mode == 2 else (p * (w * mixv)[:, None]).astype(f32)
        if mode == 3:
            o = o + f32(EPS_ILD)
        return o.transpose(1, 0, 2, 3).reshape(4, n * tc, Fe).astype(np.float64)
    st, rise = tc - ov, rise_table(ov)
    mixv = (f32(scale) * mix[:, :Fe]).astype(f32)
    res = np.zeros((4, max(rows, (n - 1) * st + tc), Fe), dtype=f32)
    for k in range(n):
        s = k * st
        for j in range(tc):
            r = s + j
            if r >= rows:
                break
            blend = k > 0 and j < ov
            up, down = (rise[j], rise[ov - 1 - j]) if blend else (f32(1), f32(0))
            if mode == 2:
                term = (p[k, :, j] * up).astype(f32)
            else:
                term = (p[k, :, j] * (w[k, j] * (mixv[r] * up).astype(f32)).astype(f32)[None]).astype(f32)
            res[:, r] = (np.float64(down) * res[:, r] + term).astype(f32)
    res = res[:, :rows]
    return (res + f32(EPS_ILD) if mode == 3 else res).astype(np.float64)


def raw_cap(S, cls, fold_tiles=0):
    """per-element cap of a raw output: (K + cap_c + the fold's roundings) U S"""
    return (NF + cr.cap_c(NF, cls) + 2 + FOLD_ROUNDINGS * fold_tiles) * U * S


def mmax_of(tc, ov):
    return cdiv(ov, tc - ov) + 1


def mask_bound(G, W1, b, F, mix, scale, mode, ov, rows, cls, exact_raw=False):
    """(bound [4][rows][Fe], scale S_out of the same shape): the caps eps_i of the raw outputs pushed through the mask and the
    fold, plus EPILOGUE_ROUNDINGS U per covering tile on the folded magnitudes; infinite where a tile with a weight has
    den_m <= sum_j eps_j.  With m_i = p_i / den, a changed p gives m_i' - m_i = ((1 - m_i) dp_i - m_i sum_{j != i} dp_j) / den', so
        |d out_i| <= scale mix sum_m weight_m ((1 - m_i) eps_i + m_i sum_{j != i} eps_j) / (den_m - sum_j eps_j)
    -- never above the (eps_i + m_i sum_j eps_j) form, and not blind where one source carries the whole mask.  A source whose
    raw output lies below the rectifier's floor by more than its cap is the floor on the device too: its eps is 0.  So where
    all four are cut the bound is the epilogue's roundings alone: convention A gives a quarter of the mixture, B and the
    stereo mask give 0 (+ 1e-13).  exact_raw: the integer probe, whose raw outputs are exact (eps = 0 everywhere).
    S_out: the first form's expression with the S_i in place of the eps_i and den_m in the denominator"""
    x, S = raw_tiles(G, W1, b, F), raw_tiles(G, W1, b, F, mul="abs")
    n, _, tc, Fe = x.shape
    eps = (NF + cr.cap_c(NF, cls) + 2) * U * S
    eps[x + eps < _floor(mode)] = 0.0
    if exact_raw:
        eps[...] = 0.0
    p = np.maximum(x, _floor(mode))
    den = p.sum(axis=1, keepdims=True) + _den_eps(mode)
    m = p / den
    se, sS = eps.sum(axis=1, keepdims=True), S.sum(axis=1, keepdims=True)
    room = den - se
    BIG = 1e200
    with np.errstate(divide="ignore", invalid="ignore"):
        bt = np.where(room > 0, ((1 - m) * eps + m * (se - eps)) / np.where(room > 0, room, 1.0), BIG)
    St = (S + m * sS) / den
    nt = 1 if ov is None else mmax_of(tc, ov)
    if ov is None:
        mx = (np.abs(mix[:, :Fe].astype(np.float64)) * scale).reshape(n, 1, tc, Fe)
        f = lambda t: (t * mx).transpose(1, 0, 2, 3).reshape(4, n * tc, Fe)
    else:
        mx = (np.abs(mix[:rows, :Fe].astype(np.float64)) * scale)[None]
        f = lambda t: fold(t.transpose(0, 2, 1, 3), ov, rows).transpose(1, 0, 2) * mx
    bound, mag, Sout = f(bt), f(m), f(St)
    bound = bound + EPILOGUE_ROUNDINGS * nt * U * mag
    if mode == 3:                                   # the constant added after the fold: its float32 value and the add
        bound = bound + 2 * U * (EPS_ILD + mag)
    bound[bound >= 1e150] = np.inf
    return bound, Sout


def pow2_elements(G, W1, b, F, mode, ov, rows):
    """[rows][Fe] bool: output elements that one tile alone produces with weight 1 (unfolded: all; folded: the frames before the
    second tile and the last tile's frames past its blend) and whose float32 denominator is a power of two: with an exact
    reciprocal the integer probe's output there is exact"""
    x = raw_tiles(G, W1, b, F)
    n, _, tc, Fe = x.shape
    den = (np.maximum(x, _floor(mode)).sum(axis=1) + _den_eps(mode)).astype(np.float32)          # [n][tc][Fe]
    q = (np.frexp(den)[0] == 0.5)
    if ov is None:
        return q.reshape(n * tc, Fe)
    st, out = tc - ov, np.zeros((rows, Fe), dtype=bool)
    if n == 1:
        out[:min(rows, tc)] = q[0, :min(rows, tc)]
        return out
    out[:min(st, rows)] = q[0, :min(st, rows)]
    lo, hi = (n - 1) * st + ov, min(rows, (n - 1) * st + tc)
    if hi > lo:
        out[lo:hi] = q[n - 1, ov:ov + hi - lo]
    return out


# ------------------------------------------------------------------------------------------------ the launchers' selection
def _stream_split(slots):
    X = max(8, int(slots / 6.5) // 8 * 8)          # six full channel groups and the partial one (4 channels = half a unit)
    return X, max(1, slots - 6 * X)


def expected(c, n_cu):
    """what dcs_debug_dsd_stage does with the case: dict(rc, kernels {role: code}, params [8])"""
    sw = SWITCHES[c["switch"]]
    d = dims(c["tc"])
    prm = [0] * 8
    lat = c["family"] == ONE_BATCH
    if c["stage"] == STAGE_DECONV2:
        n, gs = c["n"], c["gs"]
        if lat:
            if c["tc"] != 30:
                return dict(rc=EUNSUPPORTED, kernels={}, params=prm)
            return dict(rc=0, kernels={"deconv2": K_LAT_DECONV2}, params=[0, 0, 4, n * 7, 0, 0, 0, 0])
        nrb = cdiv(d["h2"], 16)
        gcols = round_up(13 * d["kh"], 16)
        if nrb > 2 or 16 * nrb * (CP + 2 + gcols) * 4 > 65536:
            return dict(rc=EUNSUPPORTED, kernels={}, params=prm)
        force = int(sw.get("DCS_DECONV2", 0))
        can_stream = nrb == 1 and d["kh"] <= 16 and c["tc"] <= 32 and d["h2"] + d["kh"] - 1 <= 32
        stream = can_stream and (force == 2 if force else n >= 4 * n_cu)
        if stream and gs and not c["no_bq"]:
            nw = 16 if n >= 1024 else 4
            X, Xt = _stream_split((1 if nw == 16 else 2) * n_cu)
            return dict(rc=0, kernels={"deconv2": K_BF16_16 if nw == 16 else K_BF16_4}, params=[X, Xt, nw, 6 * X + Xt, 0, 0, 0, 0])
        if stream:
            X, Xt = _stream_split(3 * n_cu)
            return dict(rc=0, kernels={"deconv2": K_STREAM_SPLIT if gs else K_STREAM}, params=[X, Xt, 4, 6 * X + Xt, 0, 0, 0, 0])
        k = {"deconv2": K_DECONV2}
        if gs:
            k["gsplit"] = K_GSPLIT
        return dict(rc=0, kernels=k, params=[0, 0, 4, n * 4, 0, 0, 0, 0])
    C, fold_, mode, rows = c["C"], c["ov"] is not None, c["mode"], c["rows"]
    Fe, ld = row_width(c["F"], C)
    if (fold_ and not 1 <= c["ov"] < c["tc"]) or (mode == 3 and C == 1) or (lat and not fold_):
        return dict(rc=EINVAL, kernels={}, params=prm)
    mmax = mmax_of(c["tc"], c["ov"]) if fold_ else 1
    n_clips = c["n_clips"]
    if lat:
        ok = (mmax <= LAT_MAX_COVERS and c["gs"] and c["tc"] == 30 and mode < 2 and n_clips == 1 and not c["table"] and C == 1)
        if not ok:
            return dict(rc=EINVAL, kernels={}, params=prm)
        return dict(rc=0, kernels={"final": K_LAT_FINAL + mode}, params=[0, 0, 0, 0, 1, cdiv(Fe, 64), cdiv(Fe, 64) * cdiv(rows, 16), mmax])
    if mmax > 16:
        return dict(rc=EUNSUPPORTED, kernels={}, params=prm)
    n_rg = cdiv(rows, 16)
    force = int(sw.get("DCS_FINAL_CBW", 0))
    cbw = force or (2 if n_rg * cdiv(Fe, 128) * n_clips >= 3 * n_cu else 1)
    n_colg = cdiv(Fe, 64 * cbw)
    if c["gs"] and fold_ and C == 1 and cbw == 2 and mode < 2:
        return dict(rc=0, kernels={"final": K_FINAL_BF16X3 + mode}, params=[0, 0, 0, 0, cbw, n_colg, n_rg * n_colg, mmax])
    if C == 2:
        if mode not in (2, 3):
            return dict(rc=EINVAL, kernels={}, params=prm)
        return dict(rc=0, kernels={"final": K_FINAL4 + (2 if fold_ else 0) + mode - 2}, params=[0, 0, 0, 0, 1, cdiv(Fe, 64), n_rg * cdiv(Fe, 64), mmax])
    return dict(rc=0, kernels={"final": K_FINAL + ((3 if fold_ else 0) + min(mode, 2)) * 2 + cbw - 1}, params=[0, 0, 0, 0, cbw, n_colg, n_rg * n_colg, mmax])


def clip_layout(c):
    """per clip (frames, tiles, first mixture row, first tile) and (mixture rows in all, tiles in all, the host clip table or None)"""
    tc, ov, n, rows, nc = c["tc"], c["ov"], c["n"], c["rows"], c["n_clips"]
    if c["table"]:
        clips, tab, r0, t0 = [], [], 0, 0
        for fr, nt in c["table"]:
            clips.append((fr, nt, r0, t0))
            tab += [fr * 512, fr, nt, r0, t0, fr]
            r0, t0 = r0 + fr, t0 + nt
        return clips, r0, t0, tab
    return [(rows, n, k * rows, k * n) for k in range(nc)], nc * rows, nc * n, None


def branches(c, n_cu):
    """the named branches of the kernels the case takes"""
    e = expected(c, n_cu)
    out = set()
    if e["rc"] != 0:
        return out
    k = e["kernels"]
    if c["stage"] == STAGE_DECONV2:
        code, (X, Xt, nw) = k["deconv2"], e["params"][:3]
        if code in (K_STREAM, K_STREAM_SPLIT, K_BF16_4, K_BF16_16):
            name = code_name(code)
            out.add(name + " Xt share")
            if c["n"] > X * nw:
                out.add(name + " second item round")
            if c["n"] < X * nw:
                out.add(name + " fewer items than workgroup columns")
            if dims(c["tc"])["kh"] < 15:
                out.add("short tap and row masks")
        if cdiv(dims(c["tc"])["h2"], 16) == 2:
            out.add("nrb 2")
        return out
    cbw, n_colg, n_wg = e["params"][4:7]
    Fe, _ = row_width(c["F"], c["C"])
    out.add("cbw %d" % cbw)
    if Fe % (16 * cbw) == 1:
        out.add("Nyquist-only wave")
    if n_wg % 8:
        out.add("nwg % 8 != 0")
    if c["ov"] is not None:
        st = c["tc"] - c["ov"]
        for fr, nt, _, _ in clip_layout(c)[0]:
            tcov = (nt - 1) * st + c["tc"]
            if c["table"] and cdiv(fr, 16) < cdiv(c["rows"], 16):
                out.add("early return of a short clip")
            if fr > tcov:
                out.add("dead row")
            if fr > c["ov"] + (nt - 1) * st + st:
                out.add("owner tile clamp")
            if nt > 1 and c["ov"] > st:
                out.add("mlim clipped by the last tile")
            if fr % 16:
                out.add("rows_here < 16")
    return out


BRANCHES = ({"%s %s" % (code_name(k), b) for k in (K_STREAM, K_STREAM_SPLIT, K_BF16_4, K_BF16_16) for b in ("Xt share", "second item round")} |
            {"short tap and row masks", "nrb 2", "cbw 1", "cbw 2", "Nyquist-only wave", "nwg % 8 != 0", "early return of a short clip",
             "dead row", "owner tile clamp", "mlim clipped by the last tile", "rows_here < 16",
             code_name(K_STREAM) + " fewer items than workgroup columns", code_name(K_BF16_4) + " fewer items than workgroup columns"})


# ------------------------------------------------------------------------------------------------ the case table
def _d(name, n, tc=30, switch="none", family=THROUGHPUT, gs=0, no_bq=0, g=1):
    return dict(name=name, stage=STAGE_DECONV2, n=n, tc=tc, switch=switch, family=family, gs=gs, no_bq=no_bq, g=g, C=1, F=65)


def _f(name, F, ov, n, rows, mode, switch="none", family=THROUGHPUT, gs=0, C=1, n_clips=1, table=None, kinds=("rand", "pos"), tc=30):
    return dict(name=name, stage=STAGE_FINAL, F=F, ov=ov, n=n, rows=rows if ov is not None else n * tc, mode=mode, switch=switch,
                family=family, gs=gs, C=C, n_clips=n_clips, table=table, kinds=kinds, tc=tc)


def natural_rows(n_cu, F=1025, st=5, tc=30):
    """the first size at which the final launcher takes 128-bin workgroups: (tiles, rows), rows = the frames the tiles cover"""
    rg = cdiv(3 * n_cu, cdiv(F, 128))
    n = cdiv(16 * (rg - 1) + 1 - tc, st) + 1
    return n, (n - 1) * st + tc


HARD = ("rand", "pos", "sparse", "tiny", "int")       # + the hard weight sets and the integer probe of the mask modes


def cases(n_cu=256):
    s4 = 4 * n_cu
    out = [
        # ---- transposed conv2: the one-shot kernel, the split pass behind it, the one-batch kernel
        _d("d2 one-shot 1 item", 1), _d("d2 one-shot 3 items + split", 3, gs=1), _d("d2 one-shot 5 items", 5),
        _d("d2 one-shot 96 items + split", 96, gs=1), _d("d2 one-shot tc 20", 5, tc=20), _d("d2 one-shot tc 31 (nrb 2)", 3, tc=31),
        _d("d2 one-shot tc 32 (nrb 2) + split", 3, tc=32, gs=1), _d("d2 one-shot tc 40 (kh 20)", 3, tc=40),
        _d("d2 one-batch G", 1, family=ONE_BATCH), _d("d2 one-batch Gs", 3, family=ONE_BATCH, gs=1, g=0),
        _d("d2 one-batch G + Gs", 5, family=ONE_BATCH, gs=1), _d("d2 one-batch tc 20 (refused)", 1, tc=20, family=ONE_BATCH),
        # ---- the streaming kernels at their natural sizes
        _d("d2 stream f32 at 4 n_cu", s4), _d("d2 stream split at 4 n_cu + 2", s4 + 2, gs=1, no_bq=1),
        _d("d2 stream bf16 at 4 n_cu", s4, gs=1),
        _d("d2 forced one-shot at 4 n_cu + split", s4, switch="deconv2_1", gs=1),
        # ---- forced streaming: fewer items than workgroup columns, short tap masks, <4> against <16>
        _d("d2 forced stream f32 3 items", 3, switch="deconv2_2"), _d("d2 forced stream split 7 items", 7, switch="deconv2_2", gs=1, no_bq=1),
        _d("d2 forced stream bf16 25 items", 25, switch="deconv2_2", gs=1), _d("d2 forced stream bf16 1023 items", 1023, switch="deconv2_2", gs=1),
        _d("d2 forced stream f32 tc 20", 7, tc=20, switch="deconv2_2"), _d("d2 forced stream bf16 tc 20", 7, tc=20, switch="deconv2_2", gs=1),
        _d("d2 forced stream split tc 20", 3, tc=20, switch="deconv2_2", gs=1, no_bq=1),
        _d("d2 forced stream falls back at tc 31", 3, tc=31, switch="deconv2_2", gs=1),
        _d("d2 forced stream falls back at tc 40", 3, tc=40, switch="deconv2_2"),
    ]
    nn, nr = natural_rows(n_cu, st=20)           # overlap 10: two covering tiles, a reference of a few million elements
    out += [
        # ---- final, 64-bin workgroups: conventions, overlaps, row shapes
        _f("fin A F65 ov25 T45", 65, 25, 4, 45, 0, kinds=HARD), _f("fin B F513 ov15 T49 < Tcov", 513, 15, 3, 49, 1, kinds=HARD),
        _f("fin raw F65 ov20 T63 > Tcov", 65, 20, 3, 63, 2), _f("fin A F1025 ov16 T44", 1025, 16, 2, 44, 0),
        _f("fin B F65 ov1 T59", 65, 1, 2, 59, 1), _f("fin A F65 ov26 (8 covers)", 65, 26, 5, 46, 0),
        _f("fin A F65 ov29 (refused)", 65, 29, 3, 32, 0), _f("fin A F65 one tile", 65, 25, 1, 30, 0),
        _f("fin raw F65 ov1", 65, 1, 3, 88, 2, kinds=("rand", "int")), _f("fin raw F65 ov2 dead rows", 65, 2, 3, 91, 2, kinds=("rand", "int")),
        _f("fin A F65 ov25 T81 > Tcov clamp", 65, 25, 4, 81, 0),
        _f("op A F65", 65, None, 2, 0, 0, kinds=HARD), _f("op B F513", 513, None, 2, 0, 1, kinds=HARD), _f("op raw F65", 65, None, 3, 0, 2, kinds=("rand", "int")),
        _f("fin A F65 3 clips", 65, 25, 4, 45, 0, n_clips=3),
        _f("fin B F65 ragged", 65, 25, 6, 55, 1, n_clips=2, table=((30, 1), (55, 6)), kinds=HARD),
        _f("fin mode 3 on the mono model (refused)", 65, 25, 4, 45, 3),
        # ---- the stereo model
        _f("ild fold F65", 65, 25, 4, 45, 3, C=2, kinds=HARD), _f("ild fold raw F65", 65, 20, 3, 50, 2, C=2, kinds=("rand", "int")),
        _f("ild op F65", 65, None, 2, 0, 3, C=2, kinds=HARD), _f("ild op raw F65", 65, None, 2, 0, 2, C=2, kinds=("rand", "int")),
        _f("ild A (refused)", 65, 25, 4, 45, 0, C=2),
        # ---- the one-batch kernel
        _f("lat A F513 ov25", 513, 25, 4, 45, 0, family=ONE_BATCH, gs=1, kinds=HARD), _f("lat B F65 ov15 T49", 65, 15, 3, 49, 1, family=ONE_BATCH, gs=1, kinds=HARD),
        _f("lat A F65 ov20 T63 dead rows", 65, 20, 3, 63, 0, family=ONE_BATCH, gs=1),
        _f("lat A ov26 (8 covers, refused)", 65, 26, 5, 46, 0, family=ONE_BATCH, gs=1),
        _f("lat raw (refused)", 65, 25, 4, 45, 2, family=ONE_BATCH, gs=1), _f("lat without planes (refused)", 65, 25, 4, 45, 0, family=ONE_BATCH),
        # ---- 128-bin workgroups and the bf16 x 3 kernel at their natural size
        _f("fin A natural bf16x3", 1025, 10, nn, nr, 0, gs=1, kinds=("pos",)), _f("fin B natural f32 cbw 2", 1025, 10, nn, nr, 1, kinds=("pos",)),
        _f("fin A natural size forced to 64 bins", 1025, 10, nn, nr, 0, switch="cbw_1", gs=1, kinds=("pos",)),
        # ---- ... and forced at the small sizes
        _f("cbw2 A F65 ov25 T45", 65, 25, 4, 45, 0, switch="cbw_2", kinds=HARD), _f("cbw2 B F513 ov15 T49", 513, 15, 3, 49, 1, switch="cbw_2"),
        _f("cbw2 raw F65 ov2", 65, 2, 3, 91, 2, switch="cbw_2", kinds=("rand", "int")), _f("cbw2 A F128 even", 128, 25, 4, 45, 0, switch="cbw_2"),
        _f("cbw2 op A F65", 65, None, 2, 0, 0, switch="cbw_2"), _f("cbw2 op B F128", 128, None, 2, 0, 1, switch="cbw_2", kinds=HARD),
        _f("cbw2 op raw F513", 513, None, 2, 0, 2, switch="cbw_2", kinds=("rand", "int")),
        _f("x3 A F65 ov25 T45", 65, 25, 4, 45, 0, switch="cbw_2", gs=1, kinds=HARD), _f("x3 B F513 ov15 T49", 513, 15, 3, 49, 1, switch="cbw_2", gs=1, kinds=HARD),
        _f("x3 A F128 ov20 T63", 128, 20, 3, 63, 0, switch="cbw_2", gs=1), _f("x3 A F65 ov26 (8 covers)", 65, 26, 5, 46, 0, switch="cbw_2", gs=1),
        _f("x3 B F65 ragged", 65, 25, 6, 55, 1, switch="cbw_2", gs=1, n_clips=2, table=((30, 1), (55, 6))),
        _f("x3 A F65 3 clips", 65, 25, 4, 45, 0, switch="cbw_2", gs=1, n_clips=3),
    ]
    return out


CHAIN = dict(name="chain deconv2 -> final", tc=30, F=65, ov=25, n=4, rows=45, mode=0)
