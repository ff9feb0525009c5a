"""References for the kernels of the deep score-informed graph build_ca_1x1, one launch at a time (``dcs_debug_d1_conv`` /
``dcs_debug_d1_aux``; tests/test_gpu_d1_kernels.py on the device, tests/test_d1_ref_cpu.py for what holds without one).

Everything here is written from the layouts ``D1Args`` and the header comments of csrc/deep1x1.hip / train_deep1x1.hip
document, not from the kernel's loops: a launch is a product ``A . B^T`` of an operand ``A [M][K]`` gathered from channels-last
activations (K = (filter row, tap, channel), the channel fastest) and a weight operand ``B [Npad][Kpad]``, followed by the
mode's epilogue.  ``product`` takes the multiplication as a plug, as tests/conv_ref.py does: float64 (the reference), absolute
values (``S = sum |a||b|``, to which the epilogue adds ``|b0| + |b1|``), or the in-order float32 chain ``conv_ref._chain`` (the
project's yardstick).

A case is a dict: the convolution it belongs to (``H x W`` images of ``cin`` channels -> ``cout`` channels, ``kh x kw`` filter,
column stride 2 for kw == 5 and 1 for kw == 1), the mode, and for the transposed modes the output-column parity.  A forward-type
launch (FWD, 1X1, FWDC) reads ``[images][H][W][cin]``; a transposed-type launch (TR, LAST, Q, B11) reads the convolution's output
``[images][Hc][Wc][cout]`` and writes columns of ``[H][W]``.
"""
import zlib

import numpy as np

import conv_ref as cr
import gemm_ref as gr

U = gr.U
FACTOR = gr.FACTOR
EINVAL = -1
FWD, X11, TR, LAST, FWDC, Q, B11 = range(7)
MODE_NAMES = ("FWD", "1X1", "TR", "LAST", "FWDC", "Q", "B11")
FORWARD_TYPE = (FWD, X11, FWDC)
KW, NF, BM = 5, 200, 128
AUX_TO_CL, AUX_MASK, AUX_CODE_APPLY, AUX_CODES_OUT, AUX_PACK_HOST, AUX_PACK_DEVICE = range(6)
FILTERS = (30, 50, 70, 100, 200, 200)
KH = (1, 1, 1, 1, 10, 10)
# (mode, NT, unit) of every d1::launch<> the separator (unit 0) and the trainer (unit 1) issue: N = 30 -> NT 2, 50 .. 800 -> NT 4,
# N = 4 (LAST, Q) -> NT 1
PRODUCTION = {(FWD, 2, 0), (FWD, 4, 0), (X11, 4, 0), (TR, 2, 0), (TR, 4, 0), (LAST, 1, 0),
              (FWD, 2, 1), (FWD, 4, 1), (TR, 2, 1), (TR, 4, 1), (FWDC, 2, 1), (FWDC, 4, 1), (Q, 1, 1), (B11, 4, 1)}


def cdiv(a, b):
    return -(-a // b)


def round_up(a, b):
    return cdiv(a, b) * b


def nt_for(N):
    return 1 if N <= 16 else 2 if N <= 32 else 4


def npad(N):
    return round_up(N, 16 * nt_for(N))


def ntap_of(kw, par):
    return kw if kw == 1 else (kw - par + 1) // 2


# ------------------------------------------------------------------------------------------------ geometry
def geom(c):
    """what the launch of case c is, from the documented layouts: dict(Hi, Wi, Ci (pitch), Cl (live input channels), Ho, Wo, Wq, ntap,
    K, Kpad, M, N, Co, nt, grid)"""
    s = 1 if c["kw"] == 1 else 2
    Hc, Wc = c["H"] - c["kh"] + 1, (c["W"] - c["kw"]) // s + 1
    g = dict(stride=s)
    if c["mode"] in FORWARD_TYPE:
        g.update(Hi=c["H"], Wi=c["W"], Cl=c["cin"], Ho=Hc, Wo=Wc, Wq=Wc, ntap=c["kw"], N=c["cout"])
    else:
        Wq = c["W"] if s == 1 else (c["W"] - c["par"] + 1) // 2
        g.update(Hi=Hc, Wi=Wc, Cl=c["cout"], Ho=c["H"], Wo=c["W"], Wq=Wq, ntap=ntap_of(c["kw"], c["par"]), N=c["cin"])
    g["Ci"] = round_up(g["Cl"], 4)
    g["K"] = c["kh"] * g["ntap"] * g["Ci"]
    g["Kpad"] = round_up(g["K"], 16)
    g["M"] = c["images"] * g["Ho"] * g["Wq"]
    g["Co"] = round_up(g["N"], 4)
    g["nt"] = nt_for(g["N"])
    g["grid"] = (cdiv(g["M"], BM), cdiv(g["N"], 16 * g["nt"]))
    return g


# ------------------------------------------------------------------------------------------------ operand layouts
def pack_B(W):
    """forward operand of Lasagne weights W [cout][cin][kh][kw] (a true convolution: the filter is flipped):
    B[co][(i kw + j) Cinp + ci] = W[co][ci][kh-1-i][kw-1-j], [npad(cout)][Kpad], zero elsewhere"""
    cout, cin, kh, kw = W.shape
    cinp = round_up(cin, 4)
    B = np.zeros((npad(cout), round_up(kh * kw * cinp, 16)), dtype=W.dtype)
    body = np.zeros((cout, kh, kw, cinp), dtype=W.dtype)
    body[..., :cin] = W[:, :, ::-1, ::-1].transpose(0, 2, 3, 1)
    B[:cout, :kh * kw * cinp] = body.reshape(cout, -1)
    return B


def pack_Bt(W, par):
    """transposed operand of output-column parity par: Bt[ci][(i ntap + jt) Coutp + co] = W[co][ci][kh-1-i][kw-1-(par + 2 jt)],
    [npad(cin)][Ktpad], zero elsewhere (kw == 1: the one tap, par 0)"""
    cout, cin, kh, kw = W.shape
    coutp, nt = round_up(cout, 4), ntap_of(kw, par)
    Bt = np.zeros((npad(cin), round_up(kh * nt * coutp, 16)), dtype=W.dtype)
    body = np.zeros((cin, kh, nt, coutp), dtype=W.dtype)
    flipped = W[:, :, ::-1, ::-1]                                        # [co][ci][i][j]
    body[..., :cout] = flipped[:, :, :, par::2].transpose(1, 2, 3, 0)
    Bt[:cin, :kh * nt * coutp] = body.reshape(cin, -1)
    return Bt


def internal_W(W):
    """the trainer's internal layout [kh i][kw j][cin][cout] = W[co][ci][kh-1-i][kw-1-j] (what pack_kernel reads)"""
    return np.ascontiguousarray(W[:, :, ::-1, ::-1].transpose(2, 3, 1, 0))


# ------------------------------------------------------------------------------------------------ the products
def mul64(A, B):
    return A.astype(np.float64) @ B.astype(np.float64)


def mul_abs(A, B):
    return np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64))


def mul_chain(A, B):
    """one float32 multiply-add per k, k ascending (conv_ref._chain)"""
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    return cr._chain(np.zeros((A.shape[0], B.shape[1]), dtype=np.float32), A, B)


def gather_forward(x, kh, ntap, stride):
    """x [img][Hi][Wi][Ci] -> A [img Ho Wo][(i, j, c)]: the window of output pixel (t, q) starts at row t, column stride q"""
    n, Hi, Wi, Ci = x.shape
    Ho, Wo = Hi - kh + 1, (Wi - ntap) // stride + 1
    A = np.zeros((n, Ho, Wo, kh, ntap, Ci), dtype=x.dtype)
    for i in range(kh):
        for j in range(ntap):
            A[:, :, :, i, j, :] = x[:, i:i + Ho, j:j + stride * (Wo - 1) + 1:stride, :]
    return A.reshape(n * Ho * Wo, kh * ntap * Ci)


def gather_transposed(d, kh, ntap, Ho, Wq):
    """d [img][Hi][Wi][Ci] (already times r') -> A [img Ho Wq][(i, jt, c)]: output pixel (t, q) takes d[t - i][q - jt] where that
    exists and nothing elsewhere"""
    n, Hi, Wi, Ci = d.shape
    A = np.zeros((n, Ho, Wq, kh, ntap, Ci), dtype=d.dtype)
    for i in range(kh):
        for jt in range(ntap):
            nt_, nq_ = min(Ho - i, Hi), min(Wq - jt, Wi)
            if nt_ > 0 and nq_ > 0:
                A[:, i:i + nt_, jt:jt + nq_, i, jt, :] = d[:, :nt_, :nq_, :]
    return A.reshape(n * Ho * Wq, kh * ntap * Ci)


def operand_A(c, inp, ty=np.float64):
    """the launch's first operand [M][K]: the windows of `in` (forward type) or of `in` times 0.5 code (transposed type)"""
    g = geom(c)
    x = inp["in"].reshape(c["images"], g["Hi"], g["Wi"], g["Ci"]).astype(ty)
    if c["mode"] in FORWARD_TYPE:
        return gather_forward(x, c["kh"], g["ntap"], g["stride"])
    half = (np.float32(0.5) * inp["code"].astype(np.float32)).astype(ty).reshape(x.shape)
    return gather_transposed((x * half).astype(ty), c["kh"], g["ntap"], g["Ho"], g["Wq"])


def unpack(pack, shape, dB):
    """the adjoint of an operand layout: the gradient with respect to W [cout][cin][kh][kw] of a function of pack(W), given its
    gradient dB with respect to the operand (a layout places a weight at no more than one position; weights it does not hold --
    the taps of the other parity -- get 0)"""
    n = int(np.prod(shape))
    idx = pack(np.arange(1, n + 1, dtype=np.float64).reshape(shape)).astype(np.int64)
    assert np.unique(idx[idx > 0]).size == int((idx > 0).sum())
    dW = np.zeros(n + 1)
    dW[idx.reshape(-1)] = np.asarray(dB, dtype=np.float64).reshape(-1)
    return dW[1:].reshape(shape)


def launch_ref(c, inp, mul=mul64):
    """the launch of case c on inp (see ``inputs``) under the multiplication `mul`: dict(out=..., code=... (FWD)) in the natural
    shapes of ``natural``; float64 values unless mul is mul_chain (then every step in float32)."""
    g, mode = geom(c), c["mode"]
    f32 = mul is mul_chain
    ty = np.float32 if f32 else np.float64
    absolute = mul is mul_abs
    N, K = g["N"], g["K"]
    A = operand_A(c, inp, ty)
    v = mul(A, inp["B"][:N, :K].T).astype(ty)                           # [M][N]
    b0 = np.abs(inp["b0"].astype(ty)) if absolute and "b0" in inp else inp.get("b0", np.zeros(N)).astype(ty)
    b1 = np.abs(inp["b1"].astype(ty)) if absolute and "b1" in inp else inp.get("b1", np.zeros(N)).astype(ty)
    rect = (lambda p: p) if absolute else (lambda p: np.maximum(p, ty(0)))
    res = {"v": v}
    M = g["M"]
    if mode == FWD:
        pre = (v + b0[None]).astype(ty)
        out = np.zeros((M, g["Co"]), dtype=ty)
        out[:, :N] = rect(pre) + b1[None]
        code = np.zeros((M, g["Co"]), dtype=np.uint8)
        code[:, :N] = np.where(pre > 0, 2, np.where(pre == 0, 1, 0))
        res.update(out=out, code=code, pre=pre)
    elif mode == X11:
        y = (rect((v + b0[None]).astype(ty)) + b1[None]).astype(ty)
        res["out"] = np.ascontiguousarray(y.reshape(M, N // NF, NF).transpose(1, 0, 2)) if N % NF == 0 else y[None]
    elif mode == FWDC:
        out = np.zeros((M, g["Co"]), dtype=ty)
        out[:, :N] = v * (np.float32(0.5) * inp["code"].reshape(M, g["Co"])[:, :N].astype(np.float32)).astype(ty)
        res["out"] = out
    elif mode == B11:
        out = np.zeros((M, g["Co"]), dtype=ty)
        out[:, :N] = v
        res["out"] = out
    elif mode == TR:
        out = np.zeros((c["images"], g["Ho"], g["Wq"], g["Co"]), dtype=ty)
        out[..., :N] = v.reshape(c["images"], g["Ho"], g["Wq"], N)
        res["out"] = out
    elif mode == Q:
        res["out"] = np.ascontiguousarray((v + b0[None]).astype(ty).reshape(c["images"], g["Ho"], g["Wq"], N).transpose(0, 3, 1, 2))
    else:
        res["out"] = np.ascontiguousarray(rect((v + b0[None]).astype(ty)).reshape(c["images"], g["Ho"], g["Wq"], N).transpose(3, 0, 1, 2))
    return res


def out_shape(c):
    """the whole output buffer of the launch as the device lays it out (floats)"""
    g, mode = geom(c), c["mode"]
    if mode in (FWD, FWDC, B11):
        return (g["M"], g["Co"])
    if mode == X11:
        return (cdiv(g["N"], NF), g["M"], NF)
    if mode == TR:
        return (c["images"], g["Ho"], g["Wo"], g["Co"])
    if mode == Q:
        return (c["images"], g["N"], g["Ho"], g["Wo"])
    return (c["ch_off"] + g["N"], c["n_total"], g["Ho"], g["Wo"])


def owned(c):
    """the index of the elements the launch owns inside an array of out_shape(c): everything else keeps what it held"""
    mode = c["mode"]
    if mode in (FWD, FWDC, B11, X11):
        return (Ellipsis,)
    par = c["par"]
    if mode == TR:
        return (slice(None), slice(None), slice(par, None, 2), slice(None))
    if mode == Q:
        return (slice(None), slice(None), slice(None), slice(par, None, 2))
    return (slice(c["ch_off"], None), slice(c["k_first"], c["k_first"] + c["images"]), slice(None), slice(par, None, 2))


# ------------------------------------------------------------------------------------------------ data
KINDS = ("signed", "int", "ties")


def kinds_of(c):
    return KINDS if c["mode"] == FWD else KINDS[:2]


def _rs(*parts):
    return np.random.RandomState(zlib.crc32(repr(parts).encode()) & 0x7fffffff)


def case_weights(c, kind):
    """Lasagne weights [cout][cin][kh][kw] of the case's convolution"""
    r = _rs("W", c["cin"], c["cout"], c["kh"], c["kw"], kind)
    shape = (c["cout"], c["cin"], c["kh"], c["kw"])
    if kind == "signed":
        return r.uniform(-1, 1, size=shape).astype(np.float32)
    return r.randint(-2, 3, size=shape).astype(np.float32)


def inputs(c, kind):
    """dict(in [px][Ci], code (transposed type: [px][Ci]; FWDC: [M][Co]), B, b0, b1) as the device takes them.  Pad channels hold
    value 0 and code 0, as production guarantees; the codes are random over {0, 1, 2}.  kind "ties": integer data, b0 minus a sum
    the product attains (pixel col % M of channel col) in every third channel, so that pre == 0 occurs there."""
    g, mode = geom(c), c["mode"]
    r = _rs("x", c["name"], kind)
    px = c["images"] * g["Hi"] * g["Wi"]
    x = np.zeros((px, g["Ci"]), dtype=np.float32)
    live = (px, g["Cl"])
    x[:, :g["Cl"]] = r.standard_normal(live) if kind == "signed" else r.randint(-3, 4, size=live)
    W = case_weights(c, kind)
    inp = {"in": x}
    if mode in FORWARD_TYPE:
        inp["B"] = pack_B(W)
    else:
        inp["B"] = pack_Bt(W, c["par"])
        code = np.zeros((px, g["Ci"]), dtype=np.uint8)
        code[:, :g["Cl"]] = r.randint(0, 3, size=live)
        inp["code"] = code
    if mode == FWDC:
        code = np.zeros((g["M"], g["Co"]), dtype=np.uint8)
        code[:, :g["N"]] = r.randint(0, 3, size=(g["M"], g["N"]))
        inp["code"] = code
    N = g["N"]
    if mode in (FWD, X11, LAST, Q):
        inp["b0"] = (r.uniform(-1, 1, size=N) if kind == "signed" else r.randint(-4, 5, size=N)).astype(np.float32)
    if mode in (FWD, X11):
        inp["b1"] = (r.uniform(-1, 1, size=N) if kind == "signed" else r.randint(-4, 5, size=N)).astype(np.float32)
    if kind == "ties":
        A = gather_forward(x.reshape(c["images"], g["Hi"], g["Wi"], g["Ci"]), c["kh"], g["ntap"], g["stride"])
        v = mul64(A, inp["B"][:N, :g["K"]].T)
        tie = np.arange(N) % 3 == 0                                     # the other channels keep their b0: one pixel has every sign
        inp["b0"] = np.where(tie, -v[np.arange(N) % g["M"], np.arange(N)], inp["b0"]).astype(np.float32)
    return inp


def max_partial(c, inp):
    """an upper bound of every partial sum of the launch, in any order: sum |a||b| + |b0| + |b1|"""
    top = float(np.max(launch_ref(c, inp, mul_abs)["v"]))
    return top + sum(float(np.max(np.abs(inp[k]))) for k in ("b0", "b1") if k in inp)


def live_mask(c, inp):
    """the outputs something goes into, in the natural shape of launch_ref: channels below N; TR and B11: pixels a tap reaches;
    FWDC: a code that is not 0.  Everywhere else S is 0 and the output must be exactly 0 (``gemm_ref.measure`` asks that)."""
    g, mode = geom(c), c["mode"]
    N = g["N"]
    if mode in (FWD, FWDC, B11):
        live = np.zeros((g["M"], g["Co"]), dtype=bool)
        live[:, :N] = True if mode != FWDC else inp["code"].reshape(g["M"], g["Co"])[:, :N] != 0
        return live
    if mode == TR:
        ones = np.ones((c["images"], g["Hi"], g["Wi"], 1))
        reach = gather_transposed(ones, c["kh"], g["ntap"], g["Ho"], g["Wq"]).any(axis=1).reshape(c["images"], g["Ho"], g["Wq"])
        live = np.zeros((c["images"], g["Ho"], g["Wq"], g["Co"]), dtype=bool)
        live[..., :N] = reach[..., None]
        return live
    return np.ones(launch_ref(c, inp, mul_abs)["out"].shape, dtype=bool)


# ------------------------------------------------------------------------------------------------ the case table
def _case(name, mode, images, H, W, cin, cout, kh, kw=KW, par=0, unit=0, n_total=0, k_first=0, ch_off=0):
    return dict(name=name, mode=mode, images=images, H=H, W=W, cin=cin, cout=cout, kh=kh, kw=kw, par=par, unit=unit, n_total=n_total,
                k_first=k_first, ch_off=ch_off, group="fwd" if mode in FORWARD_TYPE else "tr")


def cases():
    cs = []
    # forward type.  (images, H, W) per channel pair of the graph: M = 1 (Ho = Wo = 1), 102 (a 16-pixel tile straddles images of
    # 34 pixels), 153 (two workgroups, M % 16 = 9), 24 (images of 8 pixels), 128 (one whole workgroup), 6 and 30 (kh 10, Ho 1 / 2)
    graph = [(4, 30, 1, 3, 2, 37), (30, 50, 1, 3, 3, 38), (50, 70, 1, 3, 1, 19), (70, 100, 1, 2, 4, 35), (100, 200, 10, 3, 10, 7),
             (200, 200, 10, 3, 11, 13)]
    for mode in (FWD, FWDC):
        for cin, cout, kh, n, H, W in graph:
            cs.append(_case("%s %d->%d %dx%dx%d" % (MODE_NAMES[mode], cin, cout, n, H, W), mode, n, H, W, cin, cout, kh, unit=int(mode == FWDC)))
    cs += [_case("FWD 4->30 1x1x5 one pixel", FWD, 1, 1, 5, 4, 30, 1), _case("FWD 30->50 1x1x6", FWD, 1, 1, 6, 30, 50, 1),
           _case("FWD 50->70 1x2x8", FWD, 1, 2, 8, 50, 70, 1), _case("FWDC 4->30 1x1x5 one pixel", FWDC, 1, 1, 5, 4, 30, 1, unit=1),
           _case("FWDC 70->100 1x2x6", FWDC, 1, 2, 6, 70, 100, 1, unit=1),
           _case("FWD trainer 4->30 3x2x37", FWD, 3, 2, 37, 4, 30, 1, unit=1), _case("FWD trainer 30->50 3x3x38", FWD, 3, 3, 38, 30, 50, 1, unit=1),
           _case("FWD trainer 1x1 200->200 3x3x7", FWD, 3, 3, 7, 200, 200, 1, kw=1, unit=1)]
    for N in (16, 17, 32, 33):                                           # the boundaries of nt_for; Ci = 12: K = 60, K % 16 = 12
        cs.append(_case("FWD 12->%d 1x2x8" % N, FWD, 1, 2, 8, 12, N, 1))
        cs.append(_case("FWDC 12->%d 3x2x7" % N, FWDC, 3, 2, 7, 12, N, 1, unit=1))
    cs += [_case("1X1 200->200 3x3x7", X11, 3, 3, 7, 200, 200, 1, kw=1), _case("1X1 200->800 1x2x9", X11, 1, 2, 9, 200, 800, 1, kw=1),
           _case("1X1 200->800 3x3x17", X11, 3, 3, 17, 200, 800, 1, kw=1), _case("1X1 200->200 2x8x8", X11, 2, 8, 8, 200, 200, 1, kw=1),
           _case("1X1 200->200 1x1x5", X11, 1, 1, 5, 200, 200, 1, kw=1)]
    # transposed type, both parities.  W = 5: Wc = 1; even W: the last column has no tap (the parity-1 launch's last q is dead)
    tgraph = [(30, 50, 1, 3, 2, 6), (50, 70, 1, 3, 3, 38), (70, 100, 1, 1, 1, 5), (100, 200, 10, 3, 10, 7), (200, 200, 10, 3, 11, 8),
              (50, 70, 1, 2, 4, 32), (30, 50, 1, 1, 2, 37)]
    for cin, cout, kh, n, H, W in tgraph:
        for par in (0, 1):
            cs.append(_case("TR %d<-%d %dx%dx%d par %d" % (cin, cout, n, H, W, par), TR, n, H, W, cin, cout, kh, par=par))
    cs += [_case("TR trainer 30<-50 3x2x6 par 1", TR, 3, 2, 6, 30, 50, 1, par=1, unit=1),
           _case("TR trainer 50<-70 3x3x38 par 0", TR, 3, 3, 38, 50, 70, 1, par=0, unit=1)]
    for N in (16, 17, 32, 33):                                           # Ci = 16: the smallest tap D1Args allows a transposed launch
        cs.append(_case("TR %d<-16 1x2x8 par 0" % N, TR, 1, 2, 8, N, 16, 1, par=0))
        cs.append(_case("TR %d<-16 3x2x7 par 1" % N, TR, 3, 2, 7, N, 16, 1, par=1))
    for n, H, W, nt, kf, ch in ((3, 2, 37, 5, 1, 0), (1, 1, 6, 3, 2, 4), (2, 3, 8, 2, 0, 12), (3, 3, 38, 4, 1, 12), (1, 1, 5, 2, 1, 4),
                                (2, 4, 32, 3, 1, 0)):
        for par in (0, 1):
            cs.append(_case("LAST 4<-30 %dx%dx%d par %d tile %d of %d ch %d" % (n, H, W, par, kf, nt, ch), LAST, n, H, W, 4, 30, 1, par=par,
                            n_total=nt, k_first=kf, ch_off=ch))
    for n, H, W in ((3, 2, 6), (1, 1, 5), (3, 3, 38), (2, 3, 7), (2, 4, 32), (1, 2, 8)):
        for par in (0, 1):
            cs.append(_case("Q 4<-30 %dx%dx%d par %d" % (n, H, W, par), Q, n, H, W, 4, 30, 1, par=par, unit=1))
    cs += [_case("B11 200<-200 3x3x7", B11, 3, 3, 7, 200, 200, 1, kw=1, unit=1), _case("B11 200<-200 3x3x17", B11, 3, 3, 17, 200, 200, 1, kw=1, unit=1),
           _case("B11 200<-200 1x1x5", B11, 1, 1, 5, 200, 200, 1, kw=1, unit=1), _case("B11 200<-200 2x8x8", B11, 2, 8, 8, 200, 200, 1, kw=1, unit=1)]
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


# ------------------------------------------------------------------------------------------------ the small kernels
def to_cl(x):
    """tiles [n][4][plane] -> channels-last [n][plane][4]"""
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def codes_out(code, C):
    """code bytes [n][hw][Cp] -> [n][C][hw] floats 0 / 0.5 / 1"""
    return np.ascontiguousarray((np.float32(0.5) * code[:, :, :C].astype(np.float32)).transpose(0, 2, 1))


def code_apply(buf, code, C, per, nsum):
    """the in-place product and the partial sums in the documented order: workgroup w owns rows w per .. (w + 1) per; thread (sub,
    c) of its 256 // Cp sub-rows adds rows r0 + sub, r0 + sub + nsub, .. in order, then the sub-rows are added in order"""
    rows, Cp = buf.shape
    nsub = 256 // Cp
    out = (buf * (np.float32(0.5) * code.astype(np.float32))).astype(np.float32)
    out[nsum * per:] = buf[nsum * per:]                                 # rows no workgroup owns stay as they were
    part = np.zeros((nsum, C), dtype=np.float32)
    for w in range(nsum):
        r0, r1 = w * per, min(rows, (w + 1) * per)
        sub = np.zeros((nsub, Cp), dtype=np.float32)
        for k in range(nsub):
            for r in range(r0 + k, r1, nsub):
                sub[k] += buf[r]
        t = np.zeros(Cp, dtype=np.float32)
        for k in range(nsub):
            t += sub[k]
        part[w] = t[:C]
    return out, part


# (Cp, C): the channel pitches of the graph; (rows, per, nsum): rows below / equal to / above nsum per, and workgroups without a row
CODE_APPLY_CHANNELS = ((32, 30), (52, 50), (72, 70), (100, 100), (200, 200))
CODE_APPLY_ROWS = ((37, 10, 4), (40, 10, 4), (45, 10, 4), (15, 10, 4), (700, 64, 11))
# (cin, cout, kh, kw): the six layers, the live rows of the 1x1 layer and the whole 1x1 layer
PACK_LAYERS = ((4, 30, 1, 5), (30, 50, 1, 5), (50, 70, 1, 5), (70, 100, 1, 5), (100, 200, 10, 5), (200, 200, 10, 5), (200, 200, 1, 1),
               (200, 800, 1, 1))


def pack_weights(cin, cout, kh, kw):
    return _rs("pack", cin, cout, kh, kw).standard_normal((cout, cin, kh, kw)).astype(np.float32)


def code_apply_inputs(Cp, C, rows):
    r = _rs("code_apply", Cp, C, rows)
    return r.standard_normal((rows, Cp)).astype(np.float32), r.randint(0, 3, size=(rows, Cp)).astype(np.uint8)


MASK_KINDS = ("rand", "pos", "sparse", "tiny")


def mask_inputs(kind, n, plane, C):
    """p [4][n][plane] >= 0 (rectified outputs) and the tiles x [n][C][plane] >= 0 (magnitudes).  rand: a rectified signed
    pre-activation (half the entries exact zeros); pos: strictly positive; sparse: most bins all-zero; tiny: denominators around
    the masks' epsilon (5e-19), zeros among them"""
    r = _rs("mask", kind, n, plane, C)
    if kind == "rand":
        p = np.maximum(r.standard_normal((4, n, plane)), 0)
    elif kind == "pos":
        p = r.uniform(0.01, 1.0, size=(4, n, plane))
    elif kind == "sparse":
        p = np.maximum(r.standard_normal((4, n, plane)), 0) * (r.uniform(size=(1, n, plane)) < 0.2)
    else:
        p = 10.0 ** r.uniform(-21, -16, size=(4, n, plane)) * (r.uniform(size=(4, n, plane)) < 0.7)
    x = r.uniform(0, 2.0, size=(n, C, plane))
    return p.astype(np.float32), x.astype(np.float32)


def mask_ref(p, x, mode, mix_n):
    """float64 masks of deep1x1_ref.masked on p [4][n][plane]: [4][n][plane], and the mixture [n][plane]"""
    import deep1x1_ref
    p64 = p.astype(np.float64).transpose(1, 0, 2)[:, :, None, :]         # [n][4][1][plane]
    x64 = x.astype(np.float64)[:, :, None, :]
    want = deep1x1_ref.masked(p64, x64, mode, "ch0" if mix_n == 1 else "sum")
    mix = x64[:, 0] if mix_n == 1 else x64.sum(axis=1)
    return want[:, :, 0, :], mix[:, 0, :]
