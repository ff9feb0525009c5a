"""Shared by tests/test_train_edges_cpu.py and tests/test_gpu_train_edges.py (test infrastructure): the three trainable
graphs side by side, the constructions that put exact zeros at one site of a graph at a time, the shapes at the ends of
the accepted ranges, a restatement of csrc/train_core.hip's pick_split with the split-K GEMMs of each graph, and the
gradient comparison (relative norm and elementwise) every gradient test uses."""
import numpy as np

import train_bach10_ref
import train_ikala_ref
import train_ref


class Graph(object):
    def __init__(self, name, arch, ref, nsrc, nparams, hyper_names, ncomp):
        self.name, self.arch, self.ref, self.nsrc, self.nparams = name, arch, ref, nsrc, nparams
        self.hyper_names, self.ncomp = hyper_names, ncomp   # keywords of ref.components; loss + components
        self.branch = list(range(8, nparams - 1))           # W_k, b_k of the rectified dense layers behind z
        self.bo = nparams - 1                               # the output BiasLayer
        self.biases = [1, 2, 4, 5, 7] + list(range(9, nparams - 1, 2)) + [self.bo]


GRAPHS = {
    "dsd": Graph("dsd", "dsd", train_ref, 4, 15, ("eps", "alpha", "beta", "beta_voc"), 7),
    "ikala": Graph("ikala", "ikala_nopool", train_ikala_ref, 2, 13, ("eps", "alpha", "beta_acc", "beta_voc"), 5),
    "bach10": Graph("bach10", "bach10", train_bach10_ref, 4, 17, ("eps",), 5),
}


def setup(graph, B, tc, F, seed, bias=0.05):
    """The well-conditioned inputs of the three test_gpu_train*.py files: Glorot weights, biases 0.05 N(0, 1), output biases
    positive (0.1 + |.| for iKala and Bach10), smooth positive inputs and targets, r uniform."""
    from deepconvsep_amd import training
    g = GRAPHS[graph]
    rs = np.random.RandomState(seed)
    params = training.glorot_init(g.arch, tc, F, seed)
    for i in g.biases:
        params[i] = (bias * rs.randn(*params[i].shape)).astype(np.float32)
    params[g.bo] = np.abs(params[g.bo]) + np.float32(0.0 if graph == "dsd" else 0.1)
    x = (0.3 * rs.uniform(0, 1, size=(B, 1, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    tgt = (0.3 * rs.uniform(0, 0.5, size=(B, g.nsrc, tc, F))).astype(np.float32)
    return params, x, r, tgt


# ---------------------------------------------------------------------------------------------- exact zeros, one site at a time
TIE_CASES = ("branch0", "fc0", "q0")
TIE_SHAPES = {"dsd": (3, 10, 33), "ikala": (2, 12, 93), "bach10": (3, 6, 37)}
# eps of the q0 case: the trainers' defaults for DSD and iKala (1e-8); Bach10's default 1e-18 would put dE/dq at
# 2 x t / (eps r) ~ 1e18, so that case passes eps = 1e-6 (and every q0 case bounds r from below by 0.01)
Q0_EPS = {"dsd": 1e-8, "ikala": 1e-8, "bach10": 1e-6}


def tie_case(graph, case, B=None, tc=None, F=None, seed=3):
    """(params, x, r, tgt, hyper) with exact zeros at one site, made by zeroing parameters:

    * ``branch0``: W_k = 0, b_k = 0 -> the pre-activation of every rectified branch layer is exactly 0 (its r' multiplies
      the gradient of W_k and b_k);
    * ``fc0``: Wfc = 0, bfc = 0, b_k > 0 -> the pre-activation of z is exactly 0 (its r' multiplies the gradient of Wfc, bfc);
    * ``q0``: branch layers zeroed and output bias zero -> every output pre-activation q is exactly 0 while x != 0: the masks
      come from eps r alone and the loss kernels take r'(q = 0).  r >= 0.01 and eps = ``Q0_EPS[graph]`` keep dE/dq (of the
      order x t / (eps r)) finite in float32."""
    g = GRAPHS[graph]
    shp = TIE_SHAPES[graph]
    B, tc, F = B or shp[0], tc or shp[1], F or shp[2]
    params, x, r, tgt = setup(graph, B, tc, F, seed)
    hyper = {}
    if case in ("branch0", "q0"):
        for i in g.branch:
            params[i] = np.zeros_like(params[i])
    if case == "fc0":
        params[6], params[7] = np.zeros_like(params[6]), np.zeros_like(params[7])
        for i in g.branch[1::2]:
            params[i] = np.abs(params[i]) + np.float32(0.01)
    if case == "q0":
        params[g.bo] = np.zeros_like(params[g.bo])
        r = (0.01 + 0.99 * r).astype(np.float32)
        hyper["eps"] = Q0_EPS[graph]
    return params, x, r, tgt, hyper


def zero_rows(x, tgt, rows):
    """Rows ``rows`` of the batch become all-zero windows, as a zero slot of the feed gives them."""
    x, tgt = x.copy(), tgt.copy()
    x[list(rows)] = 0
    tgt[list(rows)] = 0
    return x, tgt


# ---------------------------------------------------------------------------------------------- split-K plans
def _cdiv(a, b):
    return -(-a // b)


def pick_split(tiles, K, target, cap):
    """train::pick_split (csrc/train_core.hip): (splits, kchunk).  dcs_trainer::launch runs splits == 1 as one slice of K."""
    s = min(max(target // max(tiles, 1), 1), cap)
    kc = _cdiv(_cdiv(K, s), 32) * 32
    if kc < 256:
        kc = _cdiv(min(256, K), 32) * 32
    return _cdiv(K, kc), kc


def split_gemms(graph, B, tc, F):
    """{name: (tiles, K, target, cap)} of every split-K GEMM of the graph (the plan() of its csrc/train_*.hip)."""
    if graph == "dsd":
        kh = tc // 2
        h2 = tc - kh + 1
        return {"dW1": (_cdiv(F + 1, 64), 4 * B * tc, 512, 64), "dW2": (_cdiv(kh * 50 + 1, 64), 4 * B * h2, 512, 64)}
    if graph == "ikala":
        w1 = (F - 30) // 3 + 1
        h2, w2 = tc - 9, w1 - 19
        flat, rows = 30 * h2 * w2, _cdiv(B, 32) * 8
        return {"dW1": (1, 3 * B * tc * w1, 512, 128), "dW2": (_cdiv(6001, 128), 3 * B * h2 * w2, 2048, 128),
                "F3": (rows, flat, 512, 128), "B3": (rows, 2 * flat, 512, 128)}
    kh = 2 * tc // 3
    w1, h2 = (F - 30) // 4 + 1, tc - kh + 1
    flat, rows = 30 * h2 * w1, _cdiv(B, 32) * 8
    return {"dW1": (1, 5 * B * tc * w1, 512, 512), "dW2": (_cdiv(kh * 30 + 1, 128), 5 * B * h2 * w1, 2048, 512),
            "F3": (rows, flat, 512, 128), "B3": (rows, 4 * flat, 512, 128)}


CAPS = {"dsd": 64, "ikala": 128, "bach10": 512}      # the largest slice count of each graph's plan()
REGIMES = ("K<32", "32<=K<256", "splits==1", "short last slice", "last slice not a multiple of 32", "slices at the cap")


def regimes(graph, B, tc, F):
    """[(gemm, splits, kchunk, K, K % kchunk, set of REGIMES)] for one shape."""
    out = []
    for name, (tiles, K, target, cap) in split_gemms(graph, B, tc, F).items():
        splits, kc = pick_split(tiles, K, target, cap)
        last = K - (splits - 1) * kc
        hit = set()
        if K < 32:
            hit.add("K<32")
        elif K < 256:
            hit.add("32<=K<256")
        if splits == 1:
            hit.add("splits==1")
        elif last < kc:
            hit.add("short last slice")
        if last % 32:
            hit.add("last slice not a multiple of 32")
        if splits == cap:
            hit.add("slices at the cap")
        out.append((name, splits, kc, K, K % kc, hit))
    return out


# (B, tc, F): one case at every bound of dsd_trainer_new / ikala_trainer_new / bach10_trainer_new with the other axes small,
# and the cases that fill the table of regimes.  DSD: kh = 2 at tc 4; F = 1; K = 16, 24, 72, 168 in dW1 / dW2; (1024, 6, 33)
# runs dW1 in 64 slices of 384, its cap.
# iKala: (1, 10, 87) has w2 = h2 = 1 (dW2's K = 3, flat = 30); (1024, 10, 87) reaches dW1's 128 slices.
# Bach10: tc 2 has kh = 1, tc 47 kh = 31; F 30 and 31 .. 33 have w1 = 1; (1024, 32, 30) runs dW1 (K = 163 840) in 512 slices
# of 320, its cap; (2, 30, 2049) runs 474.
EDGE_SHAPES = {
    "dsd": [(1, 4, 1), (1, 4, 7), (1, 6, 31), (2, 64, 33), (1024, 4, 33), (2, 30, 2049), (3, 6, 65), (7, 10, 65),
            (1024, 6, 33)],
    "ikala": [(1, 10, 87), (2, 64, 87), (1, 10, 2049), (1024, 10, 87), (3, 11, 92), (2, 12, 131)],
    "bach10": [(1, 2, 30), (2, 3, 31), (1, 47, 30), (1024, 2, 30), (2, 4, 2049), (3, 5, 41), (2, 30, 2049),
               (1024, 32, 30)],
}
# one step past each bound: ValueError
BAD_SHAPES = {
    "dsd": [(1, 2, 33), (1, 5, 33), (1, 66, 33), (1, 4, 0), (1, 4, 2050), (0, 4, 33), (1025, 4, 33)],
    "ikala": [(1, 9, 87), (1, 65, 87), (1, 10, 86), (1, 10, 2050), (0, 10, 87), (1025, 10, 87)],
    "bach10": [(1, 1, 30), (1, 48, 30), (1, 2, 29), (1, 2, 2050), (0, 2, 30), (1025, 2, 30)],
}


# ---------------------------------------------------------------------------------------------- hyper-parameters
# eps, alpha, beta (iKala: beta_acc), beta_voc, learning_rate, rho, epsilon: distinct, of moderate size, none a default of
# any graph.  rho = 0.875 is a float32 number and 1 - rho is exact in float32.
HYPER = (4e-3, 0.07, 0.2, 0.11, 0.3, 0.875, 1e-4)


# ---------------------------------------------------------------------------------------------- gradient comparison
NORM_BOUND = 1e-4     # relative Frobenius norm per parameter, the bound of the three test_gpu_train*.py files
ELEMENT_K = 8         # device error <= ELEMENT_K x the float32 restatement's own error, elementwise


def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def e32_of(g32, g64):
    """Per parameter max |g32 - g64| / max |g64|: the error of plain float32 autograd of the restatement."""
    return [float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) for a, b in zip(g32, g64)]


def check_gradients(g, g64, g32, B, label=""):
    """Per parameter: shape, relative norm <= 1e-4, and max |g - g64| <= 8 e32 max |g64| with e32 the float32 restatement's
    own error at the same inputs (a different but equally valid float32 summation order costs a small multiple of it).
    One exception, for B > 256 and the parameters 6 .. nparams - 2 only (Wfc, bfc, W_k, b_k): their gradients are GEMMs that
    reduce over the batch alone (dWfc | dbfc, dW_k | db_k: K = B, unsplit, the bias the ones row), one float32 accumulation
    chain per output, a random walk of B roundings, while torch's CPU sums are pairwise and e32 does not grow with B; there
    the bound is (8 e32 + sqrt(B) 2^-24) max |g64|.  Measured at B = 1024: bfc and b_k at 9 to 23 e32 (1.3e-6 of max |g64|
    at most; the term is 1.9e-6), every other gradient, and every gradient at B <= 256, within 8 e32.
    A parameter whose float64 gradient is exactly zero must be exactly zero.  Prints every figure, then asserts."""
    e32 = e32_of(g32, g64)
    rows = []
    for i, (a, b) in enumerate(zip(g, g64)):
        assert a.shape == b.shape, (i, a.shape, b.shape)
        top = np.abs(b).max() if b.size else 0.0
        dev = float(np.abs(np.asarray(a, np.float64) - b).max() / max(top, 1e-300)) if top else float(np.abs(a).max())
        chain = np.sqrt(B) * 2.0 ** -24 if B > 256 and 6 <= i <= len(g64) - 2 else 0.0
        rows.append((i, rel(a, b) if top else dev, dev, e32[i] if top else 0.0, ELEMENT_K * e32[i] + chain if top else 0.0))
    print("gradients %s: (parameter, relative norm error, max elementwise error / max |g64|, e32)" % label)
    for row in rows:
        print("   %2d  %.2e  %.2e  %.2e" % row[:4])
    for i, rn, dev, e, bound in rows:
        assert rn <= NORM_BOUND, (label, i, rn)
        assert dev <= bound, (label, i, dev, e, bound)
    return rows
