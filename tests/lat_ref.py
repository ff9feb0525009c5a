"""Shared by tests/test_lat_ref_cpu.py and tests/test_gpu_lat_kernels.py (test infrastructure): the one-batch kernels of
csrc/dsd_lat.hip that no other module launches alone -- ``lat_gemm_kernel<J, NA>``, ``lat_stft_kernel<9|10>``,
``lat_ifft_kernel<9|10, 4>``, ``lat_ola_kernel<2|4>`` -- held directly to float64 (``dcs_debug_lat_*`` of include/dcs.h).
The yardsticks are the project's: ``gemm_ref.FACTOR`` / ``U`` / ``measure``, ``stft_ref``'s references and bounds.

lat_gemm, the contract in float64 (``reference``).  ``Aeff`` = the float64 sum of the ``a_parts`` operand arrays, rectified if
``relu_in``; ``arow(r) = a_gdiv ? (r // a_gdiv) * a_gmul + r % a_gdiv : r``.

* ``nz <= 1``: ``C[r][c] = act(a_scale * Aeff[arow(r)][0..K) . B[:, c] + bias[c])``;
* ``nz > 1``: part z is checked on its own against the sum over ITS slices ``z * waves .. z * waves + waves - 1`` (clipped to
  ``n_slices``; ``waves = ceil(n_slices / nz)``), the bias in part 0 only, no rectifier even when ``relu`` is set;
* ``S_rc = sum_k (sum_z |a_z|) |a_scale| |b| + |bias|`` over the same k (and the bias where it is added); where S is 0 the
  output must be exactly 0 (``gemm_ref.measure``).

The float32 restatement (``restatement``): the operand is ``fl(fl(a0 + a1) + fl(a2 + a3))``, rectified if ``relu_in``, scaled;
each slice is a float32 sum in ascending k; the slices are added in ascending order; then the bias, then the activation.

The a-priori cap per element, ``|got - f64| <= n 2^-24 S`` with ``n = 8 J + waves + 3 (+ 2 for NA = 4)``, re-derived from
``lat_gemm_kernel``: a product ``a b`` meets

* two roundings in ``(a[0] + a[1]) + (a[2] + a[3])`` (NA = 4 only; the rectifier behind it is 1-Lipschitz and adds none),
* one in ``sc * av[e]``,
* at most 8 J on its accumulator: the kernel has two, ``acc0`` (elements 0 and 2 of every float4) and ``acc1`` (1 and 3); each
  receives two ``v_mfma_f32_16x16x4_f32`` per j, each of those an fmaf chain over four k (the products themselves are not rounded),
* one in ``acc0 + acc1``,
* at most ``waves`` in ``sum += part[w]`` (the first addition, to 0, and the additions of the zeros of absent waves are exact),
* one in ``sum + biasv``; ``fmaxf`` rounds nothing.

The restatement rounds the product too and runs one chain of up to 16 J per slice, so its own worst case is not this cap's; that it
stays inside the cap on every signed case all the same is checked on the CPU (tests/test_lat_ref_cpu.py).

The yardstick: per instantiation (J, NA), pooled over that instantiation's signed cases (never fewer than 1024 outputs),
``E(device) <= FACTOR * E(restatement)`` with ``E = max |x - f64| / S``.

The exact probes: integers (A parts in +-1..3, B in +-1..2, integer bias, a_scale in {1, -1, 2}: exact in any order), one-hot rows
with a_scale 1 and no bias (every operand row holds at most one 1, so the output row is a row of B, or 0 in the parts that do
not own that k), and for the rectified forms a tie set (the integer data with the bias minus an attained sum: pre-activations
of exactly 0).  All must match the float64 reference bit for bit.

The chain case: a producer with nz = 4 leaves four parts Z_z, the consumer reads them with a_parts = 4 and relu_in through the same
buffer.  With ``S1`` the producer's S over all of K and ``n1``, ``n2`` the two caps' counts, each part is within ``n1 u S1_z`` of its
float64 value, so the four-part sum the consumer forms is within ``n1 u S1`` of the float64 pre-activation, and
``sum_z |Z_z| <= (1 + n1 u) S1``; hence ``|got - f64| <= n2 u ((1 + n1 u) S1 |B2| + |b2|) + (n1 u S1) |B2|``.

Forward and inverse STFT: the cases below with ``stft_ref``'s references.  The frames scratch of ``lat_ifft_kernel`` is held to
float64 ``irfft(X_t) * w`` per source and frame, ``FACTOR`` x the distance of the float32 restatement (``torch.fft.irfft`` of the
complex64 spectrum times the float32 window, as ``stft_ref.inverse_ref32``); the output of ``lat_ola_kernel`` to the in-frame-order
float32 sum of the frames THE DEVICE WROTE divided by the in-order float32 sum of ``float32(w64^2)``, bit for bit (the build has no
fast-math: HIP's float division is correctly rounded), and end to end to ``stft_ref.inverse_ref64`` in the weighted measure.
"""
import ctypes

import numpy as np

import gemm_ref as gr
import stft_ref as sr
from oracle import stft_np

FACTOR, U = gr.FACTOR, gr.U
EINVAL = -1
MIN_POOLED = 1024

# (J, NA) that net.hip's dsd_encode reaches (net.hip:417-484) and the ones only the test aid reaches
PRODUCTION = {(3, 1): "conv1, F = 513 (net.hip:417-423)", (5, 1): "conv1, F = 1025 (net.hip:417-423)",
              (4, 1): "conv2 / bottleneck behind a complete producer (net.hip:439-446, 461-469)",
              (4, 4): "conv2 / bottleneck behind a split producer (net.hip:444, 467)",
              (2, 1): "per-source layers (net.hip:478-484)", (2, 4): "per-source layers behind the split bottleneck (net.hip:483)"}
AID_ONLY = {(1, 1), (1, 4), (3, 4), (5, 4)}


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ lat_gemm: cases
def _g(name, src, M, K, slice_len, n_slices, n_cb, n_store=None, ldc=None, stride=None, a_scale=1.0, relu=0, nz=1, a_parts=1,
       relu_in=0, a_gdiv=0, a_gmul=0, seed=0):
    n_store = n_cb * 16 if n_store is None else n_store
    assert a_parts == 4 or not relu_in                                       # the kernel rectifies the four-part sum only
    c = dict(name=name, src=src, M=M, K=K, slice_len=slice_len, n_slices=n_slices, n_cb=n_cb, n_store=n_store,
             ldc=n_store if ldc is None else ldc, a_row_stride=K if stride is None else stride, a_scale=a_scale, relu=relu, nz=nz,
             a_parts=a_parts, relu_in=relu_in, a_gdiv=a_gdiv, a_gmul=a_gmul, seed=seed)
    c["J"] = cdiv(slice_len, 16)
    c["waves"] = cdiv(n_slices, max(nz, 1))
    c["n_A1"] = int(arow(c).max()) * c["a_row_stride"] + K                  # floats of one operand part
    c["a_part_stride"] = cdiv(c["n_A1"], 4) * 4 + 8 if a_parts > 1 else 0
    c["c_part"] = (M - 1) * c["ldc"] + n_store
    c["c_part_stride"] = cdiv(c["c_part"], 4) * 4 + 12 if nz > 1 else 0
    return c


def arow(c):
    r = np.arange(c["M"], dtype=np.int64)
    return (r // c["a_gdiv"]) * c["a_gmul"] + r % c["a_gdiv"] if c["a_gdiv"] > 0 else r


def extents(c):
    """the aid's host-side extents in floats (csrc/lat_debug.hip)"""
    nzz = max(c["nz"], 1)
    return dict(A=max(c["n_A1"], 4) + (c["a_parts"] - 1) * c["a_part_stride"], Bp=c["n_slices"] * c["n_cb"] * c["J"] * 256,
                bias=c["n_cb"] * 16, C=(nzz - 1) * c["c_part_stride"] + c["c_part"])


def grid(c):
    return [c["J"], c["a_parts"], cdiv(c["M"], 16), c["n_cb"], max(c["nz"], 1), c["waves"] * 64]


def gemm_cases():
    cs = []
    add = lambda *a, **k: cs.append(_g(*a, seed=len(cs) + 1, **k))
    # ---- the production forms (dsd_encode, net.hip)
    for K, sl in ((516, 36), (1028, 68)):          # 516: slice 14 partly past K, slice 15 wholly; 1028: slice 15 holds 8 of its 68
        for nz in (1, 4):
            add("conv1_K%d_nz%d" % (K, nz), "net.hip:417-423", 37, K, sl, 16, 4, n_store=52, a_scale=0.3, nz=nz)
    for nz in (1, 4):                              # rows overlap: 15 taps of 52; nz = 4: the last workgroup owns 3 slices and an idle wave
        for parts in (1, 4):
            add("conv2_nz%d_parts%d" % (nz, parts), "net.hip:439-446", 26, 780, 52, 15, 4, n_store=52, stride=52, nz=nz, a_parts=parts)
    for M in (1, 19):
        for nz in (1, 4):
            for parts in (1, 4):
                add("fc_M%d_nz%d_parts%d" % (M, nz, parts), "net.hip:461-469", M, 832, 52, 16, 8, stride=5 * 52, relu=1, nz=nz, a_parts=parts)
    for M in (1, 21):                              # 4 slices: the launcher refuses to split them (waves < 4), production never does
        for parts in (1, 4):
            add("fc1x_M%d_parts%d" % (M, parts), "net.hip:478-484", M, 128, 32, 4, 6, n_store=90, relu=1, a_parts=parts, relu_in=int(parts == 4))
    # ---- row tails
    for M in (1, 15, 16, 17, 33):
        add("rows_J2_M%d" % M, "fc1x form", M, 128, 32, 4, 6, n_store=90, relu=1)
        add("rows_J4_M%d" % M, "conv2 form", M, 780, 52, 15, 4, n_store=52, stride=52)
    # ---- column tails
    for ns in (1, 15, 16, 17, 32):
        for pad in (0, 4):
            add("cols_%d_ldc%+d" % (ns, pad), "fc1x form", 17, 128, 32, 4, 2, n_store=ns, ldc=ns + pad, relu=ns & 1)
    # ---- slice tails: K one 4-group short of the slices; K ending inside (slice_len 4: at the end of) the first slice of the last workgroup
    for i, sl in enumerate((4, 16, 20, 52, 80)):
        parts = 4 if sl in (16, 52) else 1
        add("slices_%d_short4" % sl, "aid", 17, 8 * sl - 4, sl, 8, 2, n_store=23, a_parts=parts, relu_in=int(parts == 4), a_scale=0.3)
        add("slices_%d_nz2_first" % sl, "aid", 17, 4 * sl + 4, sl, 8, 2, n_store=23, nz=2, a_parts=parts, stride=4 * sl + 8)
    # ---- the instantiations production does not reach, with enough outputs for the yardstick
    for J, parts, sl in ((1, 1, 16), (1, 4, 12), (3, 4, 36), (5, 4, 68)):
        add("aid_J%d_NA%d" % (J, parts), "aid", 33, 15 * sl - 4, sl, 15, 4, n_store=52, a_parts=parts, relu=1, relu_in=int(parts == 4 and J != 3),
            a_scale=0.3)
    # ---- the stacked-clip row map across a row block
    add("rowmap", "net.hip:466", 17, 128, 32, 4, 6, n_store=90, relu=1, a_gdiv=3, a_gmul=7)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    for c in cs:
        assert c["M"] <= 49 and c["K"] <= 1028 and 4 <= c["waves"] <= 16, c["name"]
    return cs


def chain_cases():
    """(producer, consumer): nz = 4 parts through one buffer into a_parts = 4 with relu_in"""
    p = _g("chain_producer", "net.hip:461-469", 20, 256, 16, 16, 8, nz=4, relu=1, seed=101)
    q = _g("chain_consumer", "net.hip:478-484", 20, 128, 32, 4, 6, n_store=90, relu=1, a_parts=4, relu_in=1, seed=102)
    q["a_part_stride"] = p["c_part_stride"]
    assert q["n_A1"] == p["c_part"]
    return p, q


def kinds_of(c):
    return ["signed", "integer", "onehot"] + (["ties"] if c["relu"] and c["nz"] <= 1 else [])


def k_ranges(c):
    """[(k0, k1)] per output part"""
    nzz = max(c["nz"], 1)
    if nzz == 1:
        return [(0, min(c["K"], c["n_slices"] * c["slice_len"]))]
    w = c["waves"]
    return [(min(c["K"], z * w * c["slice_len"]), min(c["K"], min((z + 1) * w, c["n_slices"]) * c["slice_len"])) for z in range(nzz)]


# ------------------------------------------------------------------------------------------------ lat_gemm: inputs
def _hot_ks(c):
    sl, K = c["slice_len"], c["K"]
    ks = [sl - 1, sl, K - 1]
    if K % sl:
        ks.append(K - K % sl)                                              # the first k of the partly filled slice
    if sl == 52:
        ks += [48, 49, 50, 51]
    return [k for k in ks if 0 <= k < K]


def gemm_inputs(c, kind):
    """A [a_parts][n_A1] float32 (NaN where no row reads), B [K][n_cb * 16], bias [n_cb * 16] (NaN past n_store: read, never used),
    a_scale.  Computed once per (case, kind)."""
    key = (c["name"], kind)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.RandomState(7000 + 10 * c["seed"] + ["signed", "integer", "onehot", "ties"].index(kind))
    M, K, P, n1, ncol, ns = c["M"], c["K"], c["a_parts"], c["n_A1"], c["n_cb"] * 16, c["n_store"]
    idx = arow(c)[:, None] * c["a_row_stride"] + np.arange(K)[None, :]
    read = np.zeros(n1, dtype=bool)
    read[idx.reshape(-1)] = True
    a_scale = float(np.float32(c["a_scale"]))
    bias = np.full(ncol, np.nan, dtype=np.float32)
    if kind == "signed":
        blk = np.arange(n1) // max(c["a_row_stride"], 1)
        scale = 2.0 ** rng.uniform(-3, 3, size=int(blk.max()) + 1)
        A = (rng.standard_normal((P, n1)) * scale[blk][None, :]).astype(np.float32)
        A[:, rng.randint(0, n1, max(1, n1 // 16))] = 0
        cs = 2.0 ** rng.uniform(-3, 3, size=ncol)
        cs[3::17] = 0.0
        B = (rng.standard_normal((K, ncol)) * cs[None, :] + 0.0).astype(np.float32)
        B[7::13] = 0.0
        bias[:ns] = (rng.standard_normal(ns) * cs[:ns]).astype(np.float32)
    elif kind in ("integer", "ties"):
        A = (rng.randint(1, 4, (P, n1)) * rng.choice([-1, 1], (P, n1))).astype(np.float32)
        B = (rng.randint(1, 3, (K, ncol)) * rng.choice([-1, 1], (K, ncol))).astype(np.float32)
        a_scale = [1.0, -1.0, 2.0][c["seed"] % 3]
        bias[:ns] = rng.randint(-9, 10, ns).astype(np.float32)
        if kind == "ties":                                                   # column j ties in row j % M
            Ae = A.astype(np.float64).sum(axis=0)
            if c["relu_in"]:
                Ae = np.maximum(Ae, 0)
            pre = a_scale * Ae[idx] @ B.astype(np.float64)
            bias[:ns] = -pre[np.arange(ns) % M, np.arange(ns)]
    else:
        A = np.zeros((P, n1), dtype=np.float32)
        B = (rng.standard_normal((K, ncol)) * 2.0 ** rng.uniform(-3, 3, size=(1, ncol))).astype(np.float32)
        a_scale = 1.0
        bias[:ns] = 0.0
        ks = _hot_ks(c)
        hot = np.zeros((M, K), dtype=bool)                                   # what every row would see
        for r in range(M):
            k = ks[r % len(ks)] if r < 2 * len(ks) else (7 * r + 3) % K
            p = int(idx[r, k])
            seen = idx == p
            if not (hot | seen).sum(axis=1).max() > 1:                       # no row gets a second 1 (rows may overlap)
                hot |= seen
                A[r % P, p] = 1.0
        assert hot.sum(axis=1).max() == 1
    A[:, ~read] = np.nan
    _INPUTS[key] = dict(A=A, B=B, bias=bias, a_scale=a_scale, idx=idx)
    return _INPUTS[key]


_INPUTS = {}


# ------------------------------------------------------------------------------------------------ lat_gemm: references
def reference(c, inp, mode="f64"):
    """[parts][M][n_store]: the contract in float64, or (mode "abs") its S"""
    ns = c["n_store"]
    parts = inp["A"].astype(np.float64)[:, inp["idx"]]                       # [P][M][K]
    sc = float(np.float32(inp["a_scale"]))
    B = inp["B"].astype(np.float64)[:, :ns]
    bias = inp["bias"][:ns].astype(np.float64)
    if mode == "abs":
        Ae, B, bias, sc = np.abs(parts).sum(axis=0), np.abs(B), np.abs(bias), abs(sc)
    else:
        Ae = parts.sum(axis=0)
        if c["relu_in"]:
            Ae = np.maximum(Ae, 0)
    out = []
    for z, (k0, k1) in enumerate(k_ranges(c)):
        v = sc * (Ae[:, k0:k1] @ B[k0:k1])
        if z == 0:
            v = v + bias[None, :]
        if mode != "abs" and c["relu"] and c["nz"] <= 1:
            v = np.maximum(v, 0)
        out.append(v)
    return np.stack(out)


def restatement(c, inp):
    """[parts][M][n_store] float32, see the module docstring"""
    ns, sl, f32 = c["n_store"], c["slice_len"], np.float32
    p = inp["A"][:, inp["idx"]]
    Ae = (p[0] + p[1]) + (p[2] + p[3]) if c["a_parts"] == 4 else p[0]
    if c["relu_in"]:
        Ae = np.maximum(Ae, f32(0))
    Ae = np.ascontiguousarray((f32(inp["a_scale"]) * Ae).astype(f32).T)       # [K][M]
    B = inp["B"][:, :ns]
    out = []
    for z, (k0, k1) in enumerate(k_ranges(c)):
        total = np.zeros((c["M"], ns), dtype=f32)
        for s0 in range(k0, k1, sl):
            acc = np.zeros((c["M"], ns), dtype=f32)
            for k in range(s0, min(s0 + sl, k1)):
                acc += Ae[k][:, None] * B[k][None, :]
            total = total + acc
        if z == 0:
            total = total + inp["bias"][:ns][None, :]
        if c["relu"] and c["nz"] <= 1:
            total = np.maximum(total, f32(0))
        out.append(total)
    return np.stack(out)


def roundings(c):
    return 8 * c["J"] + c["waves"] + 3 + (2 if c["a_parts"] == 4 else 0)


def chain_reference(p, q, ip, iq):
    """(float64 result of the two layers, the a-priori bound of the module docstring); iq's A is not used"""
    S1 = reference(dict(p, nz=1), ip, "abs")[0]
    Z = reference(dict(p, nz=1, relu=0), ip)[0]
    B2, b2 = iq["B"].astype(np.float64)[:, :q["n_store"]], iq["bias"][:q["n_store"]].astype(np.float64)
    want = np.maximum(np.maximum(Z, 0) @ B2 + b2[None, :], 0)
    n1, n2 = roundings(p) * U, roundings(q) * U
    bound = n2 * ((1 + n1) * S1 @ np.abs(B2) + np.abs(b2)[None, :]) + (n1 * S1) @ np.abs(B2)
    return want, bound


# ------------------------------------------------------------------------------------------------ packer and argument block
def pack_b(lib, B, K, n_cb, slice_len, n_slices):
    """dcs_lat_pack_b_host: flat float32 in fragment order"""
    B = np.ascontiguousarray(B, dtype=np.float32)
    n = lib.dcs_lat_pack_b_host(B.ctypes.data_as(ctypes.c_void_p), B.shape[1], K, n_cb, slice_len, n_slices, None, 0)
    assert n == n_slices * n_cb * cdiv(slice_len, 16) * 256, n
    out = np.empty(n, dtype=np.float32)
    assert lib.dcs_lat_pack_b_host(B.ctypes.data_as(ctypes.c_void_p), B.shape[1], K, n_cb, slice_len, n_slices,
                                   out.ctypes.data_as(ctypes.c_void_p), n) == n
    return out


_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class GemmArgs(ctypes.Structure):
    """dcs_debug_lat_gemm_args of include/dcs.h"""
    _fields_ = [("A", _vp), ("n_A", _i64), ("a_row_stride", _i64), ("Bp", _vp), ("n_Bp", _i64), ("bias", _vp), ("n_bias", _i64),
                ("C", _vp), ("n_C", _i64), ("ldc", _i64), ("a_scale", ctypes.c_float), ("M", _i32), ("n_store", _i32), ("K", _i32),
                ("slice_len", _i32), ("n_slices", _i32), ("n_cb", _i32), ("relu", _i32), ("nz", _i32), ("a_parts", _i32),
                ("relu_in", _i32), ("a_gdiv", _i32), ("c_part_stride", _i64), ("a_part_stride", _i64), ("a_gmul", _i64),
                ("J", _i32), ("NA", _i32), ("grid_x", _i32), ("grid_y", _i32), ("grid_z", _i32), ("block_x", _i32)]


def fill_args(c, a_scale, ptrs, counts=None):
    """ptrs / counts {A, Bp, bias, C}: device addresses and float counts (default: the extents)"""
    a = GemmArgs()
    for k in ("a_row_stride", "ldc", "M", "n_store", "K", "slice_len", "n_slices", "n_cb", "relu", "nz", "a_parts", "relu_in", "a_gdiv",
              "c_part_stride", "a_part_stride", "a_gmul"):
        setattr(a, k, c[k])
    a.a_scale = a_scale
    n = dict(extents(c), **(counts or {}))
    for k in ("A", "Bp", "bias", "C"):
        setattr(a, k, ptrs[k])
        setattr(a, "n_" + k, n[k])
    return a


def gemm_refusals(c):
    """(label, case changes, count changes, pointer changes): each must yield DCS_EINVAL and launch nothing"""
    e = extents(c)
    out = [("%s one float short" % k, {}, {k: e[k] - 1}, {}) for k in ("A", "Bp", "bias", "C")]
    out += [("%s null" % k, {}, {}, {k: "null"}) for k in ("A", "Bp", "bias", "C")]
    out += [("%s off 16 bytes" % k, {}, {}, {k: "misaligned"}) for k in ("A", "Bp", "bias", "C")]
    out += [("negative row stride", dict(a_row_stride=-4), {}, {}), ("negative part stride", dict(a_part_stride=-4), {}, {}),
            ("negative c_part_stride", dict(c_part_stride=-4), {}, {}), ("negative ldc", dict(ldc=-c["ldc"]), {}, {}),
            ("no rows", dict(M=0), {}, {}), ("negative K", dict(K=-4), {}, {}), ("negative row map", dict(a_gdiv=3, a_gmul=-1), {}, {}),
            ("n_store above the column blocks", dict(n_store=c["n_cb"] * 16 + 1, ldc=c["n_cb"] * 16 + 1), {}, {}),
            ("n_store above ldc", dict(ldc=c["n_store"] - 1), {}, {}),
            ("parts closer than one part", dict(nz=2, c_part_stride=c["c_part"] - 1, n_slices=8), {}, {}),
            ("three waves", dict(nz=1, n_slices=3), {}, {}), ("seventeen waves", dict(nz=1, n_slices=17), {}, {}),
            ("one wave per part", dict(nz=4, n_slices=4, c_part_stride=c["c_part"] + 4), {}, {}),
            ("slice_len % 4", dict(slice_len=c["slice_len"] + 2), {}, {}), ("K % 4", dict(K=c["K"] - 2), {}, {}),
            ("a_row_stride % 4", dict(a_row_stride=c["a_row_stride"] + 2), {}, {}), ("a_part_stride % 4", dict(a_part_stride=c["a_part_stride"] + 2), {}, {}),
            ("J = 6", dict(slice_len=84), {}, {}), ("two operand parts", dict(a_parts=2), {}, {})]
    return out


# ------------------------------------------------------------------------------------------------ forward STFT
SHAPES = [(1024, 512), (1024, 256), (2048, 512), (2048, 1024)]


def ld_of(N, mode):
    F = N // 2 + 1
    return {"F": F, "F4": cdiv(F, 4) * 4, "F7": F + 7}[mode]


def forward_cases():
    """per (N, hop) and length both alignments of the samples; rows_out, ld and the phase output rotate so that every value meets
    every (N, hop) and both alignments; and a case with N + hop zero samples"""
    cs = []
    for si, (N, hop) in enumerate(SHAPES):
        lengths = [("1", 1), ("hop-1", hop - 1), ("N/2+1", N // 2 + 1), ("4hop", 4 * hop), ("7hop+37", 7 * hop + 37), ("silence", 7 * hop + 37)]
        for li, (lname, n) in enumerate(lengths):
            for skew in (0, 1):
                i = len(cs)
                cs.append(dict(name="fwd_%d_%d_%s_%s" % (N, hop, lname, "off4" if skew else "al8"), N=N, hop=hop, n_samples=n, skew=skew,
                               rows_extra=(0, 7)[(li + skew) % 2], ld=ld_of(N, ("F", "F4", "F7")[(li + skew + si) % 3]),
                               phase=bool((li // 2 + skew + si) % 2), silence=lname == "silence", seed=500 + i))
    return cs


def forward_audio(c):
    """float32 [n_samples]: the project's synth_audio (sinusoids + noise quantised to int16), as tests/stft_ref.py uses it; the
    silence cases hold N + hop zero samples from hop + 13 on: at least one whole frame of zeros"""
    from deepconvsep_amd.synth import synth_audio
    n = c["n_samples"]
    a = np.asarray(synth_audio(n, seed=c["seed"], silence=False), dtype=np.float64).reshape(-1).astype(np.float32)
    if c["silence"]:
        assert c["hop"] + 13 + c["N"] + c["hop"] <= n
        a[c["hop"] + 13:c["hop"] + 13 + c["N"] + c["hop"]] = 0
    return a


def forward_inside(c):
    """how many frames lie wholly inside the signal (the kernel's 16-byte path when the samples are 8-byte aligned)"""
    T = stft_np.frame_count(c["n_samples"], c["hop"])
    return sum(1 for t in range(T) if t * c["hop"] - c["N"] // 2 >= 0 and t * c["hop"] + c["N"] // 2 <= c["n_samples"])


# ------------------------------------------------------------------------------------------------ inverse STFT
def inverse_cases():
    cs = []
    for si, (N, hop) in enumerate(SHAPES):
        R = N // hop
        frames = sorted({1, R - 1, R, 9})
        frames += [5] * (4 - len(frames))
        for fi, T in enumerate(frames):
            full = hop * (T - 1) + N // 2
            n_out = [1, max(1, (full // 2) | 1), full, full + 5][(fi + si) % 4]
            cs.append(dict(name="inv_%d_%d_T%d_src%d_out%d" % (N, hop, T, (1, 3, 4, 5)[fi], n_out), N=N, hop=hop, T=T,
                           n_src=(1, 3, 4, 5)[fi], n_out=n_out, ld=N // 2 + 1 + 3 * ((fi + si // 2) % 2), seed=900 + len(cs)))
    # every n_out class at every (N, hop): the rotation above gives each shape all four, one per frame count
    return cs


def inverse_inputs(c):
    """mag float32 [n_src, T, F] (zero rows and bins inside), unit complex64 [T, F] at random angles: bins 0 and N / 2 carry an
    imaginary part that the transform must ignore"""
    F = c["N"] // 2 + 1
    rs = np.random.RandomState(c["seed"])
    S, T = c["n_src"], c["T"]
    mag = (0.3 * rs.uniform(0, 1, (S, T, F)) * rs.uniform(0, 1, (S, T, F))).astype(np.float32)
    if T >= 5:
        mag[:, rs.randint(0, T)] = 0
    mag[:, :, rs.randint(0, F, max(1, F // 16))] = 0
    ang = rs.uniform(-np.pi, np.pi, (T, F))
    unit = (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)
    assert np.all(unit[:, 0].imag != 0) and np.all(unit[:, -1].imag != 0)
    return mag, unit


def inverse_extents(c):
    rows = (c["T"] - 1) * c["ld"] + c["N"] // 2 + 1
    return dict(mag=(c["n_src"] - 1) * c["T"] * c["ld"] + rows, unit=rows, audio=c["n_src"] * c["n_out"], frames=c["n_src"] * c["T"] * c["N"])


def frames_ref(c, mag, unit):
    """(float64 irfft(X_t) * w, its float32 restatement), both [n_src, T, N]"""
    import torch
    N = c["N"]
    X = (mag.astype(np.float64) / sr.PRE_DIV) * np.sqrt(N) * unit.astype(np.complex128)[None]
    want = np.fft.irfft(X, N, axis=2) * sr.window(N)[None, None, :]
    a = (mag / np.float32(sr.PRE_DIV)) * np.float32(np.sqrt(N))
    X32 = (a * unit[None]).astype(np.complex64)
    X32[:, :, 0] = X32[:, :, 0].real
    X32[:, :, N // 2] = X32[:, :, N // 2].real
    f32 = torch.fft.irfft(torch.from_numpy(X32), n=N, dim=2).numpy().astype(np.float32) * sr.window(N).astype(np.float32)[None, None, :]
    return want, f32


def ola_ref(c, frames):
    """[n_src, n_out] float32: the frames that cover a sample added in frame order, divided by the in-order float32 sum of
    float32(w64^2) (csrc/api.hip: wsq_f), zeros of the normaliser -> 1"""
    N, hop, T = c["N"], c["hop"], c["T"]
    w2 = (sr.window(N) ** 2).astype(np.float32)
    n = max(hop * (T - 1) + N, N // 2 + c["n_out"])
    acc = np.zeros((frames.shape[0], n), dtype=np.float32)
    norm = np.zeros(n, dtype=np.float32)
    for t in range(T):
        acc[:, t * hop:t * hop + N] += frames[:, t]
        norm[t * hop:t * hop + N] += w2
    norm[norm == 0] = 1
    return (acc / norm[None, :])[:, N // 2:N // 2 + c["n_out"]]
