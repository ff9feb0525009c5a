"""tests/conv_ref.py itself (no GPU): the float64 operations against oracle/net_ref.py's layers, the restatements and the
integer probe, the hand-over layouts and routing words, the kernel codes against include/dcs.h, and the case table's reach
over the launchers' selection arithmetic on 256 CUs."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

import conv_ref as cr
from oracle import net_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("graph,F", [("bach10", 93), ("bach10_si1", 94), ("ikala", 306), ("ikala_nopool", 120)])
@pytest.mark.parametrize("tie", [cr.TIE_ALL, cr.TIE_FIRST])
def test_operations_are_the_oracles_layers(graph, F, tie):
    d = cr.dims(graph, F)
    W1, b1, b1b, W2, b2, b2b = cr.weights(graph, "int")               # integer data: plenty of pool ties
    x, _ = cr.tiles(graph, F, 2, "int")
    spec = net_ref.SPECS[graph]
    assert {k: d[k] for k in ("w1", "wp", "h2", "w2", "flat")} == {k: spec.dims(cr.TC, F)[k] for k in ("w1", "wp", "h2", "w2", "flat")}
    W1c, W2c = net_ref._flip(T(W1)), net_ref._flip(T(W2))
    a1b = Fnn.conv2d(T(x), W1c, stride=(1, d["sw"])) + T(b1).view(1, -1, 1, 1) + T(b1b).view(1, -1, 1, 1)
    mine = cr.conv1(x, W1, b1, b1b, d)
    assert np.array_equal(mine, a1b.numpy())
    h = net_ref._pool_fwd(a1b, d["pool"]) if d["pool"] else a1b
    if d["pool"]:
        assert np.array_equal(cr.pool(mine), h.numpy())
    a2b = Fnn.conv2d(h, W2c) + T(b2).view(1, -1, 1, 1) + T(b2b).view(1, -1, 1, 1)
    assert np.array_equal(cr.conv2(h.numpy(), W2, b2, b2b, d), a2b.numpy())
    nb = 2
    D = cr.dense_out(graph, F, 2, nb, "int")
    g = net_ref._conv_vjp(T(D), (2 * nb,) + tuple(h.shape[1:]), W2c, (1, 1), "explicit")
    assert np.array_equal(cr.conv2_t(D, W2, d), g.numpy())
    routes = None
    if d["pool"]:
        a_rep = a1b.repeat_interleave(nb, dim=0)
        g = net_ref._pool_vjp(g, a_rep, d["pool"], "all" if tie == cr.TIE_ALL else "first")
        routes = cr.pool_routes(mine, tie)
        assert np.array_equal(cr.unpool(cr.conv2_t(D, W2, d), routes, nb), g.numpy())
    o = net_ref._conv_vjp(g, (2 * nb, d["C"], cr.TC, F), W1c, (1, d["sw"]), "explicit")
    want = cr.decoder(D, W1, W2, d, graph, "f32", "f32", routes=routes, nb=nb)[0]
    assert np.array_equal(want, o.numpy())
    assert np.array_equal(cr.conv1_t(g.numpy(), W1, d), o.numpy())


@pytest.mark.parametrize("graph", list(cr.GRAPHS))
def test_integer_probe_ranges(graph):
    """every partial sum an integer below 2^24; at most 2^11 where a value is stored as f16 (the column-filter graphs: conv1's
    hand-over, conv2's map, the map between the fused decoder's layers)"""
    c1, c2, g2, o = cr.int_ranges(graph)
    assert max(c1, c2, g2, o) < 2 ** 24
    if cr.GRAPHS[graph][4] == 1:
        assert max(c1, c2, g2) <= 2 ** 11
    W = cr.weights(graph, "int")
    F = 94 if cr.GRAPHS[graph][4] == 1 else 267
    x, _ = cr.tiles(graph, F, 1, "int")
    assert np.abs(W[0]).max() <= 2 and np.abs(W[3]).max() <= 1 and 0 <= x.min() and x.max() <= 3
    assert np.abs(cr.a1_map(graph, F, 1, "int")).max() <= 2 and cr.dense_out(graph, F, 1, 1, "int").max() <= 2
    for a in W + [x]:
        assert np.array_equal(a, np.round(a))


@pytest.mark.parametrize("cls", ["f32", "bf16x3", "f16"])
@pytest.mark.parametrize("graph,F", [("bach10_si1", 93), ("ikala", 267)])
def test_restatements_equal_float64_on_the_integer_probe(graph, F, cls):
    d = cr.dims(graph, F)
    W = cr.weights(graph, "int")
    x, _ = cr.tiles(graph, F, 2, "int")
    for f16_out in (False, True):
        want, S, extra, rest, sub = cr.layer(cr.conv1, x, W[0], d, cls, bias=(W[1], W[2]), f16_out=f16_out)
        assert np.array_equal(rest, want[sub])
    a = cr.a1_tiles(cr.a1_map(graph, F, 2, "int"), 2, cr.TC)
    want, S, extra, rest, sub = cr.layer(cr.conv2, a, W[3], d, cls, bias=(W[4], W[5]))
    assert np.array_equal(rest, want[sub])
    D = cr.dense_out(graph, F, 2, 1, "int")
    routes = cr.pool_routes(cr.conv1(x, W[0], W[1], W[2], d), cr.TIE_FIRST) if d["pool"] else None
    want, S, extra, rest, sub, K, c, _ = cr.decoder(D, W[0], W[3], d, graph, cls, cls, routes=routes, nb=1, f16_mid=cls == "f16" and not d["pool"])
    assert np.array_equal(rest, want[sub]) and np.abs(want).max() < 2 ** 24


def test_restatements_are_yardsticks_on_random_data():
    """each class's float32 restatement is close to, and not equal to, the float64 result; dropping the lowest bf16 product
    group or truncating an f16 rounding is far outside FACTOR times the yardstick"""
    graph, F = "bach10", 93
    d = cr.dims(graph, F)
    W = cr.weights(graph, "rand")
    a = cr.a1_tiles(cr.a1_map(graph, F, 2, "rand"), 2, cr.TC)
    K = cr.layer_K(graph, "conv2")
    for cls in ("f32", "bf16x3", "f16"):
        want, S, extra, rest, sub = cr.layer(cr.conv2, a, W[3], d, cls, bias=(W[4], W[5]))
        e = cr.measure(rest, want[sub], S[sub])
        assert 0 < e < 50 * cr.U
        assert cr.inside_cap(rest, want[sub], S[sub], extra[sub], K, cr.cap_c(K, cls))

    def without_lowest(A, B):
        a0, a1, a2 = cr.gr.split3(np.ascontiguousarray(A, dtype=np.float32))
        b0, b1, b2 = cr.gr.split3(np.ascontiguousarray(B, dtype=np.float32))
        return (a0 @ b0 + a0 @ b1 + a1 @ b0).astype(np.float32)
    want, S, extra, rest, sub = cr.layer(cr.conv2, a, W[3], d, "bf16x3", bias=(W[4], W[5]))
    mutant = cr.conv2(a, W[3], W[4], W[5], d, mul=without_lowest, images=sub) + cr._bias32(W[4], W[5])[None, :, None, None]
    assert cr.measure(mutant, want[sub], S[sub]) > cr.gr.FACTOR * cr.measure(rest, want[sub], S[sub])


def test_layouts_and_routing_words():
    rs = np.random.RandomState(3)
    m = rs.uniform(-1, 1, (2, cr.NF, 5, 17)).astype(np.float32)
    for lay in (cr.CF, cr.CL32, cr.CL16):
        back = cr.from_layout(cr.to_layout(m, lay), lay, 2, 5, 17)
        assert np.array_equal(back[:, :cr.NF], m.astype(np.float16) if lay == cr.CL16 else m)
    assert not cr.from_layout(cr.to_layout(m, cr.CL16), cr.CL16, 2, 5, 17)[:, cr.NF:].any()
    a = rs.randint(0, 3, (2, 3, 4, 83)).astype(np.float64)
    for tie in (cr.TIE_ALL, cr.TIE_FIRST):
        r = cr.pool_routes(a, tie)
        assert not r[..., 80:].any()
        per = r[..., :80].reshape(2, 3, 4, 20, 4).sum(-1)
        assert per.min() >= 1 and (tie == cr.TIE_ALL or per.max() == 1) and (tie == cr.TIE_FIRST or per.max() > 1)
        w = cr.routing_words(r)
        assert w.shape[-1] == 3 and w.dtype == np.uint32 and cr.pool_words(83) == 4
        assert np.array_equal(cr.routes_from_words(w, 83), r)
        assert w[0, 0, 0, 0] == sum(int(r[0, 0, 0, j]) << j for j in range(32))
    a[0, 0, 0, :8] = 0
    assert cr.pool_routes(a, cr.TIE_ALL)[0, 0, 0, :8].all() and list(cr.pool_routes(a, cr.TIE_FIRST)[0, 0, 0, :8]) == [1, 0, 0, 0] * 2


def test_fold_is_conv2_then_the_bottleneck_layer():
    """fold_want against the two layers one after the other (oracle/net_ref.py's expressions), biases aside"""
    F = 267
    d = cr.dims("ikala", F)
    p = cr.fold_params(F)
    rs = np.random.RandomState(5)
    h = rs.uniform(-1, 1, (2, cr.NF, cr.TC, d["wp"]))
    a2 = Fnn.conv2d(T(h), net_ref._flip(T(p[3]))).reshape(2, -1).numpy()
    want = a2 @ p[6].astype(np.float64)
    got = h.reshape(2, -1) @ cr.fold_want(p[3], p[6], d)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-12 * np.abs(want).max() + 1e-13


def test_kernel_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "dcs.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define DCS_CONV_K_(\w+) (\d+)", text)}
    mine = {k[2:]: v for k, v in vars(cr).items() if k.startswith("K_")}
    assert header == mine and cr.K_UNLISTED not in cr.ALL_CODES
    roles = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define DCS_CONV_ROLE_(\w+) (\d+)", text)}
    assert roles == {name: i for i, name in enumerate(cr.ROLES)}
    assert set(cr.CLASS) == cr.ALL_CODES - {cr.K_POOL, cr.K_UNPOOL, cr.K_ZERO_PAD}


def test_case_table_reaches_every_code_and_branch_on_256_cus():
    cases = cr.cases(256)
    assert len({c["name"] for c in cases}) == len(cases)
    seen, br = set(), set()
    for c in cases:
        e = cr.expected(c, 256)
        if e["rc"] == 0:
            seen |= {v[0] for v in e["kernels"].values()}
            br |= cr.branches(c, 256)
            if c["switch"] != "none":
                assert e != cr.expected(dict(c, switch="none"), 256)
    assert seen == cr.ALL_CODES, sorted(cr.CODE_NAMES[k] for k in cr.ALL_CODES - seen)
    assert br == cr.BRANCHES, cr.BRANCHES - br
    assert any(cr.expected(c, 256)["rc"] == -2 for c in cases)
    # the F = 1025 forward conv2 stages fewer than five tap pairs from this image count on, and not below it
    n = cr.ikala_1025_images(256)
    assert cr._slab_ps("none", 256, n, 0, cr.TC, 83, 21, 64, 10, 20, 0, 0)[3] < 5 <= cr._slab_ps("none", 256, n - 1, 0, cr.TC, 83, 21, 64, 10, 20, 0, 0)[3]
    short = [c for c in cases if c.get("ntag") == "short_stage" and cr.expected(c, 256)["kernels"].get("conv2", (0, 0, 0, 5))[0] == cr.K_SLAB_PS_0]
    assert short and all(cr.expected(c, 256)["kernels"]["conv2"][3] < 5 for c in short)
    # F = 513 (w2 = 21, h2 = 21): three bands (8, 8, 5) of a 32-column tile, in either precision
    for mode in (0, 1):
        code, band, xt, ps = cr._slab_ps("none", 256, 1, mode, cr.TC, 40, 21, 21, 10, 20, 0, 0)
        assert (band, xt, cr.cdiv(21, band), 21 % band) == (8, 32, 3, 5)
    assert any(c["F"] == 513 and cr.expected(c, 256)["kernels"].get("conv2", (0,))[0] == cr.K_SLAB_PS_0 for c in cases)
    # other CU counts resolve to the same case names
    assert {c["name"] for c in cr.cases(304)} == {c["name"] for c in cases}
