"""What tests/d1_ref.py claims, checked without a device: the stage references composed into the whole graph equal the existing
float64 oracles, and every row of the case table satisfies the conditions that keep the GPU assertions from passing vacuously."""
import numpy as np
import pytest

import conv_ref as cr
import d1_ref as d1
import deep1x1_ref

# two small graphs: build_ca_1x1 with thin layers (the oracles take any filter counts; conv6 and the 1x1 layer keep their 200)
SHAPES = [dict(n=1, tc=3, F=256, filters=(6, 5, 7, 9, 10, 200), kh=(1, 1, 1, 1, 2, 2), nb=1, seed=3),
          dict(n=2, tc=4, F=253, filters=(5, 8, 6, 4, 12, 200), kh=(1, 1, 1, 1, 3, 2), nb=2, seed=4)]


def small_params(s):
    """All three code values in every layer.  Channel 0 of every layer has zero weights and b = 0: its pre-activation is exactly
    0, the tie r'(0) = 0.5 (code 1).  Such a channel carries nothing back, so conv1 has a second tie that does: the input is in
    eighths and filter 1 of conv1 in small integers (every sum is exact in any order), with b minus the sum its first window
    attains."""
    r = np.random.RandomState(s["seed"])
    x = r.randint(0, 9, size=(s["n"], 4, s["tc"], s["F"])) / 8.0
    P, cin = [], 4
    for k, (cout, kh) in enumerate(zip(s["filters"], s["kh"])):
        W = r.standard_normal((cout, cin, kh, d1.KW)) / np.sqrt(cin * kh * d1.KW)
        b = r.uniform(-0.1, 0.1, size=cout)
        W[0], b[0] = 0.0, 0.0
        if k == 0:
            W[1] = r.randint(-2, 3, size=W[1].shape)
            b[1] = -float(np.sum(W[1][:, 0, ::-1] * x[0, :, 0, :d1.KW]))
        P += [W, b, r.uniform(-0.1, 0.1, size=cout)]
        cin = cout
    W = r.standard_normal((d1.NF * s["nb"], d1.NF, 1, 1)) / np.sqrt(d1.NF)
    b = r.uniform(-0.1, 0.1, size=d1.NF * s["nb"])
    W[0], b[0] = 0.0, 0.0
    P += [W, b, r.uniform(-0.1, 0.1, size=d1.NF * s["nb"]), r.uniform(0.0, 0.2, size=4 * s["nb"])]
    return P, x


def compose_forward(P, x, s):
    """the six FWD launches, the 1X1 launch and per branch five TR and one LAST launch per parity, by d1_ref.launch_ref"""
    n = x.shape[0]
    h = d1.to_cl(x.reshape(n, 4, -1)).reshape(-1, 4)                    # [n tc F][4]
    H, W, cin = s["tc"], s["F"], 4
    layers, codes = [], []
    for k in range(6):
        c = d1._case("conv%d" % k, d1.FWD, n, H, W, cin, s["filters"][k], s["kh"][k])
        g = d1.geom(c)
        r = d1.launch_ref(c, {"in": h, "B": d1.pack_B(P[3 * k]), "b0": P[3 * k + 1], "b1": P[3 * k + 2]})
        layers.append(c)
        codes.append(r["code"])
        h, H, W, cin = r["out"], g["Ho"], g["Wo"], s["filters"][k]
    c11 = d1._case("1x1", d1.X11, n, H, W, d1.NF, d1.NF * s["nb"], 1, kw=1)
    src = d1.launch_ref(c11, {"in": h, "B": d1.pack_B(P[18]), "b0": P[19], "b1": P[20]})["out"]      # [br][M][200]
    outs = []
    for br in range(s["nb"]):
        g_ = src[br]
        for k in range(5, -1, -1):
            f = layers[k]
            mode = d1.TR if k > 0 else d1.LAST
            full = None
            for par in (0, 1):
                c = dict(f, mode=mode, par=par)
                gm = d1.geom(c)
                if gm["M"] == 0:
                    continue
                inp = {"in": g_, "code": codes[k], "B": d1.pack_Bt(P[3 * k], par)}
                if mode == d1.LAST:
                    inp["b0"] = P[21][4 * br:4 * br + 4]
                    c.update(n_total=n, k_first=0, ch_off=4 * br)
                r = d1.launch_ref(c, inp)["out"]
                if full is None:
                    full = np.zeros(d1.out_shape(c)[:0] + ((n, gm["Ho"], gm["Wo"], gm["Co"]) if mode == d1.TR else (4, n, gm["Ho"], gm["Wo"])))
                if mode == d1.TR:
                    full[:, :, par::2, :] = r
                else:
                    full[:, :, :, par::2] = r
            g_ = full.reshape(-1, full.shape[-1]) if mode == d1.TR else full
        outs.append(g_)                                                 # [4][n][tc][F]
    return np.concatenate(outs, axis=0).transpose(1, 0, 2, 3), codes


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: "F%d" % s["F"])
def test_stage_references_compose_to_the_graph_oracle(s):
    P, x = small_params(s)
    got, codes = compose_forward(P, x, s)
    want = deep1x1_ref.forward(P, x)
    assert got.shape == want.shape
    for k, cd in enumerate(codes):
        live = cd[:, :s["filters"][k]]
        assert set(np.unique(live)) == {0, 1, 2}, "layer %d: codes %r" % (k, np.unique(live))
    assert np.max(np.abs(want)) > 1e-3
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    # the tie convention is visible in the output: the fixtures tell r'(0) = 0.5 from 0
    assert np.max(np.abs(want - deep1x1_ref.forward(P, x, rprime0=0.0))) > 1e-6


def _full(parts, shape, axis):
    """the two parity launches' outputs side by side: columns par, par + 2, .. of `axis`"""
    full = np.zeros(shape)
    for par, r in parts.items():
        sl = [slice(None)] * len(shape)
        sl[axis] = slice(par, None, 2)
        full[tuple(sl)] = r
    return full


@pytest.mark.parametrize("s", SHAPES, ids=lambda s: "F%d" % s["F"])
def test_training_stages_reproduce_the_gradients(s):
    """FWD, TR, Q, FWDC, B11, the column sums of code_apply and the adjoints of both operand layouts, composed as
    csrc/train_deep1x1.hip composes them, against the float64 autograd gradients of tests/train_deep1x1_ref.py at its codes"""
    import torch
    import train_deep1x1_ref as tref
    import train_ref
    P, x = small_params(dict(s, nb=1))
    r_ = np.random.RandomState(s["seed"] + 10)
    n, tc, F = x.shape[0], s["tc"], s["F"]
    rnd, tgt = r_.uniform(size=(n, 1, tc, F)), r_.uniform(0, 0.5, size=(n, 4, tc, F))
    _, _, info = tref.loss_and_grads(P, x, tgt, rnd)
    out, grads, info2 = tref.loss_and_grads(P, x, tgt, rnd, codes=info["codes"])
    qt = torch.tensor(info2["q"], requires_grad=True)
    with train_ref.relu_tie(0.5):
        loss = tref.components(train_ref.rectify(qt), tref._t(x), tref._t(tgt), tref._t(rnd), eps=tref.EPS)[0]
        dq = torch.autograd.grad(loss, qt)[0].numpy()
    # forward: a_k, the codes, s = g_6, then g_{k-1} = conv_k^T(g_k c_k) and q
    cl = lambda t: d1.to_cl(t.reshape(n, 4, -1)).reshape(-1, 4)
    layers, a, code, H, W, cin = [], [cl(x)], [], tc, F, 4
    filters, khs = s["filters"] + (d1.NF,), s["kh"] + (1,)
    for k in range(7):
        c = d1._case("layer%d" % k, d1.FWD, n, H, W, cin, filters[k], khs[k], kw=d1.KW if k < 6 else 1)
        g = d1.geom(c)
        r = d1.launch_ref(c, {"in": a[k], "B": d1.pack_B(P[3 * k]), "b0": P[3 * k + 1], "b1": P[3 * k + 2]})
        want_code = np.rint(2 * info["codes"][k]).astype(np.uint8).transpose(0, 2, 3, 1).reshape(g["M"], -1)
        assert np.array_equal(r["code"][:, :g["N"]], want_code[:, :g["N"]]) and set(np.unique(want_code)) == {0, 1, 2}
        layers.append(c); a.append(r["out"]); code.append(r["code"])
        H, W, cin = g["Ho"], g["Wo"], filters[k]

    def transposed(k, gin, mode, **extra):
        """both parities of conv_k^T on gin: the assembled output [img][H][W][Co] (TR) or [img][N][H][W] (Q), and per parity the
        operand A of the launch"""
        parts, As = {}, {}
        for par in (0, 1):
            c = dict(layers[k], mode=mode, par=par)
            inp = dict({"in": gin, "code": code[k], "B": d1.pack_Bt(P[3 * k], par)}, **extra)
            parts[par], As[par] = d1.launch_ref(c, inp)["out"], d1.operand_A(c, inp)
        gm = d1.geom(c)
        shape = (n, gm["Ho"], gm["Wo"], gm["Co"]) if mode == d1.TR else (n, gm["N"], gm["Ho"], gm["Wo"])
        return _full(parts, shape, 2 if mode == d1.TR else 3), As

    g_ = {5: a[7]}                                                      # the 1x1 layer's output: g_6
    A_g = {}
    for k in range(5, 0, -1):
        full, A_g[k] = transposed(k, g_[k], d1.TR)
        g_[k - 1] = full.reshape(-1, full.shape[-1])
    q, A_g[0] = transposed(0, g_[0], d1.Q, b0=P[21][:4])
    assert np.max(np.abs(q - info2["q"])) <= 1e-12 * max(1.0, np.max(np.abs(q)))
    # backward: dg_k = c_k conv_k(dg_{k-1}) (FWDC), da_6 = W_7^T (ds c_7) (B11), da_{k-1} = conv_k^T(da_k c_k) (TR)
    dg = [cl(dq)]
    for k in range(6):
        c = dict(layers[k], mode=d1.FWDC)
        dg.append(d1.launch_ref(c, {"in": dg[k], "code": code[k], "B": d1.pack_B(P[3 * k])})["out"])
    ds = dg[6]
    c7 = dict(layers[6], mode=d1.B11)
    da = {5: d1.launch_ref(c7, {"in": ds, "code": code[6], "B": d1.pack_Bt(P[18], 0)})["out"]}
    for k in range(5, 0, -1):
        full, _ = transposed(k, da[k], d1.TR)
        da[k - 1] = full.reshape(-1, full.shape[-1])
    half = lambda k: 0.5 * code[k].astype(np.float64)
    scale = 1e-12 * max(np.max(np.abs(gr)) for gr in grads)

    def close(got, want, what):
        assert got.shape == want.shape and np.max(np.abs(got - want)) <= scale, (what, float(np.max(np.abs(got - want))), scale)

    for k in range(6):
        N = filters[k]
        D = (da[k] * half(k))[:, :N]                                    # code_apply in place; its column sums come first
        close(da[k][:, :N].sum(axis=0), grads[3 * k + 2], "BiasLayer %d" % k)
        close(D.sum(axis=0), grads[3 * k + 1], "b %d" % k)
        fw = dict(layers[k])
        dB = np.zeros(d1.pack_B(P[3 * k]).shape)
        A = d1.operand_A(fw, {"in": a[k]})
        dB[:N, :A.shape[1]] = D.T @ A
        dW = d1.unpack(d1.pack_B, P[3 * k].shape, dB)
        # the transposed convolutions carry W_k too: q's gradient dg_{k-1} against the operand of each parity launch
        prev = dg[k].reshape(n, layers[k]["H"], layers[k]["W"], -1)[..., :layers[k]["cin"]]
        for par in (0, 1):
            dBt = np.zeros(d1.pack_Bt(P[3 * k], par).shape)
            G = prev[:, :, par::2, :].reshape(-1, prev.shape[-1])
            dBt[:G.shape[1], :A_g[k][par].shape[1]] = G.T @ A_g[k][par]
            dW = dW + d1.unpack(lambda w, par=par: d1.pack_Bt(w, par), P[3 * k].shape, dBt)
        close(dW, grads[3 * k], "W %d" % k)
    Ds = ds * half(6)
    close(ds.sum(axis=0), grads[20], "BiasLayer of the 1x1 layer")
    close(Ds.sum(axis=0), grads[19], "b of the 1x1 layer")
    dB = np.zeros(d1.pack_B(P[18]).shape)
    dB[:d1.NF, :d1.NF] = Ds.T @ a[6][:, :d1.NF]
    close(d1.unpack(d1.pack_B, P[18].shape, dB), grads[18], "W of the 1x1 layer")
    close(dq.sum(axis=(0, 2, 3)), grads[21], "final bias")


def test_selection_and_grid():
    assert [d1.nt_for(N) for N in (4, 16, 17, 30, 32, 33, 50, 800)] == [1, 1, 2, 2, 2, 4, 4, 4]
    assert [d1.npad(N) for N in (4, 16, 17, 30, 32, 33, 50, 200, 800)] == [16, 16, 32, 32, 32, 64, 64, 256, 832]
    reached = {(c["mode"], d1.geom(c)["nt"], c["unit"]) for c in d1.cases()}
    assert reached >= d1.PRODUCTION, sorted(d1.PRODUCTION - reached)


def test_case_table_covers_the_edges():
    cs = d1.cases()
    gs = [d1.geom(c) for c in cs]
    for mode in range(7):
        mine = [(c, g) for c, g in zip(cs, gs) if c["mode"] == mode]
        Ms = [g["M"] for c, g in mine]
        assert any(m < 16 for m in Ms) and any(m > 128 and m % 16 for m in Ms), (d1.MODE_NAMES[mode], Ms)
        assert any(m % 128 == 0 for m in Ms), (d1.MODE_NAMES[mode], Ms)
        assert any(c["images"] > 1 and (g["Ho"] * g["Wq"]) % 16 for c, g in mine), d1.MODE_NAMES[mode]
    assert any(17 <= g["M"] <= 31 for g in gs)
    assert {g["K"] % 16 for g in gs} >= {0, 4, 8, 12}
    assert any(g["K"] == 10000 and g["M"] < 64 for g in gs)
    tr = [(c, g) for c, g in zip(cs, gs) if c["mode"] in (d1.TR, d1.LAST, d1.Q)]
    for mode in (d1.TR, d1.LAST, d1.Q):
        ws = {(c["W"], c["par"]) for c, g in tr if c["mode"] == mode}
        assert any(w == 5 for w, p in ws) and any(w % 2 == 0 and p == 1 for w, p in ws) and any(w % 2 == 0 and p == 0 for w, p in ws), (mode, ws)
    assert {c["W"] for c in cs if c["mode"] == d1.FWD} >= {5, 6, 7, 8} and {c["W"] for c, g in tr} >= {5, 6, 7, 8}
    assert {c["ch_off"] for c in cs if c["mode"] == d1.LAST} == {0, 4, 12}
    assert all(c["k_first"] + c["images"] <= c["n_total"] for c in cs if c["mode"] == d1.LAST)
    assert any(c["k_first"] > 0 and c["n_total"] > c["k_first"] + c["images"] for c in cs if c["mode"] == d1.LAST)
    assert {d1.geom(c)["N"] for c in cs if c["mode"] == d1.FWD} >= {16, 17, 32, 33, 30, 50, 70, 100, 200}
    assert {d1.geom(c)["N"] for c in cs if c["mode"] == d1.TR} >= {16, 17, 32, 33, 30, 50, 70, 100, 200}


@pytest.mark.parametrize("c", d1.cases(), ids=lambda c: c["name"])
def test_case_conditions(c):
    """the conditions under "Acceptance" that must hold for the references alone"""
    g = d1.geom(c)
    assert g["M"] >= 1
    # signed: S > 0 on every live output, exactly 0 elsewhere; the in-order restatement is inside the cap
    inp = d1.inputs(c, "signed")
    want, S, rest = (d1.launch_ref(c, inp, m)["out"] for m in (d1.mul64, d1.mul_abs, d1.mul_chain))
    live = d1.live_mask(c, inp)
    assert want.shape == S.shape == rest.shape == live.shape == np.empty(d1.out_shape(c))[d1.owned(c)].shape
    assert np.all(S[live] > 0) and not S[~live].any() and not want[~live].any()
    e = cr.measure(rest, want, S)
    assert np.isfinite(e)
    assert np.all(np.abs(rest.astype(np.float64) - want) <= (g["K"] + cr.cap_c(g["K"], "f32")) * d1.U * S)
    if "code" in inp:
        cd = inp["code"][:, :g["Cl"] if c["mode"] != d1.FWDC else g["N"]]
        assert set(np.unique(cd)) == {0, 1, 2}
        assert not inp["code"][:, (g["Cl"] if c["mode"] != d1.FWDC else g["N"]):].any()
    assert not inp["in"][:, g["Cl"]:].any()
    # integer probe: every partial sum below 2^24, so float32 is exact in any order, halves included
    pi = d1.inputs(c, "int")
    assert d1.max_partial(c, pi) < 2.0 ** 24
    w64, w32 = d1.launch_ref(c, pi)["out"], d1.launch_ref(c, pi, d1.mul_chain)["out"]
    assert np.array_equal(w64, w32.astype(np.float64))
    assert np.array_equal(w64.astype(np.float32).astype(np.float64), w64)
    if c["mode"] == d1.FWD:
        pt = d1.inputs(c, "ties")
        assert d1.max_partial(c, pt) < 2.0 ** 24
        r = d1.launch_ref(c, pt)
        pre = r["pre"]
        assert (pre == 0).any() and (pre > 0).any() and (pre < 0).any()
        assert set(np.unique(r["code"][:, :g["N"]])) == {0, 1, 2}
