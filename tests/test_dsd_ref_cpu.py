"""The float64 references of tests/dsd_ref.py against the oracle (bit for bit on integer data), the coverage of the case table
of tests/test_gpu_dsd_kernels.py on 256 CUs, and the condition under which its derived mask bound means something: in every
case at most 1 % of the output elements are vacuous or carry a bound above 1e-4 x scale x max mixture.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

import dsd_ref as dr
from oracle import net_ref, pipeline, tiling_np

N_CU = 256
CASES = dr.cases(N_CU)


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("tc", [30, 20, 31, 32, 40])
def test_deconv2_is_the_oracles_inverse_layer(tc):
    d = dr.dims(tc)
    _, W2, _ = dr.weights(1, tc, 65, "int")
    D = dr.dense(tc, 3, "int")
    assert np.abs(D).max() <= 2 and np.abs(W2).max() <= 1
    g = _t(D.transpose(0, 2, 1)[..., None])                                         # [n][co][h2][1]
    want = net_ref._conv_vjp(g, (3, dr.NF, tc, 1), net_ref._flip(_t(W2)), (1, 1), "autograd").numpy()[..., 0]
    got = dr.deconv2(D, W2, tc)
    assert np.array_equal(got, want) and np.abs(got).max() <= dr.int_ranges()["deconv2"] and got.any()
    for cls in ("f32", "bf16x3"):                                                   # exact data: every restatement is the reference
        assert np.array_equal(dr.deconv2(D, W2, tc, mul=dr.MUL[cls]).astype(np.float64), want), cls
    assert np.array_equal(dr.deconv2(D, W2, tc, mul="abs"), dr.deconv2(np.abs(D), np.abs(W2), tc))
    # the device layouts and back
    G32 = got.astype(np.float32)
    back, pad = dr.g_from_layout(dr.g_layout(G32), 3, tc)
    assert np.array_equal(back, G32) and not pad.any()
    v, planes = dr.planes_value(dr.planes_layout(G32), 3, tc)
    assert np.array_equal(v, dr.g_layout(G32))


@pytest.mark.parametrize("C", [1, 2])
def test_raw_final_is_the_oracles_inverse_layer_and_bias(C):
    tc, F, n = 30, 65, 2
    W1, _, b = dr.weights(C, tc, F, "int")
    nbr = 3 if C == 1 else 4
    G = dr.gdata(n, nbr, tc, "int")
    assert G.min() >= -1 and G.max() <= 2 and np.abs(W1).max() <= 2
    Fe, ld = dr.row_width(F, C)
    got = dr.raw_tiles(G, W1, b, F)
    W1c = net_ref._flip(_t(W1))
    for s in range(4):
        br = s if C == 2 else (0, 1, 2, 1)[s]
        x = net_ref._conv_vjp(_t(G[:, br][..., None]), (n, C, tc, F), W1c, (1, 1), "autograd").numpy()    # [n][C][tc][F]
        for ch in range(C):
            assert np.array_equal(got[:, s, :, ch * ld:ch * ld + F], x[:, ch] + np.float64(b[s * C + ch])), (s, ch)
    assert np.abs(got).max() <= dr.int_ranges()["final"]
    for cls in ("f32", "bf16x3"):
        assert np.array_equal(dr.raw_tiles_f32(G, W1, b, F, cls).astype(np.float64), got), cls
    S = dr.raw_tiles(G, W1, b, F, mul="abs")
    assert np.all(S >= np.abs(got))


@pytest.mark.parametrize("ov,kind", [(25, "rand"), (15, "rand"), (16, "rand"), (1, "int"), (2, "int"), (26, "rand")])
def test_fold_is_overlapadd_multi(ov, kind):
    n, tc, F = 5, 30, 7
    r = np.random.default_rng(ov)
    tiles = r.integers(-3, 4, (n, tc, F)).astype(np.float64) if kind == "int" else r.standard_normal((n, tc, F))
    want = tiling_np.overlapadd_multi(tiles[None, None, :, None], n, overlap=ov)[0]
    rows = want.shape[0] + 3
    got = dr.fold(tiles, ov, rows)
    assert np.array_equal(got[:want.shape[0]], want) and not got[want.shape[0]:].any()
    assert np.array_equal(dr.fold(tiles, ov, 37), want[:37])
    if kind == "int":                                                               # weights 0 and 1: the float32 fold is exact too
        f32 = dr.fold(tiles.astype(np.float32), ov, rows, rise=dr.rise_table(ov), dtype=np.float32)
        assert np.array_equal(f32.astype(np.float64), got)
        assert set(np.unique(dr.rise_table(ov))) <= {0.0, 1.0}


def test_final_against_the_pipelines_spectra():
    """deconv2 + final (convention A, folded) of the references on the dense-layer outputs of a small clip against the masked
    spectra of oracle.pipeline.separate"""
    from deepconvsep_amd.synth import synth_audio, synth_params
    tc, ov, F, N = 30, 25, 65, 128
    params = synth_params("dsd", tc, F, seed=2)
    audio = synth_audio(44100, seed=0)[:6000]
    _, mm, mag, _ = pipeline.separate("dsd", params, audio, 0.3, tc, ov, 32, N, 64, np.hanning, return_spectra=True)
    batches, n = tiling_np.generate_overlapadd(mag, F, tc, ov, 32)
    x = _t(batches.reshape(-1, 1, tc, F)[:n])
    P = [_t(p) for p in params]
    d = dr.dims(tc)
    a1 = Fnn.conv2d(x, net_ref._flip(P[0])) + (P[1] + P[2]).view(1, -1, 1, 1)
    a2 = Fnn.conv2d(a1, net_ref._flip(P[3])) + (P[4] + P[5]).view(1, -1, 1, 1)
    z = torch.relu(a2.reshape(n, -1) @ P[6] + P[7])
    D = np.stack([torch.relu(z @ P[8 + 2 * i] + P[9 + 2 * i]).reshape(n, dr.NF, d["h2"]).numpy().transpose(0, 2, 1) for i in range(3)], axis=1)
    G = dr.deconv2(D.reshape(n * 3, d["h2"], dr.NF), np.asarray(params[3], dtype=np.float64), tc).reshape(n, 3, dr.NF, tc)
    rows = min(mm.shape[1], (n - 1) * (tc - ov) + tc)
    got = dr.final(G, np.asarray(params[0], dtype=np.float64), np.asarray(params[-1], dtype=np.float64), F, mag.astype(np.float64), 1.0, 0, ov, rows)
    err = np.abs(got - mm[:, :rows]).max()
    print("\n%d tiles, %d frames: max |reference - pipeline| = %.3g of %.3g" % (n, rows, err, np.abs(mm).max()))
    assert n >= 10 and err <= 1e-12 * max(1.0, np.abs(mm).max())


def test_masks_are_the_oracles():
    """conventions A and B of net_ref.soft_mask and the stereo trainer's of net_ref.predict_ild on one tile (no fold)"""
    tc, F, n = 30, 65, 2
    W1, _, b = dr.weights(1, tc, F, "rand")
    G = dr.gdata(n, 3, tc, "rand")
    mix = dr.mixture(n * tc, F, 1, "rand")
    p = np.maximum(dr.raw_tiles(G, W1, b, F), 0.0)
    for mode, name in ((0, "A"), (1, "B")):
        want = net_ref.soft_mask("dsd", _t(p), _t(mix[:, :F].reshape(n, 1, tc, F)), eps_mode=name)
        want = np.stack([w.numpy()[:, 0] for w in want]).reshape(4, n * tc, F)
        got = dr.final(G, W1, b, F, mix, 1.0, mode, None, n * tc)
        assert np.abs(got - want).max() <= 1e-15 + 1e-12 * np.abs(want).max(), name      # A: max(x, eps r) against max(x, 0) + eps r
    e = net_ref.EPS_ILD * net_ref.RAND_ILD
    assert np.isclose(e, dr.EPS_ILD, rtol=1e-7, atol=0) and np.isclose(net_ref.EPS * net_ref.RAND, dr.EPS_A, rtol=1e-7, atol=0)


# ------------------------------------------------------------------------------------------------ selection and coverage
def test_case_table_reaches_every_kernel_and_branch():
    seen, br = set(), set()
    for c in CASES:
        e = dr.expected(c, N_CU)
        seen |= set(e["kernels"].values())
        br |= dr.branches(c, N_CU)
    assert seen == dr.ALL_CODES, sorted(dr.code_name(k) for k in dr.ALL_CODES - seen)
    assert br >= dr.BRANCHES, sorted(dr.BRANCHES - br)
    assert len({c["name"] for c in CASES}) == len(CASES)
    # a switch set runs only cases whose kernel it changes -- and the two in which forced streaming must fall back
    for c in CASES:
        if c["switch"] != "none":
            assert (dr.expected(c, N_CU) != dr.expected(dict(c, switch="none"), N_CU)) != ("falls back" in c["name"]), c["name"]
    refused = [c["name"] for c in CASES if dr.expected(c, N_CU)["rc"] != 0]
    assert len(refused) == 7, refused


def test_selection_restated():
    e = lambda **kw: dr.expected(dict(dr._d("x", 1), **kw), N_CU)
    assert e(n=1023)["kernels"] == {"deconv2": dr.K_DECONV2} and e(n=1024)["kernels"] == {"deconv2": dr.K_STREAM}
    assert e(n=1024)["params"][:4] == [112, 96, 4, 768]                              # 3 n_cu slots: 6 x 112 + 96
    assert e(n=1024, gs=1)["kernels"] == {"deconv2": dr.K_BF16_16} and e(n=1024, gs=1)["params"][:4] == [32, 64, 16, 256]
    assert e(n=1023, gs=1, switch="deconv2_2")["params"][:4] == [72, 80, 4, 512]
    assert e(n=1024, gs=1, no_bq=1)["kernels"] == {"deconv2": dr.K_STREAM_SPLIT}
    assert e(n=3, gs=1)["kernels"] == {"deconv2": dr.K_DECONV2, "gsplit": dr.K_GSPLIT}
    assert e(n=1024, tc=31)["kernels"] == {"deconv2": dr.K_DECONV2} and e(n=5000, tc=40, switch="deconv2_2")["kernels"] == {"deconv2": dr.K_DECONV2}
    assert e(n=1, tc=66)["rc"] == dr.EUNSUPPORTED
    f = lambda **kw: dr.expected(dict(dr._f("x", 1025, 25, 4, 45, 0), **kw), N_CU)
    assert f()["kernels"] == {"final": dr.K_FINAL + 3 * 2} and f()["params"][4:] == [1, 17, 51, 6]
    assert f(rows=16 * 85 + 1)["kernels"] == {"final": dr.K_FINAL + 3 * 2 + 1} and f(rows=16 * 85)["params"][4] == 1
    assert f(rows=16 * 85 + 1, gs=1)["kernels"] == {"final": dr.K_FINAL_BF16X3} and f(rows=16 * 85 + 1, gs=1, mode=2)["kernels"] == {"final": dr.K_FINAL + 5 * 2 + 1}
    assert f(ov=29)["rc"] == dr.EUNSUPPORTED and f(ov=28)["params"][7] == 15 and f(ov=30)["rc"] == dr.EINVAL
    assert f(family=dr.ONE_BATCH, gs=1)["kernels"] == {"final": dr.K_LAT_FINAL} and f(family=dr.ONE_BATCH, gs=1, ov=26)["rc"] == dr.EINVAL
    assert f(C=2, mode=3)["kernels"] == {"final": dr.K_FINAL4 + 3} and f(C=2, mode=1)["rc"] == dr.EINVAL
    assert dr.NO_CALLER == {18, 19, 20, 21, 22} and [dr.code_name(k) for k in (18, 23)] == ["final_kernel<true, 2, 1, 3>", "final_kernel<true, 3, 1, 4>"]


# ------------------------------------------------------------------------------------------------ the 1 % condition
_MASK_CASES = [c for c in CASES if c["stage"] == dr.STAGE_FINAL and c["mode"] != 2 and dr.expected(c, N_CU)["rc"] == 0]


@pytest.mark.parametrize("case", _MASK_CASES, ids=lambda c: c["name"])
def test_mask_bound_is_not_vacuous(case):
    c = case
    code = dr.expected(c, N_CU)["kernels"]["final"]
    for kind in c["kinds"]:
        if kind == "int":
            continue
        W1, _, b = dr.weights(c["C"], c["tc"], c["F"], kind)
        G_all, mix_all = dr.inputs(c, kind)
        bad = total = cut = 0
        for fr, nt, r0, t0 in dr.clip_layout(c)[0]:
            G, mix = G_all[t0:t0 + nt], mix_all[r0:r0 + fr]
            rows = fr if c["ov"] is not None else nt * c["tc"]
            bound, _ = dr.mask_bound(G, W1, b, c["F"], mix, 0.3, c["mode"], c["ov"], rows, dr.kernel_class(code))
            bad += int(np.sum(~(bound <= 1e-4 * 0.3 * float(mix.max()))))
            total += bound.size
            cut += int(np.sum(np.all(dr.raw_tiles(G, W1, b, c["F"]) < 0, axis=1)))
        print("\n%s %s: %.4f %% of the elements vacuous or above 1e-4 x scale x max mixture" % (c["name"], kind, 100.0 * bad / total))
        assert bad <= 0.01 * total, (c["name"], kind, bad / total)
        if kind in ("sparse", "tiny"):            # the hard sets are hard: all four sources cut in a large share of the tile elements
            assert cut > 0.2 * G.shape[0] * c["tc"] * bound.shape[2], (kind, cut)


def test_hard_sets_reach_the_eps_of_each_convention():
    """on the frames whose G is zero the tiny set's first source is 2 eps: its mask is 0.4 under A (floors of eps on the three
    others), 2 / 3 under B, and under the stereo mask 2e-13 / 3e-13; the sparse set gives a quarter of the mixture under A and 0
    under B there"""
    for C, mode, share in ((1, 0, 0.4), (1, 1, 2.0 / 3), (2, 3, 2.0 / 3)):
        c = dr._f("x", 65, None, 2, 0, mode, C=C)
        G, mix = dr.inputs(c, "tiny")
        mix[:] = 1.0
        W1, _, b = dr.weights(C, 30, 65, "tiny")
        out = dr.final(G, W1, b, 65, mix, 1.0, mode, None, 60)
        assert np.allclose(out[0, dr.ZERO_AT, :65] - (dr.EPS_ILD if mode == 3 else 0), share, rtol=1e-6), (mode, out[0, dr.ZERO_AT, :3])
        bound, _ = dr.mask_bound(G, W1, b, 65, mix, 1.0, mode, None, 60, "f32")
        assert bound[:, dr.ZERO_AT].max() <= (dr.NF + 64) * dr.U          # the raw cap of the first source (its S is the bias) and the epilogue
    c = dr._f("x", 65, None, 2, 0, 0)
    G, mix = dr.inputs(c, "sparse")
    W1, _, b = dr.weights(1, 30, 65, "sparse")
    assert np.allclose(dr.final(G, W1, b, 65, mix, 1.0, 0, None, 60)[:, dr.ZERO_AT], 0.25 * mix[dr.ZERO_AT, :65], rtol=1e-12)
    assert not dr.final(G, W1, b, 65, mix, 1.0, 1, None, 60)[:, dr.ZERO_AT].any()


def test_wrong_constants_fail_the_hard_sets(monkeypatch):
    """the checks of tests/test_gpu_dsd_kernels.py applied to restatements with another eps or with the two conventions swapped:
    the tiny set fails each of them (the signed and the non-negative set pass a doubled eps: that is why the hard sets exist)"""
    import test_gpu_dsd_kernels as t
    cs = {c["name"]: c for c in CASES}
    floor, den_eps = dr._floor, dr._den_eps
    variants = {"A: eps doubled": (lambda m: 2 * dr.EPS_A if m == 0 else 0.0, den_eps, "op A F65"),
                "A: B's arithmetic": (lambda m: 0.0, lambda m: dr.EPS_A, "op A F65"),
                "B: A's arithmetic": (lambda m: dr.EPS_A, lambda m: 0.0, "op B F513"),
                "B: eps doubled": (floor, lambda m: 2 * dr.EPS_A, "op B F513"),
                "stereo: the eps of B": (floor, lambda m: dr.EPS_A, "ild op F65")}
    for name, (fl, de, cn) in variants.items():
        c = cs[cn]
        code = dr.expected(c, N_CU)["kernels"]["final"]
        for kind, fails in (("tiny", True), ("rand", None)):
            G, mix = dr.inputs(c, kind)
            W1, _, b = dr.weights(c["C"], c["tc"], c["F"], kind)
            with monkeypatch.context() as mp:
                mp.setattr(dr, "_floor", fl)
                mp.setattr(dr, "_den_eps", de)
                with np.errstate(all="ignore"):
                    dev = dr.final_f32(G, W1, b, c["F"], mix, 0.3, c["mode"], None, c["rows"], "f32").astype(np.float32)
            ref = t._final_ref(c, kind, 0, "f32")
            try:
                t._check_final(name, c, kind, code, dev, *ref)
                failed = False
            except AssertionError:
                failed = True
            assert fails is None or failed == fails, (name, kind, failed)
