"""The references of tests/train_gemm_ref.py alone (no GPU): the Ax restatement against NumPy's own views, the case table's
conditions (S > 0, integer sets below 2^24, ties attained, all three signs under r'), the float32 restatement inside the cap,
the restated extent computation against brute force, and the split-K path composed against the unsplit float64 GEMM."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import train_gemm_ref as tg

CASES = tg.cases()
BY_NAME = {c["name"]: c for c in CASES}


def test_ax_equals_numpy_views():
    rs = np.random.RandomState(0)
    # row-major and transposed
    M, K = 7, 5
    a = rs.rand(M * K)
    i = tg.ax_off(tg.ax1(K), np.arange(M))[:, None] + tg.ax_off(tg.ax1(1), np.arange(K))[None, :]
    assert np.array_equal(a[i], a.reshape(M, K))
    i = tg.ax_off(tg.ax1(1), np.arange(K))[:, None] + tg.ax_off(tg.ax1(K), np.arange(M))[None, :]
    assert np.array_equal(a[i], a.reshape(M, K).T)
    # conv1 windows (train_ca.hip:73-74): x [B][NCH][tc][F], rows (b, t, w), K (ch, j), overlapping (S1 < K1)
    B, NCH, tc, F, K1, S1 = 2, 2, 3, 16, 7, 3
    w1, plane = (F - K1) // S1 + 1, tc * F
    x = rs.rand(B, NCH, tc, F)
    win = sliding_window_view(x, K1, axis=3)[:, :, :, ::S1]                    # [B][NCH][tc][w1][K1]
    want = win.transpose(0, 2, 3, 1, 4).reshape(B * tc * w1, NCH * K1)
    rows, cols = tg.ax3(w1, tc, S1, F, NCH * plane), tg.ax2(K1, 1, plane)
    i = tg.ax_off(rows, np.arange(B * tc * w1))[:, None] + tg.ax_off(cols, np.arange(NCH * K1))[None, :]
    assert np.array_equal(x.reshape(-1)[i], want)
    # d1 = 1 (tc = 1)
    x1 = rs.rand(B, NCH, 1, F)
    want = sliding_window_view(x1, K1, axis=3)[:, :, :, ::S1].transpose(0, 2, 3, 1, 4).reshape(B * w1, NCH * K1)
    i = tg.ax_off(tg.ax3(w1, 1, S1, F, NCH * F), np.arange(B * w1))[:, None] + tg.ax_off(tg.ax2(K1, 1, F), np.arange(NCH * K1))[None, :]
    assert np.array_equal(x1.reshape(-1)[i], want)
    # map positions and conv2 windows (train_ca.hip:75, 77): U [B][tc][w1][C], rows (b, h, w), K (dh, dw, c); w2 = 1 gives d0 = 1
    for w1_ in (5, 3):
        C, tc, kh, kw = 10, 4, 2, 3
        h2, w2, row1 = tc - kh + 1, w1_ - kw + 1, w1_ * C
        u = rs.rand(B, tc, w1_, C)
        win = sliding_window_view(u, (kh, kw), axis=(1, 2))                    # [B][h2][w2][C][kh][kw]
        want = win.transpose(0, 1, 2, 4, 5, 3).reshape(B * h2 * w2, kh * kw * C)
        i = (tg.ax_off(tg.ax3(w2, h2, C, row1, tc * row1), np.arange(B * h2 * w2))[:, None] +
             tg.ax_off(tg.ax2(kw * C, 1, row1), np.arange(kh * kw * C))[None, :])
        assert np.array_equal(u.reshape(-1)[i], want)
    # a K concatenation (train_ca.hip:185): [NB][B][flat] read as [B][NB flat]; d0 161 and a power of two
    for flat in (161, 64):
        NB, Bn = 3, 5
        d = rs.rand(NB, Bn, flat)
        i = tg.ax_off(tg.ax1(flat), np.arange(Bn))[:, None] + tg.ax_off(tg.ax2(flat, 1, Bn * flat), np.arange(NB * flat))[None, :]
        assert np.array_equal(d.reshape(-1)[i], d.transpose(1, 0, 2).reshape(Bn, NB * flat))
    # d0 d1 clipped at 2^30: ax2's second level never wraps
    assert tg.ax_off(tg.ax2(7, 1, 100), tg.BIG - 1) == (tg.BIG - 1) % 7 + (tg.BIG - 1) // 7 * 100


def test_table_covers_what_the_issue_lists():
    inst = {(c["tile"], c["ak"], c["bk"]) for c in CASES}
    assert inst == tg.PRODUCTION | tg.AID_ONLY and len(inst) == 12
    for key in inst:
        rows = [c for c in CASES if (c["tile"], c["ak"], c["bk"]) == key and " tails " in c["name"]]
        bm, bn = tg.BLOCK[key[0]]
        assert sorted(c["M"] for c in rows) == [1, bm - 1, bm, bm + 1, 2 * bm + 1]
        assert sorted(c["N"] for c in rows) == [1, bn - 1, bn, bn + 1, 2 * bn + 1]
        assert {(1, 1), (2 * bm + 1, 2 * bn + 1)} <= {(c["M"], c["N"]) for c in rows}
    ks = {c["K"] for c in CASES if " tails " in c["name"]}
    assert {1, 3, 31, 32, 33, 64, 95} <= ks and {k % 4 for k in ks} == {0, 1, 2, 3}
    split = [c for c in CASES if c["splits"] > 1]
    assert {c["kchunk"] for c in split} >= {32, 64} and {c["splits"] for c in split} >= {2, 3, 5}
    last = {k1 - k0 for c in split for k0, k1 in tg.slices(c)[-1:]}
    assert {1, 31, 32, 64} <= last
    assert any(c["nbatch"] == 2 and c["splits"] == 3 for c in split)
    assert any(c["partial"] and c["splits"] == 1 for c in CASES)
    ones = [c for c in CASES if c["ones_row"] < c["M"]]
    assert all(c["ones_row"] == c["M"] - 1 for c in ones) and {c["ak"] for c in ones} == {0, 1}
    assert any(c["ones_klim"] < c["K"] for c in ones) and any(c["ones_klim"] == c["K"] for c in ones)
    assert any(c["splits"] > 1 and c["ones_klim"] % c["kchunk"] for c in ones)
    bm = lambda c: tg.BLOCK[c["tile"]][0]
    assert any(c["M"] == bm(c) + 1 for c in ones) and any(0 < c["ones_row"] % bm(c) < bm(c) - 1 and c["M"] < bm(c) for c in ones)
    d0s = {m[k][0] for c in CASES for m in (c["A"], c["B"], c["C"], c["X"]) for k in ("r", "c")}
    assert {1, 7, 30, 161, 64} <= d0s
    assert any(m[k][1] == 1 and m[k][0] < tg.BIG for c in CASES for m in (c["A"],) for k in ("r", "c"))
    assert any(c["bias_cs"] == 0 and c["nbatch"] == 4 for c in CASES)
    assert any(all(c[n]["off"] for n in tg.OPERANDS) for c in CASES)
    assert {c["scale"] for c in CASES} >= {1.0, -1.0, 0.0, None}
    assert all(not (c["epi"] & tg.EPI_SAVEPRE and c["epi"] & tg.EPI_DRELU) for c in CASES)
    assert max(max(c["M"], c["N"], c["K"]) for c in CASES) <= 400


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_case(c):
    # the restated extent equals the brute-force extreme of the offsets; C (and X) address every output once
    for name in tg.OPERANDS:
        if not tg.used(c, name):
            continue
        idx = np.stack([tg.index(c, name, b) for b in range(c["nbatch"])])
        assert (int(idx.min()), int(idx.max())) == tg.extent(c, name), name
        assert idx.min() >= 0
        if name in ("C", "X") and (name == "C" or c["epi"] & tg.EPI_SAVEPRE):
            assert np.unique(idx).size == idx.size, "%s: two outputs at one address" % name
    assert all(k1 > k0 for k0, k1 in tg.slices(c)) and tg.slices(c)[-1][1] == c["K"]
    for kind in tg.kinds_of(c):
        inp = tg.inputs(c, kind)
        want, S = tg.reference(c, inp), tg.reference(c, inp, "abs")
        key = "partial" if c["partial"] else "C"
        if c["partial"] or c["scale"] != 0.0:
            live = np.ones(S[key].shape, dtype=bool)
            if c["partial"] and c["ones_row"] < c["M"]:                      # the ones row of a slice past ones_klim is all zeros
                for s, (k0, _) in enumerate(tg.slices(c) * c["nbatch"]):
                    live[s, c["ones_row"]:] = k0 < c["ones_klim"]
            assert np.all(S[key][live] > 0) and not S[key][~live].any(), "an output nothing but zeros goes into"
        if kind == "signed":
            rest = tg.reference(c, inp, "f32")
            for (k0, k1), s in zip(tg.slices(c) * c["nbatch"], range(c["nbatch"] * c["splits"])) if c["partial"] else [((0, c["K"]), slice(None))]:
                cap = (k1 - k0 + tg.roundings(c)) * tg.U * S[key][s]
                assert np.all(np.abs(rest[key][s].astype(np.float64) - want[key][s]) <= cap)
            if c["epi"] & tg.EPI_DRELU:
                x = np.concatenate([inp["X"][tg.index(c, "X", b)].reshape(-1) for b in range(c["nbatch"])])
                assert x.size < 16 or ((x > 0).any() and (x < 0).any() and (x == 0).any())
        else:
            assert tg.max_partial(c, inp) < 2 ** 24
            rest = tg.reference(c, inp, "f32")
            assert np.array_equal(rest[key].astype(np.float64), want[key]), "the integer set is not exact in float32"
            if kind == "ties":
                assert (want["pre"] == 0).any()
                assert want["pre"].size < 3 or ((want["pre"] > 0).any() and (want["pre"] < 0).any())
            if c["epi"] & tg.EPI_DRELU:
                x = np.concatenate([inp["X"][tg.index(c, "X", b)].reshape(-1) for b in range(c["nbatch"])])
                assert x.size < 16 or ((x > 0).any() and (x < 0).any() and (x == 0).any())


@pytest.mark.parametrize("name", tg.REFUSAL_CASES)
def test_refusal_rows_are_short_by_what_they_claim(name):
    c = BY_NAME[name]
    rows = dict(tg.refusals(c))
    for op in tg.OPERANDS:
        if tg.used(c, op):
            hi = max(int(tg.index(c, op, b).max()) for b in range(c["nbatch"]))
            assert 4 * (hi + 1) - rows["%s one byte short" % op][op + ".bytes"] == 1
    if c["partial"]:
        assert 4 * c["nbatch"] * c["splits"] * c["M"] * c["N"] - rows["partial one byte short"]["partial_bytes"] == 1
    for b in ("bias", "bias2"):
        if c[b]:
            hi = max(c["boff"][k][4] for k in range(c["nbatch"])) + (c["N"] - 1) * c["bias_cs"]
            assert 4 * (hi + 1) - rows[b + " one byte short"][b + "_bytes"] == 1
    assert rows["kchunk 48 with two slices" if c["partial"] else "two slices without partial"]
    assert min(rows["a negative stride"]["B.r"][2:]) < 0


def test_split_k_path_composes_to_the_unsplit_gemm():
    """partial slices -> finish / reduce, in float64, equal the unsplit float64 GEMM to 1e-12"""
    n = 0
    for c in CASES:
        if not c["partial"] or c["splits"] < 2:
            continue
        inp = tg.inputs(c, "signed")
        part = tg.reference(c, inp)["partial"].reshape(c["nbatch"], c["splits"], c["M"], c["N"])
        whole = dict(c, partial=False, splits=1, kchunk=c["K"], epi=0, bias=False, bias2=False, scale=None)
        want = tg.reference(whole, inp)["C"]
        for b in range(c["nbatch"]):
            s = np.zeros((c["M"], c["N"]))
            for z in range(c["splits"]):
                s = s + part[b, z]
            assert np.max(np.abs(s - want[b])) <= 1e-12 * max(1.0, np.max(np.abs(want[b])))
            # and the float32 helpers on the float32 slices stay within their caps of it
            p32 = part[b].astype(np.float32)
            got, _ = tg.finish_ref(p32, None, None, 0)
            assert np.max(np.abs(got - want[b])) <= 1e-4 * max(1.0, np.max(np.abs(want[b])))
            r = tg.reduce_ref(p32.reshape(c["splits"], -1), -1.0, c["N"], 1)
            assert np.array_equal(r[:c["M"] * c["N"]], -got.reshape(-1)) and np.array_equal(r[c["M"] * c["N"]:], -got[-1])
        n += 1
    assert n >= 15


def test_helper_references():
    # finish: against float64 within splits + 1 roundings; r'(0) = 0.5 exactly
    for B, N, splits, epi, bias in tg.FINISH_ROWS:
        part, b, X = tg.finish_inputs(B, N, splits, epi, bias)
        C, pre = tg.finish_ref(part, b, X, epi)
        s64 = part.astype(np.float64).sum(axis=0) + (b.astype(np.float64)[None] if bias else 0.0)
        S = np.abs(part).astype(np.float64).sum(axis=0) + (np.abs(b).astype(np.float64)[None] if bias else 0.0)
        w64 = s64 * tg.relu_d(X) if epi & tg.EPI_DRELU else s64
        w64 = np.maximum(w64, 0) if epi & tg.EPI_RELU else w64
        assert np.all(np.abs(C - w64) <= (splits + 2) * tg.U * S)
        assert (B * N) % 256 or N == 256
        if epi & tg.EPI_DRELU:
            assert (X == 0).any() and (X > 0).any() and (X < 0).any()
            assert np.array_equal(C[X == 0], (np.float32(0.5) * tg.finish_ref(part, b, X, 0)[0])[X == 0])
        else:
            assert np.array_equal(C, np.maximum(pre, 0))
    assert any((B * N) % 256 for B, N, *_ in tg.FINISH_ROWS)
    # conv1^T: the float32 chain inside (taps C1 + 1) u S; columns without a tap hold bo alone
    for which in tg.DECONV1:
        seen_untapped = False
        for row in tg.DECONV1_ROWS:
            g, W, bo = tg.deconv1_inputs(which, *row)
            q64, taps = tg.deconv1_ref(which, *row, g, W, bo)
            q32, _ = tg.deconv1_ref(which, *row, g, W, bo, "f32")
            S, _ = tg.deconv1_ref(which, *row, g, W, bo, "abs")
            assert np.all(np.abs(q32 - q64) <= ((taps * tg.C1 + 1) * tg.U)[None, None, None, :] * S)
            d = tg.deconv1_geom(which, *row)
            dead = taps == 0
            assert np.array_equal(np.flatnonzero(dead), np.arange(d["S1"] * (d["w1"] - 1) + tg.K1, row[2]))
            seen_untapped = seen_untapped or dead.any()
            assert np.array_equal(q64[..., dead], np.broadcast_to(bo.astype(np.float64)[None, :, None, None], q64.shape)[..., dead])
            assert len(set(bo.tolist())) == d["ns"]
        assert seen_untapped and any(r[2] == tg.K1 for r in tg.DECONV1_ROWS)
