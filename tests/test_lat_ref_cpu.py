"""CPU checks of tests/lat_ref.py, the references and case tables of tests/test_gpu_lat_kernels.py: the float32 restatement of
lat_gemm_kernel stays inside the a-priori cap, the float64 reference agrees with the lane emulation of tests/test_lat_cpu.py
(nz, a_parts, relu_in and the row map included, on the library's own packer), the aid's extents are what the emulated launch asks
for, the exact probes are exact, the tables reach what they claim, and the transform references restate stft_ref's.  No GPU."""
import numpy as np
import pytest

import lat_ref as lr
import stft_ref as sr
from deepconvsep_amd import _lib
from oracle import stft_np
from test_lat_cpu import _emu_gemm

CASES = lr.gemm_cases()


def _flat_a(c, inp):
    e = lr.extents(c)
    flat = np.full(e["A"], np.nan, dtype=np.float64)
    for p in range(c["a_parts"]):
        flat[p * c["a_part_stride"]:p * c["a_part_stride"] + c["n_A1"]] = inp["A"][p]
    return flat


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_reference_restatement_and_emulation(c):
    inp = lr.gemm_inputs(c, "signed")
    want, S = lr.reference(c, inp), lr.reference(c, inp, "abs")
    rest = lr.restatement(c, inp)
    assert want.shape == (max(c["nz"], 1), c["M"], c["n_store"]) and np.isfinite(want).all() and np.isfinite(rest).all()
    d = np.abs(rest.astype(np.float64) - want)
    assert np.all(d <= lr.roundings(c) * lr.U * S), "%s: the restatement is outside the cap by %.3g" % (c["name"], np.max(d / (lr.roundings(c) * lr.U * S + 1e-300)))
    assert not rest[S == 0].any() and not want[S == 0].any()
    # the lane emulation on the packed weights: index arithmetic of the production form
    lib = _lib.load()
    Bp = lr.pack_b(lib, inp["B"], c["K"], c["n_cb"], c["slice_len"], c["n_slices"])
    touched = {}
    emu = _emu_gemm(_flat_a(c, inp), c["a_row_stride"], c["M"], c["K"], Bp, c["J"], c["slice_len"], c["n_slices"], c["n_cb"], nz=c["nz"],
                    a_parts=c["a_parts"], a_part_stride=c["a_part_stride"], relu_in=c["relu_in"], a_gdiv=c["a_gdiv"], a_gmul=c["a_gmul"],
                    a_scale=float(np.float32(inp["a_scale"])), touched=touched)
    emu = emu.reshape(max(c["nz"], 1), c["M"], -1)[:, :, :c["n_store"]].copy()
    emu[0] += inp["bias"][:c["n_store"]].astype(np.float64)[None, :]
    if c["relu"] and c["nz"] <= 1:
        emu = np.maximum(emu, 0)
    assert np.isfinite(emu).all(), "the emulated lanes read an element no row owns"
    np.testing.assert_allclose(emu, want, rtol=0, atol=1e-9 * max(1.0, float(S.max())))
    # the aid's extents are exactly what the launch asks for
    e = lr.extents(c)
    assert touched["A"] + 1 == e["A"] and touched["Bp"] + 1 == e["Bp"], (touched, e)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_exact_probes_are_exact(c):
    for kind in lr.kinds_of(c):
        if kind == "signed":
            continue
        inp = lr.gemm_inputs(c, kind)
        want = lr.reference(c, inp)
        assert np.array_equal(lr.restatement(c, inp).astype(np.float64), want), (c["name"], kind)
        assert np.all(np.abs(want) < 2 ** 24)
        if kind == "ties":
            j = np.arange(c["n_store"])
            assert not want[0][j % c["M"], j].any()
        if kind == "onehot":
            A = np.nan_to_num(inp["A"])[:, inp["idx"]].sum(axis=0)              # [M][K]
            assert A.sum(axis=1).max() == 1 and set(np.unique(A)) <= {0.0, 1.0}
            k = A.argmax(axis=1)
            rows = np.where(A.any(axis=1)[:, None], inp["B"][k, :c["n_store"]], 0).astype(np.float64)
            if c["relu"] and c["nz"] <= 1:
                rows = np.maximum(rows, 0)
            assert np.array_equal(want.sum(axis=0), rows)                        # one part holds the row of B, the others 0


def test_case_table_reaches_what_it_claims():
    by = {c["name"]: c for c in CASES}
    pooled = {}
    for c in CASES:
        pooled[(c["J"], c["a_parts"])] = pooled.get((c["J"], c["a_parts"]), 0) + max(c["nz"], 1) * c["M"] * c["n_store"]
        assert c["M"] <= 49 and c["K"] <= 1028
    assert set(pooled) == set(lr.PRODUCTION) | lr.AID_ONLY and len(pooled) == 10
    assert all(n >= lr.MIN_POOLED for n in pooled.values()), pooled
    prod = {(c["J"], c["a_parts"]) for c in CASES if c["src"].startswith("net.hip") and c["name"] != "rowmap"}
    assert prod == set(lr.PRODUCTION), prod
    assert {c["J"] for c in CASES if (c["J"], c["a_parts"]) in lr.AID_ONLY} == {1, 3, 5}
    # conv1 at K1 = 516: slice 14 partly past K, slice 15 wholly; at 1028 slice 15 holds 8 of its 68
    c = by["conv1_K516_nz1"]
    assert (c["slice_len"], c["J"]) == (36, 3) and 14 * 36 < 516 < 15 * 36
    c = by["conv1_K1028_nz1"]
    assert (c["slice_len"], c["J"]) == (68, 5) and 1028 - 15 * 68 == 8
    c = by["conv2_nz4_parts1"]
    assert c["waves"] == 4 and lr.k_ranges(c)[3] == (12 * 52, 780) and c["n_A1"] == 40 * 52 and 780 % 16 == 12
    c = by["fc1x_M21_parts4"]
    assert (c["J"], c["n_store"], c["ldc"], c["relu_in"]) == (2, 90, 90, 1)
    assert int(lr.arow(by["rowmap"]).max()) == 36 and by["rowmap"]["M"] == 17
    for c in CASES:                                                              # the parts tile K
        kr = lr.k_ranges(c)
        assert kr[0][0] == 0 and kr[-1][1] == c["K"] and all(a[1] == b[0] for a, b in zip(kr, kr[1:])), c["name"]
    p, q = lr.chain_cases()
    assert lr.extents(p)["C"] == lr.extents(q)["A"]
    for c in (by["conv2_nz4_parts4"], by["fc1x_M21_parts1"]):
        assert len(lr.gemm_refusals(c)) >= 25


def test_chain_reference_bounds_its_restatement():
    p, q = lr.chain_cases()
    ip, iq = lr.gemm_inputs(p, "signed"), lr.gemm_inputs(q, "signed")
    want, bound = lr.chain_reference(p, q, ip, iq)
    parts = lr.restatement(p, ip)                                               # [4][M][128] float32
    A = np.full((4, q["n_A1"]), np.nan, dtype=np.float32)
    for z in range(4):
        A[z] = parts[z].reshape(-1)[:q["n_A1"]]
    got = lr.restatement(q, dict(iq, A=A))[0]
    assert np.all(np.abs(got - want) <= bound) and bound.max() < 1e-3 * np.abs(want).max()


def test_forward_table():
    cs = lr.forward_cases()
    assert len(cs) == 48
    for N, hop in lr.SHAPES:
        mine = [c for c in cs if (c["N"], c["hop"]) == (N, hop)]
        for skew in (0, 1):
            sub = [c for c in mine if c["skew"] == skew]
            assert {c["n_samples"] for c in sub} == {1, hop - 1, N // 2 + 1, 4 * hop, 7 * hop + 37}
            assert {c["rows_extra"] for c in sub} == {0, 7} and {c["phase"] for c in sub} == {True, False}
            assert {c["ld"] for c in sub} == {N // 2 + 1, (N // 2 + 4) // 4 * 4, N // 2 + 8}
        for c in mine:
            T = stft_np.frame_count(c["n_samples"], hop)
            inside = lr.forward_inside(c)
            if c["n_samples"] <= N // 2 + 1:
                assert inside == 0
            elif c["n_samples"] == 4 * hop:
                assert 0 < inside < T
            else:
                assert inside >= 4 > lr.forward_inside(dict(c, n_samples=4 * hop))
            if c["silence"]:
                X = sr.forward_ref64(lr.forward_audio(c), N, hop)
                assert any(not X[t].any() for t in range(T)) and any(X[t].any() for t in range(T))


def test_inverse_table_and_references():
    cs = lr.inverse_cases()
    for N, hop in lr.SHAPES:
        mine = [c for c in cs if (c["N"], c["hop"]) == (N, hop)]
        R = N // hop
        assert {1, R - 1, R, 9} <= {c["T"] for c in mine} and {c["n_src"] for c in mine} == {1, 3, 4, 5}
        assert {c["ld"] for c in mine} == {N // 2 + 1, N // 2 + 4}
        full = [c["n_out"] - (hop * (c["T"] - 1) + N // 2) for c in mine]
        assert 0 in full and 5 in full and any(c["n_out"] == 1 for c in mine) and any(c["n_out"] % 2 and c["n_out"] > 1 and f < 0 for c, f in zip(mine, full))
    for c in cs[::3]:
        mag, unit = lr.inverse_inputs(c)
        want, f32 = lr.frames_ref(c, mag, unit)
        e = lr.inverse_extents(c)
        assert e["frames"] * 4 == c["n_src"] * c["T"] * c["N"] * 4
        for s in range(c["n_src"]):
            ref64, ref32 = sr.inverse_ref64(mag[s], unit, c["N"], c["hop"]), sr.inverse_ref32(mag[s], unit, c["N"], c["hop"])
            n = min(c["n_out"], ref64.size)
            # the frame-order sum of the restated frames is stft_ref's restatement, bit for bit; of the float64 frames its reference
            assert np.array_equal(lr.ola_ref(c, f32[s:s + 1])[0, :n], ref32[:n])
            acc = np.zeros(c["hop"] * (c["T"] - 1) + c["N"])
            for t in range(c["T"]):
                acc[t * c["hop"]:t * c["hop"] + c["N"]] += want[s, t]
            norm = sr.inverse_norm(c["N"], c["hop"], c["T"], ref64.size)
            np.testing.assert_allclose(acc[c["N"] // 2:] / np.where(norm > 0, norm, 1), ref64, rtol=0, atol=1e-11)
            assert not lr.ola_ref(c, f32[s:s + 1])[0, ref64.size:].any()
