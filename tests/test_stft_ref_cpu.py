"""tests/stft_ref.py checked on the CPU: the float32 restatement against float64 on every (frameSize, hop) of the GPU file's
tables, the case tables against the list of launcher branches they are meant to reach, the clip table and the error measure."""
import numpy as np
import pytest

import stft_ref as sr
from oracle import stft_np

INV_PAIRS = sorted({(c["N"], c["hop"]) for c in sr.inverse_cases()} | set(sr.F64_INVERSE))
FWD_PAIRS = sorted({(c["N"], c["hop"]) for c in sr.forward_cases() if not c["fpw4"]} | {(1024, 16)} | set(sr.F64_FORWARD))


@pytest.mark.parametrize("N,hop", INV_PAIRS)
def test_float32_inverse_restatement_is_close_to_float64(N, hop):
    """A device bound of FACTOR x the restatement's error stays inside the project's 1e-5 only if the restatement itself is
    within 1e-5 / FACTOR; it is 6e-8 .. 2.1e-7 in the weighted measure."""
    case = sr._inv("cpu", "none", N, hop, n_out=min(30 * hop + 1, 20000) if hop > 2 else 101, n_src=1, seed=N + hop)
    mag, unit = sr.inverse_inputs(case)
    want = sr.inverse_ref64(mag[0], unit[0], N, hop)
    got = sr.inverse_ref32(mag[0], unit[0], N, hop)
    assert got.shape == want.shape == (stft_np.inverse_length(case["T"], hop, N),)
    norm = sr.inverse_norm(N, hop, case["T"], want.size)
    err = sr.weighted_error(got, want, norm)
    print("inverse (%d, %d): weighted %.3g, raw %.3g" % (N, hop, err, np.max(np.abs(got - want))))
    assert err <= sr.BOUND_INV / sr.FACTOR
    # Im at DC / Nyquist is ignored by both
    unit2 = unit.copy()
    unit2[:, :, 0] = unit2[:, :, 0].real
    unit2[:, :, N // 2] = unit2[:, :, N // 2].real
    assert np.array_equal(sr.inverse_ref64(mag[0], unit2[0], N, hop), want)
    assert np.array_equal(sr.inverse_ref32(mag[0], unit2[0], N, hop), got)
    # phase input: the same signal
    ph = np.angle(unit[0]).astype(np.float32)
    assert sr.weighted_error(sr.inverse_ref32(mag[0], None, N, hop, phase=ph), sr.inverse_ref64(mag[0], None, N, hop, phase=ph),
                             norm) <= sr.BOUND_INV / sr.FACTOR


@pytest.mark.parametrize("N,hop", FWD_PAIRS)
def test_float32_forward_restatement_is_close_to_float64(N, hop):
    case = sr._fwd("cpu", "none", N, hop, frames=12, seed=N + hop)
    a = sr.forward_audio(case)[0]
    want, got = sr.forward_ref64(a.astype(np.float32), N, hop), sr.forward_ref32(a, N, hop)
    assert got.shape == want.shape == (stft_np.frame_count(a.size, hop), N // 2 + 1)
    e_mag, e_cpx = np.max(np.abs(np.abs(got) - np.abs(want))), np.max(np.abs(got - want))
    print("forward (%d, %d): mag %.3g complex %.3g" % (N, hop, e_mag, e_cpx))
    assert e_mag <= sr.BOUND_MAG / sr.FACTOR and e_cpx <= sr.BOUND_CPX / sr.FACTOR


def test_case_tables_reach_every_regime():
    inv, fwd = set(), set()
    for c in sr.inverse_cases():
        r = sr.regimes(c)
        assert r, c["name"]
        inv |= r
    for c in sr.forward_cases():
        fwd |= sr.forward_regimes(c)
    assert not set(sr.INVERSE_REGIMES) - inv, sorted(set(sr.INVERSE_REGIMES) - inv)
    assert not set(sr.FORWARD_REGIMES) - fwd, sorted(set(sr.FORWARD_REGIMES) - fwd)
    print("inverse regimes reached:", sorted(inv))
    print("forward regimes reached:", sorted(fwd))


def test_cases_name_the_kernel_they_are_meant_for():
    by = {c["name"]: sr.expected_inverse(c) for c in sr.inverse_cases()}
    assert by["chain3_r2_nb25"] == (sr.INV_CHAIN, 3) and by["chain7_r4_2048_512_nb+0"] == (sr.INV_CHAIN, 7)
    assert by["chain_r4_2048_512_nb+1"] == (sr.INV_CHAIN, 3) and by["chain_units7_spc1"] == (sr.INV_CHAIN, 1)
    assert by["seq5_1024_256"] == (sr.INV_SEQ, 5) and by["seq1_2048_512"] == (sr.INV_SEQ, 1)
    assert by["stage_2048_512_src8"] == (sr.INV_SEQ_STAGED, 1)
    for name in ("stage_broken_nsrc3", "stage_broken_ldM8", "stage_broken_magoff", "stage_broken_ucs_odd"):
        assert by[name] == (sr.INV_CHAIN, 3), name
    assert by["ring_4096_2"][0] == sr.INV_RING and by["ring_1024_64"][0] == sr.INV_RING
    assert by["block_1024_700"][0] == sr.INV_BLOCK and by["block_1024_512"][0] == sr.INV_BLOCK
    # phase input never chains or stages
    for c in sr.inverse_cases():
        if c["public"]:
            assert sr.expected_inverse(dict(c, phase_input=True))[0] in (sr.INV_SEQ, sr.INV_RING, sr.INV_BLOCK)


def test_launcher_arithmetic():
    g = sr.chain_geometry(1024, 512, sr.n_out_for_blocks(1024, 512, 25), 3)
    assert (g["R"], g["Sb"], g["Gc"], g["last_blocks"]) == (2, 23, 2, 1)
    assert sr.chain_geometry(2048, 512, sr.n_out_for_blocks(2048, 512, 24), 1)["Sb"] == 21       # LC = R - 1 at the least
    assert sr.chain_geometry(1024, 256, sr.n_out_for_blocks(1024, 256, 57), 7)["Gc"] == 2
    assert sr.ring_slots(2048, 128) == 32 and sr.ring_slots(4096, 512) == 16 and sr.ring_slots(4096, 2) == 4096
    assert sr.ring_lds(4096, 2) <= 160 * 1024
    assert sr.block_inverse_plan(4096, 4092, 1000, 1, 256)["tw_lds"] and not sr.block_inverse_plan(4096, 4095, 1000, 1, 256)["tw_lds"]
    p = sr.block_inverse_plan(2048, 2048, 40 * 2048, 48, 256)
    assert p["PF"] == 5 and p["halved"] and p["C"] == 2
    assert sr.block_inverse_plan(8192, 2048, 1000, 1, 256)["PF"] == 17
    assert sr.block_inverse_plan(64, 16, sr.cap_n_out(256), 8, 256)["C"] == 16
    assert sr.block_inverse_plan(8192, 8192, 1000, 1, 256, size=8) is None                         # float64: DCS_EUNSUPPORTED
    assert sr.forward_block_tw_lds(4096) and not sr.forward_block_tw_lds(8192)
    assert sr.forward_block_tw_lds(2048, size=8) and not sr.forward_block_tw_lds(4096, size=8)


def test_clip_table_matches_dcs_frame_count():
    from deepconvsep_amd import _lib
    for hop in (2, 17, 256, 512, 4095):
        lengths = sr.ragged_lengths(hop) + [hop, hop + 1]
        for compact in (False, True):
            tab = sr.clip_table(lengths, hop, compact)
            assert tab.dtype == np.int64 and tab.shape == (5, sr.CLIP_TAB)
            assert [int(v) for v in tab[:, 0]] == lengths
            assert [int(v) for v in tab[:, 1]] == [_lib.frame_count(n, hop) for n in lengths]
            if compact:
                assert [int(v) for v in tab[:, 3]] == [int(v) for v in np.cumsum([0] + list(tab[:-1, 1]))]
                assert np.array_equal(tab[:, 5], tab[:, 1])
            else:
                assert (tab[:, 3] == -1).all()


def test_weighted_error_measure():
    rs = np.random.RandomState(0)
    a, norm = rs.randn(1000), rs.uniform(0, 2, 1000)
    d = rs.randn(1000)
    assert sr.weighted_error(a, a, norm) == 0.0
    e1, e3 = sr.weighted_error(a + 1e-3 * d, a, norm), sr.weighted_error(a + 3e-3 * d, a, norm)
    assert e1 > 0 and abs(e3 / e1 - 3) < 1e-9
    # a sample whose normaliser is tiny does not dominate
    norm[7], d2 = 1e-9, np.zeros(1000)
    d2[7] = 1.0
    assert sr.weighted_error(a + d2, a, norm) < 1e-9
    assert sr.weighted_error(a[:0], a[:0], norm[:0]) == 0.0
