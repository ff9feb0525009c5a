"""The float64 reference of ``dcs_mask_fold_apply`` (tests/chanmask_ref.py) checked against itself, without a GPU: it is what
tests/test_gpu_chanmask.py and tests/test_gpu_separate_channels.py hold the kernel to."""
import numpy as np
import pytest

import chanmask_ref as ref

CASES = ref.build_cases()
SMALL = sorted(k for k, v in CASES.items() if v["F"] < 100)


def _covered(c):
    """rows some tile reaches, within the case's row count"""
    return min(c["n_frames"], (c["p"].shape[1] - 1) * (c["tc"] - c["ov"]) + c["tc"]) if c["p"].shape[1] else 0


def test_the_case_table_covers_what_the_kernel_test_promises():
    vals = list(CASES.values())
    for tc, ov in ref.SHAPES:
        for n in ref.TILES:
            for conv in ref.CONVENTIONS:
                assert any((v["tc"], v["ov"], v["p"].shape[1], v["conv"]) == (tc, ov, n, conv) for v in vals), (tc, ov, n, conv)
    assert set(v["S"] for v in vals) == {1, 2, 4, 5, 8}
    assert any(v["S"] == 4 and v["p"].shape[0] == 6 for v in vals)
    assert set(v["mag"].shape[0] for v in vals) == {1, 2, 3}
    assert set((v["F"], v["ld"]) for v in vals) == {(33, 40), (70, 72), (513, 513)}
    for v in vals:
        total = v["p"].shape[1] * (v["tc"] - v["ov"]) + v["tc"]
        v["_rows"] = "below" if v["n_frames"] < total else "equal" if v["n_frames"] == total else "above"
    assert set(v["_rows"] for v in vals) == {"below", "equal", "above"}
    # every S value on every kernel path it can take, with tiles to fold
    for S in (1, 2, 4, 5, 8):
        for tc, ov in ref.SHAPES:
            path = ref.kernel_path(S, tc, ov)
            assert any(ref.kernel_path(v["S"], v["tc"], v["ov"]) == path and v["S"] == S and v["p"].shape[1] == 11 for v in vals), (S, path)
    assert set(ref.kernel_path(v["S"], v["tc"], v["ov"]) for v in vals) == {"mm3", "mm6", "loop"}
    assert ref.covering_tiles(30, 25) == 6 and ref.covering_tiles(30, 20) == 3 and ref.covering_tiles(30, 29) == 30


@pytest.mark.parametrize("name", SMALL)
def test_reference_equals_the_frame_parallel_fold(name):
    c = CASES[name]
    m = ref.tile_masks(c["p"][:c["S"]], c["conv"])
    a, b = ref.fold(m, c["ov"], c["n_frames"]), ref.fold_frame_parallel(m, c["ov"], c["n_frames"])
    assert a.shape == b.shape == (c["S"], c["n_frames"], c["F"])
    assert np.array_equal(a, b)
    est, mask = ref.chanmask_ref(c["p"][:c["S"]], c["mag"], c["ov"], c["conv"], c["n_frames"])
    assert np.array_equal(mask, a) and est.shape == (c["mag"].shape[0],) + a.shape
    assert np.array_equal(est, a[None] * c["mag"].astype(np.float64)[:, None])
    assert not mask[:, _covered(c):].any()                       # rows past the last tile


@pytest.mark.parametrize("name", [k for k in SMALL if CASES[k]["conv"] == "A"])
def test_convention_a_masks_sum_to_one_on_every_covered_row(name):
    """With overlap 1 the reference's ramp is ``np.linspace(0, 1, 1) = [0.]`` and so is its reverse (util.py:306-307): the one
    row two tiles share is ``0 * old + 0 * new``.  Those rows are zero by the reference's own arithmetic, every other covered
    row sums to 1."""
    c = CASES[name]
    _, mask = ref.chanmask_ref(c["p"][:c["S"]], c["mag"], c["ov"], "A", c["n_frames"])
    total = mask.sum(axis=0)
    rows = np.arange(_covered(c))
    st = c["tc"] - c["ov"]
    dead = (rows >= st) & (rows % st == 0) & (rows // st < c["p"].shape[1]) if c["ov"] == 1 else np.zeros(len(rows), dtype=bool)
    assert np.all(np.abs(total[rows[~dead]] - 1.0) <= 1e-15)
    assert not total[rows[dead]].any()


@pytest.mark.parametrize("name", SMALL)
def test_a_bin_with_every_source_zero(name):
    c = CASES[name]
    S = c["S"]
    assert not c["p"][:S, ..., 3].any()
    m = ref.tile_masks(c["p"][:S], c["conv"])
    assert np.all(m[..., 3] == (1.0 / S if c["conv"] == "A" else 0.0))
    # the planted column where only source 0 is present
    if S > 1:
        assert np.all(m[1:, ..., 5] <= (0.5 if c["conv"] == "A" else 0.0)) and np.all(m[0, ..., 5] > 0)
