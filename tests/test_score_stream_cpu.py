"""The references of the score stream against the oracle (no GPU): the per-frame masks of tests/score_stream_ref.py are
``filterSpec`` on the window ``(0, T)`` bit for bit, the synthetic tables hold the corner cases they promise, and the candidate
range a push looks at never drops a row that is active in one of its frames."""
import numpy as np
import pytest

from oracle import score_np

import score_stream_ref as ssr

# (ninst, T, F, nharm, boundary)
TABLES = ((1, 24, 33, 4, 9), (3, 40, 33, 4, 14), (4, 61, 65, 5, 5), (4, 97, 513, 6, 50), (2, 30, 33, 3, None))


@pytest.mark.parametrize("normalise", ["max", "sum"])
@pytest.mark.parametrize("table", TABLES, ids=lambda t: "i%d_T%d_F%d" % t[:3])
def test_frame_masks_are_filterspec_bit_for_bit(table, normalise):
    ninst, T, F, nharm, b = table
    notes = ssr.synth_table(ninst, T, F, nharm, b, seed=ninst + T)
    want = score_np.filterSpec(np.zeros((T, F), np.float32), notes, ninst, 0, T, None, normalise=normalise)
    got = ssr.all_frame_masks(notes, T, F, normalise)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got, want.reshape(T, ninst, F).transpose(1, 0, 2))
    # the definition goes on past the signal (window (0, +inf)): after every end frame nothing is on
    assert not ssr.frame_on(ssr._counting_rows(notes), ninst, T + 3, F).any()


def test_the_tables_hold_their_corner_cases():
    ninst, T, F, nharm, b = TABLES[2]
    notes = ssr.synth_table(ninst, T, F, nharm, b, seed=1)
    rows = ssr._counting_rows(notes)
    on = np.stack([ssr.frame_on(rows, ninst, t, F) for t in range(T)], axis=1)                      # [ninst, T, F]
    by_inst = [[r for r in rows if r[0] == j] for j in range(ninst)]
    assert not by_inst[ninst - 1] and (ssr.frame_masks(notes, 3, F, 'max')[ninst - 1] == 1.0).all()  # no notes: all ones
    assert any(a[1] < c[2] and c[1] < a[2] for a in by_inst[0] for c in by_inst[0] if a is not c)   # overlapping notes
    assert (on[0] & on[1]).any()                                                                    # a shared cell
    assert any(r[1] == 0 for r in rows) and any(r[2] == T for r in rows)
    assert any(f1 == F for r in rows for _, f1 in r[3])
    assert ((notes[..., 2] == 0) & (notes[..., 1] > notes[..., 0])).any()                           # midi == 0 with a duration
    pairs = notes[..., 3:].reshape(ninst, -1, nharm, 2)
    assert ((pairs[..., 1] > 0) & (pairs[..., 0] == pairs[..., 1])).any()                           # a zero-width slot, fe > 0
    assert any(r[1] <= b - 1 and r[2] >= b + 2 for r in rows)
    assert on[0, :, :].any(axis=1)[b - 1:b + 2].all()


@pytest.mark.parametrize("table", TABLES[:3], ids=lambda t: "i%d_T%d_F%d" % t[:3])
def test_candidate_range_never_drops_an_active_row(table):
    ninst, T, F, nharm, b = table
    notes = ssr.synth_table(ninst, T, F, nharm, b, seed=7)
    rows, t0, end_max = ssr.sorted_rows(notes)
    assert t0 == sorted(t0) and end_max == sorted(end_max) and len(rows) >= 3
    for a in range(T + 2):
        for e in range(a + 1, T + 3):
            lo, hi = ssr.candidate_range(t0, end_max, a, e)
            assert 0 <= lo <= hi <= len(rows)
            for i, r in enumerate(rows):
                if r[1] < e and r[2] > a:                         # active in a frame of [a, e)
                    assert lo <= i < hi, (a, e, i, r)
            # and the masks built from the candidates alone are the masks
            if e == a + 1 and a < T:
                assert np.array_equal(ssr.frame_on(rows[lo:hi], ninst, a, F), ssr.frame_on(rows, ninst, a, F))
