"""The form table of tests/row_forms.py is complete, without a device: snf_row_form is the rule, the widths reach every register form of
every entry at both of its edges, and the long row counts walk the grid-stride loop exactly two and three times."""
import pytest

from tests import row_forms as RF


def test_row_form_is_the_rule_at_every_width():
    """snf_row_form == the two-line rule for d = 1 .. 2100, aligned and not; past the widest form it refuses."""
    for aligned in (True, False):
        for d in range(1, 2101):
            assert RF.row_form(d, aligned) == RF.form_rule(d, aligned), (d, aligned)
    assert RF.row_form(2048, True) == (4, 8) and RF.row_form(2048, False) == (1, 32)
    for d, aligned in RF.TOO_WIDE + [(RF.TOO_WIDE_HL, True)]:
        assert RF.row_form(d, aligned) is None
    lib = RF.lib()
    assert lib.snf_row_form(0, 1, None, None) == -1 and lib.snf_row_form(768, 1, None, None) == 0      # outputs nullable


def test_the_forms_by_width():
    """The table alone: the forms' top widths."""
    assert [64 * v * nv for v, nv in RF.VEC4_FORMS] == [256, 512, 768, 1024, 1536, 2048]
    assert [64 * v * nv for v, nv in RF.VEC1_FORMS] == [64, 128, 192, 256, 512, 1024, 2048]
    assert len(RF.FORMS) == 13


@pytest.mark.parametrize("entry", sorted(RF.ENTRIES))
def test_every_entry_reaches_every_form_at_both_edges(entry):
    """The completeness condition: no (entry, form) pair is left out."""
    _, cases = RF.ENTRIES[entry]
    hl = entry in RF.HL_ONLY
    reached = {}
    for d, aligned in cases:
        form = RF.row_form(d, aligned)
        assert form is not None, (entry, d)
        reached.setdefault(form, set()).add(d)
    want = RF.VEC4_FORMS if hl else RF.FORMS
    assert sorted(reached) == sorted(want), (entry, sorted(set(want) - set(reached)))
    for form in want:
        bottom, top = RF.form_edges(form, hl and entry != "layernorm_rows_split3")
        if entry == "layernorm_rows_split3" and form[0] == 4:
            bottom = RF.form_edges(form, True)[0]                    # split3 runs the VEC4 forms at the hl widths
        assert {bottom, top} <= reached[form], (entry, form, bottom, top, sorted(reached[form]))


def test_the_scalar_fallback_by_alignment():
    """d % 4 == 0 with an operand off its 16-byte boundary: the scalar form, among them the true tops of NV 4 and NV 32."""
    got = [RF.row_form(d, False) for d in RF.WIDTHS_VEC1_ALIGN]
    assert got == [(1, 4), (1, 16), (1, 32)]
    assert all(RF.row_form(d, True)[0] == 4 for d in RF.WIDTHS_VEC1_ALIGN)
    assert [64 * nv for _, nv in (got[0], got[2])] == [RF.WIDTHS_VEC1_ALIGN[0], RF.WIDTHS_VEC1_ALIGN[2]]


def test_long_cases_are_a_narrow_a_middle_and_a_wide_form_per_vec():
    forms = [RF.row_form(d, a) for d, a in RF.LONG_CASES]
    assert forms == [(4, 2), (4, 3), (4, 8), (1, 4), (1, 32)]
    assert set(RF.LONG_CASES) <= set(RF.CASES) and set(RF.LONG_HL) <= set(RF.WIDTHS_HL)
    assert [RF.row_form(d, True) for d in RF.DEFERRED_WIDTHS] == [(4, 3), (4, 6), (1, 4)]
    assert (RF.DEFERRED_WIDTHS[1] + 255) // 256 == 5                                  # five column blocks
    assert [RF.row_form(d, True) for d in RF.VARLEN_WIDTHS] == [(4, 3), (1, 4)]


def test_long_row_counts_are_two_and_three_trips():
    """Without a device the library sizes its grids for 256 compute units: 8192 rows a trip of the row kernels, 4096 of the head."""
    r, rh = RF.rows_per_trip(), RF.head_rows_per_trip()
    assert (r, rh) == (8192, 4096)
    for per in (r, rh):
        two, three = RF.long_rows(per)
        assert (RF.trips(two, per), RF.trips(three, per)) == (2, 3)
        assert three - 2 * per == 5                                                  # the last trip: one full workgroup and one row
        assert all(RF.trips(n, per) == 1 for n in RF.SHORT_ROWS)
        assert RF.marked_rows(three, per) == [0, three // 2, 2 * per, three - 1]
    assert RF.long_rows(r)[1] == 16389                                               # the largest bag of the form tests
    # the deferred head's bag (2 R + 261) and the varlen bags: three trips, the last one past a 256-row band
    assert RF.trips(2 * rh + 261, rh) == 3 and RF.trips(2 * rh + 9, rh) == 3 and RF.trips(rh + 5, rh) == 2
    n = RF.colsum_long_rows()
    blocks = RF.lib().snf_colsum_blocks(n)
    assert -(-n // blocks) > 32 and n % -(-n // blocks) != 0


def test_the_deferred_pattern_differs_where_a_stale_entry_would_come_from():
    rh = RF.head_rows_per_trip()
    stride = rh // 256
    tiles_m, tiles_n = (2 * rh + 261 + 255) // 256, 5
    for tm in range(tiles_m):
        for tn in range(tiles_n):
            here = RF.deferred_pattern(tm, tn, stride)
            if tn + 1 < tiles_n:
                assert here != RF.deferred_pattern(tm, tn + 1, stride)               # the next column block
            if tm + stride < tiles_m:
                assert here != RF.deferred_pattern(tm + stride, tn, stride)          # the same wave's next trip
    bands = [tuple(RF.deferred_pattern(tm, tn, stride) for tn in range(tiles_n)) for tm in range(tiles_m)]
    # the next row band (but across a multiple of the trip stride, where the two terms in tm cancel: no pattern mod 2 has all three)
    assert all(a != b for tm, (a, b) in enumerate(zip(bands, bands[1:])) if (tm + 1) % stride)
    assert len(set(bands)) == 2 and 0 < sum(map(sum, bands)) < tiles_m * tiles_n
