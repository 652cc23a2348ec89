"""The host answers of the tiled sparse-attention forward, pinned: tools/record_attn_plans.py replayed against the built library and compared
field by field with tests/golden/attn_plans.npz, which was recorded from the build before the drivers moved into csrc/attn_drive.h and
again, with the 256 entry points added, from the build before the width shells moved into csrc/attn_width.h.  Pure host code (cu_count() falls back to the MI355X's 256 without a device)."""
import os
import sys

import numpy as np

from snuffy_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_host_answers_match_the_recorded_ones():
    import record_attn_plans as rec
    got = rec.run(_ffi.load())
    with np.load(rec.GOLDEN) as want:
        assert set(got) == set(want.files)
        for prefix, fields in (("plan", ["plan_rc", "plan_error", "plan_table_ints", "plan_workspace_bytes", "plan_n_chunks", "plan_chunk_k",
                                         "plan_short_table_rc", "plan_short_table_error", "plan_table_len"]),
                               ("workspace", ["workspace_bytes"])):
            cases = want[prefix + "_case"]
            assert np.array_equal(got[prefix + "_case"], cases)                  # the case list is the recorded one
            for f in fields:
                bad = np.nonzero(got[f] != want[f])[0]
                assert bad.size == 0, (f, cases[bad[0]], got[f][bad[0]], want[f][bad[0]])
        # the tables, integer for integer
        ends = np.cumsum(want["plan_table_len"])
        for i in np.nonzero(want["plan_table_len"])[0]:
            a, b = ends[i] - want["plan_table_len"][i], ends[i]
            assert np.array_equal(got["plan_tables"][a:b], want["plan_tables"][a:b]), want["plan_case"][i]
        # what the list covers: refusals with their texts, one, two and eight chunks, short tables
        rc, nc = want["plan_rc"], want["plan_n_chunks"]
        assert (rc != 0).any() and all(e for e in want["plan_error"][rc != 0]) and (want["plan_short_table_rc"][rc == 0] != 0).all()
        assert {1, 2, 3, 8} <= set(nc[rc == 0].tolist())
