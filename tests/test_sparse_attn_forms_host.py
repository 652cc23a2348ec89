"""ops.SPARSE_ATTN_FORMS, the form table of the tiled sparse attention, without a GPU: every record against what the library itself
answers on the host (workspace and plan entry points are pure host code), against the width rows of tests/attn_widths.py, and against
the names it holds."""
import ctypes
import inspect

import pytest

from snuffy_amd import _ffi, ops
from tests import attn_widths as W
from tests.attn_widths import _offsets

FORMS = ops.SPARSE_ATTN_FORMS
IDS = ["%s-%d" % (f.family, f.dk) for f in FORMS]
SIZES, H = [300, 5000], 2

# The predicates that answer for a record: `single` over all its key chunks, `one_launch` within one launch, `trains` where forward with
# dropout and backward run over chunks, and the varlen predicates.  Those of 64 / 128 take dk (and the varlen ones the precision).
PREDICATES = {
    ("bf16", True): dict(single=["mfma_attn_supported"], one_launch=["mfma_attn_bwd_supported", "mfma_attn_dropout_supported"],
                         trains=["mfma_attn_train_chunks_supported"]),
    ("x3", True): dict(single=["x3_attn_supported"], one_launch=["x3_attn_dropout_supported"], trains=[]),
    ("bf16", 192): dict(single=["mfma_attn_dk192_supported"], varlen="varlen_attn_dk192_supported"),
    ("bf16", 256): dict(single=["mfma_attn_dk256_supported", "mfma_attn_dk256_train_supported"], varlen="varlen_attn_dk256_supported"),
    ("x3", 192): dict(single=["x3_attn_dk192_supported"], varlen="varlen_attn_x3_dk192_supported"),
    ("x3", 256): dict(single=["x3_attn_dk256_supported"], varlen="varlen_attn_x3_dk256_supported"),
}


def _plan_rc(lib, form, entry, k):
    """Return code of a varlen plan function of the record for the bags SIZES (size query: no table)."""
    off = _offsets(SIZES)
    need, ws, nc, ck = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(-1), ctypes.c_int(-1)
    dims = (k, H, form.dk) if form.by_dk else (k, H)
    chunks = (ctypes.byref(nc), ctypes.byref(ck)) if entry.chunk_outputs else ()
    return getattr(lib, entry.c_plan)(ctypes.c_void_p(off.ctypes.data), len(SIZES), *dims, None, 0, ctypes.byref(need), ctypes.byref(ws), *chunks)


def _workspace(lib, form, k):
    fn = getattr(lib, form.c_workspace)
    if form.c_workspace == "snf_sparse_attn_fwd_workspace_bytes":
        return fn(SIZES[0], k, H, form.dk, 1)                                   # 1: the MFMA form of the shared function
    return fn(SIZES[0], k, H, form.dk) if form.by_dk else fn(SIZES[0], k, H)


@pytest.mark.parametrize("form", FORMS, ids=IDS)
def test_every_predicate_is_the_librarys_answer_at_every_key_count(form):
    """For every k from 0 to keys x chunks + 1: the single-bag predicates against `workspace bytes > 0`, the varlen predicates against
    the plan functions returning SNF_OK -- the one-launch plan is also the library's word on what one launch holds, which the one-launch
    predicates (dropout forward, one-launch backward) repeat."""
    lib = _ffi.load()
    kind = "fp32" if form.family == "x3" else "bf16"
    preds = PREDICATES[(form.family, True if form.by_dk else form.dk)]
    top = form.keys * form.chunks
    for k in range(0, top + 2):
        single = _workspace(lib, form, k) > 0
        assert single is (1 <= k <= top), k
        if form.by_dk:
            plain, chunked = (_plan_rc(lib, form, e, k) == _ffi.SNF_OK for e in form.varlen)
            assert plain is (1 <= k <= form.keys) and chunked is single, k
            assert ops.varlen_attn_supported(kind, k, form.dk) is plain, k
            assert ops.varlen_attn_chunks_supported(kind, k, form.dk) is chunked, k
            for name in preds["single"] + preds["trains"]:
                assert getattr(ops, name)(k, form.dk) is single, (name, k)
            for name in preds["one_launch"]:
                assert getattr(ops, name)(k, form.dk) is plain, (name, k)
        else:
            (entry,) = form.varlen
            assert getattr(ops, preds["varlen"])(k) is (_plan_rc(lib, form, entry, k) == _ffi.SNF_OK), k
            for name in preds["single"]:
                assert getattr(ops, name)(k) is single, (name, k)
        assert ops.sparse_attn_form_serves(form, k) is single, k
    # the predicates that take dk decline every width but their own records'
    for k in (1, 100, 128):
        for name in ("mfma_attn_supported", "mfma_attn_bwd_supported", "mfma_attn_train_chunks_supported", "mfma_attn_dropout_supported",
                     "x3_attn_supported", "x3_attn_dropout_supported"):
            assert getattr(ops, name)(k, form.dk) is (form.by_dk and k <= form.keys * form.chunks), (name, k)


def test_records_are_the_width_rows_of_the_tests():
    """Keys per launch, chunk counts and names of the rows in tests/attn_widths.py."""
    seen = 0
    for row in (W.X3_192, W.X3_256, W.MFMA_256, W.VARLEN_192, W.TRAIN_192, W.TRAIN_256):
        form = ops.sparse_attn_form("bf16" if row.family == "mfma" else row.family, row.dk)
        assert form is not None and form is ops.sparse_attn_form(getattr(row, "kind", form.family), row.dk)
        assert (row.single, row.single_takes_n) == (form.wrapper, form.takes_n), row.id
        if hasattr(row, "KMAX"):
            assert (row.KMAX, row.MAX_CHUNKS) == (form.keys, form.chunks), row.id
            assert row.plan_fn == form.varlen[-1].c_plan and row.ws_fn in (None, form.c_workspace), row.id
            assert row.varlen == ("sparse_attn_fwd_mfma_varlen" if form.family == "bf16" else "sparse_attn_fwd_x3_varlen")
            seen += 1
    assert seen == 4
    assert len({(f.family, f.dk) for f in FORMS}) == len(FORMS) == 8 and ops.sparse_attn_form("bf16", 96) is None


@pytest.mark.parametrize("form", FORMS, ids=IDS)
def test_every_name_resolves(monkeypatch, form):
    """Wrappers on ops -- with n in their signature exactly where the record says so, and reached through the module attribute by the
    dispatcher --, C names in _ffi.SIGNATURES, plan kinds in PackedBags.plan's table."""
    params = list(inspect.signature(getattr(ops, form.wrapper)).parameters)
    assert params[:3] == ["q", "v", "kp"] and (params[3] == "n") is form.takes_n and "h" in params[3:5]
    assert ("dropout" in params) is (form.c_dropout is not None) is (form.dropout_chunks > 0)
    for name in (form.c_fwd, form.c_dropout, form.c_workspace) + tuple(n for e in form.varlen for n in (e.c_plan, e.c_fwd)):
        assert name is None or name in _ffi.SIGNATURES, name
    assert len(form.varlen) == (2 if form.by_dk else 1) and [e.chunk_outputs for e in form.varlen] == [False, True][-len(form.varlen):]
    assert all(ops._VARLEN_PLANS[e.kind] is e for e in form.varlen)
    assert form.row_limits is (form.family == "bf16")
    # the dispatcher: the spy that stands in for the wrapper sees (q, v, kp[, n], h) and the keywords
    seen = []
    monkeypatch.setattr(ops, form.wrapper, lambda *a, **kw: seen.append((a, kw)))
    q = type("T", (), {"shape": (77, form.dk * H)})()
    ops.sparse_attn_fwd_form(form, q, "v", "kp", H, scale=0.5, need_attn=True)
    (args, kw), = seen
    assert args == ((q, "v", "kp", 77, H) if form.takes_n else (q, "v", "kp", H))
    assert kw == dict(scale=0.5, need_attn=True, need_lse=False, **({"dropout": None} if form.c_dropout else {}))


def test_row_limits_are_those_of_the_bf16_family():
    """n / ld beside each limit of the 32-bit row offsets; the fp32-class records have none."""
    bf16, x3 = ops.sparse_attn_form("bf16", 128), ops.sparse_attn_form("x3", 128)
    for n, ld, ok in ((0xffff00, None, True), (0xffff01, None, False), (100, (1 << 24) - 1, True), (100, 1 << 24, False),
                      (46340, 46341, True), (46341, 46341, False)):
        assert ops.sparse_attn_form_serves(bf16, 100, n, ld) is ok and ops.mfma_attn_supported(100, 128, n, ld) is ok, (n, ld)
        assert ops.sparse_attn_form_serves(x3, 100, n, ld) is True
