"""Row tail of the weight-gradient contraction (snf_gemm_tn_f32 for any bag length), the part that needs no GPU: the dispatch
predicate no longer asks for whole 32-row steps, and the tail variant of the kernel's staging costs no scratch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# scratch bytes per lane of the gemm_tn_kernel<X3, HL> instantiations in the build of the commit before the row tail (tools/scan_spills.py;
# the plane-image kernel spills one register pair in front of its loop -- outside the steady state -- and did so before)
PARENT_SCRATCH = {"<true, true>": 0, "<true, false>": 12, "<false, false>": 0}


def test_gemm_tn_supported_takes_any_bag_length():
    import torch
    from snuffy_amd import ops
    assert ops.gemm_tn_supported(2049, 256, 256)
    assert ops.gemm_tn_supported(32749, 768, 3072)
    assert ops.gemm_tn_supported(2048, 256, 256)
    assert not ops.gemm_tn_supported(1000, 256, 256)           # below 1024 rows the library contraction stays
    assert not ops.gemm_tn_supported(2049, 100, 256)           # 8-column granules
    assert not ops.gemm_tn_supported(2049, 64, 64)             # an output too small for the matrix cores
    a = torch.zeros(2049, 3 * 256, dtype=torch.bfloat16)
    assert not ops.gemm_tn_supported(2049, 256, 256, a, a)     # CPU images never reach the kernel


def test_one_pass_chain_predicate_does_not_ask_for_whole_steps(monkeypatch):
    """autograd._x3_train_hl_ok on a 256-CU device: a bag of 16 389 rows at D = 768 qualifies like one of 16 384."""
    from snuffy_amd import autograd as SA
    from snuffy_amd import ops

    class _Lib:
        @staticmethod
        def snf_device_cu_count():
            return 256

    monkeypatch.setattr(ops._ffi, "load", lambda: _Lib)
    monkeypatch.setattr(ops, "GEMM_HL", True)
    monkeypatch.setattr(ops, "GEMM_TN", True)
    monkeypatch.setattr(SA, "X3_TRAIN_HL", True)
    assert SA._x3_train_hl_ok(16384, 768, 3072)
    assert SA._x3_train_hl_ok(16389, 768, 3072)
    assert SA._x3_train_hl_ok(32749, 768, 3072)
    assert not SA._x3_train_hl_ok(3000, 768, 3072)             # too few 256 x 256 tiles for the chip
    assert not SA._x3_train_hl_ok(16389, 776, 3104)            # hl images come in 32-column groups


def test_gemm_tn_kernels_keep_their_scratch():
    """Every gemm_tn_kernel instantiation (bf16, plane x3, interleaved x3) needs no more scratch than before it had a row tail."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "gemm_tn.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    mine = {name.split("gemm_tn_kernel")[1].split("(")[0]: scratch for (_, _, scratch, _, _), name in zip(ks, names) if "gemm_tn_kernel<" in name}
    assert sorted(mine) == sorted(PARENT_SCRATCH), mine
    bad = {inst: scratch for inst, scratch in mine.items() if scratch > PARENT_SCRATCH[inst]}
    assert not bad, bad
