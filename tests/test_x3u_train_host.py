"""fp32-class training attention at the head widths outside the pipelined x 3 kernels (dk = 96 / 192 / 256), the part that needs no GPU:
the routing predicate and its switch, the shapes of the in-kernel dropout form, the C ABI entry, and the register / scratch figures of the
DROP instantiations of the LDS pooling pass."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TAKEN = [(900, 256), (500, 192), (900, 96), (300, 96), (1024, 256)]
LEFT = [(200, 128), (900, 128), (256, 64), (1025, 256), (900, 264), (100, 83)]


def test_x3u_train_ok_by_shape(monkeypatch):
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    monkeypatch.setattr(SA, "X3U_TRAINING", True)
    monkeypatch.setattr(SF, "FP32_ATTENTION", "x3")
    for k, dk in TAKEN:
        assert SA.x3u_train_ok(k, dk) is True, (k, dk)
    for k, dk in LEFT:
        assert SA.x3u_train_ok(k, dk) is False, (k, dk)


def test_x3u_train_ok_follows_the_switch_and_the_exact_setting(monkeypatch):
    from snuffy_amd import autograd as SA
    from snuffy_amd import functional as SF
    assert isinstance(SA.X3U_TRAINING, bool)
    monkeypatch.setattr(SF, "FP32_ATTENTION", "x3")
    monkeypatch.setattr(SA, "X3U_TRAINING", False)
    assert not any(SA.x3u_train_ok(k, dk) for k, dk in TAKEN + LEFT)
    monkeypatch.setattr(SA, "X3U_TRAINING", True)
    monkeypatch.setattr(SF, "FP32_ATTENTION", "exact")
    assert not any(SA.x3u_train_ok(k, dk) for k, dk in TAKEN + LEFT)


def test_x3u_attn_dropout_supported():
    from snuffy_amd import ops
    assert ops.x3u_attn_dropout_supported(900, 256) and ops.x3u_attn_dropout_supported(4, 16)
    for k, dk in ((901, 256), (1028, 192), (8, 24)):
        assert not ops.x3u_attn_dropout_supported(k, dk), (k, dk)
    for k in range(1, 1030):                                                     # the definition, over the whole key range
        for dk in (16, 96, 192, 256, 264):
            assert ops.x3u_attn_dropout_supported(k, dk) == (ops.x3u_attn_supported(k, dk) and k % 4 == 0)


def test_abi_has_the_dropout_entry():
    from snuffy_amd import _ffi
    assert os.path.exists(_ffi.LIB_PATH), "libsnuffy_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "snf_sparse_attn_fwd_x3u_dropout_f32")
    res, args = _ffi.SIGNATURES["snf_sparse_attn_fwd_x3u_dropout_f32"]
    plain = _ffi.SIGNATURES["snf_sparse_attn_fwd_x3u_f32"][1]
    assert res is ctypes.c_int
    assert args == plain[:10] + [ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64] + plain[10:]


def test_sparse_attn_fwd_x3u_takes_a_dropout_argument():
    import inspect
    from snuffy_amd import ops
    assert inspect.signature(ops.sparse_attn_fwd_x3u).parameters["dropout"].default is None


def test_drop_instantiations_registers_and_scratch():
    """pt_v_lds_kernel<CT, DROP>: all eight instantiations are built and none has scratch or a spilled register (the kernel is
    __launch_bounds__(256, 2) with 128 accumulator registers at CT = 4)."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.isdir(objdir) or not os.path.exists(os.path.join(objdir, "sparse_attn_generic.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = scan_spills.kernels(objdir)
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    seen = {}
    for (obj, _, scratch, spilled, vgpr), name in zip(ks, names):
        if "pt_v_lds_kernel<" not in name:
            continue
        args = [a.strip() for a in name.split("<", 1)[1].split(">")[0].split(",")]
        assert obj == "sparse_attn_generic.o" and len(args) == 2, (obj, name)
        assert scratch == 0 and spilled == 0, (name, scratch, spilled)
        assert 0 < vgpr <= 256, (name, vgpr)
        seen[(int(args[0]), args[1] == "true")] = vgpr
    assert set(seen) == {(ct, drop) for ct in (1, 2, 3, 4) for drop in (False, True)}, sorted(seen)
