"""The FFN output projection's split of the last round without its sum (snf_gemm_hl_deferred_f32), the head that adds the deferred K
part as it reads (snf_ln_mean_head_deferred_f32) and the model switch (ops.GEMM_HL_DEFERRED)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (m, n, k) on a 256-CU device: 12 tiles on a 16-workgroup grid, four XCDs with one remainder tile each (the first three);
# 384 tiles on 256 workgroups, 16 remainder tiles per XCD (config B's geometry at a sixth of its K)
GEMM_SHAPES = [(900, 768, 3072), (777, 520, 512), (1024, 768, 512), (32768, 768, 512)]
REMAINDER_TILES = {(900, 768, 3072): 4, (777, 520, 512): 4, (1024, 768, 512): 4, (32768, 768, 512): 128}


def _operands(m, n, k):
    from snuffy_amd import ops
    g = torch.Generator().manual_seed(m + n + k)
    a = (torch.randn(m, k, generator=g) * 0.5).to(DEV)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(DEV)
    b = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(m, n, generator=g).to(DEV)
    return a, w, b, res, ops.split_hl_rows(a), ops.split_hl_weight(w)


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_deferred_gemm_against_the_plain_walk_and_fp64(m, n, k, monkeypatch):
    """c + (slab where the map says so) against the plain tile walk (2e-6 scale) and fp64 (8e-6 scale), twice the same bits, a dirty
    workspace changes nothing, and the map names exactly the slabs that were written."""
    from snuffy_amd import ops
    nb = ops.gemm_hl_deferred_ws_bytes(m, n, k)
    assert nb > 0                                                     # the shape splits on this device
    a, w, b, res, a_hl, w_hl = _operands(m, n, k)
    ws = torch.full((nb,), 0xAB, dtype=torch.uint8, device=DEV)       # dirty: the call writes the whole map itself
    c, dk = ops.gemm_hl_deferred(a_hl, w_hl, b, resid=res, workspace=ws)
    z = dk.add_to(c)
    tm, tn = (m + 255) // 256, (n + 255) // 256
    assert tuple(dk.tile_map.shape) == (tm, tn) and dk.ws is ws
    # the map: non-zero exactly at the tiles whose slab was written (a slab nobody wrote still holds the 0xAB fill), one slab per tile
    written = (dk.slabs.view(torch.int32).view(dk.slabs.shape[0], -1) != -0x54545455).any(dim=1).nonzero().flatten().tolist()
    named = sorted((dk.tile_map[dk.tile_map != 0] - 1).tolist())
    assert named == written and len(named) == REMAINDER_TILES[(m, n, k)]
    assert int(dk.tile_map.min()) == 0 and int(dk.tile_map.max()) <= dk.slabs.shape[0]
    # bit-reproducible, from a clean and from a dirty workspace (fresh from the allocator)
    c2, dk2 = ops.gemm_hl_deferred(a_hl, w_hl, b, resid=res)
    assert torch.equal(c2, c) and torch.equal(dk2.tile_map, dk.tile_map) and torch.equal(dk2.add_to(c2), z)
    del c2, dk2
    for _ in range(2):
        junk = torch.full((nb,), 0xAB, dtype=torch.uint8, device=DEV)
        del junk                                                      # the next allocation of this size gets the same block back, dirty
        c3, dk3 = ops.gemm_hl_deferred(a_hl, w_hl, b, resid=res)
        assert torch.equal(dk3.add_to(c3), z)
        del c3, dk3
    monkeypatch.setattr(ops, "GEMM_HL_SPLITK", False)
    plain = ops.gemm_hl(a_hl, w_hl, b, resid=res)
    scale = max(1.0, plain.abs().max().item())
    d_plain = (z - plain).abs().max().item()
    rows = torch.cat([torch.arange(0, min(300, m)), torch.arange(max(m - 300, 0), m)]).unique()
    ref = a[rows].cpu().double() @ w.cpu().double().t() + b.cpu().double() + res[rows].cpu().double()
    d_ref = (z[rows.to(DEV)].cpu().double() - ref).abs().max().item()
    print("deferred gemm %s: |z - plain| = %.3e, |z - fp64| = %.3e, scale %.3f" % ((m, n, k), d_plain, d_ref, scale))
    assert d_plain <= 2e-6 * scale
    assert d_ref <= 8e-6 * scale


def test_deferred_gemm_refuses_what_it_does_not_do():
    from snuffy_amd import _ffi, ops
    lib = _ffi.load()
    m, n, k = 900, 768, 512
    _, _, b, _, a_hl, w_hl = _operands(m, n, k)
    nb = ops.gemm_hl_deferred_ws_bytes(m, n, k)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    out = torch.empty(m, n, device=DEV)

    def call(act, odt, mm=m):
        return lib.snf_gemm_hl_deferred_f32(ops._p(a_hl), a_hl.stride(0), ops._p(w_hl), w_hl.stride(0), ops._p(b), None, 0, mm, n, k,
                                            _ffi.ACT_CODES[act], ops._p(out), out.stride(0), odt, ops._p(ws), nb, ops._stream())
    assert call("relu", _ffi.DT_F32) == _ffi.SNF_EUNSUPPORTED
    assert call("none", _ffi.DT_BF16) == _ffi.SNF_EUNSUPPORTED
    assert ops.gemm_hl_deferred_ws_bytes(100000, 768, 512) == 0       # many full rounds: no split, and the entry says so
    with pytest.raises(ValueError):
        ops.gemm_hl_deferred(torch.zeros(256, 2 * k, dtype=torch.bfloat16, device=DEV), w_hl, b)
    assert call("none", _ffi.DT_F32) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def head_cases():
    """(z, DeferredK, z summed) at n = 900 and n = 777, d = 768, made once."""
    from snuffy_amd import ops
    out = {}
    for n in (900, 777):
        _, _, b, res, a_hl, w_hl = _operands(n, 768, 512)
        assert ops.gemm_hl_deferred_ws_bytes(n, 768, 512) > 0
        z, dk = ops.gemm_hl_deferred(a_hl, w_hl, b, resid=res)
        assert int((dk.tile_map != 0).sum()) == 4
        out[n] = (z, dk, dk.add_to(z))
    return out


@pytest.mark.parametrize("n", [900, 777])
@pytest.mark.parametrize("addends", ["none", "slot", "all"])
def test_head_adds_the_deferred_part_first(head_cases, n, addends):
    """logits, pooled and z_out are bit for bit those of the same kernel on the summed z."""
    from snuffy_amd import ops
    z, dk, zsum = head_cases[n]
    d, kk = 768, 200
    g = torch.Generator().manual_seed(n)
    gamma, beta = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
    wh, bh = torch.randn(2, d, generator=g).to(DEV), torch.randn(2, generator=g).to(DEV)
    kw = {}
    if addends != "none":
        sel = torch.randperm(n, generator=g)[:kk]
        slot = torch.full((n,), -1, dtype=torch.int32)
        slot[sel] = torch.arange(kk, dtype=torch.int32)
        kw.update(slot=slot.to(DEV), delta_rows=torch.randn(kk, d, generator=g).to(DEV))
    if addends == "all":
        kw.update(add_bf16=torch.randn(n, d, generator=g).to(DEV).to(torch.bfloat16), add_bias=torch.randn(d, generator=g).to(DEV))
    for want_z in (False, True):
        got = ops.ln_mean_head(z, gamma, beta, 1e-5, wh, bh, want_z=want_z, deferred=dk, **kw)
        ref = ops.ln_mean_head(zsum, gamma, beta, 1e-5, wh, bh, want_z=want_z, **kw)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        if want_z:
            assert torch.equal(got[2], ref[2])
            if addends == "none":
                assert torch.equal(got[2], zsum)
        else:
            assert got[2] is None


def _smallest_hl_bag(d, f):
    """The smallest bag from 900 rows up that takes the one-pass (hl) path AND whose FFN output projection splits its last round."""
    from snuffy_amd import ops
    for n in [900] + [256 * t + 1 for t in range(4, 200)]:
        if ops.hl_eligible(n, 2 * d, d) and ops.hl_eligible(n, f, d) and ops.hl_eligible(n, d, f) and ops.gemm_hl_deferred_ws_bytes(n, d, f):
            return n
    raise AssertionError("no hl bag below 51 k rows splits on this device")


def test_model_switch_on_against_off_and_graph_replay(monkeypatch):
    from snuffy_amd import functional as SF
    from snuffy_amd import ops
    from snuffy_amd.snuffy import build_milnet
    D, h, lam = 768, 6, 200
    torch.manual_seed(0)
    net = build_milnet(D, h, "relu", lam, 0.0, 1)
    for _, p in net.named_parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)
    f = net.b_classifier.encoder.layers[0].feed_forward.w_1.weight.shape[0]
    N = _smallest_hl_bag(D, f)
    print("model test at N = %d" % N)
    x = torch.randn(1, N, D, generator=torch.Generator().manual_seed(1)).to(DEV)
    net = net.to(DEV).eval().configure(precision="fp32", return_attention=False)
    layer = net.b_classifier.encoder.layers[0]
    seen = []
    real = ops.gemm_hl_deferred
    monkeypatch.setattr(ops, "gemm_hl_deferred", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    with torch.no_grad():
        monkeypatch.setattr(ops, "GEMM_HL_DEFERRED", True)
        c_on, y_on, _ = net(x)
        sel_on = layer.last_selection[0].clone()
        assert seen, "the deferred form was not taken"
        # materialize() of the deferred Parts == base + addend
        feats, scores = net._critic(x)
        parts, _ = net.b_classifier.encoder.run_layers(*SF.check_bag(feats, scores))
        assert parts.deferred is not None and not parts.plain
        want = parts.deferred.add_to(parts.base)
        want[parts.slot >= 0] += parts.delta[parts.slot[parts.slot >= 0].long()]
        assert torch.equal(SF.materialize(parts), want)
        # graph replay == eager, bit for bit
        net.configure(graph_max_patches=1 << 20)
        outs = [net(x) for _ in range(3)]
        assert getattr(net, "_graphs", None), "the forward was not captured"
        for c_g, y_g, _ in outs:
            assert torch.equal(c_g, c_on) and torch.equal(y_g, y_on)
        net.configure(graph_max_patches=0)
        n_seen = len(seen)
        monkeypatch.setattr(ops, "GEMM_HL_DEFERRED", False)
        c_off, y_off, _ = net(x)
        sel_off = layer.last_selection[0]
        assert len(seen) == n_seen
    assert torch.equal(sel_on, sel_off) and torch.equal(c_on, c_off)
    err = (y_on - y_off).abs().max().item()
    print("switch on vs off: |dlogit| = %.3e" % err)
    assert err < 1e-3                                                 # the fp32 bound of tests/test_gpu_configs.py against the oracle
