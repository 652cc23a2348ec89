"""The multiclass model's batched inference route (snuffy_multiclass.PACK_BATCH): a [B, N, D] batch as ONE packed launch set per layer
and one head launch, against the row loop (same selections, bit for bit) and the CPU oracle run row by row on the product's selection.
PACK_BATCH is forced on here, whatever value ships."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import snuffy_oracle as orc
from tests.helpers import tol_for                 # the project's flat gates: fp32 1e-3, bf16 1e-2

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 2
_NETS = {}


def make_net(D, h, lam, depth, r=0.5):
    """(state dict on the CPU, model on the GPU), built once per shape."""
    from snuffy_amd import snuffy_multiclass as smc
    key = (D, h, lam, depth, r)
    if key not in _NETS:
        torch.manual_seed(D + h + lam + depth)
        layer = smc.EncoderLayer(D, smc.MultiHeadedAttention(h, D), smc.PositionwiseFeedForward(D, 4 * D, "relu"), C, 0.0, lam, r)
        net = smc.MILNet(smc.FCLayer(D, C), smc.BClassifier(smc.Encoder(layer, depth), C, D))
        for p in net.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)
            else:
                torch.nn.init.normal_(p, std=0.1)
        for l in net.b_classifier.encoder.layers:                 # LayerNorm scales around one
            for sub in l.sublayer:
                sub.norm.weight.data.add_(1.0)
        net.b_classifier.encoder.norm.weight.data.add_(1.0)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        _NETS[key] = (sd, net.to(DEV).eval())
    return _NETS[key]


class Spy:
    """Records (rows, packed is not None) of every SF.encoder_layer / SF.head call."""

    def __init__(self, monkeypatch):
        from snuffy_amd import functional as SF
        self.layer_calls, self.head_calls = [], []
        enc, head = SF.encoder_layer, SF.head

        def spy_enc(x2, sel, layer, need_attn, precision, packed=None, **kw):
            self.layer_calls.append((x2.shape[0], packed is not None))
            return enc(x2, sel, layer, need_attn, precision, packed=packed, **kw)

        def spy_head(parts, norm, linear, packed=None):
            self.head_calls.append(packed is not None)
            return head(parts, norm, linear, packed=packed)

        monkeypatch.setattr(SF, "encoder_layer", spy_enc)
        monkeypatch.setattr(SF, "head", spy_head)


def oracle_rows(x, sd, h, sels):
    """The CPU oracle row by row with the selection forced to the product's: encoder layers, LayerNorm, mean, linear -- the
    composition of oracle.milnet_forward_multiclass.  sels: per layer [B, K] int64."""
    import torch.nn.functional as F
    classes = F.linear(x, sd["i_classifier.fc.0.weight"], sd["i_classifier.fc.0.bias"])
    p_all = None
    for l, sel in enumerate(sels):
        outs, ps = [], []
        for i in range(x.shape[0]):
            z, p, _ = orc.encoder_layer(x[i], None, sd, f"b_classifier.encoder.layers.{l}.", h, "relu", 0, 0.0, forced_sel=sel[i])
            outs.append(z)
            ps.append(p)
        x, p_all = torch.stack(outs), torch.stack(ps)
    xn = orc.layer_norm(x, sd["b_classifier.encoder.norm.weight"], sd["b_classifier.encoder.norm.bias"])
    logits = F.linear(xn.mean(dim=1), sd["b_classifier.linear.weight"], sd["b_classifier.linear.bias"])
    return classes, logits, p_all


CASES = [(300, 128, 2, 12, 1), (300, 256, 2, 12, 1), (700, 128, 2, 160, 1), (300, 128, 2, 12, 2)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_d%d_h%d_lam%d_depth%d" % c)
def test_batched_forward_matches_row_loop_selection_and_oracle(case, B, precision, monkeypatch):
    from snuffy_amd import snuffy_multiclass as smc
    N, D, h, lam, depth = case
    sd, net = make_net(D, h, lam, depth)
    net.configure(precision=precision, return_attention=True, sampler="reference")
    layers = list(net.b_classifier.encoder.layers)
    x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(N + B))
    xg = x.to(DEV)
    # the row loop's selections
    monkeypatch.setattr(smc, "PACK_BATCH", False)
    np.random.seed(17)
    with torch.no_grad():
        net(xg)
    loop_sel = [tuple(t.cpu() for t in l.last_selection) for l in layers]
    # the batched route
    monkeypatch.setattr(smc, "PACK_BATCH", True)
    spy = Spy(monkeypatch)
    np.random.seed(17)
    with torch.no_grad():
        classes, logits, A = net(xg)
    assert spy.layer_calls == [(B * N, True)] * depth and spy.head_calls == [True]
    sels = []
    for l, (t0, r0) in zip(layers, loop_sel):
        t1, r1 = l.last_selection
        assert torch.equal(t1.cpu(), t0) and torch.equal(r1.cpu(), r0)
        sels.append(torch.cat((t0, r0), dim=1))
    K = sels[-1].shape[1]
    assert K >= 2 and (lam != 160 or K > 256)                      # the third case runs above one key chunk
    assert tuple(A.shape) == (B, h, N, K) and tuple(logits.shape) == (B, C)
    classes_ref, logits_ref, p_ref = oracle_rows(x, sd, h, sels)
    tol = tol_for(precision, depth)
    err_c = float((classes.cpu() - classes_ref).abs().max())
    err_l = float((logits.cpu() - logits_ref).abs().max())
    err_a = float((A.cpu() - p_ref).abs().max())
    print("multiclass batch %s B=%d %s: |dclasses|=%.2e |dlogits|=%.2e |dA|=%.2e (tol %.0e)" % (case, B, precision, err_c, err_l, err_a, tol))
    assert err_c <= 2e-5
    assert err_l <= tol and err_a <= tol


def test_row_loop_is_kept_below_the_kernel_widths_and_under_autograd(monkeypatch):
    from snuffy_amd import snuffy_multiclass as smc
    monkeypatch.setattr(smc, "PACK_BATCH", True)
    B, N = 2, 300
    # dk = 32: no packed kernel takes it
    sd, net = make_net(64, 2, 12, 1)
    net.configure(precision="fp32", return_attention=True, sampler="reference")
    x = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    spy = Spy(monkeypatch)
    np.random.seed(3)
    with torch.no_grad():
        _, logits, A = net(x)
    assert spy.layer_calls == [(N, False)] * B and spy.head_calls == [False] * B
    assert tuple(A.shape)[:3] == (B, 2, N) and tuple(logits.shape) == (B, C)
    # autograd on: the row loop, whatever the shape
    sd, net = make_net(128, 2, 12, 1)
    net.configure(precision="fp32", return_attention=False, sampler="reference")
    x = torch.randn(B, N, 128, generator=torch.Generator().manual_seed(2)).to(DEV)
    spy.layer_calls.clear()
    spy.head_calls.clear()
    np.random.seed(3)
    with torch.enable_grad():
        net(x)
    assert spy.layer_calls == [(N, False)] * B and spy.head_calls == [False] * B
    # B = 1 and the switch off: the row loop as well
    spy.layer_calls.clear()
    with torch.no_grad():
        net(x[:1])
        monkeypatch.setattr(smc, "PACK_BATCH", False)
        net(x)
    assert spy.layer_calls == [(N, False)] * 3
