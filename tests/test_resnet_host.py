"""ResNet-18 SimCLR patch extractor, the part that needs no GPU: the convolution plan of the library (output dims, tile counts,
refusals), the state-dict key order (torchvision's, because checkpoints load by position), SimCLR-shaped and roi.py-shaped checkpoints,
and compute_feats' backbone switch."""
import argparse
import os
import sys
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (cin, cout, kh, stride) of every convolution of the network, in forward order of first use
LAYER_CONVS = [(3, 64, 7, 2), (64, 64, 3, 1), (64, 128, 3, 2), (64, 128, 1, 2), (128, 128, 3, 1), (128, 256, 3, 2), (128, 256, 1, 2),
               (256, 256, 3, 1), (256, 512, 3, 2), (256, 512, 1, 2), (512, 512, 3, 1)]


def _block_keys(prefix, down, norm):
    keys = []
    for conv, bn in (("conv1", "bn1"), ("conv2", "bn2")):
        keys.append("%s.%s.weight" % (prefix, conv))
        keys += ["%s.%s.%s" % (prefix, bn, n) for n in norm]
    if down:
        keys.append(prefix + ".downsample.0.weight")
        keys += ["%s.downsample.1.%s" % (prefix, n) for n in norm]
    return keys


def torchvision_keys(batch):
    """state_dict().keys() of torchvision.models.resnet18(norm_layer=...) with fc = Identity, written out."""
    norm = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"] if batch else []
    keys = ["conv1.weight"] + ["bn1." + n for n in norm]
    for layer in (1, 2, 3, 4):
        keys += _block_keys("layer%d.0" % layer, layer > 1, norm)
        keys += _block_keys("layer%d.1" % layer, False, norm)
    return keys


INSTANCE_KEYS = [
    "conv1.weight",
    "layer1.0.conv1.weight", "layer1.0.conv2.weight", "layer1.1.conv1.weight", "layer1.1.conv2.weight",
    "layer2.0.conv1.weight", "layer2.0.conv2.weight", "layer2.0.downsample.0.weight", "layer2.1.conv1.weight", "layer2.1.conv2.weight",
    "layer3.0.conv1.weight", "layer3.0.conv2.weight", "layer3.0.downsample.0.weight", "layer3.1.conv1.weight", "layer3.1.conv2.weight",
    "layer4.0.conv1.weight", "layer4.0.conv2.weight", "layer4.0.downsample.0.weight", "layer4.1.conv1.weight", "layer4.1.conv2.weight",
]


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


@pytest.mark.parametrize("b,h,w", [(512, 224, 224), (2, 64, 64), (2, 72, 88), (3, 23, 18)])
def test_plan_every_layer_shape(b, h, w):
    """Output dims and tile counts (128 output pixels x 64 channels per workgroup) of every convolution of the network."""
    from snuffy_amd import ops
    ho, wo, m, tm, tn, ws = ops.conv2d_plan(b, h, w, 3, 64, 7, 2)
    assert (ho, wo) == (_out(h, 7, 2), _out(w, 7, 2)) and m == b * ho * wo and tm == -(-m // 128) and tn == 1 and ws == 0
    hh, ww = _out(ho, 3, 2), _out(wo, 3, 2)                    # max-pool
    for cin, cout, kh, stride in LAYER_CONVS[1:]:
        ho, wo, m, tm, tn, ws = ops.conv2d_plan(b, hh, ww, cin, cout, kh, stride)
        assert (ho, wo) == (_out(hh, kh, stride), _out(ww, kh, stride))
        assert m == b * ho * wo and tm == -(-m // 128) and tn == cout // 64 and ws == 0
        assert ops.conv2d_supported(b, hh, ww, cin, cout, kh, stride)
        if kh == 3 and stride == 2:
            nxt = (ho, wo)
        if kh == 1:                                            # the downsample convolution agrees with the block's strided 3x3
            assert (ho, wo) == nxt
            hh, ww = nxt


def test_plan_known_values_224():
    from snuffy_amd import ops
    assert ops.conv2d_plan(512, 224, 224, 3, 64, 7, 2) == (112, 112, 512 * 112 * 112, 50176, 1, 0)
    assert ops.conv2d_plan(512, 56, 56, 64, 64, 3, 1) == (56, 56, 512 * 56 * 56, 12544, 1, 0)
    assert ops.conv2d_plan(512, 14, 14, 256, 512, 3, 2) == (7, 7, 25088, 196, 8, 0)
    assert ops.conv2d_plan(3, 9, 11, 64, 128, 3, 2) == (5, 6, 90, 1, 2, 0)        # 30 pixels per image: a tile straddles images
    assert ops.conv2d_plan(3, 9, 11, 64, 128, 1, 2) == (5, 6, 90, 1, 2, 0)
    assert ops.conv2d_plan(3, 3, 3, 512, 512, 3, 1) == (3, 3, 27, 1, 8, 0)


def test_plan_refusals():
    from snuffy_amd import SnuffyHipError, ops
    for cin, cout, kh, stride in [(96, 64, 3, 1), (64, 96, 3, 1), (32, 64, 3, 1), (64, 64, 5, 1), (64, 64, 5, 2), (64, 64, 1, 1),
                                  (64, 64, 3, 3), (3, 64, 3, 1), (3, 128, 7, 2), (64, 64, 7, 2)]:
        assert not ops.conv2d_supported(2, 16, 16, cin, cout, kh, stride), (cin, cout, kh, stride)
        with pytest.raises(SnuffyHipError):
            ops.conv2d_plan(2, 16, 16, cin, cout, kh, stride)
    with pytest.raises(SnuffyHipError):
        ops.conv2d_plan(0, 16, 16, 64, 64, 3, 1)


def test_ops_refuse_cpu_tensors():
    from snuffy_amd import SnuffyHipError, ops
    with pytest.raises(SnuffyHipError):
        ops.conv_pack_weight(torch.zeros(64, 64, 3, 3))
    with pytest.raises(SnuffyHipError):
        ops.conv2d_nhwc(torch.zeros(1, 4, 4, 64), torch.zeros(64, 576, dtype=torch.bfloat16), None, 3, 1)
    with pytest.raises(SnuffyHipError):
        ops.instnorm_stats_nhwc(torch.zeros(1, 4, 4, 64))
    with pytest.raises(SnuffyHipError):
        ops.maxpool3x3s2_nhwc(torch.zeros(1, 4, 4, 64))


def test_state_dict_keys_are_torchvisions():
    from snuffy_amd.resnet import ResNet18
    inst = ResNet18("instance")
    assert list(inst.state_dict().keys()) == INSTANCE_KEYS == torchvision_keys(False)
    bat = ResNet18("batch")
    keys = list(bat.state_dict().keys())
    assert keys == torchvision_keys(True) and len(keys) == 20 + 20 * 5
    assert keys[:7] == ["conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked",
                        "layer1.0.conv1.weight"]
    i = keys.index("layer2.0.bn2.num_batches_tracked")
    assert keys[i + 1:i + 4] == ["layer2.0.downsample.0.weight", "layer2.0.downsample.1.weight", "layer2.0.downsample.1.bias"]
    assert not any(p.requires_grad for p in inst.parameters()) and not any(p.requires_grad for p in bat.parameters())
    sd = inst.state_dict()
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and tuple(sd["layer4.0.downsample.0.weight"].shape) == (512, 256, 1, 1)
    with pytest.raises(ValueError):
        ResNet18("group")
    with pytest.raises(ValueError):
        inst.configure("fp16")


def _simclr_checkpoint(model, seed=0):
    """What the SimCLR trainer saves: the backbone's tensors under Sequential names (features.N...), then the projection head."""
    g = torch.Generator().manual_seed(seed)
    ck = OrderedDict()
    for i, (k, v) in enumerate(model.state_dict().items()):
        ck["features.%d.%s" % (i, k.split(".", 1)[-1])] = torch.randn(v.shape, generator=g)
    ck["l1.weight"], ck["l1.bias"] = torch.randn(512, 512, generator=g), torch.randn(512, generator=g)
    ck["l2.weight"], ck["l2.bias"] = torch.randn(256, 512, generator=g), torch.randn(256, generator=g)
    return ck


def test_simclr_checkpoint_loads_by_position(tmp_path):
    from snuffy_amd import compute_feats as cf
    from snuffy_amd import vit
    from snuffy_amd.resnet import ResNet18
    emb = vit.IClassifier(ResNet18(), 512, 1)
    ck = _simclr_checkpoint(emb.feature_extractor)
    assert len(ck) == 24
    path = tmp_path / "dsmil_simclr.pth"
    torch.save(ck, path)
    fc_w, fc_b = emb.fc.weight.detach().clone(), emb.fc.bias.detach().clone()
    args = argparse.Namespace(weights=str(path), embedder="SimCLR", backbone="resnet18")
    msg = cf._load_model_weights(args, emb)
    assert sorted(msg.missing_keys) == ["fc.bias", "fc.weight"] and not msg.unexpected_keys
    for (k, v), src in zip(emb.feature_extractor.state_dict().items(), list(ck.values())[:20]):
        assert torch.equal(v, src), k
    assert torch.equal(emb.fc.weight, fc_w) and torch.equal(emb.fc.bias, fc_b)
    assert not any(p.requires_grad for p in emb.feature_extractor.parameters())


def test_roi_style_dict_loads_by_name():
    """roi.py:318-330: IClassifier(resnet18(norm_layer=InstanceNorm2d) with fc = Identity, 512, ...) and its own state dict."""
    from snuffy_amd import vit
    from snuffy_amd.resnet import ResNet18
    g = torch.Generator().manual_seed(1)
    src = OrderedDict(("feature_extractor." + k, torch.randn(v.shape, generator=g)) for k, v in ResNet18().state_dict().items())
    src["fc.weight"], src["fc.bias"] = torch.randn(2, 512, generator=g), torch.randn(2, generator=g)
    emb = vit.IClassifier(ResNet18(norm_layer="instance"), 512, 2)
    msg = emb.load_state_dict(src, strict=False)
    assert not msg.missing_keys and not msg.unexpected_keys
    assert list(emb.state_dict().keys()) == list(src.keys())
    for k, v in emb.state_dict().items():
        assert torch.equal(v, src[k]), k


def test_get_embedder_backbone():
    from snuffy_amd import compute_feats as cf
    from snuffy_amd.resnet import ResNet18
    args = argparse.Namespace(backbone="resnet18", norm_layer="instance", embedder="SimCLR", precision="bf16", patch_size=16)
    model, nf = cf.get_embedder_backbone(args)
    assert isinstance(model, ResNet18) and nf == 512 and model.norm_layer == "instance" and model.precision == "bf16"
    assert not any(p.requires_grad for p in model.parameters())
    args.norm_layer = "batch"
    model, nf = cf.get_embedder_backbone(args)
    assert nf == 512 and model.norm_layer == "batch" and "bn1.running_var" in model.state_dict()
    assert cf.device_preprocess(args)
    args.device_preprocess = 0
    assert not cf.device_preprocess(args)
    tf = cf.bag_dataset(argparse.Namespace(backbone="resnet18", batch_size=2, num_workers=0, transform=1, device_preprocess=0),
                        [])[0].dataset.transform
    assert isinstance(tf, cf.TileTransform) and tf.resize is None and not tf.normalize          # the reference's [ToTensor()]


def test_vit_backbones_unchanged():
    """The ViT branches answer as before; an unknown backbone is still refused (the parent passes this one by design)."""
    from snuffy_amd import compute_feats as cf
    from snuffy_amd import vit
    args = argparse.Namespace(backbone="vit_tiny", embedder="DINO", patch_size=16, precision="fp32")
    model, nf = cf.get_embedder_backbone(args)
    assert isinstance(model, vit.VisionTransformer) and nf == 192
    args = argparse.Namespace(backbone="vit_small", embedder="DINO_adapter", patch_size=16, adapter_ffn_scalar="1.0", ffn_num=8,
                              precision="fp32")
    model, nf = cf.get_embedder_backbone(args)
    assert isinstance(model, vit.VisionTransformer) and nf == 384
    with pytest.raises(ValueError):
        cf.get_embedder_backbone(argparse.Namespace(backbone="resnet50", embedder="SimCLR", patch_size=16))
    assert cf.device_preprocess(argparse.Namespace(backbone="vit_small"))
    assert not cf.device_preprocess(argparse.Namespace(backbone="resnet50"))


def test_new_kernels_keep_everything_in_registers():
    """No kernel of csrc/resnet.hip uses scratch (tools/scan_spills.py on the built objects; DESIGN has the register and LDS figures)."""
    import scan_spills
    objdir = os.path.join(scan_spills.ROOT, "snuffy_amd", "build")
    if not os.path.exists(os.path.join(objdir, "resnet.o")):
        pytest.skip("no build objects here (the library was built elsewhere)")
    try:
        ks = [k for k in scan_spills.kernels(objdir) if k[0] == "resnet.o"]
    except RuntimeError as exc:
        pytest.skip(str(exc))
    names = scan_spills.demangle([k[1] for k in ks])
    assert sum("conv2d_nhwc_kernel<" in n for n in names) == 13          # 3 forms x (x3, bf16 from f32, bf16 from bf16) + 2 x 2 stems
    assert any("instnorm_stats_kernel<" in n for n in names) and any("norm_act_nhwc_kernel<" in n for n in names)
    bad = [(n[:100], k[2], k[3]) for k, n in zip(ks, names) if k[2] or k[3]]
    assert not bad, bad
