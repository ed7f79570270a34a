"""HOPRegNet on the HIP kernels, the parts that need no GPU: the C ABI of the MANO-with-gradient kernels, the trunk-only parameter
layout with the regression heads (reference keys, shapes, padding), and the CPU model still being what a config without DEVICE builds."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "artiboost_hip.h")


def _cfg(bb, **kw):
    return dict({"TYPE": "HOPRegNet", "PRETRAINED": "", "BACKBONE": {"TYPE": bb, "PRETRAINED": False, "FREEZE_BATCHNORM": False},
                 "HEAD": {"TYPE": "ManoBranch", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True,
                          "MANO_ASSETS_ROOT": "assets/mano_v1_2"},
                 "DATA_PRESET": {"IMAGE_SIZE": [224, 224], "CENTER_IDX": 9}}, **kw)


def test_header_declares_the_mano_pca_ops_with_checks_and_the_library_exports_them():
    txt = open(HEADER).read()
    for name in ("ab_mano_pca_fwd", "ab_mano_pca_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert re.search(r"@check\s+%s:" % name, txt), name
    from artiboost_amd import _lib
    lib = _lib.cdll()
    assert hasattr(lib, "ab_mano_pca_fwd") and hasattr(lib, "ab_mano_pca_bwd")
    from artiboost_amd import gen_torch_ops
    c = gen_torch_ops.contracts()
    assert any("g_betas" in cl for cl in c["ab_mano_pca_bwd"]) and any("full_pose" in cl for cl in c["ab_mano_pca_fwd"])


@pytest.mark.parametrize("bb,layers", [("ResNet18", (2, 2, 2, 2)), ("ResNet34", (3, 4, 6, 3))])
def test_trunk_only_store_has_the_reference_keys(bb, layers):
    from artiboost_amd.hpregnet import HOPRegNet
    from artiboost_amd.hybridnet import ParamStore
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "hpregnet_keys.json")))[bb]
    ref = {k: s for k, s in keys.items() if not k.startswith(HOPRegNet.MANO_LAYER_PREFIX)}
    st = ParamStore(device="cpu", layers=layers, reg_heads=15)
    ours = {k: list(v.shape) for k, v in st.reference_state_dict().items()}
    assert ours == ref, sorted(set(ours) ^ set(ref))[:8]
    assert not any(k.startswith(("backbone.", "hybrid_head.", "box_head.")) for k in ours)
    # the 18-, 10- and 9-wide outputs are padded to multiples of REG_PAD in the kernel layout
    for name, w in (("mano_branch.pose_reg", 18), ("mano_branch.shape_reg.0", 10), ("obj_transfhead.final_layer", 9)):
        assert st.entries[name + ".weight"].kshape[0] == -(-w // st.REG_PAD) * st.REG_PAD
        assert st.entries[name + ".bias"].kshape[0] % 4 == 0


@pytest.mark.parametrize("bb,layers", [("ResNet18", (2, 2, 2, 2)), ("ResNet34", (3, 4, 6, 3))])
def test_cpu_model_state_round_trips_through_the_store_bit_identically(bb, layers):
    from artiboost_amd import hpregnet
    from artiboost_amd.hybridnet import ParamStore
    torch.manual_seed(0)
    net = hpregnet.HOPRegNet(**_cfg(bb))
    with torch.no_grad():                      # non-trivial BatchNorm state too
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(); m.running_var.uniform_(0.5, 2.0); m.num_batches_tracked.fill_(7)
                m.weight.normal_(); m.bias.normal_()
    sd = net.state_dict()
    st = ParamStore(device="cpu", layers=layers, reg_heads=15)
    st.init_reference_like(seed=3)
    st.load_reference_state_dict(sd)
    back = st.reference_state_dict()
    assert list(back) == list(sd)
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    # padding rows of the padded heads are zero, weight and bias
    for name, w in (("mano_branch.pose_reg", 18), ("mano_branch.shape_reg.0", 10), ("obj_transfhead.final_layer", 9)):
        assert not st.view(name + ".weight")[w:].any() and not st.view(name + ".bias")[w:].any(), name
    # ... and back into a fresh CPU module
    net2 = hpregnet.HOPRegNet(**_cfg(bb))
    net2.load_state_dict(back, strict=True)
    for k, v in net2.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_without_a_hip_device_the_config_builds_the_torch_module():
    from artiboost_amd import hpregnet
    from artiboost_amd import registry as R
    for extra in ({}, {"DEVICE": "cpu"}):
        net = R.build_arch_model_list(dict(_cfg("ResNet34"), PREVIOUS=[], **extra), preset_cfg={"IMAGE_SIZE": [224, 224], "CENTER_IDX": 0})[0]
        assert type(net) is hpregnet.HOPRegNet
        assert isinstance(net.base_net, hpregnet.ResNet34) and not hasattr(net, "store")


def test_hip_device_selects_the_hip_model_class():
    """Only the dispatch is checked here (building needs the device): a HIP device name goes to regnet.HOPRegNetHIP."""
    from artiboost_amd import hpregnet, regnet
    seen = {}

    class Probe(regnet.HOPRegNetHIP):
        def __init__(self, **cfg):        # noqa: D401  (stands in for the device build)
            seen.update(cfg)

    orig = regnet.HOPRegNetHIP
    regnet.HOPRegNetHIP = Probe
    try:
        obj = hpregnet.HOPRegNet(**_cfg("ResNet34", DEVICE="cuda:0"))
    finally:
        regnet.HOPRegNetHIP = orig
    assert isinstance(obj, Probe) and seen["DEVICE"] == "cuda:0"
