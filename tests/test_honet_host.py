"""CPU: HoNet -- the torch module against the reference's own values (tests/golden/honet.npz, honet_keys.json; written by
tests/gen_honet_golden.py), the Hasson-2020 remapping, registry / config / alias surface, the mesh-query producer of the synthetic loader,
the HoNet head set of the trunk-only parameter layout (and the HOPRegNet layout staying where it was), and the C ABI of the recovery
kernels."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CFG = os.path.join(ROOT, "config", "ho3dv2_honet_mi355x.yaml")


def _cfg(**kw):
    return dict({"TYPE": "HoNet", "PRETRAINED": "", "BACKBONE": {"TYPE": "ResNet18", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
                 "HEAD": {"TYPE": "ManoBranch", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True,
                          "MANO_ASSETS_ROOT": "assets/mano_v1_2"},
                 "DATA_PRESET": {"IMAGE_SIZE": [224, 224], "CENTER_IDX": 9}, "OBJ_TRANS_FACTOR": 100.0, "OBJ_SCALE_FACTOR": 0.0001}, **kw)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "honet.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def net():
    from artiboost_amd.honet import HoNet
    torch.manual_seed(0)
    return HoNet(**_cfg())


class _Stub(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, *a, **k):
        return dict(self.value) if isinstance(self.value, dict) else self.value


def _run_on_golden(g, with_corners, dtype=torch.float32):
    """The torch module's recover_mano / recover_object / forward tail with the generator's stubs in place of the sub-modules."""
    from artiboost_amd.honet import HoNet
    from gen_honet_golden import hand_verts
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)      # noqa: E731
    hst, ost = t(g["hand_st"]).requires_grad_(True), t(g["obj_st"]).requires_grad_(True)
    m = HoNet.__new__(HoNet)
    torch.nn.Module.__init__(m)
    m.proj2d_func = __import__("artiboost_amd.hpregnet", fromlist=["x"]).batch_persp_proj2d
    m.obj_trans_factor, m.obj_scale_factor = (float(v) for v in g["factors"])
    B, (H, W) = hst.shape[0], (int(v) for v in g["image_hw"])
    m.base_net = _Stub({"res_layer4_mean": torch.zeros(B, 512, dtype=dtype)})
    m.mano_branch = _Stub({"joints_3d": t(g["joints_3d"]), "hand_verts_3d": t(hand_verts())})
    m.mano_transhead, m.obj_transhead = _Stub(hst), _Stub(ost)
    m.dummy = torch.nn.Parameter(torch.zeros(1))
    samples = {"image": torch.zeros(B, 3, H, W), "cam_intr": t(g["cam_intr"]), "obj_verts_can": t(g["obj_verts_can"]), "corners_can": t(g["corners_can"])}
    if with_corners:
        samples["corners_3d"] = torch.zeros(B, 8, 3)
    return m(samples), hst, ost


@pytest.mark.parametrize("with_corners", [True, False])
def test_cpu_module_reproduces_the_reference(golden, with_corners):
    from gen_honet_golden import probe
    tag = "" if with_corners else "nc_"
    res, hst, ost = _run_on_golden(golden, with_corners)
    assert sorted(res) == list(golden[tag + "keys"])
    assert sorted(k for k, v in res.items() if v is None) == list(golden[tag + "none_keys"])
    for k, v in res.items():
        if v is not None and k not in ("joints_3d", "hand_verts_3d"):
            ref = golden[k]
            assert tuple(v.shape) == ref.shape, k
            # fp32 rounding of values up to a few hundred (pixels) / about one (metres)
            np.testing.assert_allclose(v.detach().numpy(), ref, rtol=2e-6, atol=2e-6 * max(1.0, float(np.abs(ref).max())), err_msg=k)
    probe(res).backward()
    for name, p in (("g_hand_st", hst), ("g_obj_st", ost)):
        ref = golden[tag + name]
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=2e-5, atol=2e-6 * np.abs(ref).max(), err_msg=name)


def test_recover_3d_proj_is_the_reference_function(golden):
    from artiboost_amd.honet import HoNet
    import inspect
    sig = inspect.signature(HoNet.recover_3d_proj)
    assert list(sig.parameters) == ["objpoints3d", "camintr", "est_scale", "est_trans", "input_res", "off_z"] and sig.parameters["off_z"].default == 0.4
    assert isinstance(inspect.getattr_static(HoNet, "recover_3d_proj"), staticmethod)
    t = torch.from_numpy
    H, W = (int(v) for v in golden["image_hw"])
    tf, sf = (float(v) for v in golden["factors"])
    args = (t(golden["obj_verts_can"]), t(golden["cam_intr"]), t(golden["obj_st"][:, :1]).view(-1, 1, 1) * sf, t(golden["obj_st"][:, 1:3]).unsqueeze(1) * tf)
    rec, c = HoNet.recover_3d_proj(*args, input_res=(W, H))
    assert torch.equal(rec, t(golden["p3d_recons"])) and torch.equal(c, t(golden["p3d_center"]))
    rec, c = HoNet.recover_3d_proj(*args, input_res=(W, H), off_z=0.25)
    assert torch.equal(rec, t(golden["p3d_recons_z25"])) and torch.equal(c, t(golden["p3d_center_z25"]))


def test_state_dict_keys_are_the_reference_class_minus_the_mano_buffers(net, golden_dir):
    from artiboost_amd.hpregnet import HOPRegNet
    keys = json.load(open(os.path.join(golden_dir, "honet_keys.json")))["ResNet18"]
    ref = {k: s for k, s in keys.items() if not k.startswith(HOPRegNet.MANO_LAYER_PREFIX)}
    assert len(ref) < len(keys)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == ref


def test_hasson_checkpoint_names_load_strictly(net):
    from artiboost_amd.honet import HoNet
    sd = net.state_dict()
    hasson = {}
    for k, v in sd.items():
        k = k.replace("obj_transhead", "scaletrans_branch_obj").replace("mano_transhead.", "scaletrans_branch.")
        hasson["module." + k] = v + 1.0 if v.dtype.is_floating_point else v
    hasson["module.mano_branch.mano_layer_right.th_shapedirs"] = torch.zeros(778, 3, 10)
    hasson["module.mano_branch.mano_layer_left.th_shapedirs"] = torch.zeros(778, 3, 10)
    other = HoNet(**_cfg())
    other.load_state_dict(hasson, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k] + 1.0 if v.dtype.is_floating_point else sd[k]), k
    with pytest.raises(RuntimeError):
        other.load_state_dict(dict(hasson, **{"module.scaletrans_branch_hand.weight": torch.zeros(1)}), strict=True)


def test_registry_config_alias_and_refusals():
    import yaml
    import artiboost_amd.criterions  # noqa: F401  (registers the losses)
    from artiboost_amd import registry as R
    from artiboost_amd.honet import HoNet
    from anakin.models.honetMANO import HoNet as H2
    from anakin.models import HoNet as H3
    assert H2 is HoNet and H3 is HoNet and R.MODEL.get("HoNet") is HoNet
    cfg = yaml.safe_load(open(CFG))
    assert cfg["ARCH"]["TYPE"] == "HoNet" and cfg["ARCH"]["BACKBONE"]["TYPE"] == "ResNet18" and cfg["ARCH"]["HEAD"]["NCOMPS"] == 15
    assert [c["TYPE"] for c in cfg["CRITERION"]] == ["ManoLoss", "ObjLoss"] and cfg["MANAGER"]["MESH_QUERIES"] > 0
    model = R.build_from_cfg(cfg["ARCH"], R.MODEL, default_args=dict(DATA_PRESET=cfg["DATA_PRESET"]))
    assert type(model) is HoNet and model.obj_trans_factor == 100 and model.obj_scale_factor == 0.0001
    assert model.mano_transhead.final_layer.out_features == 3 and model.obj_transhead.final_layer.out_features == 6
    R.build_criterion_loss_list(cfg["CRITERION"], preset_cfg=cfg["DATA_PRESET"], LAMBDAS=cfg["LAMBDAS"])
    with pytest.raises(NotImplementedError, match="MANO_FHB_ADAPTOR"):
        HoNet(**_cfg(MANO_FHB_ADAPTOR=True))
    with pytest.raises(ValueError):
        HoNet.TransHead(512, 9)


def test_module_forward_runs_end_to_end_with_and_without_corners(net):
    torch.manual_seed(1)
    B, N = 2, 40
    K = torch.tensor([[400.0, 0, 32], [0, 400.0, 32], [0, 0, 1]]).repeat(B, 1, 1)
    s = {"image": torch.randn(B, 3, 64, 64) * 0.2, "cam_intr": K, "obj_verts_can": torch.randn(B, N, 3) * 0.05, "corners_can": torch.randn(B, 8, 3) * 0.05}
    net.eval()
    with torch.no_grad():
        a = net(dict(s, corners_3d=torch.zeros(B, 8, 3)))
        b = net(s)
    assert a["obj_verts_3d_abs"].shape == (B, N, 3) and a["corners_3d"].shape == (B, 8, 3) and a["mano_pca_pose"].shape == (B, 18)
    assert b["corners_3d"] is None and b["corners_3d_abs"] is None and b["corners_2d"] is None and set(a) == set(b)
    assert torch.equal(a["obj_verts_3d"], b["obj_verts_3d"]) and a["boxroot_3d_abs"] is a["obj_center"]


# ------------------------------------------------------------------------------------------------ the loader's mesh queries
def test_mesh_query_producer():
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.render import SAMPLE_DTYPE
    from artiboost_amd.synth import ArtiBoostLoader, add_mesh_queries, mesh_vertex_table
    import yaml
    cfg = yaml.safe_load(open(CFG))
    assets = SceneAssets("HO3D", seed=1)
    B, n = 5, cfg["MANAGER"]["MESH_QUERIES"]
    rng = np.random.default_rng(3)

    def rot(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)

    pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose[b, :3, :3], pose[b, :3, 3] = q * np.sign(np.linalg.det(q)), rng.normal(size=3) * 0.05 + (0, 0, 0.5)
    rm = np.stack([rot(a) for a in rng.uniform(-0.2, 0.2, B)])
    T = pose.copy()
    T[:, :3, :3], T[:, :3, 3] = rm @ pose[:, :3, :3], np.einsum("bij,bj->bi", rm, pose[:, :3, 3])
    samples = np.zeros(B, SAMPLE_DTYPE)
    samples["obj_pose"] = pose.reshape(B, 16)
    oid = torch.tensor([0, 3, 1, 1, 2])
    verts = torch.from_numpy(rng.normal(size=(B, 778, 3)).astype(np.float32) * 0.05 + np.float32([0, 0, 0.5]))
    static = {"obj_transf": torch.from_numpy(T), "root_joint": torch.from_numpy(rng.normal(size=(B, 3)).astype(np.float32) * 0.05),
              "obj_id": oid, "_samples": torch.from_numpy(samples.view(np.uint8).reshape(B, -1).copy()), "_hand_verts": verts}
    mk = lambda m: ArtiBoostLoader.from_assets(assets, m, cfg["DATA_PRESET"], B, 0, device="cpu")      # noqa: E731
    off = mk({k: v for k, v in cfg["MANAGER"].items() if k != "MESH_QUERIES"})
    items = {k: v for k, v in static.items() if not k.startswith("_")}
    before = dict(items)
    assert off.add_mesh_queries(items, static) is items and items.keys() == before.keys() and all(items[k] is before[k] for k in items)
    on = mk(cfg["MANAGER"])
    on.add_mesh_queries(items, static)
    assert set(items) - set(before) == {"obj_verts_can", "obj_verts_3d", "hand_verts_3d"} and all(items[k] is before[k] for k in before)
    assert items["obj_verts_can"].shape == (B, n, 3) == items["obj_verts_3d"].shape and items["hand_verts_3d"].shape == (B, 778, 3)
    table = mesh_vertex_table(assets, n)
    for b in range(B):      # canonical vertices of the sample's own object
        v = assets.obj_verts[assets.obj_vert_off[oid[b]]:assets.obj_vert_off[oid[b] + 1]]
        assert np.isin(table[oid[b]].view([("", np.float32)] * 3), np.ascontiguousarray(v, np.float32).view([("", np.float32)] * 3)).all()
    can, R, t, root = items["obj_verts_can"], static["obj_transf"][:, :3, :3], static["obj_transf"][:, :3, 3], static["root_joint"]
    torch.testing.assert_close(items["obj_verts_3d"] + root[:, None], torch.einsum("bij,bnj->bni", R, can) + t[:, None], rtol=0, atol=2e-7)
    torch.testing.assert_close(items["hand_verts_3d"] + root[:, None], torch.einsum("bij,bnj->bni", torch.from_numpy(rm), verts), rtol=0, atol=3e-7)
    again = add_mesh_queries(dict(before), torch.from_numpy(table), oid, verts, torch.from_numpy(pose))
    assert torch.equal(again["obj_verts_3d"], items["obj_verts_3d"])


# ------------------------------------------------------------------------------------------------ parameter layout, C ABI
def _parent_hopregnet_layout(layers):
    """Entry names, kernel shapes and offsets of the HOPRegNet trunk-only layout, computed from the construction rule alone (the parent
    commit's): the trunk's entries, ManoBranch, obj_transfhead; every tensor rounded up to 64 floats."""
    from artiboost_amd.hybridnet import ParamStore
    trunk = ParamStore(device="cpu", layers=layers, box_head=False)
    rows = [(n, e.kshape) for n, e in trunk.entries.items() if n.startswith("backbone.")]
    for name, o, i in (("mano_branch.base_layer.0", 512, 512), ("mano_branch.base_layer.2", 512, 512), ("mano_branch.pose_reg", 18, 512),
                       ("mano_branch.shape_reg.0", 10, 512), ("obj_transfhead.decoder.0", 256, 512), ("obj_transfhead.final_layer", 9, 256)):
        op = -(-o // 8) * 8
        rows += [(name + ".weight", (op, 1, 1, i)), (name + ".bias", (op,))]
    out, off = [], 0
    for n, shp in rows:
        out.append((n, tuple(shp), off))
        off += -(-int(np.prod(shp)) // 64) * 64
    return out, off


@pytest.mark.parametrize("layers", [(2, 2, 2, 2), (3, 4, 6, 3)])
def test_hopregnet_layout_is_unchanged_and_honet_layout_has_its_heads(layers):
    from artiboost_amd.hybridnet import ParamStore
    want, total = _parent_hopregnet_layout(layers)
    st = ParamStore(device="cpu", layers=layers, reg_heads=15)
    assert [(n, tuple(e.kshape), e.offset) for n, e in st.entries.items()] == want and st.total == total
    ho = ParamStore(device="cpu", layers=layers, reg_heads=15, reg_model="HoNet")
    names = list(ho.entries)
    shared = [n for n in st.entries if not n.startswith("obj_transfhead.")]
    assert names[:len(shared)] == shared and all(ho.entries[n].offset == st.entries[n].offset for n in shared)
    tail = names[len(shared):]
    assert tail == [h + s for h in ("mano_transhead.decoder.0", "mano_transhead.final_layer", "obj_transhead.decoder.0", "obj_transhead.final_layer")
                    for s in (".weight", ".bias")]
    assert ho.entries["mano_transhead.final_layer.weight"].kshape == (8, 1, 1, 256) and ho.entries["mano_transhead.final_layer.weight"].ref_shape == (3, 256)
    assert ho.entries["obj_transhead.final_layer.bias"].kshape == (8,) and ho.entries["obj_transhead.final_layer.bias"].ref_shape == (6,)
    assert all(k.startswith(("base_net.", "mano_branch.", "mano_transhead.", "obj_transhead.")) for k in ho.reference_state_dict())
    with pytest.raises(ValueError):
        ParamStore(device="cpu", layers=layers, reg_heads=15, reg_model="Other")


def test_cpu_model_state_round_trips_through_the_honet_store(net, golden_dir):
    from artiboost_amd.hybridnet import ParamStore
    st = ParamStore(device="cpu", layers=(2, 2, 2, 2), reg_heads=15, reg_model="HoNet")
    sd = net.state_dict()
    st.load_reference_state_dict(sd, strict=True)
    back = st.reference_state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(back[k], v), k
    # padding rows of the 3- and 6-wide heads are zero
    assert st.view("mano_transhead.final_layer.weight")[3:].abs().max() == 0 and st.view("obj_transhead.final_layer.bias")[6:].abs().max() == 0


def test_header_declares_the_recovery_ops_and_the_library_exports_them():
    txt = open(os.path.join(ROOT, "include", "artiboost_hip.h")).read()
    for name in ("ab_honet_recover_fwd", "ab_honet_recover_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt) and re.search(r"@check\s+%s:" % name, txt), name
    from artiboost_amd import _lib, gen_torch_ops
    lib = _lib.cdll()
    c = gen_torch_ops.contracts()
    assert any(cl.startswith("strided:") and "obj_st" in cl for cl in c["ab_honet_recover_fwd"])
    assert any("workspace" in cl for cl in c["ab_honet_recover_bwd"])
    # host-side queries: chunks of the vertex dimension and the backward's workspace
    nc = lib.ab_honet_recover_chunks
    chunk = next(n for n in range(1, 1 << 16) if nc(n + 1) == 2)
    assert nc(1) == 1 and nc(chunk) == 1 and nc(2 * chunk) == 2 and nc(2 * chunk + 1) == 3 and nc(0) == 0
    assert lib.ab_honet_recover_workspace(3, chunk + 1) == 3 * 3 * 16 * 4 and lib.ab_honet_recover_workspace(0, 5) == 0
    # the generated dispatcher source is current
    src = open(os.path.join(ROOT, "artiboost_amd", "csrc", "torch_ops_gen.cpp")).read()
    assert "honet_recover_bwd(" in src and "honet_recover_fwd(" in src
