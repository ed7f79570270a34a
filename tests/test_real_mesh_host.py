"""Mesh queries of REAL frames, host side: datasets.HO3D.get_hand_params / mesh_vertex_table / get_mesh_annots and its
second cache file, realdata.real_mesh_maps against the per-point float64 chain of HOdata.__getitem__ written out here, against the batch's
own CORNERS_3D / OBJ_TRANSF, and against tests/golden/real_mesh.npz -- the getters of the REAL reference class on the same miniature tree
(tests/gen_real_mesh_golden.py; MANO unpinned at the manotorch call) -- and the refusals of RealBatcher / MixedLoader.  No GPU."""
import glob
import os
import pickle

import numpy as np
import pytest
import torch

import ho3d_fake_tree as T
import pose_oracle as po
from artiboost_amd.realdata import HOdataSource, MixedLoader, RealBatcher, assemble_real_gt_batch, real_mesh_maps
from artiboost_amd.registry import Queries

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_mesh.npz")
PRESET = {"USE_CACHE": True, "FILTER_NO_CONTACT": False, "FILTER_THRESH": 0.0, "BBOX_EXPAND_RATIO": 1.2, "FULL_IMAGE": False,
          "IMAGE_SIZE": [224, 224], "CENTER_IDX": 0, "CROP_MODEL": "hand_obj"}
E = np.diag([1.0, -1.0, -1.0])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ho3d")
    T.build(str(root), seed=7)
    return str(root)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.fixture(scope="module")
def hand(gold):
    from artiboost_amd.assets import make_hand_model
    return make_hand_model(int(gold["hand_seed"]))


def _ds(tree, split="train", **kw):
    from artiboost_amd import datasets as D
    return D.HO3D(DATA_ROOT=tree, DATA_SPLIT=split, SPLIT_MODE="paper", AUG=split == "train", AUG_PARAM=None, DATA_PRESET=dict(PRESET), **kw)


def _meta(tree, ds, i):
    seq, frame = ds.ann["frames"][i]
    with open(os.path.join(tree, "HO3D", ds.subfolder, seq, "meta", frame + ".pkl"), "rb") as f:
        return pickle.load(f, encoding="latin1")


# ------------------------------------------------------------------------------------------------ reader
def test_hand_params_equal_the_pickles_and_test_frames_get_the_substitution(tree, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, "train")
    for i in range(len(ds)):
        a = _meta(tree, ds, i)
        pose, shape, tsl = ds.get_hand_params(i)
        assert pose.dtype == shape.dtype == tsl.dtype == np.float32 and pose.shape == (48,) and shape.shape == (10,) and tsl.shape == (3,)
        np.testing.assert_array_equal(pose, a["handPose"])
        np.testing.assert_array_equal(shape, a["handBeta"])
        np.testing.assert_array_equal(tsl, a["handTrans"])
    te = _ds(tree, "test")
    for i in range(len(te)):
        pose, shape, tsl = te.get_hand_params(i)
        assert not pose.any() and not shape.any()
        np.testing.assert_array_equal(tsl, np.asarray(_meta(tree, te, i)["handJoints3D"], np.float32))      # ho3d.py:171-175
    m = ds.get_mesh_annots(4)
    assert set(m) == {"hand_pose", "hand_shape", "hand_tsl", "table_row"}
    table, rows = ds.mesh_vertex_table(5)
    assert m["table_row"] == rows[ds.ann["obj_name"][4]] and table.shape == (len(T.OBJS), 5, 3)


def test_mano_cache_round_trips_and_the_annotation_cache_keeps_its_bytes(tree, tmp_path, monkeypatch):
    runs = {}
    for name in ("without", "with"):
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        ds = _ds(tree, "train")
        ds.get_annots(0)
        files = sorted(os.path.basename(p) for p in glob.glob(str(d / "common" / "cache" / "HO3D" / "*")))
        assert len(files) == 1 and files[0].endswith(".ab.pkl") and not files[0].endswith(".mano.ab.pkl")      # written on first use only
        if name == "with":
            first = [ds.get_mesh_annots(i) for i in range(len(ds))]
            again = _ds(tree, "train")                      # second construction: both files from the cache
            for i in range(len(ds)):
                for k in ("hand_pose", "hand_shape", "hand_tsl"):
                    np.testing.assert_array_equal(again.get_mesh_annots(i)[k], first[i][k])
            mano = str(d / "common" / "cache" / "HO3D" / files[0][:-len(".ab.pkl")]) + ".mano.ab.pkl"
            with open(mano, "rb") as f:
                blob = pickle.load(f)
            assert set(blob) == {"frames", "pose", "shape", "tsl"} and blob["pose"].shape == (len(ds), 48)
            blob["pose"][2, 7] = 123.0                      # the file IS what a later run reads ...
            with open(mano, "wb") as f:
                pickle.dump(blob, f, protocol=4)
            assert _ds(tree, "train").get_hand_params(2)[0][7] == 123.0
            blob["frames"] = blob["frames"][::-1]           # ... unless it belongs to another frame list: read again from the pickles
            with open(mano, "wb") as f:
                pickle.dump(blob, f, protocol=4)
            np.testing.assert_array_equal(_ds(tree, "train").get_hand_params(2)[0], first[2]["hand_pose"])
            assert not glob.glob(str(d / "common" / "cache" / "HO3D" / "*.tmp"))
        with open(d / "common" / "cache" / "HO3D" / files[0], "rb") as f:
            runs[name] = f.read()
    assert runs["with"] == runs["without"]


@pytest.mark.parametrize("n", [1, 157, 300])
def test_mesh_vertex_table_index_rule(tree, tmp_path, monkeypatch, n):
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, "train")
    table, rows = ds.mesh_vertex_table(n)
    assert table.dtype == np.float32 and table.shape == (3, n, 3) and sorted(rows) == sorted(T.OBJS) and sorted(rows.values()) == [0, 1, 2]
    for i in range(len(ds)):
        v = ds.get_obj_verts_can(i)[0]
        assert len(v) == 200
        idx = (np.arange(n) * 200) // n if n <= 200 else np.arange(n) % 200
        np.testing.assert_array_equal(table[ds.get_mesh_annots(i)["table_row"]], v[idx])
    if n == 300:
        np.testing.assert_array_equal(table[:, 200:], table[:, :100])


# ------------------------------------------------------------------------------------------------ maps
def _chain(p, T_base, flip, rot, root):
    """hodata.py:336-343 (flip), :364-381 (rotation with float32 entries, root subtraction), per point, float64.  T_base: 4x4 or None."""
    rm = np.array([[np.cos(rot), -np.sin(rot), 0], [np.sin(rot), np.cos(rot), 0], [0, 0, 1]]).astype(np.float32).astype(np.float64)
    out = np.zeros_like(p)
    for i, x in enumerate(p):
        if T_base is not None:
            x = T_base[:3, :3] @ x + T_base[:3, 3]
        if flip:
            x = x * np.array([-1.0, 1.0, 1.0])
        out[i] = rm @ x - root
    return out


def _apply(m, p):
    m = np.asarray(m, np.float64)
    return p @ m[:, :3].T + m[:, 3]


def _case(ds, idxs, draws, left=None, center_idx=0):
    anns = [dict(ds.get_annots(i)) for i in idxs]
    if left is not None:
        anns[left]["side"] = "left"
    r = assemble_real_gt_batch(anns, [224, 224], ds.raw_size, draws, center_idx, 1.2, 0.1, 0.1, ds.sides)
    ma = [ds.get_mesh_annots(i) for i in idxs]
    return anns, ma, r, real_mesh_maps(anns, ma, r, center_idx)


@pytest.mark.parametrize("mode", ["plain", "aug", "aug_left"])
def test_maps_against_the_per_point_chain(tree, hand, tmp_path, monkeypatch, mode):
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, "train")
    idxs = list(range(len(ds)))
    draws = None if mode == "plain" else RealBatcher(ds, PRESET, aug=True, device="cpu", seed=5).draw(len(idxs))
    left = 3 if mode == "aug_left" else None
    anns, ma, r, (obj_map, hand_map) = _case(ds, idxs, draws, left, center_idx=9)
    assert obj_map.shape == hand_map.shape == (len(idxs), 3, 4) and obj_map.dtype == hand_map.dtype == np.float32
    assert list(r["flip"]) == [s == left for s in range(len(idxs))]
    table, _ = ds.mesh_vertex_table(157)
    worst = 0.0
    for s, i in enumerate(idxs):
        rot = 0.0 if draws is None else draws["rot"][s]
        root = np.asarray(r[Queries.ROOT_JOINT][s], np.float64)
        can = table[ma[s]["table_row"]].astype(np.float64)
        want = _chain(can, np.asarray(anns[s]["obj_transf"], np.float64), bool(r["flip"][s]), rot, root)
        e_obj = np.abs(_apply(obj_map[s], can) - want).max()
        v = po.mano_lbs(hand, ma[s]["hand_pose"][None].astype(np.float64), ma[s]["hand_shape"][None].astype(np.float64))[0][0]
        want_h = _chain((v + ma[s]["hand_tsl"].astype(np.float64)) @ E.T, None, bool(r["flip"][s]), rot, root)
        e_hand = np.abs(_apply(hand_map[s], v) - want_h).max()
        worst = max(worst, e_obj, e_hand)
        assert e_obj <= 5e-7 and e_hand <= 5e-7, (mode, s, e_obj, e_hand)
        # the map applied to CORNERS_CAN reproduces the batch's CORNERS_3D, the flipped sample included
        got_c = _apply(obj_map[s], np.asarray(anns[s]["corners_can"], np.float64))
        assert np.abs(got_c - r[Queries.CORNERS_3D][s]).max() <= 2e-6
        if not r["flip"][s]:      # the synthetic half's formula on the batch's own OBJ_TRANSF (the reference leaves OBJ_TRANSF unflipped)
            Tb = np.asarray(r[Queries.OBJ_TRANSF][s], np.float64)
            assert np.abs(_apply(obj_map[s], can) - (can @ Tb[:3, :3].T + Tb[:3, 3] - root)).max() <= 2e-6
        else:
            Tb = np.asarray(r[Queries.OBJ_TRANSF][s], np.float64)
            assert np.abs(_apply(obj_map[s], can) - (can @ Tb[:3, :3].T + Tb[:3, 3] - root)).max() > 1e-3
    print(f"real_mesh_maps {mode}: max |map - chain| = {worst:.3e} m")


@pytest.mark.parametrize("split", ["train", "test"])
def test_maps_against_the_reference_getters_without_augmentation(tree, hand, gold, tmp_path, monkeypatch, split):
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, split)
    idxs = list(range(len(ds)))
    assert len(ds) == int(gold[f"{split}.n"])
    anns, ma, r, (obj_map, hand_map) = _case(ds, idxs, None)
    table, _ = ds.mesh_vertex_table(157)
    sel = (np.arange(157) * 200) // 157
    for s in idxs:
        pre = f"{split}.{s}."
        root = np.asarray(r[Queries.ROOT_JOINT][s], np.float64)
        np.testing.assert_allclose(root, gold[pre + "joints_3d"][0], atol=3e-6, rtol=0)
        can = ds.get_obj_verts_can(s)[0]
        np.testing.assert_allclose(can, gold[pre + "obj_verts_can"], atol=1e-7, rtol=0)
        got = _apply(obj_map[s], can.astype(np.float64)) + root
        assert np.abs(got - gold[pre + "obj_verts_transf"]).max() <= 3e-6
        got_n = _apply(obj_map[s], table[ma[s]["table_row"]].astype(np.float64)) + root
        assert np.abs(got_n - gold[pre + "obj_verts_transf"][sel]).max() <= 3e-6
        v = po.mano_lbs(hand, ma[s]["hand_pose"][None].astype(np.float64), ma[s]["hand_shape"][None].astype(np.float64))[0][0]
        assert np.abs(_apply(hand_map[s], v) + root - gold[pre + "hand_verts_3d"]).max() <= 3e-6


# ------------------------------------------------------------------------------------------------ RealBatcher / MixedLoader
def test_assemble_adds_the_mesh_arrays_only_when_asked(tree, hand, tmp_path, monkeypatch):
    from artiboost_amd.synth import ManoLayerHIP
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, "train")
    mano = ManoLayerHIP(hand, device="cpu")
    on = RealBatcher(ds, PRESET, aug=True, device="cpu", seed=3, mesh_queries=157, mano=mano)
    off = RealBatcher(ds, PRESET, aug=True, device="cpu", seed=3)
    assert off.mesh_queries == 0 and off.mano is None
    draws = on.draw(4)
    a, b = on.assemble([5, 0, 7, 2], draws), off.assemble([5, 0, 7, 2], draws)
    assert "mesh" not in b and set(a) - set(b) == {"mesh"}
    for k in b["gt"]:
        np.testing.assert_array_equal(a["gt"][k], b["gt"][k])
    m = a["mesh"]
    assert m["pose"].shape == (4, 48) and m["shape"].shape == (4, 10) and m["obj_map"].shape == m["hand_map"].shape == (4, 3, 4)
    assert m["row"].dtype == np.int64 and list(m["row"]) == [ds.get_mesh_annots(i)["table_row"] for i in (5, 0, 7, 2)]
    np.testing.assert_array_equal(m["pose"][1], ds.get_hand_params(0)[0])


def test_refusals(tree, hand, tmp_path, monkeypatch):
    from artiboost_amd.synth import ManoLayerHIP
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree, "train")
    mano = ManoLayerHIP(hand, device="cpu")
    with pytest.raises(ValueError, match="mano"):
        RealBatcher(ds, PRESET, device="cpu", mesh_queries=157)

    class Bare(HOdataSource):
        def __len__(self):
            return 4

    with pytest.raises(ValueError, match="Bare"):
        RealBatcher(Bare(), PRESET, device="cpu", mesh_queries=157, mano=mano)
    with pytest.raises(NotImplementedError, match="Bare"):
        Bare().get_mesh_annots(0)
    RealBatcher(Bare(), PRESET, device="cpu")                 # without the argument nothing is asked of the source

    class Synth:                                              # what MixedLoader.update() reads of an ArtiBoostLoader
        use_synth, epoch, synth_len, image_plane = True, {}, 9, "f32"

        def __init__(self, mesh_queries):
            self.mesh_queries, self.batch_size = mesh_queries, MixedLoader.n_synth_for(4, 9, 9)

    real = RealBatcher(ds, PRESET, device="cpu", compute_dtype=torch.float32, mesh_queries=157, mano=mano)
    assert MixedLoader(real, Synth(157), 4).n_synth == 2
    for other in (0, 300):
        with pytest.raises(ValueError, match=f"157.*{other}"):
            MixedLoader(real, Synth(other), 4)
    assert MixedLoader(RealBatcher(ds, PRESET, device="cpu", compute_dtype=torch.float32), Synth(300), 4).n_synth == 2      # as before
