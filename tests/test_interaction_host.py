"""Hand-object interaction measures on the host: the float64 torch route (`metrics.interaction_values_torch`) against
analytic values -- boxes, flipped faces, lattice volumes, an icosphere, one open triangle, degenerate inputs, rigid invariance --,
`ObjectMeshTable` from the stand-in assets and from a dataset reader, `InteractionMetric` on CPU tensors through the evaluator, and the
header contract with its generated op.  The meshes and helpers are shared with tests/test_gpu_interaction.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
H = 0.005
BOX_FACES = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)


def box_mesh(lo, hi, flip=False):
    """8 vertices (x fastest) and 12 outward faces of the axis-aligned box [lo, hi]; flip: every face reversed."""
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    v = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in (0, 1) for j in (0, 1) for i in (0, 1)], F64)
    return v, (BOX_FACES[:, [0, 2, 1]] if flip else BOX_FACES).copy()


def icosphere(r, level):
    """Icosahedron subdivided `level` times (20 x 4^level faces), vertices on the sphere of radius r, outward faces."""
    from artiboost_amd.assets import _subdivide
    t = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], F64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                  [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(level):
        v, f = _subdivide(v, f)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    return r * v, f.astype(np.int32)


def rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def table_of(meshes, hand=None, ids=None):
    """ObjectMeshTable of [(verts, faces)], class ids 1.. unless given; hand: (rest verts, faces) of the "hand" mesh."""
    from artiboost_amd.metrics import ObjectMeshTable
    hm = None if hand is None else {"v_template": np.asarray(hand[0], np.float32), "faces": np.asarray(hand[1], np.int32)}
    return ObjectMeshTable(meshes, ids or list(range(1, len(meshes) + 1)), hm)


ONE_TRI = (np.array([[0.03, 0, 0], [0, 0.03, 0], [0, 0, 0.03]], F64), np.array([[0, 1, 2]], np.int32))
TINY_HAND = box_mesh([-1, -1, -1], [1, 1, 1])


def run_route(table, hand, rows, rot, tsl, dtype=torch.float64, device="cpu", kernel=False, hand_faces=None, hand_orient=None, **kw):
    """One call of the torch route (or of the kernel) on numpy inputs -> dict of numpy arrays.  hand_faces / hand_orient: instead of the table's."""
    from artiboost_amd import kernels as K
    from artiboost_amd.metrics import interaction_values_torch
    tb = table.on(device)
    t = lambda a, d=dtype: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=d).contiguous()      # noqa: E731
    B = len(hand)
    fn = K.interaction if kernel else interaction_values_torch
    hf = tb["hand_faces"] if hand_faces is None else t(np.asarray(hand_faces).reshape(-1, 3), torch.int32)
    o = fn(t(hand), hf, table.hand_orient if hand_orient is None else hand_orient, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"],
           tb["obj_orient"], t(rows, torch.int64), t(np.asarray(rot).reshape(B, 3, 3)), t(np.asarray(tsl).reshape(B, 3)), **kw)
    lat = o.pop("lattice", None)
    out = {k: v.cpu().numpy() for k, v in o.items()}
    if lat is not None:
        out["lattice"] = [None if x is None else tuple(y.cpu().numpy() for y in x) for x in lat]
    return out


def box_sdf(q, lo, hi):
    c, half = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
    e = np.abs(q - c) - half
    outside = np.linalg.norm(np.maximum(e, 0), axis=1)
    return np.where((e < 0).all(1), e.max(1), outside)


LO, HI = np.float32([-0.03, -0.02, -0.05]).astype(F64), np.float32([0.03, 0.02, 0.05]).astype(F64)      # the table holds fp32 coordinates
QUERIES = np.array([[0, 0, 0], [0.02, 0.01, 0.04], [-0.029, 0, 0], [0.01, -0.019, -0.049],                       # inside
                    [0.04, 0, 0], [0, 0.03, 0.01], [0.05, 0.04, 0], [-0.04, 0, 0.07], [0.05, 0.03, 0.08], [-0.031, -0.021, -0.051], [0.0, 0.0, 0.2]], F64)
I3, Z3 = np.eye(3)[None], np.zeros((1, 3))


# ------------------------------------------------------------------------------------------------ 1. analytic values of the float64 route
@pytest.mark.parametrize("flip", [False, True])
def test_box_winding_number_and_signed_distance_are_analytic(flip):
    tb = table_of([box_mesh(LO, HI, flip)], TINY_HAND)
    assert tb.orient.tolist() == [-1.0 if flip else 1.0]
    got = run_route(tb, QUERIES[None], [0], I3, Z3, flags=1, want_sdf=True)
    want = box_sdf(QUERIES, LO, HI)
    inside = want < 0
    print("wind", got["wind"][0], "sdf error", np.abs(got["sdf"][0] - want).max())
    assert np.abs(got["wind"][0] - inside).max() <= 1e-12
    assert np.abs(got["sdf"][0] - want).max() <= 1e-15
    r = got["rows"][0]
    assert got["counts"][0].tolist() == [4, 0, 0, 0] and abs(r[0] + want[:4].min()) <= 1e-15 and abs(r[1] + want[:4].mean()) <= 1e-15
    assert abs(r[0] - 0.02) < 1e-8 and abs(r[2] - np.abs(want).min()) <= 1e-15 and r[3] == 4 / len(QUERIES) and r[4] == 1.0 and np.isnan(r[5:]).all()


def _lattice_box(n_lo, n_hi, h=H):
    """Faces at h (n + 3/4): an odd multiple of h / 4 away from the lattice planes h (i + 1/2)."""
    return h * (np.asarray(n_lo, F64) + 0.75), h * (np.asarray(n_hi, F64) + 0.75)


def test_overlapping_boxes_give_the_exact_lattice_volume():
    hand_lo, hand_hi = _lattice_box([-4, -3, 96], [6, 5, 104])
    obj_lo, obj_hi = _lattice_box([1, -8, 99], [12, 2, 110])
    t = np.array([[0.01, -0.02, 0.5]])
    tb = table_of([box_mesh(obj_lo - t[0], obj_hi - t[0])], box_mesh(hand_lo, hand_hi))
    got = run_route(tb, box_mesh(hand_lo, hand_hi)[0][None], [0], I3, t)
    n = (6 - 1) * (2 - -3) * (104 - 99)
    assert got["counts"][0].tolist()[1:] == [n, n, 0], got["counts"]
    overlap = np.minimum(hand_hi, obj_hi) - np.maximum(hand_lo, obj_lo)
    assert abs(got["rows"][0, 5] - overlap.prod()) <= 1e-12 * overlap.prod() and got["rows"][0, 5] == n * H ** 3
    # a flipped hand mesh with its orientation, a quarter-turn pose of the object, half the voxel (the boxes on ITS lattice): the same rule
    hand_lo, hand_hi = _lattice_box([-8, -6, 192], [12, 10, 208], H / 2)
    obj_lo, obj_hi = _lattice_box([2, -16, 198], [24, 4, 220], H / 2)
    R = np.array([[[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]])
    can = (box_mesh(obj_lo - t[0], obj_hi - t[0])[0]) @ R[0]                          # R can + t is the same box
    tb2 = table_of([(can, BOX_FACES)], box_mesh(hand_lo, hand_hi, flip=True))
    assert tb2.hand_orient == -1.0
    got2 = run_route(tb2, box_mesh(hand_lo, hand_hi)[0][None], [0], R, t, voxel=H / 2)
    n2 = (12 - 2) * (4 - -6) * (208 - 198)
    assert got2["counts"][0].tolist()[1:] == [n2, n2, 0] and got2["rows"][0, 5] == n2 * (H / 2) ** 3


def test_disjoint_boxes_have_no_lattice_and_contact_follows_the_threshold():
    hand = box_mesh([0.1, 0, 0.5], [0.12, 0.02, 0.52])
    tb = table_of([box_mesh(LO, HI)], hand)
    for gap, contact in ((0.02, 0.0), (0.004, 1.0)):
        t = np.array([[0.1 - gap - 0.03, 0.01, 0.51]])                                 # the object's +x face `gap` short of the hand's -x face
        got = run_route(tb, hand[0][None], [0], I3, t)
        assert got["counts"][0].tolist() == [0, 0, 0, 0] and got["rows"][0, 5] == 0.0
        assert abs(got["rows"][0, 2] - (0.1 - (t[0, 0] + HI[0]))) <= 1e-15 and abs(got["rows"][0, 2] - gap) < 1e-8 and got["rows"][0, 4] == contact and got["rows"][0, 0] == 0.0 and got["rows"][0, 1] == 0.0


def test_a_lattice_past_max_voxels_is_capped_and_leaves_the_vertex_quantities():
    hand_lo, hand_hi = _lattice_box([-4, -3, 96], [6, 5, 104])
    t = np.array([[0.0, 0.0, 0.5]])
    tb = table_of([box_mesh(LO, HI)], box_mesh(hand_lo, hand_hi))
    hv = box_mesh(hand_lo, hand_hi)[0][None]
    full, cap = run_route(tb, hv, [0], I3, t), run_route(tb, hv, [0], I3, t, max_voxels=50)
    assert full["counts"][0, 3] == 0 and full["counts"][0, 1] > 50 and full["counts"][0, 2] > 0
    assert cap["counts"][0].tolist() == [full["counts"][0, 0], full["counts"][0, 1], 0, 1] and np.isnan(cap["rows"][0, 5])
    assert np.array_equal(cap["rows"][0, :5], full["rows"][0, :5])


def test_depth_below_an_icosphere_is_within_the_facet_sagitta():
    r, delta = 0.05, 0.008
    v, f = icosphere(r, 3)
    assert len(f) == 1280
    sag = r - np.abs(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])) /
                     np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)).min()
    d = np.random.default_rng(3).standard_normal((40, 3))
    q = (r - delta) * d / np.linalg.norm(d, axis=1, keepdims=True)
    R, t = rotation(5)[None], np.array([[0.02, -0.01, 0.5]])
    got = run_route(table_of([(v, f)], TINY_HAND), (q @ R[0].T + t)[None], [0], R, t, flags=1, want_sdf=True)
    print(f"sagitta {sag:.3e}  pen_max {got['rows'][0, 0]:.6f}  depths in [{-got['sdf'].max():.6f}, {-got['sdf'].min():.6f}]")
    assert 0 < sag < 3e-4 and got["counts"][0, 0] == 40 and got["rows"][0, 3] == 1.0
    assert delta - sag - 1e-12 <= got["rows"][0, 0] <= delta + 1e-12 and (got["sdf"] < 0).all() and (-got["sdf"] >= delta - sag - 1e-12).all()
    assert np.abs(got["wind"] - 1.0).max() <= 1e-12


def test_posing_hand_and_object_by_one_rigid_map_changes_nothing():
    v, f = icosphere(0.04, 1)
    tb = table_of([(v, f), box_mesh(LO, HI)], TINY_HAND)
    rng = np.random.default_rng(8)
    hand = rng.uniform(-0.06, 0.06, (2, 65, 3))
    R, t = np.stack([rotation(1), rotation(2)]), rng.uniform(-0.02, 0.02, (2, 3))
    a = run_route(tb, hand, [1, 0], R, t, flags=1, want_sdf=True)
    G, g = rotation(9), np.array([0.03, -0.02, 0.5])
    b = run_route(tb, hand @ G.T + g, [1, 0], G @ R, t @ G.T + g, flags=1, want_sdf=True)
    for k in ("sdf", "wind"):
        assert np.abs(a[k] - b[k]).max() <= 1e-12, k
    assert np.abs(a["rows"][:, :5] - b["rows"][:, :5]).max() <= 1e-12 and np.array_equal(a["counts"], b["counts"]) and 0 < a["counts"][:, 0].min()


def test_one_open_triangle_gives_its_solid_angle_fraction():
    tb = table_of([ONE_TRI], TINY_HAND)
    q = np.array([[0, 0, 0], [0.01, 0.01, 0.01], [1.0, 1.0, 1.0]], F64)               # the corner of the octant; on the plane; far behind
    got = run_route(tb, q[None], [0], I3, Z3, flags=1, want_sdf=True)
    assert tb.orient[0] == 1.0 and abs(got["wind"][0, 0] - 1 / 8) <= 1e-15 and abs(abs(got["wind"][0, 1]) - 0.5) <= 1e-6      # 0.03 as fp32: a nanometre off the plane
    assert abs(got["sdf"][0, 0] - float(np.float32(0.03)) / math.sqrt(3)) <= 1e-15 and abs(got["sdf"][0, 1]) <= 1e-8 and got["counts"][0, 0] == 0
    # far away the triangle is seen as area x cos / r^2
    n = np.ones(3) / math.sqrt(3)
    want = -(math.sqrt(3) / 2 * (0.03 * math.sqrt(2)) ** 2 / 2) * 1 / np.linalg.norm(q[2] - 0.01) ** 2 / (4 * math.pi)
    assert abs(got["wind"][0, 2] - want) <= 2e-3 * abs(want) and n @ (q[2] - 0.01) > 0


def test_repeated_index_faces_are_dropped_and_degenerate_inputs_stay_finite():
    from artiboost_amd.metrics import drop_repeated_faces
    v, f = box_mesh(LO, HI)
    padded = np.concatenate([f, [[0, 0, 1], [2, 3, 3], [5, 4, 5]], f[:2]])                # three repeats and two coincident triangles
    assert np.array_equal(drop_repeated_faces(padded), np.concatenate([f, f[:2]]))
    tb = table_of([(v, padded)], (TINY_HAND[0], np.concatenate([TINY_HAND[1], [[7, 7, 7]]])))
    assert tb.face_off.tolist() == [0, 14] and len(tb.hand_faces) == 12
    q = np.concatenate([v[:3], [[0, 0, 0], (v[0] + v[1]) / 2]])                            # on vertices, inside, on an edge
    got = run_route(tb, q[None], [0], I3, Z3, flags=1, want_sdf=True)
    assert all(np.isfinite(got[k]).all() for k in ("sdf", "wind")) and np.isfinite(got["rows"][0, :5]).all()
    assert np.abs(got["sdf"][0, [0, 1, 2, 4]]).max() <= 1e-15 and abs(got["sdf"][0, 3] + HI[1]) <= 1e-15
    with pytest.raises(ValueError):
        table_of([(v, [[0, 0, 1]])])


# ------------------------------------------------------------------------------------------------ 2. ObjectMeshTable
_ASSETS = {}


def stand_in_assets(name="HO3D"):
    from artiboost_amd.assets import SceneAssets
    if name not in _ASSETS:
        _ASSETS[name] = SceneAssets(name, seed=1)
    return _ASSETS[name]


def test_object_mesh_table_from_the_stand_in_assets():
    from artiboost_amd.metrics import ObjectMeshTable, mesh_orientation
    a = stand_in_assets()
    tb = ObjectMeshTable.from_assets(a)
    assert tb.row_of == {9: 0, 12: 1, 5: 2, 11: 3} and tb.orient.tolist() == [-1.0] * 4 and tb.n_obj == 4      # "outward" in assets.make_object's comment; the signed volumes are negative
    assert np.array_equal(tb.vert_off, a.obj_vert_off) and np.array_equal(tb.face_off, a.obj_face_off) and tb.face_off[1] == 3968
    assert np.array_equal(tb.verts, a.obj_verts) and np.array_equal(tb.faces, a.obj_faces)
    assert np.array_equal(tb.rows(torch.tensor([11, 9, 5, 12, 7, 400])).numpy(), [3, 0, 2, 1, -1, -1])
    assert len(tb.hand_faces) <= 1538 and tb.hand_faces.max() < 778 and tb.hand_orient == mesh_orientation(a.hand["v_template"], tb.hand_faces)
    w = run_route(tb, np.zeros((1, 1, 3)), [0], I3, Z3, flags=1, want_sdf=True)["wind"]
    assert abs(w[0, 0] - 1.0) < 2e-3                                                   # tubes with small end holes: not watertight


def test_object_mesh_table_from_a_dataset_reader(tmp_path):
    import ho3d_fake_tree as T
    from artiboost_amd import datasets as D
    from artiboost_amd.metrics import ObjectMeshTable, drop_repeated_faces
    T.build(str(tmp_path), seed=7)
    ds = D.HO3D(DATA_ROOT=str(tmp_path), DATA_SPLIT="train", SPLIT_MODE="paper", AUG=False, AUG_PARAM=None,
                DATA_PRESET={"USE_CACHE": False, "FILTER_NO_CONTACT": False, "FILTER_THRESH": 0.0, "BBOX_EXPAND_RATIO": 1.2, "FULL_IMAGE": False,
                             "IMAGE_SIZE": [224, 224], "CENTER_IDX": 0, "CROP_MODEL": "root_obj"})
    tb = ObjectMeshTable.from_dataset(ds, {"v_template": TINY_HAND[0], "faces": TINY_HAND[1]})
    assert tb.obj_ids == [ds.name2id[o] for o in sorted(T.OBJS)] and tb.vert_off.tolist() == [0, 200, 400, 600]
    for r, o in enumerate(sorted(T.OBJS)):
        idx = next(i for i in range(len(ds)) if ds.ann["obj_name"][ds.sample_idxs[i]] == o)
        assert np.array_equal(tb.verts[200 * r:200 * (r + 1)], ds.get_obj_verts_can(idx)[0])
        assert np.array_equal(tb.faces[tb.face_off[r]:tb.face_off[r + 1]], drop_repeated_faces(ds.get_obj_faces(idx)))
        c = ds.get_annots(idx)["corners_can"]
        assert np.abs(tb.verts[200 * r:200 * (r + 1)].min(0) - c.min(0)).max() < 1e-6       # the canonical frame of corners_can
    assert set(tb.orient.tolist()) <= {-1.0, 1.0}


# ------------------------------------------------------------------------------------------------ 3. the metric class through the evaluator
def metric_batch(B, seed, dtype=torch.float64):
    """(table, preds, targs): a "hand" box poked into an icosphere / a box at half a metre; the annotation is another pose of the same pair."""
    rng = np.random.default_rng(seed)
    hand_lo, hand_hi = np.array([-0.02, -0.015, -0.01]), np.array([0.02, 0.015, 0.01])
    hv0, hf = box_mesh(hand_lo, hand_hi)
    hv0 = np.concatenate([hv0, rng.uniform(hand_lo, hand_hi, (40, 3))])                  # 48 "hand" vertices; the extra ones belong to no face
    tb = table_of([icosphere(0.04, 2), box_mesh(LO, HI)], (hv0, hf), ids=[5, 9])
    out = []
    for _ in range(2):
        R = np.stack([rotation(int(s)) for s in rng.integers(0, 1000, B)])
        t = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.02, 0.02, (B, 3))
        Rh = np.stack([rotation(int(s)) for s in rng.integers(0, 1000, B)])
        off = rng.uniform(-1, 1, (B, 3))
        off = off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(0.02, 0.075, (B, 1))
        hand = np.einsum("bij,nj->bni", Rh, hv0) + (t + off)[:, None]
        out.append((hand, R, t))
    (hand, R, t), (ghand, gR, gt) = out
    ids = rng.choice([5, 9], B)
    root = ghand[:, 0]
    T = np.tile(np.eye(4), (B, 1, 1)); T[:, :3, :3], T[:, :3, 3] = gR, gt
    tt = lambda a: torch.as_tensor(a).to(dtype)      # noqa: E731
    preds = {"hand_verts_3d_abs": tt(hand), "box_rot_rotmat": tt(R), "boxroot_3d_abs": tt(t).reshape(B, 1, 3)}
    targs = {"hand_verts_3d": tt(ghand - root[:, None]), "root_joint": tt(root), "obj_transf": tt(T), "obj_idx": torch.as_tensor(ids)}
    return tb, preds, targs


def expected_interaction(tb, batches, prefix=""):
    """The float64 measures over all samples, by run_route on the groups' inputs."""
    per = []
    for preds, targs in batches:
        if prefix:
            hand, T = (targs["hand_verts_3d"] + targs["root_joint"][:, None]).double().numpy(), targs["obj_transf"].double().numpy()
            R, t = T[:, :3, :3], T[:, :3, 3]
        else:
            hand, R, t = (preds[k].double().numpy() for k in ("hand_verts_3d_abs", "box_rot_rotmat", "boxroot_3d_abs"))
        per.append(run_route(tb, hand, tb.rows(targs["obj_idx"]).numpy(), R, t))
    rows, cnt = np.concatenate([p["rows"] for p in per]), np.concatenate([p["counts"] for p in per])
    ok = cnt[:, 3] == 0
    return {prefix + "pen_depth_mm": 1e3 * rows[:, 0].mean(), prefix + "pen_mean_mm": 1e3 * rows[:, 1].mean(), prefix + "min_dist_mm": 1e3 * rows[:, 2].mean(),
            prefix + "inside_frac": rows[:, 3].mean(), prefix + "contact_ratio": rows[:, 4].mean(), prefix + "inter_vol_cm3": 1e6 * rows[ok, 5].mean(),
            prefix + "capped": int((~ok).sum())}


def build_interaction(tb, **cfg):
    from artiboost_amd import registry as R
    return R.build_evaluator_metric_list([dict({"TYPE": "InteractionMetric"}, **cfg)], {"CENTER_IDX": 0})[0].set_obj_meshes(tb)


def test_interaction_metric_on_cpu_tensors_through_the_evaluator(caplog):
    import logging
    from anakin.metrics.interaction import InteractionMetric as Alias
    from artiboost_amd.metrics import Evaluator, InteractionMetric
    tb, p1, t1 = metric_batch(3, 11)
    _, p2, t2 = metric_batch(5, 12)
    m = build_interaction(tb, REPORT_GT=True)
    assert type(m) is InteractionMetric is Alias and (m.contact_thr, m.voxel, m.max_voxels, m.volume) == (0.005, 0.005, 262144, True)
    ev = Evaluator({}, [m])
    ev.feed_all(p1, t1)
    ev.feed_all(p2, t2)
    got = ev.get_measures_all()
    want = dict(expected_interaction(tb, [(p1, t1), (p2, t2)]), **expected_interaction(tb, [(p1, t1), (p2, t2)], "gt_"))
    print(got)
    assert set(got) == set(want) and got["capped"] == 0 and got["pen_depth_mm"] > 1.0 and 0 < got["contact_ratio"] < 1 and got["inter_vol_cm3"] > 0
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-9, (k, got[k], v)
    assert "pen_depth_mm:" in str(ev) and "gt_inter_vol_cm3:" in str(ev)
    # a batch without the prediction's rotation: its group is skipped and logged once; the annotation's group still counts
    bare = {k: v for k, v in p1.items() if k != "box_rot_rotmat"}
    with caplog.at_level(logging.WARNING, logger="anakin"):
        ev.feed_all(bare, t1)
        ev.feed_all(bare, t1)
    assert len([r for r in caplog.records if "box_rot_rotmat" in r.getMessage()]) == 1
    again = ev.get_measures_all()
    assert again["pen_depth_mm"] == got["pen_depth_mm"] and m.sums[""][8] == 8 and m.sums["gt_"][8] == 14
    ev.reset_all()
    assert ev.get_measures_all() == {} and m.sums == {}
    # VOLUME false: no volume measures; a small MAX_VOXELS: capped samples are counted and left out of the volume's mean
    assert set(Evaluator({}, [build_interaction(tb, VOLUME=False)]).get_measures_all()) == set()
    nv = build_interaction(tb, VOLUME=False)
    nv.feed(p1, t1)
    assert set(nv.get_measures()) == {"pen_depth_mm", "pen_mean_mm", "min_dist_mm", "inside_frac", "contact_ratio"}
    cap = build_interaction(tb, MAX_VOXELS=30)
    cap.feed(p2, t2)
    ref = run_route(tb, p2["hand_verts_3d_abs"].numpy(), tb.rows(t2["obj_idx"]).numpy(), p2["box_rot_rotmat"].numpy(), p2["boxroot_3d_abs"].numpy(), max_voxels=30)
    assert cap.get_measures()["capped"] == int(ref["counts"][:, 3].sum()) > 0
    with pytest.raises(RuntimeError, match="no object meshes"):
        from artiboost_amd import registry as R
        R.build_evaluator_metric_list([{"TYPE": "InteractionMetric"}], {})[0].feed(p1, t1)


def test_the_yaml_is_the_mesh_metrics_file_plus_one_entry():
    import yaml
    from artiboost_amd import registry as R
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_mi355x.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_meshmetrics_mi355x.yaml")))
    assert cfg["EVALUATOR"][:-1] == base["EVALUATOR"] and {k: v for k, v in cfg.items() if k != "EVALUATOR"} == {k: v for k, v in base.items() if k != "EVALUATOR"}
    m = R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"])[-1]
    assert type(m).__name__ == "InteractionMetric" and m.table.row_of == {9: 0, 12: 1, 5: 2, 11: 3} and not m.report_gt


# ------------------------------------------------------------------------------------------------ 4. header contract, generated op
def test_header_contract_and_generated_op():
    from artiboost_amd import _lib as L
    from artiboost_amd import gen_torch_ops, kernels
    txt = open(gen_torch_ops.HEADER).read()
    assert re.search(r"@check\s+ab_interaction:", txt) and re.search(r"\bint\s+ab_interaction\s*\(", txt) and re.search(r"\blong\s+ab_interaction_workspace\s*\(", txt)
    assert {"ab_interaction", "ab_interaction_workspace"} <= set(L.declared_symbols())
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    cons = gen_torch_ops.contracts()["ab_interaction"]
    assert any("ab_interaction_workspace(B,Nh,max_voxels)" in c for c in cons)
    assert [p for p in decl["ab_interaction"] if p[1] in ("obj_row", "hand_orient", "counts", "stream")] == [("float", "hand_orient"), ("const int64_t*", "obj_row"),
                                                                                                            ("int32_t*", "counts"), ("void*", "stream")]
    src = open(gen_torch_ops.OUT).read()
    assert 'm.def("interaction(' in src and 'm.impl("interaction", &w_interaction);' in src and "w_interaction_workspace" in src
    _, schema, body = gen_torch_ops.schema_and_wrapper("int", "ab_interaction", decl["ab_interaction"], cons)
    assert body in src and f'm.def("{schema}");' in src                         # the committed source is what the generator writes
    for name, col in kernels.IA_ROW.items():
        macro = {"volume": "AB_IA_VOL"}.get(name, "AB_IA_" + name.upper())
        assert re.search(rf"#define {macro} {col}\b", txt), name
    assert (kernels.IA_VERTS, kernels.IA_VOLUME) == (1, 2) and re.search(r"#define AB_IA_ROW 8\b", txt)
    block = txt[txt.index("Hand-object interaction measures"):txt.index("long ab_interaction_workspace")]
    assert re.search(r"not captured in a hipGraph", block) and "o w(q) > 0.5" in block
    hip = open(os.path.join(ROOT, "artiboost_amd", "csrc", "interact.hip")).read()
    assert "never captured in a hipGraph" in hip and "atomic" not in hip.replace("No atomics", "")
