"""ab_interaction (csrc/interact.hip) on the device against `metrics.interaction_values_torch` in float64 on the same
inputs (run on the device's float64 units: the stand-in meshes would take minutes on the host): every shape at which the kernel takes
another path, its flags and optional outputs, determinism and independence of the batch around a sample, `InteractionMetric` on HIP tensors,
the dispatcher op's refusals, and one HoNet forward fed through an evaluator that holds the metric.  Nothing here captures a graph.

Bounds (none is a recorded figure; every figure is printed before it is asserted):
  |sdf|, pen_max, pen_mean, min_dist   the larger of 4 x the error of the fp32 torch-CPU route against float64 on that case and
                                       16 x 2^-24 x max |coordinate| of the case (the rule of section 23).
  wind                                 the larger of 4 x the fp32 torch-CPU route's error and sqrt(F) x 2^-24, F the faces of the sample's object.
  inside flags, n_inside, n_both,      equal to float64's; a hand vertex or lattice point is left out only when its float64 o w lies within
  contact                              1e-3 of 0.5 for the mesh in question (for `contact` also a min_dist within the distance bound of the
                                       threshold); at most 1 % of a case's queries / lattice points may be left out, asserted on the float64
                                       side.  n_both is a count, so the rule reads |device - float64| <= the number of such lattice points.
  n_lattice                            n_both <= n_lattice <= MAX_VOXELS only: the box may differ from float64's by a boundary layer, whose
                                       points lie on the face of one mesh's box and are inside at most one mesh."""
import os

import numpy as np
import pytest
import torch

from test_interaction_host import (BOX_FACES, F64, H, LO, HI, ONE_TRI, box_mesh, build_interaction, icosphere, metric_batch, rotation, run_route,
                                   stand_in_assets, table_of)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
_CACHE = {}


def small_table():
    """{1 triangle, box, icosphere of 20, 80 and 1 280 faces}: irregular vertex and face offsets."""
    if "small" not in _CACHE:
        _CACHE["small"] = table_of([ONE_TRI, box_mesh(LO, HI), icosphere(0.035, 0), icosphere(0.04, 1), icosphere(0.045, 3)], box_mesh(LO / 2, HI / 2))
        assert _CACHE["small"].face_off.tolist() == [0, 1, 13, 33, 113, 1393] and _CACHE["small"].vert_off.tolist() == [0, 3, 11, 23, 65, 707]
    return _CACHE["small"]


def small_case(B, Nh, seed, rows=None, far=()):
    """Hand point sets around posed objects of the small table at 0.45 - 0.55 m: the first 8 points are a box (the "hand" mesh of the
    volume, BOX_FACES), the others fill 1.5 x that box; samples in `far` stand 0.3 m off their object (disjoint boxes)."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows if rows is not None else rng.permutation(5)[np.arange(B) % 5])
    R = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    t = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.45, 0.55, B)], 1)
    half = np.array([0.02, 0.015, 0.025])
    bx = box_mesh(-half, half)[0]
    pts = np.concatenate([bx[None].repeat(B, 0), rng.uniform(-1.5, 1.5, (B, max(Nh - 8, 0), 3)) * half], 1)[:, :max(Nh, 1)]
    if Nh < 8:
        pts = rng.uniform(-0.5, 0.5, (B, Nh, 3)) * half
    Rh = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    off = rng.uniform(-0.02, 0.02, (B, 3))
    if Nh < 8:
        off *= 0.25                                                              # well inside the object
    for b in far:
        off[b] += [0.3, 0.0, 0.0]
    hand = np.einsum("bij,bnj->bni", Rh, pts) + (t + off)[:, None]
    hf = BOX_FACES if Nh >= 8 else np.zeros((1, 3), np.int32)
    return dict(table=small_table(), hand=hand.astype(np.float32), rows=rows, rot=R.astype(np.float32), tsl=t.astype(np.float32), hand_faces=hf, hand_orient=1.0)


def stand_in_case(B, seed, table=None, obj_rows=None):
    """The stand-in hand posed by ab_mano_lbs at the assets' grasps, objects at 0.45 - 0.55 m depth."""
    from artiboost_amd.assets import make_grasps
    from artiboost_amd.metrics import ObjectMeshTable
    from artiboost_amd.synth import ManoLayerHIP
    a = stand_in_assets()
    table = table or _CACHE.setdefault("ho3d", ObjectMeshTable.from_assets(a))
    rng = np.random.default_rng(seed)
    rows = np.asarray(obj_rows if obj_rows is not None else rng.integers(0, table.n_obj, B))
    pose, shape, tsl = make_grasps(4, 50, seed=6)
    g = rng.integers(0, 50, B)
    o = rows % 4
    verts = ManoLayerHIP(a.hand)(torch.from_numpy(pose[o, g]).cuda(), torch.from_numpy(shape[o, g]).cuda())[0].cpu().numpy().astype(F64) + tsl[o, g][:, None]
    R = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    t = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.45, 0.55, B)], 1)
    hand = np.einsum("bij,bnj->bni", R, verts) + t[:, None]
    return dict(table=table, hand=hand.astype(np.float32), rows=rows, rot=R.astype(np.float32), tsl=t.astype(np.float32))


def _call(case, kernel, **kw):
    c = dict(case)
    table = c.pop("table")
    dtype, device = kw.pop("dtype", torch.float32 if kernel else torch.float64), kw.pop("device", "cuda")
    out = run_route(table, c.pop("hand"), c.pop("rows"), c.pop("rot"), c.pop("tsl"), dtype=dtype, device=device, kernel=kernel, **c, **kw)
    if kernel:
        torch.cuda.synchronize()
    return out


def check(tag, case, flags=3, **kw):
    """One kernel call against float64 (device) and the fp32 torch-CPU route; every figure printed before it is asserted.  -> (got, ref)"""
    table, hand, rows = case["table"], case["hand"], np.asarray(case["rows"])
    B, Nh = hand.shape[:2]
    max_voxels, voxel, thr = kw.get("max_voxels", 262144), kw.get("voxel", H), kw.get("contact_thr", 0.005)
    got = _call(case, True, flags=flags, want_sdf=True, **kw)
    ref = _call(case, False, flags=flags, want_sdf=True, want_lattice=True, **kw)
    nf = (table.face_off[1:] - table.face_off[:-1])[rows]
    if flags & 1:
        cpu = _call(case, False, dtype=torch.float32, device="cpu", flags=1, want_sdf=True, **kw)
        big = max(np.abs(hand).max(), np.abs(case["tsl"]).max() + np.abs(table.verts).max() * 1.8)
        e_cpu_d = float(np.abs(np.abs(cpu["sdf"].astype(F64)) - np.abs(ref["sdf"])).max())
        bound_d = max(4 * e_cpu_d, 16 * 2.0 ** -24 * big)
        err_d = float(np.abs(np.abs(got["sdf"].astype(F64)) - np.abs(ref["sdf"])).max())
        e_cpu_w = np.abs(cpu["wind"].astype(F64) - ref["wind"]).max(1)
        bound_w = np.maximum(4 * e_cpu_w, np.sqrt(nf) * 2.0 ** -24)
        err_w = np.abs(got["wind"].astype(F64) - ref["wind"]).max(1)
        print(f"{tag} |sdf|: kernel {err_d:.3e}  cpu-fp32 {e_cpu_d:.3e}  ratio {err_d / max(e_cpu_d, 1e-30):.2f}  bound {bound_d:.3e}")
        print(f"{tag} wind: kernel {err_w.max():.3e}  cpu-fp32 {e_cpu_w.max():.3e}  ratio {err_w.max() / max(e_cpu_w.max(), 1e-30):.2f}  bound {bound_w.min():.3e} (F {nf.tolist()})")
        W = WORST.setdefault(tag.split(" ")[0], {})
        W.update(sdf=err_d, sdf_cpu=e_cpu_d, wind=float(err_w.max()), wind_cpu=float(e_cpu_w.max()))
        assert np.isfinite(got["sdf"]).all() and np.isfinite(got["wind"]).all()
        assert err_d <= bound_d and (err_w <= bound_w).all(), (tag, err_d, bound_d, err_w, bound_w)
        amb = np.abs(ref["wind"] - 0.5) < 1e-3
        assert amb.sum() <= 0.01 * amb.size, (tag, amb.sum())                                      # the cap, on the float64 side
        in_k, in_r = got["sdf"] < 0, ref["sdf"] < 0
        assert np.array_equal(in_k[~amb], in_r[~amb]) and np.array_equal(in_k, got["wind"] > 0.5), tag
        assert np.array_equal(got["counts"][:, 0], in_k.sum(1)) and (np.abs(got["counts"][:, 0] - ref["counts"][:, 0]) <= amb.sum(1)).all()
        d = np.abs(ref["sdf"])
        din = np.where(in_k, d, 0.0)                                                                # float64 distances, the device's flags
        want = np.stack([din.max(1), din.sum(1) / np.maximum(in_k.sum(1), 1), d.min(1), in_k.sum(1) / Nh], 1)
        err_r = np.abs(got["rows"][:, :4].astype(F64) - want).max(0)
        print(f"{tag} rows: pen_max {err_r[0]:.3e}  pen_mean {err_r[1]:.3e}  min_dist {err_r[2]:.3e}  inside_frac {err_r[3]:.3e}  n_inside {got['counts'][:, 0].tolist()}  left out {int(amb.sum())}")
        assert (err_r[:3] <= bound_d).all() and err_r[3] <= 1e-6, (tag, err_r)
        sure = (amb.sum(1) == 0) & (np.abs(d.min(1) - thr) > bound_d)
        assert np.array_equal(got["rows"][sure, 4], ref["rows"][sure, 4]) and np.isin(got["rows"][:, 4], (0.0, 1.0)).all(), tag
    else:
        assert np.isnan(got["rows"][:, :5]).all() and (got["counts"][:, 0] == 0).all()
    if flags & 2:
        k, r = got["counts"].astype(np.int64), ref["counts"].astype(np.int64)
        amb = np.zeros(B, np.int64)
        for b, lat in enumerate(ref["lattice"]):
            if lat is not None:
                _, wo, wh = lat
                amb[b] = ((np.abs(wo - 0.5) < 1e-3) | ((wo > 0.5) & (np.abs(wh - 0.5) < 1e-3))).sum()
        print(f"{tag} volume: n_lattice {k[:, 1].tolist()} (float64 {r[:, 1].tolist()})  n_both {k[:, 2].tolist()} (float64 {r[:, 2].tolist()})  capped {k[:, 3].tolist()}  left out {amb.tolist()}")
        assert (amb <= 0.01 * np.maximum(r[:, 1], 1)).all(), (tag, amb)
        assert np.array_equal(k[:, 3], r[:, 3]) and (np.abs(k[:, 2] - r[:, 2]) <= amb).all(), tag
        ok = k[:, 3] == 0
        assert (k[ok, 2] <= k[ok, 1]).all() and (k[ok, 1] <= max_voxels).all() and (k[~ok, 1] > max_voxels).all() and (k[~ok, 2] == 0).all()
        assert np.isnan(got["rows"][~ok, 5]).all() and np.allclose(got["rows"][ok, 5], k[ok, 2] * voxel ** 3, rtol=1e-6, atol=0)
    else:
        assert np.isnan(got["rows"][:, 5]).all() and (got["counts"][:, 1:] == 0).all()
    assert np.isnan(got["rows"][:, 6:]).all()
    return got, ref


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
def test_one_vertex_against_a_box():
    case = small_case(1, 1, 1, rows=[1])
    got, _ = check("(1,1,box)", case)
    assert got["counts"][0, 0] == 1 and got["counts"][0, 2] == 0                    # inside the box; a hand "mesh" of one point has no volume


@pytest.mark.parametrize("B,Nh,voxel", [(2, 65, H), (3, 255, H), (2, 257, H), (2, 65, H / 2)])
def test_small_table_shapes_vs_float64(B, Nh, voxel):
    case = small_case(B, Nh, 100 + Nh + B, rows=[4, 1, 3][:B] if Nh != 255 else [2, 4, 0])
    got, ref = check(f"({B},{Nh},small{'' if voxel == H else ',2.5mm'})", case, voxel=voxel)
    assert got["counts"][:, 2].max() > 0 and got["counts"][:, 0].max() > 0


def test_stand_in_ho3d_objects_with_posed_hands():
    case = stand_in_case(3, 5, obj_rows=[1, 3, 0])
    assert (case["table"].face_off[1:] - case["table"].face_off[:-1]).tolist() == [3968] * 4 and case["hand"].shape == (3, 778, 3)
    got, ref = check("(3,778,HO3D)", case)
    assert got["counts"][:, 0].max() > 10 and got["counts"][:, 2].max() > 10
    again = _call(case, True, flags=3, want_sdf=True)                               # two calls give the same bits in every output
    assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in got)


def test_one_dexycb_stand_in_object():
    from artiboost_amd.assets import make_object
    from artiboost_amd.draw import hand_model_faces
    a = stand_in_assets()
    if "dex" not in _CACHE:
        o = make_object(2, 8192, 3)                                                 # what SceneAssets("DexYCB", seed=1) holds as its third object
        _CACHE["dex"] = table_of([(o["verts"], o["faces"])], (a.hand["v_template"], hand_model_faces(a.hand)))
    tb = _CACHE["dex"]
    assert tb.face_off[1] == 16128 and tb.orient[0] == -1.0
    check("(2,778,DexYCB)", stand_in_case(2, 9, table=tb, obj_rows=[0, 0]))


@pytest.mark.parametrize("Fh", [1, 255, 1025, 1538])
def test_hand_scan_of_the_volume_at_every_tile_count(Fh):
    from artiboost_amd.metrics import mesh_orientation
    case = stand_in_case(1, 21, obj_rows=[2])
    hf = case["table"].hand_faces[:Fh]
    case.update(hand_faces=hf, hand_orient=mesh_orientation(stand_in_assets().hand["v_template"], hf))
    got, ref = check(f"(Fh={Fh})", case, flags=2)
    assert got["counts"][0, 1] > 1000 and (Fh < 1538 or got["counts"][0, 2] > 0)


def test_a_capped_sample_beside_an_uncapped_one_and_disjoint_boxes():
    case = small_case(3, 257, 41, rows=[4, 1, 3], far=(1,))
    got, ref = check("(3,257,far)", case)
    n = got["counts"][:, 1]
    assert n[1] == 0 and got["counts"][1].tolist() == [0, 0, 0, 0] and got["rows"][1, 5] == 0.0 and got["rows"][1, 4] == 0.0 and got["rows"][1, 2] > 0.1
    assert n[0] != n[2] and min(n[0], n[2]) > 8
    mv = int(n[0] + n[2]) // 2
    cap, _ = check("(3,257,capped)", case, max_voxels=mv)
    big = 0 if n[0] > n[2] else 2
    assert cap["counts"][big, 3] == 1 and cap["counts"][2 - big, 3] == 0 and cap["counts"][big, 1] == n[big]
    for k in ("sdf", "wind"):
        assert np.array_equal(cap[k], got[k])
    assert np.array_equal(cap["rows"][:, :5], got["rows"][:, :5]) and np.array_equal(cap["rows"][2 - big], got["rows"][2 - big], equal_nan=True)


# ------------------------------------------------------------------------------------------------ 2. determinism, batch independence, flags
def _take(case, idx):
    return {k: (v[list(idx)] if k in ("hand", "rows", "rot", "tsl") else v) for k, v in case.items()}


def test_a_sample_does_not_depend_on_its_batch():
    case = small_case(4, 257, 77, rows=[4, 2, 1, 3])
    full = _call(case, True, want_sdf=True)
    twice = _call(case, True, want_sdf=True)
    assert all(np.array_equal(full[k], twice[k], equal_nan=True) for k in full)
    for s in range(4):
        alone = _call(_take(case, [s]), True, want_sdf=True)
        second = _call(_take(case, [(s + 1) % 4, s]), True, want_sdf=True)
        for k in full:
            assert np.array_equal(alone[k][0], full[k][s], equal_nan=True) and np.array_equal(second[k][1], full[k][s], equal_nan=True), (k, s)
    for r in range(1, 4):                                                            # every sample at each position of four
        order = [(p - r) % 4 for p in range(4)]
        rolled = _call(_take(case, order), True, want_sdf=True)
        for k in full:
            assert np.array_equal(rolled[k], full[k][order], equal_nan=True), (k, r)


def test_each_flag_alone_gives_the_bits_of_both_together():
    case = small_case(3, 65, 55, rows=[3, 4, 1])
    both = _call(case, True, flags=3, want_sdf=True)
    v, vol = _call(case, True, flags=1, want_sdf=True), _call(case, True, flags=2)
    assert np.array_equal(v["rows"][:, :5], both["rows"][:, :5]) and np.isnan(v["rows"][:, 5:]).all() and np.array_equal(v["sdf"], both["sdf"]) and np.array_equal(v["wind"], both["wind"])
    assert np.array_equal(v["counts"][:, 0], both["counts"][:, 0]) and not v["counts"][:, 1:].any()
    assert np.array_equal(vol["rows"][:, 5], both["rows"][:, 5]) and np.isnan(vol["rows"][:, :5]).all() and np.isnan(vol["rows"][:, 6:]).all()
    assert np.array_equal(vol["counts"][:, 1:], both["counts"][:, 1:]) and not vol["counts"][:, 0].any() and sorted(vol) == ["counts", "rows"]
    assert both["counts"][:, 2].max() > 0


# ------------------------------------------------------------------------------------------------ 3. the class on HIP tensors
def _to(d, dev, dtype=None):
    return {k: (v.to(dev).to(dtype) if torch.is_tensor(v) and v.dtype.is_floating_point and dtype else v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def test_metric_on_hip_tensors_matches_the_class_on_cpu_float64_and_reads_nothing_back():
    from artiboost_amd.metrics import Evaluator
    tb, p1, t1 = metric_batch(3, 11)
    _, p2, t2 = metric_batch(5, 12)
    for p, t in ((p1, t1), (p2, t2)):                                                 # the exclusions: none of these inputs is ambiguous
        for hand, R, tt in ((p["hand_verts_3d_abs"], p["box_rot_rotmat"], p["boxroot_3d_abs"]),
                            (t["hand_verts_3d"] + t["root_joint"][:, None], t["obj_transf"][:, :3, :3], t["obj_transf"][:, :3, 3])):
            ref = run_route(tb, hand.numpy(), tb.rows(t["obj_idx"]).numpy(), R.numpy(), tt.numpy(), want_sdf=True, want_lattice=True)
            assert (np.abs(ref["wind"] - 0.5) >= 1e-3).all() and (np.abs(ref["rows"][:, 2] - 0.005) > 1e-6).all()
            assert all(lat is None or ((np.abs(lat[1] - 0.5) >= 1e-3) & ~((lat[1] > 0.5) & (np.abs(lat[2] - 0.5) < 1e-3))).all() for lat in ref["lattice"])
    out = {}
    for dev in ("cpu", "cuda"):
        ev = Evaluator({}, [build_interaction(tb, REPORT_GT=True)])
        ev.feed_all(_to(p1, dev), _to(t1, dev))
        if dev == "cuda":                                                             # the table is on the device now: nothing below may wait for it
            m = ev._metrics_list[0]
            p2d, t2d = _to(p2, dev), _to(t2, dev)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                tensors, names = m.feed_device(p2d, t2d, memo={})
                assert names == ["", "gt_"] and all(x.is_cuda and x.shape == (9,) for x in tensors)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        ev.feed_all(_to(p2, dev), _to(t2, dev))
        out[dev] = ev.get_measures_all()
    assert set(out["cuda"]) == set(out["cpu"]) and len(out["cpu"]) == 14
    for k, v in out["cpu"].items():
        print(f"{k}: cpu float64 {v:.6f}  device {out['cuda'][k]:.6f}")
        assert abs(out["cuda"][k] - v) <= 1e-3, k                                     # mm, cm^3, and pure numbers that are ratios of counts


def test_one_call_per_group_and_feed_all(monkeypatch):
    from artiboost_amd import kernels as K
    from artiboost_amd.metrics import Evaluator
    calls = []
    real = K.interaction
    monkeypatch.setattr(K, "interaction", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    tb, p, t = metric_batch(3, 13)
    ev = Evaluator({}, [build_interaction(tb, REPORT_GT=True), build_interaction(tb, REPORT_GT=False)])
    ev.feed_all(_to(p, "cuda", torch.float32), _to(t, "cuda", torch.float32))
    assert len(calls) == 2 and ev.get_measures_all()["capped"] == 0                 # the second metric is served by the memo


# ------------------------------------------------------------------------------------------------ 4. the dispatcher op's refusals
def test_dispatcher_op_refusals():
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    L.lib()
    op = torch.ops.artiboost_hip.interaction
    tb = small_table().on("cuda")
    B, Nh, mv = 2, 5, 512
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    ws = torch.zeros(int(torch.ops.artiboost_hip.interaction_workspace(B, Nh, mv)), dtype=torch.uint8, device="cuda")
    eye = torch.eye(3, device="cuda").repeat(B, 1, 1).contiguous()

    def args(**kw):
        a = dict(hand_verts=z(B, Nh, 3), hand_faces=tb["hand_faces"], Nh=Nh, Fh=12, hand_orient=1.0, obj_verts=tb["obj_verts"], obj_faces=tb["obj_faces"],
                 vert_off=tb["vert_off"], face_off=tb["face_off"], obj_orient=tb["obj_orient"], n_obj=5, obj_row=torch.tensor([1, 4], device="cuda"), rot=eye,
                 tsl=z(B, 3), B=B, contact_thr=0.005, voxel=0.005, max_voxels=mv, flags=3, rows=z(B, 8),
                 counts=torch.zeros(B, 4, dtype=torch.int32, device="cuda"), sdf=None, wind=None, workspace=ws)
        a.update(kw)
        return list(a.values())
    op(*args())                                                                  # the well-formed call goes through
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        op(*args(hand_verts=torch.zeros(B, Nh, 3)))
    with pytest.raises(RuntimeError, match="'hand_verts' holds"):
        op(*args(hand_verts=z(B * Nh * 3 - 1)))
    with pytest.raises(RuntimeError, match="'sdf' holds"):
        op(*args(sdf=z(B, Nh - 1)))
    with pytest.raises(RuntimeError, match="'face_off' holds"):
        op(*args(face_off=tb["face_off"][:5].contiguous()))
    with pytest.raises(RuntimeError, match="bytes"):
        op(*args(workspace=ws[:-1]))
    for bad in (dict(flags=0), dict(flags=4), dict(voxel=0.0), dict(contact_thr=-1.0), dict(max_voxels=0), dict(hand_orient=0.5), dict(Fh=0), dict(rows=None)):
        with pytest.raises(RuntimeError, match="argument error"):
            op(*args(**bad))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="device tensors"):
        c = small_case(1, 8, 3)
        run_route(c["table"], c["hand"], c["rows"], c["rot"], c["tsl"], dtype=torch.float32, device="cpu", kernel=True)
    with pytest.raises(ValueError, match="obj_row"):
        K.interaction(z(B, Nh, 3), tb["hand_faces"], 1.0, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"],
                      torch.tensor([1, 4], device="cuda", dtype=torch.int32), eye, z(B, 3))


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_honet_forward_through_an_evaluator_that_holds_the_metric():
    import yaml
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import Evaluator
    from test_gpu_honet import ARCH, PRESET, _batch
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_mi355x.yaml")))
    torch.manual_seed(0)
    model = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32"), preset_cfg=PRESET)[0]
    model.eval()
    batch = _batch(4, 31, N=30)
    batch.update(obj_id=torch.tensor([1, 2, 3, 0]), persp_id=torch.tensor([0, 1, 2, 3]), grasp_id=torch.tensor([3, 4, 5, 6]), is_synth=torch.ones(4, dtype=torch.int64),
                 obj_idx=torch.tensor([9, 12, 5, 11]))
    with torch.no_grad():
        preds = model(batch)
    assert preds["hand_verts_3d_abs"].is_cuda and preds["box_rot_rotmat"].shape == (4, 3, 3)
    ev = Evaluator(cfg, R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"]))
    ev.feed_all(preds, batch, losses={})
    got = ev.get_measures_all()
    m = ev.metrics_list[-1]
    case = dict(table=m.table, hand=preds["hand_verts_3d_abs"].detach().float().cpu().numpy(), rows=m.table.rows(batch["obj_idx"]).numpy(),
                rot=preds["box_rot_rotmat"].detach().float().cpu().numpy(), tsl=preds["boxroot_3d_abs"].detach().float().reshape(4, 3).cpu().numpy())
    ref = _call(case, False, want_sdf=True, want_lattice=True)
    names = ("pen_depth_mm", "pen_mean_mm", "min_dist_mm", "inside_frac", "contact_ratio", "inter_vol_cm3", "capped")
    print({k: got[k] for k in names}, ref["counts"].tolist())
    assert all(np.isfinite(got[k]) for k in names)
    ok = ref["counts"][:, 3] == 0
    assert got["capped"] == int((~ok).sum())
    amb_v = (np.abs(ref["wind"] - 0.5) < 1e-3).sum()
    amb_l = sum(0 if lat is None else int(((np.abs(lat[1] - 0.5) < 1e-3) | ((lat[1] > 0.5) & (np.abs(lat[2] - 0.5) < 1e-3))).sum()) for lat in ref["lattice"])
    assert amb_v <= 0.01 * ref["wind"].size and amb_l <= 0.01 * max(int(ref["counts"][:, 1].sum()), 1)
    want = {"pen_depth_mm": 1e3 * ref["rows"][:, 0].mean(), "pen_mean_mm": 1e3 * ref["rows"][:, 1].mean(), "min_dist_mm": 1e3 * ref["rows"][:, 2].mean(),
            "inside_frac": ref["rows"][:, 3].mean(), "contact_ratio": ref["rows"][:, 4].mean(), "inter_vol_cm3": 1e6 * ref["rows"][ok, 5].mean() if ok.any() else float("nan")}
    for k, v in want.items():
        # a vertex or lattice point left out moves a mean by at most its share: one vertex of 778 by 1 / 778 of the largest depth, one lattice point by h^3
        slack = (amb_v / 778.0 * 1e3 * float(np.abs(ref["sdf"]).max()) if k.endswith("_mm") else amb_v / 778.0) if k != "inter_vol_cm3" else amb_l * 0.125
        print(f"{k}: device {got[k]:.6f}  float64 {v:.6f}  slack {slack:.3e}")
        assert abs(got[k] - v) <= 1e-3 + slack or (np.isnan(v) and np.isnan(got[k])), k


def test_print_the_error_table():
    """(last: the measured kernel errors and their ratio to the fp32 torch-CPU route's, for DESIGN.md section 24)"""
    for tag, w in WORST.items():
        print(f"{tag}: |sdf| {w['sdf']:.2e} (cpu {w['sdf_cpu']:.2e}, ratio {w['sdf'] / max(w['sdf_cpu'], 1e-30):.2f})  wind {w['wind']:.2e} (cpu {w['wind_cpu']:.2e}, ratio {w['wind'] / max(w['wind_cpu'], 1e-30):.2f})")
