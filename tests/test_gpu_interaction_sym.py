"""ab_interaction_sym (csrc/interact_sym.hip) on the device against `metrics.interaction_sym_values_torch` in float64
on the same inputs (run on the device's float64 units): every object vertex count around the chunk of 256 and every hand face count around
the tile of 512, the stand-in meshes, determinism and independence of the batch around a sample, the optional outputs,
`InteractionMetric(SYMMETRIC=True)` on HIP tensors, the dispatcher op's refusals, and one HoNet forward fed through an evaluator built from
the symmetric YAML.  Nothing here captures a graph.

Bounds (the rules of section 24; none is a recorded figure; every figure is printed before it is asserted):
  |sdf_obj|, obj_pen_max, obj_pen_mean,   the larger of 4 x the error of the fp32 torch-CPU route against float64 on that case and
  obj_min_dist                            16 x 2^-24 x max |coordinate| of the case.
  wind_obj                                the larger of 4 x the fp32 torch-CPU route's error and sqrt(Fh) x 2^-24.
  inside flags, n_obj_inside,             equal to float64's; an object vertex is left out only when its float64 o w lies within 1e-3 of 0.5
  obj_contact                             (for `obj_contact` also an obj_min_dist within the distance bound of the threshold); at most 1 % of a
                                          case's object vertices may be left out, asserted on the float64 side.
  NaN                                     sdf_obj and wind_obj are NaN exactly at i >= No_r; counts[:, 1] == No_r."""
import os

import numpy as np
import pytest
import torch

from test_gpu_interaction import _take, _to, stand_in_case
from test_interaction_host import F64, HI, LO, ONE_TRI, box_mesh, build_interaction, icosphere, metric_batch, rotation, run_route, stand_in_assets, table_of
from test_interaction_sym_host import run_sym

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}
_CACHE = {}
HALF = np.array([0.015, 0.01, 0.025])                                              # the half extents of the "hand" box of the small cases
COUNTS = [3, 8, 255, 256, 257, 642]


def count_table():
    """One packed table of objects of 3 (one triangle), 8 (box), 255, 256, 257 (the box plus unreferenced vertices inside 1.5 x the box) and
    642 vertices (the level-3 icosphere: three chunks of 256, the last partial); the hand is the box of HALF."""
    if "count" not in _CACHE:
        rng = np.random.default_rng(2)
        bv, bf = box_mesh(LO, HI)
        padded = [(np.concatenate([bv, rng.uniform(-1.5, 1.5, (n - 8, 3)) * HI]), bf) for n in (255, 256, 257)]
        _CACHE["count"] = table_of([ONE_TRI, (bv, bf)] + padded + [icosphere(0.045, 3)], box_mesh(-HALF, HALF))
        assert (_CACHE["count"].vert_off[1:] - _CACHE["count"].vert_off[:-1]).tolist() == COUNTS and _CACHE["count"].no_max == 642
    return _CACHE["count"]


def box_hand_case(table, rows, seed, far=()):
    """The box hand (8 vertices, 12 faces) poked into posed objects of `table` at 0.45 - 0.55 m; samples in `far` stand 0.3 m off."""
    rng = np.random.default_rng(seed)
    B = len(rows)
    R = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    t = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.45, 0.55, B)], 1)
    Rh = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    off = rng.uniform(-0.02, 0.02, (B, 3))
    for b in far:
        off[b] += [0.3, 0.0, 0.0]
    hand = np.einsum("bij,nj->bni", Rh, box_mesh(-HALF, HALF)[0]) + (t + off)[:, None]
    return dict(table=table, hand=hand.astype(np.float32), rows=np.asarray(rows), rot=R.astype(np.float32), tsl=t.astype(np.float32))


def _call(case, kernel, **kw):
    c = dict(case)
    table = c.pop("table")
    dtype, device = kw.pop("dtype", torch.float32 if kernel else torch.float64), kw.pop("device", "cuda")
    out = run_sym(table, c.pop("hand"), c.pop("rows"), c.pop("rot"), c.pop("tsl"), dtype=dtype, device=device, kernel=kernel, **c, **kw)
    if kernel:
        torch.cuda.synchronize()
    return out


def check(tag, case, **kw):
    """One kernel call against float64 (device) and the fp32 torch-CPU route; every figure printed before it is asserted.  -> (got, ref)"""
    table, hand, rows = case["table"], case["hand"], np.clip(np.asarray(case["rows"]), 0, case["table"].n_obj - 1)
    B, thr = len(hand), kw.get("contact_thr", 0.005)
    Fh = len(case["hand_faces"]) if "hand_faces" in case else len(table.hand_faces)
    no = (table.vert_off[1:] - table.vert_off[:-1])[rows]
    got = _call(case, True, want_sdf=True, **kw)
    ref = _call(case, False, want_sdf=True, **kw)
    cpu = _call(case, False, dtype=torch.float32, device="cpu", want_sdf=True, **kw)
    valid = np.arange(table.no_max)[None] < no[:, None]
    for k in ("sdf_obj", "wind_obj"):
        assert got[k].shape == (B, table.no_max) and np.array_equal(np.isnan(got[k]), ~valid) and np.array_equal(np.isnan(ref[k]), ~valid), (tag, k)
    assert np.array_equal(got["counts"][:, 1], no) and np.array_equal(ref["counts"][:, 1], no)
    z = lambda a: np.where(valid, a, 0.0)      # noqa: E731
    big = max(np.abs(hand).max(), np.abs(case["tsl"]).max() + np.abs(table.verts).max() * 1.8)
    e_cpu_d = float(z(np.abs(np.abs(cpu["sdf_obj"].astype(F64)) - np.abs(ref["sdf_obj"]))).max())
    bound_d = max(4 * e_cpu_d, 16 * 2.0 ** -24 * big)
    err_d = float(z(np.abs(np.abs(got["sdf_obj"].astype(F64)) - np.abs(ref["sdf_obj"]))).max())
    e_cpu_w = z(np.abs(cpu["wind_obj"].astype(F64) - ref["wind_obj"])).max(1)
    bound_w = np.maximum(4 * e_cpu_w, np.sqrt(Fh) * 2.0 ** -24)
    err_w = z(np.abs(got["wind_obj"].astype(F64) - ref["wind_obj"])).max(1)
    print(f"{tag} |sdf_obj|: kernel {err_d:.3e}  cpu-fp32 {e_cpu_d:.3e}  ratio {err_d / max(e_cpu_d, 1e-30):.2f}  bound {bound_d:.3e}")
    print(f"{tag} wind_obj: kernel {err_w.max():.3e}  cpu-fp32 {e_cpu_w.max():.3e}  ratio {err_w.max() / max(e_cpu_w.max(), 1e-30):.2f}  bound {bound_w.min():.3e} (Fh {Fh}, No {no.tolist()})")
    WORST.setdefault(tag.split(" ")[0], {}).update(sdf=err_d, sdf_cpu=e_cpu_d, wind=float(err_w.max()), wind_cpu=float(e_cpu_w.max()))
    assert err_d <= bound_d and (err_w <= bound_w).all(), (tag, err_d, bound_d, err_w, bound_w)
    amb = valid & (np.abs(z(ref["wind_obj"]) - 0.5) < 1e-3)
    assert amb.sum() <= 0.01 * valid.sum(), (tag, amb.sum())                                       # the cap, on the float64 side
    in_k, in_r = valid & (z(got["sdf_obj"]) < 0), valid & (z(ref["sdf_obj"]) < 0)
    assert np.array_equal(in_k[~amb], in_r[~amb]) and np.array_equal(in_k, valid & (z(got["wind_obj"]) > 0.5)), tag
    assert np.array_equal(got["counts"][:, 0], in_k.sum(1)) and (np.abs(got["counts"][:, 0] - ref["counts"][:, 0]) <= amb.sum(1)).all()
    d = np.abs(z(ref["sdf_obj"]))
    din = np.where(in_k, d, 0.0)                                                                    # float64 distances, the device's flags
    want = np.stack([din.max(1), din.sum(1) / np.maximum(in_k.sum(1), 1), np.where(valid, d, np.inf).min(1), in_k.sum(1) / no], 1)
    err_r = np.abs(got["rows"][:, :4].astype(F64) - want).max(0)
    print(f"{tag} rows: obj_pen_max {err_r[0]:.3e}  obj_pen_mean {err_r[1]:.3e}  obj_min_dist {err_r[2]:.3e}  obj_inside_frac {err_r[3]:.3e}  n_obj_inside {got['counts'][:, 0].tolist()}  left out {int(amb.sum())}")
    assert (err_r[:3] <= bound_d).all() and err_r[3] <= 1e-6, (tag, err_r)
    sure = (amb.sum(1) == 0) & (np.abs(want[:, 2] - thr) > bound_d)
    assert np.array_equal(got["rows"][sure, 4], ref["rows"][sure, 4]) and np.isin(got["rows"][:, 4], (0.0, 1.0)).all(), tag
    assert np.isnan(got["rows"][:, 5:]).all() and got["rows"].shape == (B, 8) and got["counts"].shape == (B, 2)
    return got, ref


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("row", range(6))
def test_object_vertex_counts_across_the_chunk(row):
    got, _ = check(f"(1,No={COUNTS[row]})", box_hand_case(count_table(), [row], 300 + row))
    assert got["counts"][0, 1] == COUNTS[row]


def test_a_batch_that_mixes_object_sizes():
    """3, 642, 256 and 257 vertices in one call with No_max = 642: workgroups that leave early, their NaN fill, a partial last chunk."""
    got, _ = check("(4,mixed)", box_hand_case(count_table(), [0, 5, 3, 4], 311))
    assert got["counts"][:, 1].tolist() == [3, 642, 256, 257] and got["counts"][:, 0].max() > 0


@pytest.mark.parametrize("Fh", [1, 511, 512, 513, 0])
def test_hand_face_counts_across_the_tile(Fh):
    """Slices hand_faces[:Fh] of the stand-in hand (0: the whole kept list, three tiles) against one HO3D stand-in object."""
    from artiboost_amd.metrics import mesh_orientation
    case = stand_in_case(1, 21, obj_rows=[2])
    hf = case["table"].hand_faces[:Fh] if Fh else case["table"].hand_faces
    assert len(hf) == Fh or (Fh == 0 and 1024 < len(hf) <= 1538)
    case.update(hand_faces=hf, hand_orient=mesh_orientation(stand_in_assets().hand["v_template"], hf))
    got, _ = check(f"(Fh={len(hf)})", case)
    assert got["counts"][0, 1] == 2048


@pytest.mark.parametrize("Nh", [3, 8])
def test_the_smallest_hands_against_a_stand_in_object(Nh):
    """Nh = 3, Fh = 1 (one triangle) and Nh = 8, Fh = 12 (the box hand) against one HO3D stand-in object."""
    case = stand_in_case(1, 21, obj_rows=[2])
    hv, hf = (ONE_TRI[0] - 0.01, ONE_TRI[1]) if Nh == 3 else box_mesh(-HALF, HALF)
    hand = (hv + [0.01, 0.0, 0.02]) @ case["rot"][0].astype(F64).T + case["tsl"][0]
    case.update(hand=hand[None].astype(np.float32), hand_faces=hf, hand_orient=1.0)
    got, _ = check(f"(Nh={Nh},Fh={len(hf)})", case)
    assert case["hand"].shape == (1, Nh, 3) and (Nh == 3 or got["counts"][0, 0] > 0)


def test_stand_in_ho3d_objects_with_posed_hands():
    case = stand_in_case(3, 5, obj_rows=[1, 3, 0])
    assert case["hand"].shape == (3, 778, 3) and case["table"].no_max == 2048 and 1024 < len(case["table"].hand_faces) <= 1538
    got, ref = check("(3,2048,HO3D)", case)
    assert got["counts"][:, 0].max() > 10
    again = _call(case, True, want_sdf=True)                                        # two calls give the same bits in every output
    assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in got)


def test_one_dexycb_stand_in_object():
    from artiboost_amd.assets import make_object
    from artiboost_amd.draw import hand_model_faces
    a = stand_in_assets()
    if "dex" not in _CACHE:
        o = make_object(2, 8192, 3)                                                 # what SceneAssets("DexYCB", seed=1) holds as its third object
        _CACHE["dex"] = table_of([(o["verts"], o["faces"])], (a.hand["v_template"], hand_model_faces(a.hand)))
    tb = _CACHE["dex"]
    assert tb.no_max == 8192
    check("(2,8192,DexYCB)", stand_in_case(2, 9, table=tb, obj_rows=[0, 0]))


# ------------------------------------------------------------------------------------------------ 2. determinism, batch independence, outputs
def test_a_sample_does_not_depend_on_its_batch():
    case = box_hand_case(count_table(), [5, 2, 1, 4], 77)
    full = _call(case, True, want_sdf=True)
    twice = _call(case, True, want_sdf=True)
    assert all(np.array_equal(full[k], twice[k], equal_nan=True) for k in full) and np.isnan(full["sdf_obj"][1:]).any() and full["counts"][:, 0].max() > 0
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


def test_a_call_without_the_optional_outputs_gives_the_same_rows_and_counts():
    case = box_hand_case(count_table(), [4, 0, 5], 55)
    a, b = _call(case, True, want_sdf=True), _call(case, True)
    assert sorted(b) == ["counts", "rows"] and np.array_equal(a["rows"], b["rows"], equal_nan=True) and np.array_equal(a["counts"], b["counts"])


def test_a_disjoint_sample_beside_touching_ones():
    got, _ = check("(3,far)", box_hand_case(count_table(), [3, 1, 4], 41, far=(1,)))
    r = got["rows"][1]
    assert got["counts"][1].tolist() == [0, 8] and r[0] == 0.0 and r[1] == 0.0 and r[2] > 0.1 and r[3] == 0.0 and r[4] == 0.0
    assert (got["counts"][[0, 2], 0] > 0).all() and (got["rows"][[0, 2], 4] == 1.0).all()


# ------------------------------------------------------------------------------------------------ 3. the class on HIP tensors
def _groups(p, t):
    return ((p["hand_verts_3d_abs"], p["box_rot_rotmat"], p["boxroot_3d_abs"]),
            (t["hand_verts_3d"] + t["root_joint"][:, None], t["obj_transf"][:, :3, :3], t["obj_transf"][:, :3, 3]))


def test_symmetric_metric_on_hip_tensors_matches_the_class_on_cpu_float64_and_reads_nothing_back():
    from artiboost_amd.metrics import Evaluator
    tb, p1, t1 = metric_batch(3, 11)
    _, p2, t2 = metric_batch(5, 12)
    for p, t in ((p1, t1), (p2, t2)):                                                 # the exclusions: none of these inputs is ambiguous
        for hand, R, tt in _groups(p, t):
            rows = tb.rows(t["obj_idx"]).numpy()
            one = run_route(tb, hand.numpy(), rows, R.numpy(), tt.numpy(), flags=1, want_sdf=True)
            rev = run_sym(tb, hand.numpy(), rows, R.numpy(), tt.numpy(), want_sdf=True)
            assert (np.abs(one["wind"] - 0.5) >= 1e-3).all() and (np.abs(one["rows"][:, 2] - 0.005) > 1e-6).all()
            assert not (np.abs(rev["wind_obj"] - 0.5) < 1e-3).any() and (np.abs(rev["rows"][:, 2] - 0.005) > 1e-6).all()
    out = {}
    for dev in ("cpu", "cuda"):
        ev = Evaluator({}, [build_interaction(tb, REPORT_GT=True, SYMMETRIC=True, VOLUME=False)])
        ev.feed_all(_to(p1, dev), _to(t1, dev))
        if dev == "cuda":                                                             # the table is on the device now: nothing below may wait for it
            m = ev._metrics_list[0]
            p2d, t2d = _to(p2, dev), _to(t2, dev)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                tensors, names = m.feed_device(p2d, t2d, memo={})
                assert names == ["", "gt_"] and all(x.is_cuda and x.shape == (15,) for x in tensors)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        ev.feed_all(_to(p2, dev), _to(t2, dev))
        out[dev] = ev.get_measures_all()
    assert set(out["cuda"]) == set(out["cpu"]) and len(out["cpu"]) == 22
    for k, v in out["cpu"].items():
        print(f"{k}: cpu float64 {v:.6f}  device {out['cuda'][k]:.6f}")
        assert abs(out["cuda"][k] - v) <= 1e-3, k                                     # mm, and pure numbers that are ratios of counts


def test_one_call_of_each_entry_point_per_group(monkeypatch):
    from artiboost_amd import kernels as K
    from artiboost_amd.metrics import Evaluator
    calls = {"one": [], "sym": []}
    real, real_sym = K.interaction, K.interaction_sym
    monkeypatch.setattr(K, "interaction", lambda *a, **k: (calls["one"].append(a[0].shape), real(*a, **k))[1])
    monkeypatch.setattr(K, "interaction_sym", lambda *a, **k: (calls["sym"].append(a[0].shape), real_sym(*a, **k))[1])
    tb, p, t = metric_batch(3, 13)
    ev = Evaluator({}, [build_interaction(tb), build_interaction(tb, SYMMETRIC=True), build_interaction(tb, SYMMETRIC=True)])
    ev.feed_all(_to(p, "cuda", torch.float32), _to(t, "cuda", torch.float32))
    assert len(calls["one"]) == 1 and len(calls["sym"]) == 1 and "sym_pen_depth_mm" in ev.get_measures_all()      # the memo serves the others
    calls["one"].clear(); calls["sym"].clear()
    Evaluator({}, [build_interaction(tb, REPORT_GT=True)]).feed_all(_to(p, "cuda", torch.float32), _to(t, "cuda", torch.float32))
    assert len(calls["one"]) == 2 and not calls["sym"]                               # SYMMETRIC false: the calls of before, and no other


# ------------------------------------------------------------------------------------------------ 4. the dispatcher op's refusals
def test_dispatcher_op_refusals():
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    L.lib()
    op = torch.ops.artiboost_hip.interaction_sym
    tb = count_table().on("cuda")
    B, Nh, nm = 2, 8, 642
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    ws = torch.zeros(int(torch.ops.artiboost_hip.interaction_sym_workspace(B, Nh, nm)), dtype=torch.uint8, device="cuda")
    assert ws.numel() == B * (Nh * 3 + 3 * 4) * 4
    eye = torch.eye(3, device="cuda").repeat(B, 1, 1).contiguous()

    def args(**kw):
        a = dict(hand_verts=z(B, Nh, 3), hand_faces=tb["hand_faces"], Nh=Nh, Fh=12, hand_orient=1.0, obj_verts=tb["obj_verts"], vert_off=tb["vert_off"], n_obj=6,
                 obj_row=torch.tensor([1, 5], device="cuda"), rot=eye, tsl=z(B, 3), B=B, No_max=nm, contact_thr=0.005, rows=z(B, 8),
                 counts=torch.zeros(B, 2, dtype=torch.int32, device="cuda"), sdf_obj=None, wind_obj=None, workspace=ws)
        a.update(kw)
        return list(a.values())
    op(*args())                                                                  # the well-formed call goes through
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        op(*args(hand_verts=torch.zeros(B, Nh, 3)))
    with pytest.raises(RuntimeError, match="'hand_verts' holds"):
        op(*args(hand_verts=z(B * Nh * 3 - 1)))
    with pytest.raises(RuntimeError, match="'sdf_obj' holds"):
        op(*args(sdf_obj=z(B, nm - 1)))
    with pytest.raises(RuntimeError, match="'vert_off' holds"):
        op(*args(vert_off=tb["vert_off"][:6].contiguous()))
    with pytest.raises(RuntimeError, match="bytes"):
        op(*args(workspace=ws[:-1]))
    for bad in (dict(Fh=0), dict(No_max=0), dict(hand_orient=0.5), dict(contact_thr=-1.0), dict(rows=None)):
        with pytest.raises(RuntimeError, match="argument error"):
            op(*args(**bad))
    torch.cuda.synchronize()
    c = box_hand_case(count_table(), [1], 3)
    with pytest.raises(RuntimeError, match="device tensors"):
        run_sym(c["table"], c["hand"], c["rows"], c["rot"], c["tsl"], dtype=torch.float32, device="cpu", kernel=True)
    with pytest.raises(ValueError, match="obj_row"):
        K.interaction_sym(z(B, Nh, 3), tb["hand_faces"], 1.0, tb["obj_verts"], tb["vert_off"], torch.tensor([1, 5], device="cuda", dtype=torch.int32), eye, z(B, 3), nm)


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_honet_forward_through_an_evaluator_built_from_the_symmetric_yaml():
    import yaml
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import IA_SYM_MEASURES, Evaluator
    from test_gpu_honet import ARCH, PRESET, _batch
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_sym_mi355x.yaml")))
    torch.manual_seed(0)
    model = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32"), preset_cfg=PRESET)[0]
    model.eval()
    batch = _batch(4, 31, N=30)      # seed 31: checked on the device, the float64 side leaves out no object vertex and no hand vertex (the cap below)
    batch.update(obj_id=torch.tensor([1, 2, 3, 0]), persp_id=torch.tensor([0, 1, 2, 3]), grasp_id=torch.tensor([3, 4, 5, 6]), is_synth=torch.ones(4, dtype=torch.int64),
                 obj_idx=torch.tensor([9, 12, 5, 11]))
    with torch.no_grad():
        preds = model(batch)
    ev = Evaluator(cfg, R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"]))
    ev.feed_all(preds, batch, losses={})
    got = ev.get_measures_all()
    m = ev.metrics_list[-1]
    assert m.symmetric
    hand, rows = preds["hand_verts_3d_abs"].detach().float().cpu().numpy(), m.table.rows(batch["obj_idx"]).numpy()
    rot, tsl = preds["box_rot_rotmat"].detach().float().cpu().numpy(), preds["boxroot_3d_abs"].detach().float().reshape(4, 3).cpu().numpy()
    one = run_route(m.table, hand, rows, rot, tsl, device="cuda", flags=1, want_sdf=True)
    rev = run_sym(m.table, hand, rows, rot, tsl, device="cuda", want_sdf=True)
    print({k: got[k] for k in IA_SYM_MEASURES}, rev["counts"].tolist())
    assert all(np.isfinite(got[k]) for k in IA_SYM_MEASURES)
    amb_h, amb_o = int((np.abs(one["wind"] - 0.5) < 1e-3).sum()), int((np.abs(rev["wind_obj"] - 0.5) < 1e-3).sum())
    assert amb_h <= 0.01 * one["wind"].size and amb_o <= 0.01 * rev["wind_obj"].size                # the cap, on the float64 side
    near = int(((np.abs(one["rows"][:, 2] - 0.005) < 1e-6) | (np.abs(rev["rows"][:, 2] - 0.005) < 1e-6)).sum())
    o, r = one["rows"], rev["rows"]
    want = {"obj_pen_depth_mm": 1e3 * r[:, 0].mean(), "obj_pen_mean_mm": 1e3 * r[:, 1].mean(), "obj_min_dist_mm": 1e3 * r[:, 2].mean(), "obj_inside_frac": r[:, 3].mean(),
            "sym_pen_depth_mm": 1e3 * np.maximum(o[:, 0], r[:, 0]).mean(), "sym_contact_ratio": np.maximum(o[:, 4], r[:, 4]).mean()}
    deepest = 1e3 * max(float(np.abs(one["sdf"]).max()), float(np.nanmax(np.abs(rev["sdf_obj"]))))
    for k, v in want.items():
        # a vertex left out moves a mean over vertices by at most its share of the largest depth, a maximum or a flag of its sample by all of it
        slack = {"obj_pen_mean_mm": amb_o / 2048.0 * deepest, "obj_inside_frac": amb_o / 2048.0, "obj_min_dist_mm": 0.0,
                 "sym_contact_ratio": (min(amb_o + amb_h, 4) + near) / 4.0}.get(k, min(amb_o + amb_h, 4) / 4.0 * deepest)
        print(f"{k}: device {got[k]:.6f}  float64 {v:.6f}  slack {slack:.3e}")
        assert abs(got[k] - v) <= 1e-3 + slack, k


def test_print_the_error_table():
    """(last: the measured kernel errors and their ratio to the fp32 torch-CPU route's, for DESIGN.md section 27)"""
    for tag, w in WORST.items():
        print(f"{tag}: |sdf_obj| {w['sdf']:.2e} (cpu {w['sdf_cpu']:.2e}, ratio {w['sdf'] / max(w['sdf_cpu'], 1e-30):.2f})  wind_obj {w['wind']:.2e} (cpu {w['wind_cpu']:.2e}, ratio {w['wind'] / max(w['wind_cpu'], 1e-30):.2f})")
