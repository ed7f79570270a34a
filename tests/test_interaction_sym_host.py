"""The symmetric interaction measures on the host: the float64 torch route of the reverse direction
(`metrics.interaction_sym_values_torch`: the object's vertices against the hand mesh) against analytic values -- a small sphere inside a
"hand" box that the one-sided measures cannot see, a flipped hand, one open triangle, an object outside, rigid invariance, a packed table of
irregular objects --, `InteractionMetric(SYMMETRIC=True)` on CPU tensors through the evaluator, the YAML and the header contract with its
generated op.  `run_sym` is shared with tests/test_gpu_interaction_sym.py."""
import math
import os
import re

import numpy as np
import torch

from test_interaction_host import (F64, HI, I3, LO, ONE_TRI, Z3, box_mesh, box_sdf, build_interaction, icosphere, metric_batch, rotation,
                                   run_route, table_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND_LO, HAND_HI = np.array([-0.02, -0.015, -0.01]), np.array([0.02, 0.015, 0.01])      # the "hand" box of the issue: 40 x 30 x 20 mm


def run_sym(table, hand, rows, rot, tsl, dtype=torch.float64, device="cpu", kernel=False, hand_faces=None, hand_orient=None, no_max=None, **kw):
    """One call of the torch route of the reverse direction (or of the kernel) on numpy inputs -> dict of numpy arrays."""
    from artiboost_amd import kernels as K
    from artiboost_amd.metrics import interaction_sym_values_torch
    tb = table.on(device)
    t = lambda a, d=dtype: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=d).contiguous()      # noqa: E731
    B = len(hand)
    fn = K.interaction_sym if kernel else interaction_sym_values_torch
    hf = tb["hand_faces"] if hand_faces is None else t(np.asarray(hand_faces).reshape(-1, 3), torch.int32)
    o = fn(t(hand), hf, table.hand_orient if hand_orient is None else hand_orient, tb["obj_verts"], tb["vert_off"], t(rows, torch.int64),
           t(np.asarray(rot).reshape(B, 3, 3)), t(np.asarray(tsl).reshape(B, 3)), table.no_max if no_max is None else no_max, **kw)
    return {k: v.cpu().numpy() for k, v in o.items()}


def sphere_in_box(flip=False):
    """The 5 mm level-1 icosphere (42 vertices) at (4, -3, 2) mm inside the "hand" box, both posed by one rigid map at half a metre.
    -> (table, hand [1,8,3], rot, tsl, the sphere's vertices in the hand's frame)"""
    tb = table_of([icosphere(0.005, 1)], box_mesh(HAND_LO, HAND_HI, flip))
    G, g = rotation(17), np.array([0.03, -0.02, 0.5])
    c = np.array([0.004, -0.003, 0.002])
    hand = (box_mesh(HAND_LO, HAND_HI)[0] @ G.T + g)[None]
    return tb, hand, G[None], (G @ c + g)[None], tb.verts.astype(F64) + c


# ------------------------------------------------------------------------------------------------ 1. analytic values of the float64 route
def test_a_small_sphere_inside_the_hand_box_is_seen_only_by_the_reverse_direction():
    """The one-sided route on the same inputs gives n_inside = 0 and contact = 0 (no hand vertex is inside the sphere, the nearest is
    16.6 mm away); the reverse direction finds all 42 sphere vertices inside the box, the deepest at the analytic box distance (between the centre's
    8 mm and the box's half height of 10 mm; 9.545 mm for this orientation of the sphere)."""
    tb, hand, R, t, q = sphere_in_box()
    assert tb.no_max == 42 and tb.hand_orient == 1.0
    got = run_sym(tb, hand, [0], R, t, want_sdf=True)
    want = box_sdf(q, HAND_LO, HAND_HI)
    err = np.abs(got["sdf_obj"][0] - want).max()
    print(f"sdf_obj error {err:.3e}  obj_pen_max {1e3 * got['rows'][0, 0]:.6f} mm  wind in [{got['wind_obj'].min():.15f}, {got['wind_obj'].max():.15f}]")
    assert (want < 0).all() and got["counts"][0].tolist() == [42, 42] and err <= 1e-12
    r = got["rows"][0]
    assert abs(r[0] + want.min()) <= 1e-12 and 0.008 < r[0] < 0.010 and abs(r[1] + want.mean()) <= 1e-12 and abs(r[2] + want.max()) <= 1e-12
    assert r[3] == 1.0 and r[4] == 1.0 and np.isnan(r[5:]).all() and np.abs(got["wind_obj"][0] - 1.0).max() <= 1e-12
    one = run_route(tb, hand, [0], R, t, flags=1)
    print(f"one-sided: n_inside {one['counts'][0, 0]}  pen_max {one['rows'][0, 0]}  contact {one['rows'][0, 4]}  min_dist {1e3 * one['rows'][0, 2]:.3f} mm")
    assert one["counts"][0, 0] == 0 and one["rows"][0, 0] == 0.0 and one["rows"][0, 4] == 0.0 and abs(1e3 * one["rows"][0, 2] - 16.6) < 0.05


def test_a_flipped_hand_with_its_orientation_gives_the_same_flags():
    tb, hand, R, t, q = sphere_in_box()
    a = run_sym(tb, hand, [0], R, t, want_sdf=True)
    fl, *_ = sphere_in_box(flip=True)
    assert fl.hand_orient == -1.0 and np.array_equal(fl.hand_faces, tb.hand_faces[:, [0, 2, 1]])
    b = run_sym(fl, hand, [0], R, t, want_sdf=True)
    assert np.array_equal(b["counts"], a["counts"]) and np.array_equal(b["sdf_obj"] < 0, a["sdf_obj"] < 0) and np.abs(b["wind_obj"] - a["wind_obj"]).max() <= 1e-12
    wrong = run_sym(fl, hand, [0], R, t, hand_orient=1.0, want_sdf=True)          # the orientation is the host's: without it nothing is inside
    assert wrong["counts"][0, 0] == 0 and np.abs(wrong["wind_obj"] + a["wind_obj"]).max() <= 1e-12


def test_a_hand_of_one_open_triangle_gives_its_solid_angle_fraction():
    q = np.array([[0, 0, 0], [-0.01, -0.01, -0.01], [1.0, 1.0, 1.0]], F64)              # the corner of the octant; behind it; far in front
    tb = table_of([(q, [[0, 1, 2]])], ONE_TRI)
    assert tb.hand_orient == 1.0 and len(tb.hand_faces) == 1
    got = run_sym(tb, ONE_TRI[0][None], [0], I3, Z3, want_sdf=True)
    w = got["wind_obj"][0]
    assert abs(w[0] - 1 / 8) <= 1e-15 and 0 < w[1] < 1 / 8 and got["counts"][0].tolist() == [0, 3] and (got["sdf_obj"] > 0).all()
    assert abs(got["sdf_obj"][0, 0] - 0.03 / math.sqrt(3)) <= 1e-15 and got["rows"][0, 0] == 0.0 and got["rows"][0, 1] == 0.0 and got["rows"][0, 3] == 0.0
    want = -(math.sqrt(3) / 2 * (0.03 * math.sqrt(2)) ** 2 / 2) * 1 / np.linalg.norm(q[2] - 0.01) ** 2 / (4 * math.pi)      # area x cos / r^2
    assert abs(w[2] - want) <= 2e-3 * abs(want)


def test_an_object_outside_the_hand_has_no_depth_and_contact_follows_the_threshold():
    h = 0.005
    tb = table_of([box_mesh([-h] * 3, [h] * 3)], box_mesh(HAND_LO, HAND_HI))
    hand = box_mesh(HAND_LO, HAND_HI)[0][None]
    gap = 0.004
    t = np.array([[HAND_HI[0] + gap + h, 0.0, 0.0]])                                     # the object's -x face `gap` off the hand's +x face
    want = t[0, 0] + tb.verts[:, 0].astype(F64).min() - HAND_HI[0]
    for thr, contact in ((0.003, 0.0), (0.005, 1.0), (want + 1e-9, 1.0), (want - 1e-9, 0.0)):
        got = run_sym(tb, hand, [0], I3, t, contact_thr=thr)
        r = got["rows"][0]
        assert got["counts"][0].tolist() == [0, 8] and r[0] == 0.0 and r[1] == 0.0 and r[3] == 0.0 and r[4] == contact, (thr, r)
        assert abs(r[2] - want) <= 1e-15 and abs(r[2] - gap) < 1e-8


def test_posing_hand_and_object_by_one_rigid_map_changes_nothing():
    tb = table_of([icosphere(0.012, 1), box_mesh(LO / 4, HI / 4)], box_mesh(HAND_LO, HAND_HI))
    rng = np.random.default_rng(8)
    R, t = np.stack([rotation(1), rotation(2)]), rng.uniform(-0.02, 0.02, (2, 3))
    Rh = np.stack([rotation(3), rotation(4)])
    hand = np.einsum("bij,nj->bni", Rh, box_mesh(HAND_LO, HAND_HI)[0]) + (t + [[0.015, 0.0, 0.0], [0.0, 0.01, 0.005]])[:, None]
    a = run_sym(tb, hand, [0, 1], R, t, want_sdf=True)
    G, g = rotation(9), np.array([0.03, -0.02, 0.5])
    b = run_sym(tb, hand @ G.T + g, [0, 1], G @ R, t @ G.T + g, want_sdf=True)
    for k in ("sdf_obj", "wind_obj"):
        assert np.nanmax(np.abs(a[k] - b[k])) <= 1e-12 and np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
    assert np.abs(a["rows"][:, :5] - b["rows"][:, :5]).max() <= 1e-12 and np.array_equal(a["counts"], b["counts"])
    assert (a["counts"][:, 0] > 0).all() and (a["counts"][:, 0] < a["counts"][:, 1]).all()      # each object partly inside its hand


def test_each_sample_reads_its_own_object_of_a_packed_table():
    meshes = [ONE_TRI, box_mesh(LO / 4, HI / 4), icosphere(0.012, 1)]                    # 3, 8 and 42 vertices
    tb = table_of(meshes, box_mesh(HAND_LO, HAND_HI))
    assert tb.vert_off.tolist() == [0, 3, 11, 53] and tb.no_max == 42
    rng = np.random.default_rng(4)
    rows = np.array([2, 0, 1, -1, 7])                                                    # the last two are clamped to rows 0 and 2
    B = len(rows)
    R, t = np.stack([rotation(int(s)) for s in range(20, 20 + B)]), np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.02, 0.02, (B, 3))
    hand = np.einsum("bij,nj->bni", np.stack([rotation(int(s)) for s in range(40, 40 + B)]), box_mesh(HAND_LO, HAND_HI)[0]) + (t + rng.uniform(-0.01, 0.01, (B, 3)))[:, None]
    got = run_sym(tb, hand, rows, R, t, want_sdf=True)
    n = np.array([42, 3, 8, 3, 42])
    assert got["counts"][:, 1].tolist() == n.tolist() and got["sdf_obj"].shape == (B, 42)
    for k in ("sdf_obj", "wind_obj"):
        assert np.array_equal(np.isnan(got[k]), np.arange(42)[None] >= n[:, None]), k
    for b, r in enumerate([2, 0, 1, 0, 2]):
        alone = run_sym(table_of([meshes[r]], box_mesh(HAND_LO, HAND_HI)), hand[b:b + 1], [0], R[b:b + 1], t[b:b + 1], want_sdf=True)
        assert np.array_equal(alone["sdf_obj"][0], got["sdf_obj"][b, :n[b]]) and np.array_equal(alone["wind_obj"][0], got["wind_obj"][b, :n[b]])
        assert np.array_equal(alone["rows"][0], got["rows"][b], equal_nan=True) and np.array_equal(alone["counts"][0], got["counts"][b])
        assert got["rows"][b, 3] == got["counts"][b, 0] / n[b]
    assert got["counts"][:, 0].max() > 0
    short = run_sym(tb, hand, rows, R, t, want_sdf=True, no_max=5)                      # a smaller no_max: the first 5 vertices of each object
    assert short["counts"][:, 1].tolist() == [5, 3, 5, 3, 5] and np.array_equal(short["sdf_obj"][1], got["sdf_obj"][1, :5], equal_nan=True)


# ------------------------------------------------------------------------------------------------ 2. the metric class through the evaluator
def expected_sym(tb, batches, prefix=""):
    """The float64 measures of the reverse direction and the two-sided ones over all samples, formed by hand from the two routes' rows."""
    one, rev = [], []
    for preds, targs in batches:
        if prefix:
            hand, T = (targs["hand_verts_3d"] + targs["root_joint"][:, None]).double().numpy(), targs["obj_transf"].double().numpy()
            R, t = T[:, :3, :3], T[:, :3, 3]
        else:
            hand, R, t = (preds[k].double().numpy() for k in ("hand_verts_3d_abs", "box_rot_rotmat", "boxroot_3d_abs"))
        rows = tb.rows(targs["obj_idx"]).numpy()
        one.append(run_route(tb, hand, rows, R, t, flags=1)["rows"])
        rev.append(run_sym(tb, hand, rows, R, t)["rows"])
    one, rev = np.concatenate(one), np.concatenate(rev)
    return {prefix + "obj_pen_depth_mm": 1e3 * rev[:, 0].mean(), prefix + "obj_pen_mean_mm": 1e3 * rev[:, 1].mean(), prefix + "obj_min_dist_mm": 1e3 * rev[:, 2].mean(),
            prefix + "obj_inside_frac": rev[:, 3].mean(), prefix + "sym_pen_depth_mm": 1e3 * np.maximum(one[:, 0], rev[:, 0]).mean(),
            prefix + "sym_contact_ratio": np.maximum(one[:, 4], rev[:, 4]).mean()}


def test_symmetric_interaction_metric_on_cpu_tensors_through_the_evaluator():
    from anakin.metrics.interaction import IA_SYM_MEASURES as Alias
    from artiboost_amd.metrics import IA_MEASURES, IA_SYM_MEASURES, Evaluator
    assert Alias is IA_SYM_MEASURES
    tb, p1, t1 = metric_batch(3, 11)
    _, p2, t2 = metric_batch(5, 12)
    m, plain = build_interaction(tb, SYMMETRIC=True, REPORT_GT=True), build_interaction(tb, REPORT_GT=True)
    assert m.symmetric and not plain.symmetric
    ev = Evaluator({}, [m])
    ev_plain = Evaluator({}, [plain])
    for p, t in ((p1, t1), (p2, t2)):
        ev.feed_all(p, t)
        ev_plain.feed_all(p, t)
    got, base = ev.get_measures_all(), ev_plain.get_measures_all()
    print(got)
    # SYMMETRIC false: exactly the one-sided names; SYMMETRIC true: those, with the same values, and the six new ones per group
    assert set(base) == {pre + k for pre in ("", "gt_") for k in IA_MEASURES}
    assert set(got) == set(base) | {pre + k for pre in ("", "gt_") for k in IA_SYM_MEASURES}
    assert all(got[k] == v for k, v in base.items())
    want = dict(expected_sym(tb, [(p1, t1), (p2, t2)]), **expected_sym(tb, [(p1, t1), (p2, t2)], "gt_"))
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-9, (k, got[k], v)
    assert got["obj_pen_depth_mm"] > 1.0 and got["sym_pen_depth_mm"] >= max(got["pen_depth_mm"], got["obj_pen_depth_mm"]) and got["sym_contact_ratio"] >= got["contact_ratio"]
    assert "sym_pen_depth_mm:" in str(ev) and "gt_obj_inside_frac:" in str(ev) and "obj_" not in str(ev_plain) and "sym_" not in str(ev_plain)
    assert m.sums[""].shape == (15,) and plain.sums[""].shape == (9,) and m.sums[""][8] == 8
    ev.reset_all()
    assert ev.get_measures_all() == {} and m.sums == {}
    # a plain and a symmetric metric in one evaluator: the same measures from both, the symmetric one's extra
    both = Evaluator({}, [build_interaction(tb), build_interaction(tb, SYMMETRIC=True)])
    both.feed_all(p1, t1)
    assert set(both.get_measures_all()) == set(IA_MEASURES) | set(IA_SYM_MEASURES)


def test_the_yaml_is_the_interaction_file_with_symmetric_set():
    import yaml
    from artiboost_amd import registry as R
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_sym_mi355x.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_mi355x.yaml")))
    assert cfg["EVALUATOR"][-1].pop("SYMMETRIC") is True and "SYMMETRIC" not in base["EVALUATOR"][-1] and cfg == base
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_sym_mi355x.yaml")))
    m = R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"])[-1]
    assert type(m).__name__ == "InteractionMetric" and m.symmetric and m.table.no_max == 2048 and not m.report_gt
    assert not R.build_evaluator_metric_list(base["EVALUATOR"], base["DATA_PRESET"])[-1].symmetric


# ------------------------------------------------------------------------------------------------ 3. header contract, generated op
def test_header_contract_and_generated_op():
    from artiboost_amd import _lib as L
    from artiboost_amd import gen_torch_ops, kernels
    txt = open(gen_torch_ops.HEADER).read()
    assert re.search(r"@check\s+ab_interaction_sym:", txt) and re.search(r"\bint\s+ab_interaction_sym\s*\(", txt) and re.search(r"\blong\s+ab_interaction_sym_workspace\s*\(", txt)
    assert {"ab_interaction_sym", "ab_interaction_sym_workspace"} <= set(L.declared_symbols())
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    cons = gen_torch_ops.contracts()["ab_interaction_sym"]
    assert any("ab_interaction_sym_workspace(B,Nh,No_max)" in c for c in cons)
    assert [p[1] for p in decl["ab_interaction_sym"]] == ["hand_verts", "hand_faces", "Nh", "Fh", "hand_orient", "obj_verts", "vert_off", "n_obj", "obj_row", "rot", "tsl",
                                                          "B", "No_max", "contact_thr", "rows", "counts", "sdf_obj", "wind_obj", "workspace", "stream"]
    assert [p for p in decl["ab_interaction_sym"] if p[1] in ("obj_row", "hand_orient", "counts")] == [("float", "hand_orient"), ("const int64_t*", "obj_row"), ("int32_t*", "counts")]
    src = open(gen_torch_ops.OUT).read()
    assert 'm.def("interaction_sym(' in src and 'm.impl("interaction_sym", &w_interaction_sym);' in src and "w_interaction_sym_workspace" in src
    for rt, name in (("int", "ab_interaction_sym"), ("long", "ab_interaction_sym_workspace")):
        _, schema, body = gen_torch_ops.schema_and_wrapper(rt, name, decl[name], gen_torch_ops.contracts().get(name, ()))
        assert body in src and f'm.def("{schema}");' in src                     # the committed source is what the generator writes
    for name, col in kernels.IAS_ROW.items():
        assert re.search(rf"#define AB_IAS_{name.upper()} {col}\b", txt), name
    assert re.search(r"#define AB_IAS_ROW 8\b", txt) and sorted(kernels.IAS_ROW.values()) == [0, 1, 2, 3, 4] and kernels.IAS_COUNTS == {"n_obj_inside": 0, "n_obj_verts": 1}
    block = txt[txt.index("Symmetric interaction measures"):txt.index("long ab_interaction_sym_workspace")]
    assert re.search(r"not captured in a hipGraph", block) and "o w > 0.5" in block and "No atomics" in block and "comment block of ab_interaction" in block
    hip = open(os.path.join(ROOT, "artiboost_amd", "csrc", "interact_sym.hip")).read()
    assert "never captured in a hipGraph" in hip and "atomic" not in hip.lower() and '#include "ia_tile.h"' in hip
