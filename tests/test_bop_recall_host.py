"""BOP average recall on the host: the CPU routes of `BOPRecall` (metrics.vsd_values_numpy, mspd_values_torch, the torch
MSSD) and the stage restatement tests/bop_raster_ref.py against tests/golden/bop_recall.npz -- what the reference's own bop_toolkit functions
returned for these inputs (tests/gen_bop_recall_golden.py) --, the diameter fallback, the recall arithmetic with a sample exactly on a
threshold, the two-phase feeds, the header contracts.  The golden batch and the table helpers are shared with tests/test_gpu_bop_recall.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

import bop_raster_ref as RR
from test_interaction_host import table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_G = {}


def golden():
    if not _G:
        g = np.load(os.path.join(ROOT, "tests", "golden", "bop_recall.npz"))
        _G.update({k: g[k] for k in g.files})
    return _G


def golden_meshes():
    g = golden()
    return [(g["verts.0"], g["faces.0"]), (g["verts.1"], g["faces.1"])]


def golden_table():
    return table_of(golden_meshes(), ids=[1, 2])


def golden_batch(dtype=torch.float32):
    """(preds, targs) of the golden inputs; obj_verts_can padded to one length by repeating each mesh's first vertex (a maximum ignores it)."""
    g = golden()
    B = len(g["obj_idx"])
    meshes = golden_meshes()
    V = max(len(v) for v, _ in meshes)
    can = np.stack([np.concatenate([meshes[i - 1][0], np.repeat(meshes[i - 1][0][:1], V - len(meshes[i - 1][0]), 0)]) for i in g["obj_idx"]])
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = g["rot_gt"], g["tsl_gt"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dtype)      # noqa: E731
    preds = {"box_rot_rotmat": t(g["rot_est"]), "boxroot_3d_abs": t(g["tsl_est"]).reshape(B, 1, 3)}
    targs = {"obj_transf": t(T), "obj_idx": torch.as_tensor(g["obj_idx"]), "cam_intr": t(g["cam_intr"]), "obj_verts_can": t(can), "depth": t(g["depth_test"])}
    return preds, targs


def build_bop(table=None, **cfg):
    from artiboost_amd import registry as R
    g = golden()
    base = dict(TYPE="BOPRecall", MODEL_INFO=json.loads(str(g["model_info"])), MAX_SYM_DISC_STEP=float(g["step"]), DEPTH_TEST="key")
    m = R.build_evaluator_metric_list([dict(base, **cfg)], {"CENTER_IDX": 0, "IMAGE_SIZE": [int(g["W"]), int(g["H"])]})[0]
    return m.set_obj_meshes(table if table is not None else golden_table())


def _vsd_cpu(**kw):
    from artiboost_amd.metrics import vsd_values_numpy
    g, tb = golden(), golden_table()
    return vsd_values_numpy(tb.verts, tb.faces, tb.vert_off, tb.face_off, 162, g["obj_idx"] - 1, g["rot_est"], g["tsl_est"], g["rot_gt"], g["tsl_gt"],
                            g["cam_intr"], int(g["W"]), int(g["H"]), float(g["delta"]), [float(t) for t in g["taus"]], g["diameter"].astype(np.float32),
                            depth_test=g["depth_test"], **kw)


# ------------------------------------------------------------------------------------------------ 1. the routes against the reference's numbers
def test_cpu_vsd_route_reproduces_the_reference_exactly():
    g = golden()
    out = _vsd_cpu(want_depth=True)
    c = out["counts"].numpy()
    assert np.array_equal(c[:, 0], g["union"]) and np.array_equal(c[:, 1], g["union"] - g["inter"])
    e64 = np.where(c[:, :1] > 0, (c[:, 2:] + c[:, 1:2]) / np.maximum(c[:, :1], 1).astype(np.float64), 1.0)
    assert np.array_equal(e64, g["vsd"])                                       # the same integers over the same integer, in float64
    assert np.array_equal(out["err"].numpy(), g["vsd"].astype(np.float32))
    assert g["union"].min() > 100 and (g["vsd"][2] == 0).all() and (g["vsd"][5] == 1).all() and 0 < g["vsd"][1, 0] < 1      # the golden is not trivial


def test_restatement_equals_the_reference_and_the_cpu_route():
    g = golden()
    ref = RR.vsd_ref(golden_meshes(), g["obj_idx"] - 1, g["rot_est"], g["tsl_est"], g["rot_gt"], g["tsl_gt"], g["cam_intr"], int(g["W"]), int(g["H"]),
                     float(g["delta"]), [float(t) for t in g["taus"]], g["diameter"].astype(np.float32), depth_test=g["depth_test"])
    assert np.array_equal(ref["err64"], g["vsd"]) and np.array_equal(ref["counts"][:, 0], g["union"])
    out = _vsd_cpu(want_depth=True)
    assert np.array_equal(out["depth"].numpy().view(np.uint32), ref["depth"].view(np.uint32))
    assert np.array_equal(out["counts"].numpy(), ref["counts"])
    # the occluder: a box between the camera and every object
    from test_interaction_host import box_mesh
    ov, of = box_mesh([-0.02, -0.05, 0.3], [0.0, 0.05, 0.32])
    occ = np.repeat(np.asarray(ov, np.float32)[None], len(g["obj_idx"]), 0)
    ref2 = RR.vsd_ref(golden_meshes(), g["obj_idx"] - 1, g["rot_est"], g["tsl_est"], g["rot_gt"], g["tsl_gt"], g["cam_intr"], int(g["W"]), int(g["H"]),
                      float(g["delta"]), [float(t) for t in g["taus"]], g["diameter"].astype(np.float32), depth_test=g["depth_test"], occ_verts=occ, occ_faces=of)
    out2 = _vsd_cpu(want_depth=True, occ_verts=occ, occ_faces=of)
    assert np.array_equal(out2["depth"].numpy().view(np.uint32), ref2["depth"].view(np.uint32)) and np.array_equal(out2["counts"].numpy(), ref2["counts"])
    assert not np.array_equal(ref2["counts"], ref["counts"]) and (ref2["depth"][:, 2] > 0).any()


def _sym_tables_f64():
    from artiboost_amd.criterions import get_symmetry_transformations
    g = golden()
    info = json.loads(str(g["model_info"]))
    syms = [get_symmetry_transformations(info[str(i)], float(g["step"])) for i in (1, 2)]
    kmax = max(len(s) for s in syms)
    R, t = np.zeros((2, kmax, 3, 3)), np.zeros((2, kmax, 3))
    for i, s in enumerate(syms):
        for k in range(kmax):
            x = s[k] if k < len(s) else s[0]
            R[i, k], t[i, k] = x["R"], np.asarray(x["t"]).reshape(3) / 1000.0
    return torch.from_numpy(R), torch.from_numpy(t), torch.tensor([len(s) for s in syms], dtype=torch.int32)


def test_cpu_mspd_route_matches_the_reference_in_float64():
    from artiboost_amd.metrics import mspd_values_torch
    g = golden()
    p, t = golden_batch(torch.float64)
    R, tt, cnt = _sym_tables_f64()
    assert cnt.tolist() == [1, 12]
    got = mspd_values_torch(t["obj_verts_can"], t["obj_transf"], t["obj_idx"], R, tt, cnt, t["cam_intr"], pred_R=p["box_rot_rotmat"],
                            pred_t=p["boxroot_3d_abs"].reshape(-1, 3)).numpy()
    err = np.abs(got - g["mspd"]).max()
    print("mspd float64 route against the reference, px:", err)
    assert err <= 1e-9                                                              # ~1e4 x 2^-53 x 216 px; the two differ in operation order only
    # a point behind the camera in either pose: +inf
    p2 = {k: v.clone() for k, v in p.items()}
    p2["boxroot_3d_abs"][0, 0, 2] = -0.5
    t2 = {k: v.clone() for k, v in t.items()}
    t2["obj_transf"][1, 2, 3] = 0.01
    bad = mspd_values_torch(t2["obj_verts_can"], t2["obj_transf"], t2["obj_idx"], R, tt, cnt, t2["cam_intr"], pred_R=p2["box_rot_rotmat"],
                            pred_t=p2["boxroot_3d_abs"].reshape(-1, 3)).numpy()
    assert np.isinf(bad[:2]).all() and np.array_equal(bad[2:], got[2:])


def test_diameter_fallback_equals_calc_pts_diameter():
    from artiboost_amd.metrics import calc_pts_diameter
    g = golden()
    m = build_bop()
    assert np.array_equal(m._diam, g["diameter"])
    assert calc_pts_diameter(g["verts.1"], block=7) == g["diameter"][1]
    info = json.loads(str(g["model_info"]))
    info["2"]["diameter"] = 81.5                                                    # mm in models_info.json
    assert build_bop(MODEL_INFO=info)._diam.tolist() == [g["diameter"][0], 0.0815]


def test_the_class_on_cpu_tensors_gives_the_reference_recalls():
    g = golden()
    # none of the golden's samples sits within fp32 reach of an MSSD / MSPD threshold (the class runs these two in fp32 here)
    th = np.arange(0.05, 0.51, 0.05)
    d = g["diameter"][g["obj_idx"] - 1]
    assert (np.abs(g["mssd"][:, None] / (th[None] * d[:, None]) - 1) > 1e-4).all()
    assert (np.abs(g["mspd"][:, None] / (np.arange(5, 51, 5)[None] * int(g["W"]) / 640.0) - 1) > 1e-4).all()
    m = build_bop()
    p, t = golden_batch()
    val = m.values(p, t)
    c = val["vsd_counts"].numpy()
    assert np.array_equal(c[:, 0], g["union"]) and np.array_equal(c[:, 1], g["union"] - g["inter"])
    assert np.abs(val["mssd"].numpy() - g["mssd"]).max() <= 1e-6 and np.abs(val["mspd"].numpy() - g["mspd"]).max() <= 1e-3
    m.feed(p, t)
    got = m.get_measures()
    for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD"):
        assert abs(got[k] - float(g["recall." + k])) <= 1e-12, (k, got[k])
    for k in ("vsd", "mssd", "mspd"):
        assert np.allclose(got["recall_" + k], g["recall." + k], atol=1e-12) and isinstance(got["recall_" + k], list)
    assert set(k for k in got if k.endswith(".ar")) == {"1.ar", "2.ar"} and abs((got["1.ar"] + got["2.ar"]) / 2 - got["AR"]) < 1e-12      # three samples each
    assert "AR_VSD:" in str(m)


# ------------------------------------------------------------------------------------------------ 2. recall arithmetic
def test_recall_arithmetic_is_strict_below_the_threshold():
    m = build_bop()
    T = len(m.taus)
    # union 20: comp + cost = 1, 2, 3 -> e = 0.05, 0.1, 0.15 in float64, as bop_toolkit forms them.  np.arange(0.05, 0.51, 0.05) holds
    # 0.05, 0.1 and 0.15000000000000002: the first two samples sit exactly on a threshold and are NOT hits there; the third is below "0.15".
    counts = torch.tensor([[20, 1] + [0] * T, [20, 2] + [0] * T, [20, 1] + [2] * T, [0, 0] + [0] * T], dtype=torch.int32)
    d = float(m._diam[0])
    p0 = float(m.thresholds[2][0])
    val = dict(obj_idx=torch.tensor([1, 1, 1, 1]), vsd_counts=counts, mssd=torch.tensor([0.05 * d, np.nextafter(0.05 * d, 0), 0.32 * d, 1.0], dtype=torch.float64),
               mspd=torch.tensor([p0, np.nextafter(p0, 0), 3.1, 1e9], dtype=torch.float64))
    h, oi = m.hits(val, torch.device("cpu"))
    assert oi.tolist() == [0, 0, 0, 0] and h.shape == (4, 3, T, 10)
    assert h[0, 0, 0].tolist() == [0] + [1] * 9 and h[1, 0, 0].tolist() == [0, 0] + [1] * 8 and h[2, 0, 0].tolist() == [0, 0] + [1] * 8 and h[3, 0].sum() == 0
    assert float(BOP19()[2]) > 0.15 and h[0, 0].sum() == 9 * T
    assert h[0, 1, 0].tolist() == [0] + [1] * 9 and h[1, 1, 0].tolist() == [1] * 10 and h[2, 1, 0].sum() == 4 and h[3, 1].sum() == 0 and h[:, 1, 1:].sum() == 0
    assert h[0, 2, 0].tolist() == [0] + [1] * 9 and h[1, 2, 0].tolist() == [1] * 10 and h[2, 2, 0].tolist() == [0] * 8 + [1, 1] and h[3, 2].sum() == 0
    # MSPD thresholds scale with the image width: 48 / 640 x (5 .. 50)
    assert np.allclose(m.thresholds[2], 0.075 * np.arange(5, 51, 5)) and np.array_equal(m.thresholds[0], BOP19()) and m.delta == 0.015


def BOP19():
    from artiboost_amd.metrics import BOP19_STEPS
    return BOP19_STEPS


def test_two_phase_feeds_equal_the_blocking_feed_and_a_bare_batch_is_skipped_once(caplog):
    import logging
    from artiboost_amd.metrics import Evaluator
    p, t = golden_batch()
    half = lambda d, s: {k: v[s] for k, v in d.items()}      # noqa: E731
    a, b = build_bop(), build_bop()
    ev = Evaluator({}, [a])
    ev.feed_all(half(p, slice(0, 2)), half(t, slice(0, 2)))
    ev.feed_all(half(p, slice(2, 6)), half(t, slice(2, 6)))
    b.feed(p, t)
    assert ev.get_measures_all() == b.get_measures() and a.count == b.count == 6
    bare = {k: v for k, v in t.items() if k != "cam_intr"}
    with caplog.at_level(logging.WARNING, logger="anakin"):
        ev.feed_all(p, bare)
        ev.feed_all(p, bare)
    assert len([r for r in caplog.records if "cam_intr" in r.getMessage()]) == 1 and a.count == 6
    a.reset()
    assert a.get_measures() == {}


def test_depth_test_none_and_hand_modes_on_cpu_tensors():
    from test_interaction_host import box_mesh
    g = golden()
    p, t = golden_batch()
    m = build_bop(DEPTH_TEST="none")
    c = m.values(p, {k: v for k, v in t.items() if k != "depth"})["vsd_counts"].numpy()
    ref = RR.vsd_ref(golden_meshes(), g["obj_idx"] - 1, g["rot_est"], g["tsl_est"], g["rot_gt"], g["tsl_gt"], g["cam_intr"], int(g["W"]), int(g["H"]),
                     float(g["delta"]), [float(x) for x in g["taus"]], g["diameter"].astype(np.float32))
    assert np.array_equal(c, ref["counts"])
    hv, hf = box_mesh([-0.02, -0.05, -0.01], [0.0, 0.05, 0.01])
    tb = table_of(golden_meshes(), (hv, hf), ids=[1, 2])
    mh = build_bop(tb, DEPTH_TEST="hand")
    B = len(g["obj_idx"])
    root = np.tile(np.float32([0.0, 0.0, 0.31]), (B, 1))
    th = dict(t, hand_verts_3d=torch.from_numpy(np.repeat(np.asarray(hv, np.float32)[None], B, 0)), root_joint=torch.from_numpy(root))
    ch = mh.values(p, th)["vsd_counts"].numpy()
    occ = np.asarray(hv, np.float32)[None] + root[:, None]
    refh = RR.vsd_ref(golden_meshes(), g["obj_idx"] - 1, g["rot_est"], g["tsl_est"], g["rot_gt"], g["tsl_gt"], g["cam_intr"], int(g["W"]), int(g["H"]),
                      float(g["delta"]), [float(x) for x in g["taus"]], g["diameter"].astype(np.float32), occ_verts=occ, occ_faces=tb.hand_faces)
    assert np.array_equal(ch, refh["counts"]) and not np.array_equal(ch, c)


# ------------------------------------------------------------------------------------------------ 3. the boundary
def test_contracts_parse_and_the_declarations_match_the_wrappers():
    from artiboost_amd import _lib as L
    from artiboost_amd import gen_torch_ops
    txt = open(os.path.join(ROOT, "include", "artiboost_hip.h")).read()
    for name in ("ab_mspd", "ab_vsd"):
        assert re.search(rf"@check\s+{name}:", txt) and re.search(rf"\bint\s+{name}\s*\(", txt) and re.search(rf"\blong\s+{name}_workspace\s*\(", txt)
    assert {"ab_mspd", "ab_mspd_workspace", "ab_vsd", "ab_vsd_workspace"} <= set(L.declared_symbols())
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    cons = gen_torch_ops.contracts()
    lines = gen_torch_ops.checks_for("ab_vsd", decl["ab_vsd"][:-1], cons["ab_vsd"])
    assert any("ck_host" in l and "taus_host" in l for l in lines) and any("ab_vsd_workspace(B,max_obj_verts,Nv,W,H,T)" in c for c in cons["ab_vsd"])
    assert any("depth_out" in c and "B*3*H*W" in c for c in cons["ab_vsd"])
    gen_torch_ops.checks_for("ab_mspd", decl["ab_mspd"][:-1], cons["ab_mspd"])
    assert any(c.startswith("bytes workspace") for c in cons["ab_mspd"]) and ("const float*", "cam_intr") in decl["ab_mspd"]
    _, schema, body = gen_torch_ops.schema_and_wrapper("int", "ab_vsd", decl["ab_vsd"], cons["ab_vsd"])
    assert "Tensor(a!)? counts" in schema and "float delta" in schema and "ab_vsd(" in body
    assert "w_vsd(" in open(os.path.join(ROOT, "artiboost_amd", "csrc", "torch_ops_gen.cpp")).read()      # the committed translation unit is current
    # the constants of stage A, stated three times: header, package, restatement
    from artiboost_amd import kernels as K
    assert re.search(r"#define AB_VSD_NEAR 0\.01f", txt) and re.search(r"#define AB_VSD_RANGE 4194304\b", txt) and re.search(r"#define AB_VSD_MAX_TAUS 16\b", txt)
    assert (K.VSD_NEAR, K.VSD_RANGE, K.VSD_MAX_TAUS) == (0.01, 4194304, 16) and float(RR.NEAR) == float(np.float32(0.01)) and RR.RANGE == 4194304
    lib = L.cdll()
    assert lib.ab_mspd_workspace(3, 65, 4000) == 3 * 2 * 4 and lib.ab_vsd_workspace(3, 162, 8, 48, 40, 10) == 3 * (2 * 162 + 8) * 16 + 3 * 4 * 12 * 4


def test_ar_still_refuses_vsd_and_mspd_and_points_at_bop_recall():
    from artiboost_amd import metrics as M
    g = golden()
    for k in ("USE_VSD", "USE_MSPD"):
        with pytest.raises(NotImplementedError):
            M.AR(USE_MSSD=True, MODEL_INFO=json.loads(str(g["model_info"])), **{k: True})
    assert "BOPRecall" in M.AR.__doc__ and M.METRIC.get("BOPRecall") is M.BOPRecall
