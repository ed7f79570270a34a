"""MSSD (AR, ValMetricAR2) with each object's TRUE symmetry set, and the two-phase feeds of the PCK family and ValMetricAR2 -- the parts
that need no GPU.  Golden: tests/golden/mssd.npz = the reference's own MSSD.feed and ValMetricAR2 on seeded inputs
(tests/gen_mssd_golden.py): four objects with sets of 1, 2, 12 and 24 transforms, of which the two with a continuous symmetry do not
contain the identity (BOP enumerates the discretised rotations from i = 1).  `mssd_f64` below is the float64 restatement the GPU tests
(tests/test_gpu_mssd.py) share.

Bound: 2e-6 m (the bound tests/test_gpu_honet.py holds positions to).  Measured: the CPU route is within 3.2e-8 m of the golden and of
the restatement."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mssd.npz")
EVAL_GOLD = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
TOL_M = 2e-6
STEP, CENTER_IDX = 0.25, 9
AR_TAGS = [(pts, cen, ycb) for pts in "vc" for cen in (0, 1) for ycb in (0, 1)]


def golden():
    g = np.load(GOLD)
    t = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("t.")}
    p = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")}
    return g, p, t, json.loads(str(g["model_info"]))


def cfg_for(info, pts="v", cen=0, ycb=0, step=STEP):
    return dict(USE_MSSD=True, MODEL_INFO=info, MAX_SYM_DISC_STEP=step, MSSD_USE_CORNERS=pts == "c", MSSD_USE_CENTER_IDX=bool(cen),
                USE_HO3D_YCB=bool(ycb), DATA_PRESET={"CENTER_IDX": CENTER_IDX})


def true_sets(base):
    """[(R [K,3,3], t [K,3])] float64, one per object: the first sym_count entries of a _MSSDBase table (what the kernel is given)."""
    return [(base.R[i, :c].double().cpu().numpy(), base.t[i, :c, :, 0].double().cpu().numpy()) for i, c in enumerate(base.sym_count.tolist())]


def mssd_f64(can, transf, obj_idx, sets, pred_R=None, pred_t=None, pred_pts=None, center=None, ycb=False):
    """bopAR.py:131-175 restated in float64 with every object's own set: min over the set of max over the points of
    || R_gt sym(can) + t_gt - pred - c ||.  obj_idx 1-based, clamped into the table; ycb: sym(x) = ext (S.R (ext x) + S.t)."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)      # noqa: E731
    can, transf, pred_R, pred_t, pred_pts, center = f(can), f(transf), f(pred_R), f(pred_t), f(pred_pts), f(center)
    ext = np.diag([1.0, -1.0, -1.0]) if ycb else np.eye(3)
    out = np.zeros(can.shape[0])
    for b in range(can.shape[0]):
        R, t = sets[min(max(int(obj_idx[b]) - 1, 0), len(sets) - 1)]
        sym = (np.einsum("kij,vj->kvi", R, can[b] @ ext.T) + t[:, None]) @ ext.T
        gt = sym @ transf[b, :3, :3].T + transf[b, :3, 3]
        pred = pred_pts[b] if pred_pts is not None else can[b] @ pred_R[b].reshape(3, 3).T + pred_t[b].reshape(3)
        d = gt - pred[None] - (center[b] if center is not None else 0.0)
        out[b] = np.sqrt((d * d).sum(-1)).max(1).min()
    return out


def restated(p, t, info, pts, cen, ycb):
    """The float64 value of every golden sample, from the un-folded table of a plain _MSSDBase."""
    import artiboost_amd.metrics as M
    sets = true_sets(M._MSSDBase(**cfg_for(info)))
    c = (t["root_joint"] - p["joints_3d_abs"][:, CENTER_IDX]).numpy() if cen else None
    if pts == "c":
        return mssd_f64(t["corners_can"], t["obj_transf"], t["obj_idx"], sets, pred_pts=p["corners_3d_abs"], center=c, ycb=bool(ycb))
    return mssd_f64(t["obj_verts_can"], t["obj_transf"], t["obj_idx"], sets, pred_R=p["box_rot_rotmat"], pred_t=p["boxroot_3d_abs"], center=c,
                    ycb=bool(ycb))


def check_golden_measures(g, p, t, info, label=""):
    """AR and ValMetricAR2 fed the golden batch on the tensors' device, against the reference's recorded results.  -> max error in metres."""
    import artiboost_amd.metrics as M
    worst = 0.0
    for pts, cen, ycb in AR_TAGS:
        tag = f"ar.{pts}.c{cen}.y{ycb}"
        a = M.AR(**cfg_for(info, pts, cen, ycb))
        _, v = a.mssd.values(p, t)
        err = float(np.abs(v.double().cpu().numpy() - g[f"{tag}.sample"]).max())
        print(f"{label}{tag}: max |route - reference| per sample = {err:.3e} m")
        worst = max(worst, err)
        assert err <= TOL_M, (tag, err)
        a.feed(p, t)
        meas = a.get_measures()
        assert sorted(meas) == [str(k) for k in g[f"{tag}.keys"]]
        np.testing.assert_allclose([meas[k] for k in sorted(meas)], g[f"{tag}.vals"], rtol=0, atol=TOL_M * 1000.0, err_msg=tag)      # mm
    for pts in "vc":
        for ycb in (0, 1):
            tag = f"val.{pts}.y{ycb}"
            m = M.ValMetricAR2(**cfg_for(info, pts, 0, ycb))
            m.feed(p, t)
            avg = m.get_measures_averaged()
            assert [list(k) for k in sorted(avg)] == g[f"{tag}.ids"].tolist(), tag
            got = np.array([avg[k] for k in sorted(avg)], np.float64)
            worst = max(worst, float(np.abs(got - g[f"{tag}.vals"]).max()) / 1000.0)
            np.testing.assert_allclose(got, g[f"{tag}.vals"], rtol=0, atol=TOL_M * 1000.0, err_msg=tag)
            assert m.get_measures()["mssd"] is m.storage
    return worst


def test_cpu_route_reproduces_the_reference_and_the_float64_true_set_restatement():
    """Fails before this change: the identity-padded table scored the perfectly predicted samples 2 and 4 of the 12-set object 0.0 m,
    the reference 0.0275 m and 0.0271 m."""
    import artiboost_amd.metrics as M
    g, p, t, info = golden()
    assert g["ar.v.c0.y0.sample"][2] > 0.02 and g["ar.v.c0.y0.sample"][4] > 0.02 and g["ar.v.c0.y0.sample"][0] == 0.0
    worst = check_golden_measures(g, p, t, info, "cpu ")
    for pts, cen, ycb in AR_TAGS:
        _, v = M._MSSDBase(**cfg_for(info, pts, cen, ycb)).values(p, t)
        want = restated(p, t, info, pts, cen, ycb)
        err = float(np.abs(v.double().numpy() - want).max())
        worst = max(worst, err)
        assert err <= TOL_M, (pts, cen, ycb, err)
        assert float(np.abs(want - g[f"ar.{pts}.c{cen}.y{ycb}.sample"]).max()) <= TOL_M        # the restatement itself against the reference
    print(f"cpu route: max error {worst:.3e} m (bound {TOL_M:.1e})")


def test_table_keeps_true_counts_and_padding_a_row_changes_no_value():
    import artiboost_amd.metrics as M
    g, p, t, info = golden()
    full = M._MSSDBase(**cfg_for(info))
    assert full.sym_count.dtype == torch.int32 and full.sym_count.tolist() == [1, 2, 12, 24] and tuple(full.R.shape) == (4, 24, 3, 3)
    for i, c in enumerate(full.sym_count.tolist()):
        assert torch.equal(full.R[i, c:], full.R[i, :1].expand(24 - c, 3, 3)) and torch.equal(full.t[i, c:], full.t[i, :1].expand(24 - c, 3, 1))
    assert not torch.equal(full.R[2, 0], torch.eye(3))                                   # the continuous set starts at the first rotation, not at the identity
    # objects 1 and 2 alone: a table of Kmax = 2 -- the same samples in the 24-wide table give the same bits
    short = M._MSSDBase(**cfg_for({k: info[k] for k in ("1", "2")}))
    assert tuple(short.R.shape) == (2, 2, 3, 3)
    keep = torch.tensor([b for b, o in enumerate(t["obj_idx"].tolist()) if o <= 2])
    ps, ts = {k: v[keep] for k, v in p.items()}, {k: v[keep] for k, v in t.items()}
    assert torch.equal(short.values(ps, ts)[1], full.values(ps, ts)[1]) and torch.equal(full.values(ps, ts)[1], full.values(p, t)[1][keep])
    # the folded USE_HO3D_YCB table: sign flips of the plain one
    ycb = M._MSSDBase(**cfg_for(info, ycb=1))
    ext = torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    assert torch.equal(ycb.R, ext @ full.R @ ext) and torch.equal(ycb.t, ext @ full.t)


def _eval_batches():
    g = np.load(EVAL_GOLD)
    t = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("t.")}
    p = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("p.")}
    info = json.loads(str(g["model_info"]))
    B = t["obj_idx"].shape[0]
    cuts = [(0, 5), (5, 8), (8, B)]
    return info, [({k: v[a:b] for k, v in p.items()}, {k: v[a:b] for k, v in t.items()}) for a, b in cuts]


def eval_metric_list(info):
    import artiboost_amd.metrics as M
    ar = dict(USE_MSSD=True, MODEL_INFO=info, MAX_SYM_DISC_STEP=0.25, MSSD_USE_CORNERS=True, DATA_PRESET={"CENTER_IDX": 0})
    return [M.Hand3DPCKMetric(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=20), M.Obj3DPCKMetric(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=20), M.AR(**ar),
            M.ValMetricAR2(**ar), M.Mean3DEPE(VAL_KEYS=["joints_3d_abs"], MILLIMETERS=True)]


def same_measures(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            assert sorted(x) == sorted(y) and all(np.array_equal(np.asarray(x[i]), np.asarray(y[i])) for i in x), k
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (k, x, y)


def test_two_phase_feeds_exist_and_an_evaluator_equals_per_batch_feeds_exactly():
    import artiboost_amd.metrics as M
    info, batches = _eval_batches()
    for cls in (M.PCKMetric, M.ValMetricAR2):
        assert "feed_device" in vars(cls) and "feed_host" in vars(cls), cls
    # the parts: distances and mask of the PCK family, ids / obj_idx / mm values of ValMetricAR2
    p, t = batches[0]
    pck = M.Hand3DPCKMetric(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=20)
    dist, vis = pck.feed_device(p, t)
    assert dist.dtype == torch.float32 and vis.dtype == torch.uint8 and tuple(dist.shape) == tuple(vis.shape) == (5, 21)
    want = torch.sqrt(torch.sum((p["joints_3d"] - t["joints_3d"]) ** 2, dim=-1)).numpy()
    mask = t["joints_vis"].numpy().astype(bool)
    pck.feed(p, t)
    assert pck.count == 5 and all(pck.data[i] == want[mask[:, i], i].tolist() for i in range(21))      # the same numbers, bit for bit
    val = eval_metric_list(info)[3]
    ids, oi, mm = val.feed_device(p, t)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (5, 4) and oi.dtype == torch.int64 and mm.dtype == torch.float32
    assert torch.equal(ids[:, 3], t["is_synth"].long()) and torch.equal(oi, t["obj_idx"]) and torch.equal(mm, val.mssd.values(p, t)[1] * 1000.0)
    # stable obj_idx order, last write wins: a later class overwrites an earlier one on a repeated triplet, whatever the batch order
    val.reset()
    val.feed_host([np.array([[1, 2, 3, 1], [1, 2, 3, 1], [1, 2, 3, 0], [4, 4, 4, 1]]), np.array([3, 1, 3, 2]), np.array([30.0, 10.0, 99.0, 20.0], np.float32)])
    assert val.storage == {(1, 2, 3): np.float32(30.0), (4, 4, 4): np.float32(20.0)}
    assert M.ValMetricAR2(USE_MSSD=False).feed_device(p, t) is None
    # an Evaluator against blocking per-batch feeds
    ev = M.Evaluator({}, eval_metric_list(info))
    ref = eval_metric_list(info)
    for p, t in batches:
        ev.feed_all(p, t, {})
        for m in ref:
            m.feed(p, t)
    got = ev.get_measures_all()
    want = {}
    for m in ref:
        want.update(m.get_measures())
    same_measures(got, want)
    assert str(ev) == " | ".join(s for s in (str(m) for m in ref) if s)


def test_ab_mssd_contract_parses_and_its_declaration_matches_the_wrapper():
    from artiboost_amd import _lib, gen_torch_ops, kernels
    txt = open(os.path.join(ROOT, "include", "artiboost_hip.h")).read()
    gen = open(os.path.join(ROOT, "artiboost_amd", "csrc", "torch_ops_gen.cpp")).read()
    cons = gen_torch_ops.contracts()
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    assert re.search(r"\bint\s+ab_mssd\s*\(", txt) and re.search(r"\blong\s+ab_mssd_workspace\s*\(", txt) and re.search(r"@check\s+ab_mssd:", txt)
    for name in ("ab_mssd", "ab_mssd_workspace"):
        assert hasattr(_lib.cdll(), name) and 'm.impl("%s", &w_%s);' % (name[3:], name[3:]) in gen, name
    params = decl["ab_mssd"]
    assert params[-1] == ("void*", "stream") and ("const int64_t*", "obj_idx") in params and ("const int32_t*", "sym_count") in params
    gen_torch_ops.checks_for("ab_mssd", params[:-1], cons["ab_mssd"])                  # asserts on unknown names / unreadable clauses
    assert any(cl.startswith("bytes workspace") for cl in cons["ab_mssd"]) and any("sym_count" in cl for cl in cons["ab_mssd"])
    # the wrapper takes the declaration's input pointers, in its order; it derives the integers and allocates the output and the workspace
    inputs = [pn for ty, pn in params if ty.startswith("const") and ty.endswith("*")]
    assert inputs == ["can", "obj_transf", "obj_idx", "sym_R", "sym_t", "sym_count", "pred_R", "pred_t", "pred_pts", "center"]
    assert list(inspect.signature(kernels.mssd).parameters) == inputs + ["out"]
    assert [pn for ty, pn in params if not ty.endswith("*")] == ["n_obj", "Kmax", "B", "V"]
    assert [pn for ty, pn in params if ty.endswith("*") and not ty.startswith("const")] == ["mssd", "workspace", "stream"]
    # one fp32 partial per sample and chunk of 64 symmetries
    lib = _lib.cdll()
    assert lib.ab_mssd_workspace(3, 64, 10) == 3 * 4 and lib.ab_mssd_workspace(3, 65, 4000) == 3 * 2 * 4 and lib.ab_mssd_workspace(64, 628, 8) == 64 * 10 * 4
    with pytest.raises(RuntimeError):                                                  # no quiet fall-back: CPU tensors are refused by the wrapper
        kernels.mssd(torch.zeros(1, 4, 3), torch.eye(4)[None], torch.ones(1, dtype=torch.int64), torch.eye(3).reshape(1, 1, 3, 3),
                     torch.zeros(1, 1, 3), torch.ones(1, dtype=torch.int32), pred_R=torch.eye(3)[None], pred_t=torch.zeros(1, 3))
