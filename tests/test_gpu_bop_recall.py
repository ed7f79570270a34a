"""ab_vsd (csrc/bop_recall.hip) and ab_mspd (csrc/mssd.hip) on the device.

ab_vsd against the stage restatement tests/bop_raster_ref.py: depth images bit-equal, counts equal, errors bit-equal after the same fp32 rounding
-- stages A to D are written so that this holds; there is no tolerance.  B = 3 on a 48 x 40 image (non-square, partial 32 x 32 tiles on both
axes), a 12-triangle box and icospheres of 320 and 1 280 faces.  Then the golden inputs: what the reference's own vsd returned.
ab_mspd against float64 (metrics.mspd_values_torch in float64, which tests/test_bop_recall_host.py holds to the reference's mspd within
1e-9 px): the worst absolute error is printed, and bounded by MSPD_BOUND_PX = 4 x the worst measured over these cases on one MI355X.
fp32 rounding of a chain of 8 - 10 operations at |u| <= 256 px sets the scale (2^-24 x 256 px x 10 = 1.5e-4 px).
Then determinism and independence of the batch, `BOPRecall` on HIP tensors against the class on CPU tensors, the dispatcher's refusals and
one HoNet forward through an evaluator that holds the metric."""
import os

import numpy as np
import pytest
import torch

import bop_raster_ref as RR
from test_bop_recall_host import build_bop, golden, golden_batch, golden_meshes, golden_table
from test_interaction_host import box_mesh, icosphere, rotation, table_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B = 48, 40, 3
TAUS = [float(np.float32(t)) for t in np.arange(0.05, 0.51, 0.05)]
DELTA = float(np.float32(0.015))
MSPD_MEASURED_PX = 1.77e-5       # worst |ab_mspd - float64| over the cases below, measured once on one MI355X
MSPD_BOUND_PX = 4 * MSPD_MEASURED_PX
_CACHE = {}
WORST = {}


def meshes():
    if "meshes" not in _CACHE:
        ms = [box_mesh([-0.03, -0.02, -0.045], [0.03, 0.02, 0.045]), icosphere(0.04, 2), icosphere(0.045, 3)]
        _CACHE["meshes"] = [(np.asarray(v, np.float32), np.asarray(f, np.int32)) for v, f in ms]
        assert [len(f) for _, f in _CACHE["meshes"]] == [12, 320, 1280]
        hv, hf = box_mesh([-0.02, -0.05, -0.01], [0.0, 0.05, 0.01])
        _CACHE["table"] = table_of(_CACHE["meshes"], (hv, hf))
        _CACHE["diam"] = np.asarray([np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)) for v, _ in _CACHE["meshes"]], np.float32)
    return _CACHE["meshes"]


def scene(name):
    """rows, poses, intrinsics, depth_test, occluder of one case (numpy, fp32)."""
    meshes()
    rng = np.random.default_rng(sum(map(ord, name)))
    rows = np.array([0, 1, 2])
    Rg = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    tg = np.stack([rng.uniform(-0.01, 0.01, B), rng.uniform(-0.01, 0.01, B), rng.uniform(0.45, 0.55, B)], 1)
    Re = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    Re[1] = Rg[1]                               # one sample differs by its translation only
    te = tg + rng.uniform(-0.01, 0.01, (B, 3))
    K = np.tile(np.array([[150.0, 0, 23.5], [0, 148.0, 19.25], [0, 0, 1]]), (B, 1, 1))
    K[:, :2, 2] += rng.uniform(-1, 1, (B, 2))
    depth, occ = None, None
    if name == "borders":                       # straddles the right and the bottom border
        tg[:, 0], tg[:, 1] = 0.07, 0.06
        te = tg + rng.uniform(-0.01, 0.01, (B, 3))
    elif name == "est_off":                     # the estimate entirely off-screen: the union is visib_gt
        te[:, 0] = 0.9
    elif name == "both_off":
        te[:, 0], tg[:, 1] = 0.9, -0.9
    elif name == "near":                        # the box so close that triangles cross the near plane (vertices at Z <= 0.01 m)
        rows = np.array([0, 0, 0])
        tg[:, 2], te[:, 2] = [0.04, 0.03, 0.05], [0.045, 0.03, 0.035]
    elif name == "depth_zero":
        depth = np.zeros((B, H, W), np.float32)
    elif name == "plane":                       # a plane through the object's centre over the left half of the image, a wall elsewhere
        depth = np.full((B, H, W), 2.0, np.float32)
        depth[:, :, :24] = tg[:, 2].astype(np.float32)[:, None, None]
        depth[2, ::3] = 0.0                     # and rows without a measurement
    elif name == "hand":                        # the occluder: a thin box 0.2 m in front of the camera, shifted per sample
        occ = np.asarray(box_mesh([-0.02, -0.05, -0.01], [0.0, 0.05, 0.01])[0], np.float32)[None] + np.float32([[[0.0, 0, 0.3]], [[0.01, 0, 0.25]], [[-0.01, 0.01, 0.35]]])
        depth = np.zeros((B, H, W), np.float32)
        depth[0, 10:20] = 0.2                   # a measurement in front of everything on some rows
        assert _CACHE["table"].hand_faces.shape == (12, 3)
    elif name == "identical":
        Re, te = Rg.copy(), tg.copy()
    else:
        assert name == "inside"
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    return dict(rows=rows, Re=f32(Re), te=f32(te), Rg=f32(Rg), tg=f32(tg), K=f32(K), depth=depth, occ=occ)


def run_kernel(s, tb=None, diam=None, want_depth=True, W=W, H=H):
    from artiboost_amd import kernels as Kn
    tb = tb or _CACHE["table"]
    d = tb.on("cuda")
    t = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dt).contiguous()      # noqa: E731
    mv = int((tb.vert_off[1:] - tb.vert_off[:-1]).max())
    out = Kn.vsd(d["obj_verts"], d["obj_faces"], d["vert_off"], d["face_off"], mv, t(s["rows"], torch.int64), t(s["Re"]), t(s["te"]), t(s["Rg"]), t(s["tg"]),
                 t(s["K"]), W, H, DELTA, TAUS, t(diam if diam is not None else _CACHE["diam"]), depth_test=t(s["depth"]), occ_verts=t(s["occ"]),
                 occ_faces=d["hand_faces"] if s["occ"] is not None else None, want_depth=want_depth)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_ref(s):
    return RR.vsd_ref(meshes(), s["rows"], s["Re"], s["te"], s["Rg"], s["tg"], s["K"], W, H, DELTA, TAUS, _CACHE["diam"], depth_test=s["depth"],
                      occ_verts=s["occ"], occ_faces=_CACHE["table"].hand_faces if s["occ"] is not None else None)


CASES = ("inside", "borders", "est_off", "both_off", "near", "depth_zero", "plane", "hand", "identical")


# ------------------------------------------------------------------------------------------------ 1. ab_vsd against the restatement
@pytest.mark.parametrize("name", CASES)
def test_vsd_equals_the_restatement_bit_for_bit(name):
    s = scene(name)
    got, ref = run_kernel(s), run_ref(s)
    c = ref["counts"]
    print(name, "union", c[:, 0].tolist(), "complement", c[:, 1].tolist(), "cost at the first and last tau", c[:, 2].tolist(), c[:, -1].tolist())
    nd = (got["depth"].view(np.uint32) != ref["depth"].view(np.uint32)).sum()
    print(name, "depth words that differ:", int(nd), "| covered pixels est / gt / test:", [int((ref["depth"][:, i] > 0).sum()) for i in range(3)])
    assert nd == 0
    assert np.array_equal(got["counts"], c)
    assert np.array_equal(got["err"].view(np.uint32), ref["err"].view(np.uint32))
    # what the case is about
    if name in ("inside", "borders", "plane", "hand", "depth_zero"):
        assert (c[:, 0] > 0).all() and (ref["depth"][:, 0] > 0).any() and (ref["depth"][:, 1] > 0).any()
    if name == "borders":
        assert (ref["depth"][:, 1, :, -1] > 0).any() and (ref["depth"][:, 1, -1, :] > 0).any()
    if name == "est_off":
        assert not (ref["depth"][:, 0] > 0).any() and (c[:, 0] == (ref["depth"][:, 1] > 0).sum((1, 2))).all() and (ref["err"] == 1).all()
    if name == "both_off":
        assert (c == 0).all() and (ref["err"] == 1).all()
    if name == "near":
        z = RR.pose_points(s["Rg"][1], s["tg"][1], meshes()[0][0])[:, 2]
        assert (z <= RR.NEAR).any() and (z > RR.NEAR).any() and (ref["depth"][:, 1] > 0).any()      # vertices on both sides of the plane: some faces dropped, some drawn
    if name == "plane":
        assert (c[:, 1] > 0).any() and (ref["depth"][2, 2, ::3] == 0).all()
    if name == "hand":
        assert (ref["depth"][:, 2] > 0).any() and (ref["depth"][0, 2, 10:20] == np.float32(0.2)).all()
    if name == "identical":
        assert (c[:, 1:] == 0).all() and (ref["err"] == 0).all() and (c[:, 0] > 0).all()
    if name == "depth_zero":
        none = run_kernel(dict(s, depth=None))
        assert all(np.array_equal(none[k], got[k]) for k in got)                          # no depth_test and an all-zero one are the same thing


def test_vsd_on_the_golden_inputs_gives_what_the_reference_returned():
    g = golden()
    tb = golden_table().set_hand({"v_template": np.asarray(box_mesh([-1, -1, -1], [1, 1, 1])[0], np.float32), "faces": box_mesh([-1, -1, -1], [1, 1, 1])[1]})
    s = dict(rows=g["obj_idx"] - 1, Re=g["rot_est"], te=g["tsl_est"], Rg=g["rot_gt"], tg=g["tsl_gt"], K=g["cam_intr"], depth=g["depth_test"], occ=None)
    got = run_kernel(s, tb=tb, diam=g["diameter"].astype(np.float32), want_depth=False, W=int(g["W"]), H=int(g["H"]))
    assert np.array_equal(got["counts"][:, 0], g["union"]) and np.array_equal(got["counts"][:, 1], g["union"] - g["inter"])
    assert np.array_equal(got["err"], g["vsd"].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 2. ab_mspd against float64
def sym_table():
    """Three objects: the identity alone; 12 rotations about z; 314 rotations about a tilted axis with an offset (crosses the 64-lane chunks)."""
    if "sym" not in _CACHE:
        def rots(n, axis, off):
            axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
            Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            Rs = [np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx for a in 2 * np.pi * np.arange(1, n + 1) / (n + 1)]
            return [(R, (np.eye(3) - R) @ np.asarray(off, np.float64)) for R in Rs]
        sets = [[(np.eye(3), np.zeros(3))], rots(12, [0, 0, 1], [0, 0, 0]), rots(314, [0.2, 1, 0.1], [0.005, -0.003, 0])]
        kmax = 314
        R, t = np.zeros((3, kmax, 3, 3), np.float32), np.zeros((3, kmax, 3), np.float32)
        for i, s in enumerate(sets):
            for k in range(kmax):
                R[i, k], t[i, k] = s[k] if k < len(s) else s[0]
        _CACHE["sym"] = (torch.from_numpy(R), torch.from_numpy(t), torch.tensor([1, 12, 314], dtype=torch.int32))
    return _CACHE["sym"]


def mspd_case(V, points, seed, Bm=6):
    rng = np.random.default_rng(seed)
    can = (rng.uniform(-1, 1, (Bm, V, 3)) * [0.03, 0.045, 0.06]).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (Bm, 1, 1))
    T[:, :3, :3] = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, Bm)])
    T[:, :3, 3] = np.stack([rng.uniform(-0.05, 0.05, Bm), rng.uniform(-0.05, 0.05, Bm), rng.uniform(0.45, 0.6, Bm)], 1)
    Rp = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, Bm)]).astype(np.float32)
    Rp[::2] = T[::2, :3, :3]
    tp = (T[:, :3, 3] + rng.uniform(-0.01, 0.01, (Bm, 3))).astype(np.float32)
    K = np.tile(np.float32([[250.0, 0, 128], [0, 245.0, 120], [0, 0, 1]]), (Bm, 1, 1))          # |u| <= 256 px
    oi = np.array([1, 2, 3, 3, 2, 1])[:Bm]
    a = dict(can=can, T=T, oi=oi, K=K)
    if points:
        a["pts"] = (np.einsum("bij,bvj->bvi", Rp, can) + tp[:, None] + rng.normal(size=(Bm, V, 3)) * 0.003).astype(np.float32)
    else:
        a["Rp"], a["tp"] = Rp, tp
    return a


def run_mspd(a, kernel):
    from artiboost_amd import kernels as Kn
    from artiboost_amd.metrics import mspd_values_torch
    dev, dt = ("cuda", torch.float32) if kernel else ("cpu", torch.float64)
    t = lambda x: torch.as_tensor(x).to(device=dev, dtype=dt).contiguous()      # noqa: E731
    R, tt, cnt = sym_table()
    mode = dict(pred_pts=t(a["pts"])) if "pts" in a else dict(pred_R=t(a["Rp"]), pred_t=t(a["tp"]))
    fn = Kn.mspd if kernel else mspd_values_torch
    out = fn(t(a["can"]), t(a["T"]), torch.as_tensor(a["oi"]).to(dev), R.to(device=dev, dtype=dt), tt.to(device=dev, dtype=dt), cnt.to(dev), t(a["K"]), **mode)
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("V,points", [(8, True), (513, False), (513, True), (1025, False)])
def test_mspd_against_float64(V, points):
    a = mspd_case(V, points, 100 + V + int(points))
    got, ref = run_mspd(a, True), run_mspd(a, False)
    err = np.abs(got - ref).max()
    WORST[(V, points)] = err
    print(f"mspd V={V} {'points' if points else 'rigid'}: float64 {np.round(ref, 4).tolist()} px; worst |device - float64| {err:.3e} px; bound {MSPD_BOUND_PX:.3e} px")
    assert np.isfinite(ref).all() and ref.max() <= 256 and ref.min() > 0
    assert err <= MSPD_BOUND_PX


def test_mspd_is_inf_behind_the_camera_and_for_an_empty_set():
    from artiboost_amd import kernels as Kn
    a = mspd_case(8, False, 5)
    a["tp"][0, 2] = -0.5                                      # the prediction behind the camera
    a["T"][1, 2, 3] = 0.01                                    # the ground truth straddling Z = 0
    got = run_mspd(a, True)
    base = run_mspd(mspd_case(8, False, 5), True)
    assert np.isinf(got[:2]).all() and np.array_equal(got[2:], base[2:])
    R, tt, cnt = sym_table()
    t = lambda x: torch.as_tensor(x).cuda().contiguous()      # noqa: E731
    e = Kn.mspd(t(a["can"]), t(a["T"]), t(a["oi"]), R.cuda(), tt.cuda(), torch.zeros(3, dtype=torch.int32, device="cuda"), t(a["K"]), pred_R=t(a["Rp"]), pred_t=t(a["tp"]))
    assert torch.isinf(e).all()


# ------------------------------------------------------------------------------------------------ 3. determinism, independence of the batch
def test_a_sample_depends_on_neither_its_place_nor_its_batch_nor_the_call():
    s = scene("plane")
    full, again = run_kernel(s), run_kernel(s)
    assert all(np.array_equal(full[k].view(np.uint32) if full[k].dtype == np.float32 else full[k], again[k].view(np.uint32) if again[k].dtype == np.float32 else again[k]) for k in full)
    take = lambda idx: {k: (v[idx] if v is not None else None) for k, v in s.items()}      # noqa: E731
    perm = [2, 0, 1]
    p = run_kernel(take(perm))
    for k in full:
        assert np.array_equal(p[k].view(np.uint32) if p[k].dtype == np.float32 else p[k], (full[k].view(np.uint32) if full[k].dtype == np.float32 else full[k])[perm]), k
    one = run_kernel(take([1]))
    assert np.array_equal(one["counts"][0], full["counts"][1]) and np.array_equal(one["depth"].view(np.uint32)[0], full["depth"].view(np.uint32)[1])
    a = mspd_case(513, False, 9)
    m = run_mspd(a, True)
    assert np.array_equal(m, run_mspd(a, True))
    sub = {k: v[[3, 1]] for k, v in a.items()}
    assert np.array_equal(run_mspd(sub, True), m[[3, 1]])


# ------------------------------------------------------------------------------------------------ 4. the class on HIP tensors
def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def test_metric_on_hip_tensors_matches_the_class_on_cpu_tensors_and_reads_nothing_back():
    from artiboost_amd.metrics import Evaluator
    p, t = golden_batch()
    half = lambda d, s: {k: v[s].contiguous() for k, v in d.items()}      # noqa: E731
    out, hits = {}, {}
    for dev in ("cpu", "cuda"):
        m = build_bop()
        ev = Evaluator({}, [m])
        ev.feed_all(_to(half(p, slice(0, 2)), dev), _to(half(t, slice(0, 2)), dev))
        if dev == "cuda":                                                             # the tables are on the device now: nothing below may wait for it
            p2, t2 = _to(half(p, slice(2, 6)), dev), _to(half(t, slice(2, 6)), dev)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                tensors = m.feed_device(p2, t2, memo={})
                assert len(tensors) == 1 and tensors[0].is_cuda and m._hits.is_cuda and m._hits.shape == (2, 3, 10, 10)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            m.feed_host([x.cpu().numpy() for x in tensors])
        else:
            ev.feed_all(half(p, slice(2, 6)), half(t, slice(2, 6)))
        out[dev], hits[dev] = ev.get_measures_all(), m._hits.cpu().numpy()
    g = golden()
    assert np.array_equal(hits["cuda"][:, 0], hits["cpu"][:, 0]) and hits["cpu"][:, 0].sum() > 0          # VSD hits: exact
    assert np.array_equal(hits["cuda"], hits["cpu"])                                                      # no golden sample is within fp32 reach of a threshold
    for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD"):
        print(f"{k}: cpu {out['cpu'][k]:.6f}  device {out['cuda'][k]:.6f}  reference {float(g['recall.' + k]):.6f}")
        assert abs(out["cuda"][k] - float(g["recall." + k])) <= 1e-12 and out["cuda"][k] == out["cpu"][k]
    # the per-sample values behind them
    m = build_bop()
    val = m.values(_to(p, "cuda"), _to(t, "cuda"))
    assert np.abs(val["mspd"].cpu().numpy() - g["mspd"]).max() <= max(MSPD_BOUND_PX, 1e-3) and np.abs(val["mssd"].cpu().numpy() - g["mssd"]).max() <= 1e-6


def test_one_call_per_batch_through_the_memo(monkeypatch):
    from artiboost_amd import kernels as Kn
    from artiboost_amd.metrics import Evaluator
    calls = []
    real = Kn.vsd
    monkeypatch.setattr(Kn, "vsd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    p, t = golden_batch()
    a = build_bop()
    ev = Evaluator({}, [a])
    ev.feed_all(_to(p, "cuda"), _to(t, "cuda"))
    memo = {}
    a.feed_device(_to(p, "cuda"), _to(t, "cuda"), memo=memo)
    a.feed_device(_to(p, "cuda"), _to(t, "cuda"), memo=memo)
    assert len(calls) == 2 and int(a._cnt.sum()) == 18


# ------------------------------------------------------------------------------------------------ 5. the dispatcher ops' refusals
def test_dispatcher_op_refusals():
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as Kn
    L.lib()
    meshes()
    tb = _CACHE["table"].on("cuda")
    ns = torch.ops.artiboost_hip
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    T, mv = 10, 642
    ws = torch.zeros(int(ns.vsd_workspace(B, mv, 8, W, H, T)), dtype=torch.uint8, device="cuda")
    eye = torch.eye(3, device="cuda").repeat(B, 1, 1).contiguous()
    Kc = torch.tensor([[150.0, 0, 24], [0, 150, 20], [0, 0, 1]], device="cuda").repeat(B, 1, 1).contiguous()
    tz = torch.tensor([[0, 0, 0.5]], device="cuda").repeat(B, 1).contiguous()

    def args(**kw):
        a = dict(obj_verts=tb["obj_verts"], obj_faces=tb["obj_faces"], vert_off=tb["vert_off"], face_off=tb["face_off"], n_obj=3, max_obj_verts=mv,
                 rows=torch.tensor([0, 1, 2], device="cuda"), rot_est=eye, tsl_est=tz, rot_gt=eye, tsl_gt=tz, cam_intr=Kc, B=B, W=W, H=H, depth_test=z(B, H, W),
                 occ_verts=z(B, 8, 3), occ_faces=tb["hand_faces"], Nv=8, Nf=12, delta=0.015, taus_host=torch.tensor(TAUS), T=T, diameter=z(3) + 0.1,
                 normalized_by_diameter=1, counts=torch.zeros(B, 2 + T, dtype=torch.int32, device="cuda"), err=z(B, T), depth_out=z(B, 3, H, W), workspace=ws)
        a.update(kw)
        return list(a.values())
    ns.vsd(*args())                                                              # the well-formed call goes through
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        ns.vsd(*args(rot_est=torch.zeros(B, 9)))
    with pytest.raises(RuntimeError, match="must be a CPU tensor"):
        ns.vsd(*args(taus_host=torch.tensor(TAUS).cuda()))
    with pytest.raises(RuntimeError, match="must be Int"):
        ns.vsd(*args(obj_faces=tb["obj_faces"].long()))
    with pytest.raises(RuntimeError, match="must be Float"):
        ns.vsd(*args(depth_test=z(B, H, W).double()))
    with pytest.raises(RuntimeError, match="'depth_test' holds"):
        ns.vsd(*args(depth_test=z(B, H, W - 1)))
    with pytest.raises(RuntimeError, match="'depth_out' holds"):
        ns.vsd(*args(depth_out=z(B, 2, H, W)))
    with pytest.raises(RuntimeError, match="'counts' holds"):
        ns.vsd(*args(counts=torch.zeros(B, 1 + T, dtype=torch.int32, device="cuda")))
    with pytest.raises(RuntimeError, match="'occ_verts' holds"):
        ns.vsd(*args(occ_verts=z(B, 7, 3)))
    with pytest.raises(RuntimeError, match="bytes"):
        ns.vsd(*args(workspace=ws[:-1]))
    for bad in (dict(T=0), dict(T=17, taus_host=torch.zeros(17), counts=torch.zeros(B, 19, dtype=torch.int32, device="cuda"), err=z(B, 17)), dict(delta=-1.0),
                dict(W=8193, depth_test=None, depth_out=None), dict(occ_faces=None), dict(occ_verts=None, occ_faces=None), dict(err=None), dict(max_obj_verts=0)):
        with pytest.raises(RuntimeError, match="argument error|bytes"):
            ns.vsd(*args(**bad))
    # ab_mspd
    R, tt, cnt = sym_table()
    a = mspd_case(8, False, 5)
    t = lambda x: torch.as_tensor(x).cuda().contiguous()      # noqa: E731
    wm = torch.zeros(int(ns.mspd_workspace(6, 314, 8)), dtype=torch.uint8, device="cuda")
    base = dict(can=t(a["can"]), obj_transf=t(a["T"]), obj_idx=t(a["oi"]), sym_R=R.cuda(), sym_t=tt.cuda(), sym_count=cnt.cuda(), n_obj=3, Kmax=314, pred_R=t(a["Rp"]),
                pred_t=t(a["tp"]), pred_pts=None, cam_intr=t(a["K"]), B=6, V=8, mspd=z(6), workspace=wm)
    ns.mspd(*base.values())
    for kw, pat in ((dict(cam_intr=z(6, 8)), "'cam_intr' holds"), (dict(obj_idx=t(a["oi"]).int()), "must be Long"), (dict(workspace=wm[:-1]), "bytes"),
                    (dict(pred_pts=t(a["can"])), "argument error"), (dict(pred_R=None), "argument error"), (dict(cam_intr=None), "argument error")):
        with pytest.raises(RuntimeError, match=pat):
            ns.mspd(*dict(base, **kw).values())
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="rows"):
        d = _CACHE["table"].on("cuda")
        Kn.vsd(d["obj_verts"], d["obj_faces"], d["vert_off"], d["face_off"], mv, torch.tensor([0, 1, 2], device="cuda", dtype=torch.int32), eye, tz, eye, tz, Kc, W, H,
               DELTA, TAUS, z(3) + 0.1)
    with pytest.raises(ValueError, match="rigid mode"):
        Kn.mspd(t(a["can"]), t(a["T"]), t(a["oi"]), R.cuda(), tt.cuda(), cnt.cuda(), t(a["K"]))


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_honet_forward_through_an_evaluator_that_holds_the_metric():
    import yaml
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import BOPRecall, Evaluator
    from test_gpu_honet import ARCH, PRESET, _batch
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_bop_mi355x.yaml")))
    torch.manual_seed(0)
    model = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32"), preset_cfg=PRESET)[0]
    model.eval()
    batch = _batch(4, 31, N=30)
    T = torch.eye(4).repeat(4, 1, 1)
    T[:, :3, 3] = batch["root_joint"] + torch.tensor([0.03, 0.0, 0.02])
    batch.update(obj_id=torch.tensor([1, 2, 3, 0]), persp_id=torch.tensor([0, 1, 2, 3]), grasp_id=torch.tensor([3, 4, 5, 6]), is_synth=torch.ones(4, dtype=torch.int64),
                 obj_idx=torch.tensor([9, 12, 5, 11]), obj_transf=T)
    with torch.no_grad():
        preds = model(batch)
    preset = dict(cfg["DATA_PRESET"], IMAGE_SIZE=PRESET["IMAGE_SIZE"])                  # the model above takes 128 x 128 crops
    ev = Evaluator(cfg, R.build_evaluator_metric_list(cfg["EVALUATOR"], preset))
    m = ev.metrics_list[-1]
    assert isinstance(m, BOPRecall) and m.depth_test == "hand" and m.image_size == [128, 128] and np.isfinite(m._diam[[4, 8, 10, 11]]).all()
    ev.feed_all(preds, batch, losses={})
    got = ev.get_measures_all()
    print({k: got[k] for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")}, m._cnt.tolist())
    assert all(0.0 <= got[k] <= 1.0 for k in ("AR", "AR_VSD", "AR_MSSD", "AR_MSPD")) and int(m._cnt.sum()) == 4 and {"5.ar", "9.ar", "11.ar", "12.ar"} <= set(got)
    # the same prediction through the class on CPU tensors: the VSD counts are equal, so are its hits
    cpu = R.build_evaluator_metric_list([cfg["EVALUATOR"][-1]], preset)[0]
    pc = {k: v.detach().float().cpu() for k, v in preds.items() if torch.is_tensor(v)}
    vd, vc = m.values(preds, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}), cpu.values(pc, batch)
    assert np.array_equal(vd["vsd_counts"].cpu().numpy(), vc["vsd_counts"].numpy())
    assert np.array_equal(m.hits(vd, torch.device("cuda"))[0][:, 0].cpu().numpy(), cpu.hits(vc, torch.device("cpu"))[0][:, 0].numpy())


def test_print_the_mspd_error_table():
    """(last: the measured errors, for DESIGN.md section 25)"""
    for k, v in WORST.items():
        print(f"mspd V={k[0]} points={k[1]}: worst |device - float64| {v:.3e} px")
    if WORST:
        print(f"worst over the cases {max(WORST.values()):.3e} px; MSPD_MEASURED_PX {MSPD_MEASURED_PX:.3e}; bound {MSPD_BOUND_PX:.3e}")
