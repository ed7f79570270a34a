"""The leaderboard mesh metrics on the host: MeanAlignedEPE, MeshFScore and MeanSurfaceDist build from config
dicts and from the new YAML; the torch (CPU-tensor) route against an independent float64 numpy restatement (numpy.linalg.svd, a brute-force
distance matrix, strict <); averaging over feeds; the evaluator's two feeding modes; absent keys; the header contract and the generated op.

The restatement (`mesh_ref64`) and the inputs (`draw_case`) are shared with tests/test_gpu_mesh_metrics.py.

Bounds of the fp32 torch route against float64 (both read the same fp32 inputs):
  unaligned distances and means   16 x 2^-24 x max |coordinate| of the case: the root addition, three differences and the length each round
                                  once at the size of a coordinate; 16 ulp leaves room for all of them and for the mean's summation.
  aligned quantities              64 x 2^-24 x max |coordinate|: P' = s R Pc + centroid(G) inherits the error of R, the orthogonal polar
                                  factor of the 3x3 correlation, whose condition number is 2 / (sigma_2 + sigma_3) of the normalised
                                  correlation -- below 10 for every cloud drawn here (a flat hand box: sigma ~ (0.85, 0.45, 0.13); the
                                  coplanar target has sigma_3 = 0 but sigma_2 stays) -- acting on correlation entries that carry a few ulp
                                  each, and is applied to |Pc| <= 0.2 m, less than half the largest coordinate; 64 ulp of the largest
                                  coordinate (2 um at 0.5 m) covers 10 x that with the unaligned roundings on top.
  counts                          a point whose float64 distance lies within the distance bound of a threshold may fall on either side."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
THR = (0.005, 0.015)
ROW = {"epe": 0, "ra_epe": 1, "pa_epe": 2, "scale": 3, "mean_pg": 4, "mean_gp": 5, "pa_mean_pg": 6, "pa_mean_gp": 7, "f": 8, "pa_f": 12}
BOX = np.array([0.18, 0.10, 0.03])
SHAPES = [(5, 21, 21), (5, 778, 778), (3, 257, 63)]
KINDS5 = ("generic", "mirrored", "near", "coplanar", "generic")


def draw_case(B, N, M, seed, kinds=None, with_root=True):
    """-> pred [B,N,3], targ [B,M,3], root [B,3] or None (fp32).  Target clouds uniform in a 0.18 x 0.10 x 0.03 m box near z = 0.5 m.  N == M:
    the prediction is the target + N(0, 4 mm) per coordinate, or by `kinds`: `mirrored` (the target mirrored in x about its centroid,
    + N(0, 0.1 mm)), `near` (1 um noise), `coplanar` (a target with z = const, 4 mm noise).  N != M: an independent cloud of the same box,
    shifted by a few millimetres."""
    rng = np.random.default_rng(seed)
    kinds = kinds or ["generic"] * B
    rel = (rng.random((B, M, 3)) - 0.5) * BOX
    for b, k in enumerate(kinds):
        if k == "coplanar":
            rel[b, :, 2] = 0.0078125
    root = np.array([0.02, -0.03, 0.5]) + 0.02 * rng.standard_normal((B, 3))
    G = rel + root[:, None]
    if N == M:
        pred = G + 0.004 * rng.standard_normal((B, N, 3))
        for b, k in enumerate(kinds):
            if k == "mirrored":
                c = G[b].mean(0)
                pred[b] = (G[b] - c) * [-1.0, 1.0, 1.0] + c + 1e-4 * rng.standard_normal((N, 3))
            elif k == "near":
                pred[b] = G[b] + 1e-6 * rng.standard_normal((N, 3))
    else:
        pred = (rng.random((B, N, 3)) - 0.5) * BOX + root[:, None] + 0.003 * rng.standard_normal((B, 1, 3))
    if with_root:
        return pred.astype(np.float32), rel.astype(np.float32), root.astype(np.float32)
    return pred.astype(np.float32), G.astype(np.float32), None


def _nn64(Q, G):
    D = np.sqrt(((Q[:, None, :] - G[None, :, :]) ** 2).sum(-1))
    return D.min(1), D.min(0)


def mesh_ref64(pred, targ, root, center_idx=-1, thresholds=THR):
    """The definitions in float64 numpy on the fp32 inputs, one sample at a time.  -> dict: rows [B,16] (NaN where undefined), counts
    [B,T,4], d_pg / d_gp / pa_d_pg / pa_d_gp, aligned [B,N,3] (N == M >= 3), pa_epe_proper [B] (the same fit restricted to proper rotations)."""
    P = np.asarray(pred, F64)
    G = np.asarray(targ, F64) + (0.0 if root is None else np.asarray(root, F64)[:, None])
    B, N, M, T = P.shape[0], P.shape[1], G.shape[1], len(thresholds)
    rows, counts = np.full((B, 16), np.nan), np.zeros((B, T, 4), np.int64)
    o = dict(rows=rows, counts=counts, d_pg=np.zeros((B, N)), d_gp=np.zeros((B, M)), pa_d_pg=np.full((B, N), np.nan), pa_d_gp=np.full((B, M), np.nan),
             aligned=np.full((B, N, 3), np.nan), pa_epe_proper=np.full(B, np.nan))
    for b in range(B):
        scans = [("", P[b])]
        if N == M:
            rows[b, 0] = np.linalg.norm(P[b] - G[b], axis=1).mean()
            if center_idx >= 0:
                rows[b, 1] = np.linalg.norm((P[b] - P[b, center_idx]) - (G[b] - G[b, center_idx]), axis=1).mean()
        if N == M and N >= 3:
            mp, mg = P[b].mean(0), G[b].mean(0)
            Pc, Gc = P[b] - mp, G[b] - mg
            U, S, Vt = np.linalg.svd(Gc.T @ Pc)
            s = S.sum() / (Pc ** 2).sum()
            Pa = s * Pc @ (U @ Vt).T + mg
            rows[b, 2], rows[b, 3], o["aligned"][b] = np.linalg.norm(Pa - G[b], axis=1).mean(), s, Pa
            D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])          # Kabsch / Umeyama: the determinant corrected
            o["pa_epe_proper"][b] = np.linalg.norm(((S * np.diag(D)).sum() / (Pc ** 2).sum()) * Pc @ (U @ D @ Vt).T + mg - G[b], axis=1).mean()
            scans.append(("pa_", Pa))
        for k, (pre, Q) in enumerate(scans):
            d_pg, d_gp = _nn64(Q, G[b])
            o[pre + "d_pg"][b], o[pre + "d_gp"][b] = d_pg, d_gp
            rows[b, ROW[pre + "mean_pg"]], rows[b, ROW[pre + "mean_gp"]] = d_pg.mean(), d_gp.mean()
            for t, thr in enumerate(thresholds):
                counts[b, t, 2 * k], counts[b, t, 2 * k + 1] = (d_pg < thr).sum(), (d_gp < thr).sum()
                pr, rc = counts[b, t, 2 * k] / N, counts[b, t, 2 * k + 1] / M
                rows[b, ROW[pre + "f"] + t] = 2 * pr * rc / (pr + rc) if pr + rc > 0 else 0.0
    return o


def ambiguous(ref, tol_plain, tol_pa, thresholds=THR):
    """[B,T,4] number of points whose float64 distance lies within the distance tolerance of the threshold; asserts the 1 % cap."""
    B, T = ref["counts"].shape[:2]
    amb = np.zeros((B, T, 4), np.int64)
    for j, (name, tol) in enumerate((("d_pg", tol_plain), ("d_gp", tol_plain), ("pa_d_pg", tol_pa), ("pa_d_gp", tol_pa))):
        d = ref[name]
        if np.isnan(d).all():
            continue
        for t, thr in enumerate(thresholds):
            amb[:, t, j] = (np.abs(d - thr) <= tol).sum(1)
            assert (amb[:, t, j] <= 0.01 * d.shape[1]).all(), (name, thr, amb[:, t, j], d.shape[1])
    return amb


def f_of_counts(counts, N, M):
    """[B,T,2]: F of the (pg, gp) and of the (pa_pg, pa_gp) integer counts."""
    c = np.asarray(counts, F64)
    out = np.zeros(c.shape[:2] + (2,))
    for k in range(2):
        pr, rc = c[:, :, 2 * k] / N, c[:, :, 2 * k + 1] / M
        out[:, :, k] = np.where(pr + rc > 0, 2 * pr * rc / np.maximum(pr + rc, 1e-300), 0.0)
    return out


def check_against_ref(what, got, ref, tol_plain, tol_pa, N, M, amb, have_pa=True, thresholds=THR):
    """rows, counts and (when present) distances of one route against the float64 restatement; every figure printed before it is asserted."""
    rows, counts = np.asarray(got["rows"], F64), np.asarray(got["counts"])
    T = len(thresholds)
    plain = ["mean_pg", "mean_gp"] + (["epe"] if N == M else []) + (["ra_epe"] if N == M and not np.isnan(ref["rows"][:, 1]).all() else [])
    pa = ["pa_epe", "scale", "pa_mean_pg", "pa_mean_gp"] if have_pa else []
    for name in plain + pa:
        tol = tol_pa if name in pa else tol_plain
        if name == "scale":
            tol = tol_pa / 0.1                 # a pure number: the aligned cloud's error over its extent (the centred box reaches 0.1 m)
        err = np.abs(rows[:, ROW[name]] - ref["rows"][:, ROW[name]]).max()
        print(f"{what} {name}: error {err:.3e}  bound {tol:.3e}")
        assert np.isfinite(rows[:, ROW[name]]).all() and err <= tol, (what, name, err, tol)
    for name in ("d_pg", "d_gp") + (("pa_d_pg", "pa_d_gp") if have_pa else ()):
        if name in got:
            tol = tol_pa if name.startswith("pa_") else tol_plain
            err = np.abs(np.asarray(got[name], F64) - ref[name]).max()
            print(f"{what} {name}: error {err:.3e}  bound {tol:.3e}")
            assert err <= tol, (what, name, err, tol)
    ncol = 4 if have_pa else 2
    diff = np.abs(counts[:, :, :ncol].astype(np.int64) - ref["counts"][:, :, :ncol])
    print(f"{what} counts: largest difference {diff.max()}  ambiguous points at most {amb[:, :, :ncol].max()}  F in [{np.nanmin(ref['rows'][:, 8:8 + T]):.3f}, {np.nanmax(ref['rows'][:, 8:8 + T]):.3f}]")
    assert (diff <= amb[:, :, :ncol]).all(), (what, diff, amb)
    f = f_of_counts(counts, N, M)
    for k, col in enumerate(("f", "pa_f")[:ncol // 2]):
        assert np.abs(rows[:, ROW[col]:ROW[col] + T] - f[:, :, k]).max() <= 1e-6, (what, col)


def tolerances(pred, targ, root):
    big = max(np.abs(pred).max(), np.abs(np.asarray(targ, F64) + (0.0 if root is None else np.asarray(root, F64)[:, None])).max())
    return 16 * 2.0 ** -24 * big, 64 * 2.0 ** -24 * big


_CASES = {}


def shared_case(B, N, M):
    """The three shapes of host test 2, drawn once, with their float64 reference (left unchanged)."""
    if (B, N, M) not in _CASES:
        case = draw_case(B, N, M, 1000 + N + M, KINDS5[:B] if N == M else None)
        _CASES[(B, N, M)] = (case, mesh_ref64(*case, center_idx=0 if N == 21 else -1))
    return _CASES[(B, N, M)]


# ------------------------------------------------------------------------------------------------ 1. registry and YAML
def _evaluator_cfg():
    import yaml
    return yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_meshmetrics_mi355x.yaml")))


def test_registry_builds_the_three_metrics_and_the_yaml_builds_its_evaluator():
    from artiboost_amd import metrics as MT
    from artiboost_amd import registry as R
    preset = {"CENTER_IDX": 0}
    built = R.build_evaluator_metric_list([{"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["joints_3d_abs"], "ALIGN": ["root", "procrustes"], "MILLIMETERS": True},
                                           {"TYPE": "MeshFScore", "VAL_KEYS": ["hand_verts_3d_abs"], "THRESHOLDS_MM": [5, 15, 2.5]},
                                           {"TYPE": "MeanSurfaceDist", "VAL_KEYS": ["obj_verts_3d_abs"]}], preset)
    assert [type(m) for m in built] == [MT.MeanAlignedEPE, MT.MeshFScore, MT.MeanSurfaceDist]
    assert built[0].align == ["root", "procrustes"] and built[0].center_idx == 0 and built[1].thresholds == [0.005, 0.015, 0.0025]
    assert built[1].align == ["none", "procrustes"] and not built[2].to_millimeters
    for bad in ({"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["joints_3d_abs"], "ALIGN": ["none"]},
                {"TYPE": "MeshFScore", "VAL_KEYS": ["hand_verts_3d_abs"], "ALIGN": ["root"]},
                {"TYPE": "MeshFScore", "VAL_KEYS": ["hand_verts_3d_abs"], "THRESHOLDS_MM": [1, 2, 3, 4, 5]}):
        with pytest.raises(ValueError):
            R.build_evaluator_metric_list(bad, preset)
    cfg = _evaluator_cfg()
    base = __import__("yaml").safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_mi355x.yaml")))
    assert cfg["EVALUATOR"][:3] == base["EVALUATOR"] and {k: v for k, v in cfg.items() if k != "EVALUATOR"} == {k: v for k, v in base.items() if k != "EVALUATOR"}
    ms = R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"])
    assert [type(m).__name__ for m in ms][3:] == ["MeanAlignedEPE", "MeshFScore", "MeanSurfaceDist"]
    assert ms[3].val_keys_list == ["joints_3d_abs", "hand_verts_3d_abs"] and ms[4].thresholds_mm == [5.0, 15.0] and ms[5].val_keys_list == ["obj_verts_3d_abs"]
    from anakin.metrics.meshmetric import MeanAlignedEPE, MeanSurfaceDist, MeshFScore
    assert (MeanAlignedEPE, MeshFScore, MeanSurfaceDist) == (MT.MeanAlignedEPE, MT.MeshFScore, MT.MeanSurfaceDist)


# ------------------------------------------------------------------------------------------------ 2. the torch route against float64
@pytest.mark.parametrize("B,N,M", SHAPES)
def test_torch_route_matches_the_float64_restatement(B, N, M):
    from artiboost_amd.metrics import mesh_values_torch
    (pred, targ, root), ref = shared_case(B, N, M)
    tol_plain, tol_pa = tolerances(pred, targ, root)
    amb = ambiguous(ref, tol_plain, tol_pa)
    paired = N == M
    flags, center = (7 if paired else 4), (0 if N == 21 else -1)
    got = mesh_values_torch(*(torch.from_numpy(a) for a in (pred, targ, root)), center_idx=center, thresholds=THR, flags=flags, want_dist=True)
    got = {k: v.numpy() for k, v in got.items()}
    assert got["rows"].dtype == np.float32 and got["counts"].dtype == np.int32 and got["counts"].shape == (B, 2, 4)
    check_against_ref(f"torch-cpu ({B},{N},{M})", got, ref, tol_plain, tol_pa, N, M, amb, have_pa=paired)
    f = ref["rows"][:, 8:10]
    assert f.min() >= 0.0 and f.max() <= 1.0 and (paired or np.isnan(got["rows"][:, [0, 1, 2, 3, 6, 7, 12, 13]]).all())
    assert np.isnan(got["rows"][:, [10, 11, 14, 15]]).all()                  # thresholds past T
    if paired:
        rows, r64 = got["rows"], ref["rows"]
        # mirrored: aligned by a reflection, far below what the best proper rotation leaves
        print(f"mirrored ({N}): pa_epe {rows[1, 2]:.3e}  proper-rotation fit {ref['pa_epe_proper'][1]:.3e}")
        assert rows[1, 2] < 0.1 * ref["pa_epe_proper"][1] and abs(r64[1, 2] - ref["pa_epe_proper"][1]) > 0.002
        assert abs(ref["pa_epe_proper"][0] - r64[0, 2]) < 1e-12               # a generic sample needs no reflection: the two fits coincide
        assert r64[2, 2] < 3e-6 and rows[2, 2] < 3e-6 + tol_pa                # near-perfect: micrometres
        assert np.isfinite(rows[3]).sum() == (12 if N == 21 else 11) and np.isfinite(got["pa_d_pg"][3]).all()     # coplanar: finite
        # the alignment is a least-squares optimum: it cannot raise the RMS error
        assert (np.sqrt(((ref["aligned"] - (targ.astype(F64) + root.astype(F64)[:, None])) ** 2).sum(-1).mean(1)) <=
                np.sqrt(((pred.astype(F64) - (targ.astype(F64) + root.astype(F64)[:, None])) ** 2).sum(-1).mean(1)) + 1e-15).all()
    # float64 tensors through the same expression: the restatement up to the 1e-8 guards of the two norms (relative 1e-8 / |Pc| in the scale)
    got64 = mesh_values_torch(*(torch.from_numpy(a).double() for a in (pred, targ, root)), center_idx=center, thresholds=THR, flags=flags)
    cols = [c for c in range(16) if np.isfinite(ref["rows"][0, c]) and (paired or c in (4, 5, 8, 9))]
    np.testing.assert_allclose(got64["rows"].numpy()[:, cols], ref["rows"][:, cols], rtol=0, atol=2e-7)


def test_groups_not_asked_for_are_nan_and_bad_shapes_are_refused():
    from artiboost_amd.metrics import mesh_values_torch
    (pred, targ, root), _ = shared_case(5, 21, 21)
    p, t, r = (torch.from_numpy(a) for a in (pred, targ, root))
    full = mesh_values_torch(p, t, r, center_idx=0, thresholds=THR, flags=7)["rows"]
    for flags, cols in ((1, [0, 1]), (2, [2, 3]), (4, [4, 5, 8, 9]), (6, [2, 3, 4, 5, 6, 7, 8, 9, 12, 13])):
        rows = mesh_values_torch(p, t, r, center_idx=0, thresholds=THR, flags=flags)["rows"]
        assert torch.equal(torch.isfinite(rows[0]).nonzero().flatten(), torch.tensor(cols)) and torch.equal(rows[:, cols], full[:, cols]), flags
    assert torch.isnan(mesh_values_torch(p, t, r, center_idx=-1, flags=1)["rows"][:, 1]).all()
    a = mesh_values_torch(p, t + r[:, None], None, center_idx=0, thresholds=THR, flags=7)["rows"]          # the root folded into the target
    assert torch.equal(a.nan_to_num(-1.0), full.nan_to_num(-1.0))
    with pytest.raises(ValueError):
        mesh_values_torch(p, t[:, :20], r, flags=7)
    with pytest.raises(ValueError):
        mesh_values_torch(p[:, :2], t[:, :2], r, flags=2)


# ------------------------------------------------------------------------------------------------ 3. - 5. the classes and the evaluator
def batch_dicts(B, seed, device="cpu", with_hand=True):
    """(preds, targs) of one validation batch: 21 joints, 778 hand vertices, 300 object vertices (the object target padded by repetition
    from 200 points, as the mesh queries pad)."""
    preds, targs = {}, {}
    for key, n, s in (("joints_3d", 21, 0), ("hand_verts_3d", 778, 1), ("obj_verts_3d", 300, 2)):
        pred, targ, root = draw_case(B, n, n, seed + s)
        if key == "obj_verts_3d":
            targ[:, 200:] = targ[:, :100]
        if with_hand or not key.startswith("hand"):
            targs[key] = torch.from_numpy(targ).to(device)
        preds[key + "_abs"] = torch.from_numpy(pred - root[:, None] + draw_case(B, 1, 1, seed)[2][:, None]).to(device)
    targs["root_joint"] = torch.from_numpy(draw_case(B, 1, 1, seed)[2]).to(device)
    return preds, targs


EVAL_CFG = [{"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["joints_3d_abs"], "ALIGN": ["root", "procrustes"], "MILLIMETERS": True},
            {"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["hand_verts_3d_abs"], "MILLIMETERS": True},
            {"TYPE": "MeshFScore", "VAL_KEYS": ["hand_verts_3d_abs"]},
            {"TYPE": "MeanSurfaceDist", "VAL_KEYS": ["obj_verts_3d_abs"], "MILLIMETERS": True}]
MEASURES = {"joints_3d_abs_pa_mepe", "joints_3d_abs_ra_mepe", "hand_verts_3d_abs_pa_mepe", "hand_verts_3d_abs_f5", "hand_verts_3d_abs_f15",
            "hand_verts_3d_abs_pa_f5", "hand_verts_3d_abs_pa_f15", "obj_verts_3d_abs_adds"}


def build_metrics(cfg=None):
    from artiboost_amd import registry as R
    return R.build_evaluator_metric_list(cfg or EVAL_CFG, {"CENTER_IDX": 0})


def expected_measures(batches):
    """The float64 mean over ALL samples of the per-sample values."""
    per = {k: [] for k in MEASURES}
    for preds, targs in batches:
        root = targs["root_joint"].cpu().numpy()
        for key, n in (("joints_3d", 21), ("hand_verts_3d", 778), ("obj_verts_3d", 300)):
            if key not in targs or preds[key + "_abs"] is None:
                continue
            ref = mesh_ref64(preds[key + "_abs"].cpu().numpy(), targs[key].cpu().numpy(), root, center_idx=0 if n == 21 else -1)["rows"]
            k = key + "_abs"
            if n == 300:
                per[k + "_adds"] += list(1000 * ref[:, 5])
                continue
            per[k + "_pa_mepe"] += list(1000 * ref[:, 2])
            if n == 21:
                per[k + "_ra_mepe"] += list(1000 * ref[:, 1])
            else:
                for c, name in ((8, "_f5"), (9, "_f15"), (12, "_pa_f5"), (13, "_pa_f15")):
                    per[k + name] += list(ref[:, c])
    return {k: float(np.mean(v)) for k, v in per.items() if v}


def measures_close(got, want, n_f=778):
    """Distances in mm to 64 ulp of half a metre; an F-score may move by a few ambiguous points of its 778."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, v in want.items():
        tol = 4.0 / n_f if re.search(r"_f[\d.]+$", k) else 1000 * 64 * 2.0 ** -24 * 0.6
        assert abs(got[k] - v) <= tol, (k, got[k], v, tol)


def test_two_feeds_of_different_batch_sizes_average_over_all_samples():
    from artiboost_amd.metrics import Evaluator
    batches = [batch_dicts(3, 50), batch_dicts(5, 60)]
    ev = Evaluator({}, build_metrics())
    for p, t in batches:
        ev.feed_all(p, t)
    got = ev.get_measures_all()
    assert set(got) == MEASURES
    measures_close(got, expected_measures(batches))
    assert all(m.avg_meters and all(a.count == 8 for a in m.avg_meters.values()) for m in ev.metrics_list)
    assert "hand_verts_3d_abs_f5:" in str(ev) and "obj_verts_3d_abs_adds:" in str(ev)
    # feed is feed_device + feed_host; reset forgets
    ms = build_metrics()
    for m in ms:
        for p, t in batches:
            m.feed(p, t)
    assert {k: v for m in ms for k, v in m.get_measures().items()} == got
    ev.reset_all()
    assert all(a.count == 0 for m in ev.metrics_list for a in m.avg_meters.values())


def test_one_values_call_per_key_and_feed_all(monkeypatch):
    from artiboost_amd import metrics as MT
    calls = []
    real = MT.mesh_values_torch
    monkeypatch.setattr(MT, "mesh_values_torch", lambda *a, **k: (calls.append(a[0].shape[1]), real(*a, **k))[1])
    ev = MT.Evaluator({}, build_metrics())
    ev.feed_all(*batch_dicts(2, 70))
    assert sorted(calls) == [21, 300, 778]               # three metrics, two of them over hand_verts_3d_abs: one call per key


def test_max_lag_one_equals_blocking():
    from artiboost_amd.metrics import Evaluator
    batches = [batch_dicts(2, 80), batch_dicts(3, 90), batch_dicts(2, 100)]
    out = []
    for lag in (1, 0):
        ev = Evaluator({}, build_metrics(), max_lag=lag)
        for p, t in batches:
            ev.feed_all(p, t)
        out.append(ev.get_measures_all())
    assert out[0] == out[1] and set(out[0]) == MEASURES


def test_an_absent_key_is_skipped_and_logged_once(caplog):
    import logging
    from artiboost_amd.metrics import Evaluator
    full, bare = batch_dicts(3, 110), batch_dicts(2, 120, with_hand=False)        # the second: no hand annotation (HO3D's evaluation split)
    bare[0]["obj_verts_3d_abs"] = None                                             # ... and a prediction a model reports as None
    ev = Evaluator({}, build_metrics())
    with caplog.at_level(logging.WARNING, logger="anakin"):
        ev.feed_all(*bare)
        ev.feed_all(*full)
        ev.feed_all(*bare)
    msgs = [r.getMessage() for r in caplog.records if "skipped" in r.getMessage()]
    assert sorted(re.search(r"'(\w+)'", m).group(1) for m in msgs) == ["hand_verts_3d_abs", "hand_verts_3d_abs", "obj_verts_3d_abs"]   # once per metric and key
    assert sorted(m.split(":")[0] for m in msgs) == ["MeanAlignedEPE", "MeanSurfaceDist", "MeshFScore"]
    got = ev.get_measures_all()
    want = expected_measures([full])
    want.update({k: v for k, v in expected_measures([bare, full, bare]).items() if k.startswith("joints_3d_abs")})
    measures_close(got, want)
    counts = {k: a.count for m in ev.metrics_list for k, a in m.avg_meters.items()}
    assert counts["joints_3d_abs_pa_mepe"] == 7 and counts["hand_verts_3d_abs_f5"] == 3 and counts["obj_verts_3d_abs_adds"] == 3


def test_root_alignment_needs_a_joint_array_and_alignment_needs_pairs():
    from artiboost_amd import registry as R
    p, t = batch_dicts(2, 130)
    m = R.build_evaluator_metric_list({"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["hand_verts_3d_abs"], "ALIGN": ["root"]}, {"CENTER_IDX": 0})[0]
    with pytest.raises(ValueError, match="21-joint"):
        m.feed(p, t)
    p["obj_verts_3d_abs"] = p["obj_verts_3d_abs"][:, :257]
    adds = R.build_evaluator_metric_list({"TYPE": "MeanSurfaceDist", "VAL_KEYS": ["obj_verts_3d_abs"]}, {"CENTER_IDX": 0})[0]
    adds.feed(p, t)                                                                # N != M is what ADD-S allows
    assert np.isfinite(adds.get_measures()["obj_verts_3d_abs_adds"])
    for cfg in ({"TYPE": "MeanAlignedEPE", "VAL_KEYS": ["obj_verts_3d_abs"]}, {"TYPE": "MeshFScore", "VAL_KEYS": ["obj_verts_3d_abs"]}):
        with pytest.raises(ValueError, match="N == M"):
            R.build_evaluator_metric_list(cfg, {"CENTER_IDX": 0})[0].feed(p, t)


# ------------------------------------------------------------------------------------------------ 6. header contract, generated op
def test_header_contract_and_generated_op():
    from artiboost_amd import _lib as L
    from artiboost_amd import gen_torch_ops, kernels
    txt = open(gen_torch_ops.HEADER).read()
    assert re.search(r"@check\s+ab_mesh_metrics:", txt) and re.search(r"\bint\s+ab_mesh_metrics\s*\(", txt) and re.search(r"\blong\s+ab_mesh_metrics_workspace\s*\(", txt)
    assert {"ab_mesh_metrics", "ab_mesh_metrics_workspace"} <= set(L.declared_symbols())
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    cons = gen_torch_ops.contracts()["ab_mesh_metrics"]
    lines = gen_torch_ops.checks_for("ab_mesh_metrics", decl["ab_mesh_metrics"][:-1], cons)
    assert any("ck_host" in l and "thresholds_host" in l for l in lines) and any("ab_mesh_metrics_workspace(B,N,M)" in c for c in cons)
    assert [p for p in decl["ab_mesh_metrics"] if p[1] in ("counts", "stream")] == [("int32_t*", "counts"), ("void*", "stream")]
    src = open(gen_torch_ops.OUT).read()
    assert 'm.def("mesh_metrics(' in src and 'm.impl("mesh_metrics", &w_mesh_metrics);' in src and "w_mesh_metrics_workspace" in src
    _, schema, body = gen_torch_ops.schema_and_wrapper("int", "ab_mesh_metrics", decl["ab_mesh_metrics"], cons)
    assert body in src and f'm.def("{schema}");' in src                         # the committed source is what the generator writes
    # the layout the wrapper and the header agree on
    for name, col in kernels.MM_ROW.items():
        macro = {"f": "AB_MM_F", "pa_f": "AB_MM_PA_F"}.get(name, "AB_MM_" + name.upper())
        assert re.search(rf"#define {macro} {col}\b", txt), name
    assert kernels.MM_ROW == ROW and (kernels.MM_PAIRED, kernels.MM_PROCRUSTES, kernels.MM_NN) == (1, 2, 4)
    assert re.search(r"not captured in a hipGraph", txt[txt.index("Leaderboard mesh metrics"):txt.index("long ab_mesh_metrics_workspace")])
