"""ab_mesh_metrics (csrc/mesh_metrics.hip) on the device against the float64 restatement of
tests/test_mesh_metrics_host.py: every shape at which the kernel takes another path, its flags and optional outputs, determinism and
independence of the batch around a sample, the three metric classes and the evaluator on HIP tensors, the dispatcher op's refusals, and one
HoNet forward fed through the evaluator of config/ho3dv2_honet_meshmetrics_mi355x.yaml.  Nothing here captures a graph.

Bounds (none is a recorded figure; every figure is printed before it is asserted):
  unaligned distances, means and paired errors   16 x 2^-24 x max |coordinate| of the case, absolute: both sides read the same fp32 inputs
                                                 and the only roundings are the root addition, the differences and the length.
  aligned quantities (pa_*, scale)               the larger of 4 x the error of the fp32 torch-CPU route against float64 on the same inputs
                                                 and the unaligned floor (for the pure number `scale`: 16 x 2^-24).
  counts                                         |device - float64| <= the number of points whose float64 distance lies within the distance
                                                 bound of the threshold; such points are at most 1 % of any (sample, direction, threshold),
                                                 asserted on the float64 side first.  F equals the formula on the device's own counts to 1e-6."""
import os

import numpy as np
import pytest
import torch

from test_mesh_metrics_host import (F64, KINDS5, ROW, THR, batch_dicts, build_metrics, draw_case, expected_measures, f_of_counts, mesh_ref64,
                                    MEASURES)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = ("d_pg", "d_gp", "pa_d_pg", "pa_d_gp")
PLAIN = ("epe", "ra_epe", "mean_pg", "mean_gp", "d_pg", "d_gp")
ALIGNED = ("pa_epe", "scale", "pa_mean_pg", "pa_mean_gp", "pa_d_pg", "pa_d_gp")
WORST = {"ratio": 0.0}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kernel(case, center=-1, thresholds=THR, flags=7, want_dist=True):
    from artiboost_amd import kernels as K
    pred, targ, root = case
    o = K.mesh_metrics(_dev(pred), _dev(targ), _dev(root), center_idx=center, thresholds=thresholds, flags=flags, want_dist=want_dist)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _cpu_route(case, center, flags):
    from artiboost_amd.metrics import mesh_values_torch
    pred, targ, root = case
    t = lambda a: None if a is None else torch.from_numpy(a)      # noqa: E731
    return {k: v.numpy() for k, v in mesh_values_torch(t(pred), t(targ), t(root), center_idx=center, thresholds=THR, flags=flags, want_dist=True).items()}


def _get(o, name):
    return np.asarray(o[name] if name in DIST else o["rows"][:, ROW[name]], F64)


def _bounds(case, ref, cpu, paired):
    """{quantity: bound}; the aligned ones from the torch-CPU route's own error against float64."""
    pred, targ, root = case
    big = max(np.abs(pred).max(), np.abs(np.asarray(targ, F64) + (0.0 if root is None else np.asarray(root, F64)[:, None])).max())
    floor = 16 * 2.0 ** -24 * big
    b = {k: (floor, 0.0) for k in PLAIN}
    if paired:
        for k in ALIGNED:
            e_cpu = float(np.abs(_get(cpu, k) - _get(ref, k)).max())
            b[k] = (max(4.0 * e_cpu, 16 * 2.0 ** -24 if k == "scale" else floor), e_cpu)
    return b


def _ambiguous(ref, bounds, paired):
    B, T = ref["counts"].shape[:2]
    amb = np.zeros((B, T, 4), np.int64)
    for j, name in enumerate(DIST[:4 if paired else 2]):
        for t, thr in enumerate(THR):
            amb[:, t, j] = (np.abs(ref[name] - thr) <= bounds[name][0]).sum(1)
            assert (amb[:, t, j] <= 0.01 * ref[name].shape[1]).all(), (name, thr, amb[:, t, j])      # the cap, before the device is looked at
    return amb


def _check(tag, case, got, center=-1):
    """One kernel result (all groups the shapes allow) against float64; -> (the float64 reference, the bounds)."""
    pred, targ, root = case
    N, M = pred.shape[1], targ.shape[1]
    paired = N == M and N >= 3
    ref = mesh_ref64(pred, targ, root, center_idx=center)
    cpu = _cpu_route(case, center, 7 if paired else 4)
    bounds = _bounds(case, ref, cpu, paired)
    amb = _ambiguous(ref, bounds, paired)
    for name in PLAIN + (ALIGNED if paired else ()):
        if name in ("epe", "ra_epe") and (not paired or (name == "ra_epe" and center < 0)):
            continue
        bound, e_cpu = bounds[name]
        err = float(np.abs(_get(got, name) - _get(ref, name)).max())
        ratio = err / e_cpu if e_cpu > 0 else float("nan")
        print(f"{tag} {name}: kernel {err:.3e}  cpu-fp32 {e_cpu:.3e}  ratio {ratio:.2f}  bound {bound:.3e}")
        if name in ALIGNED and e_cpu > 0 and err > 16 * 2.0 ** -24 * 0.5:
            WORST["ratio"] = max(WORST["ratio"], ratio)
        assert np.isfinite(_get(got, name)).all() and err <= bound, (tag, name, err, bound)
    ncol = 4 if paired else 2
    diff = np.abs(got["counts"].astype(np.int64) - ref["counts"])[:, :, :ncol]
    print(f"{tag} counts: largest difference {diff.max()}  ambiguous at most {amb.max()}  F in [{np.nanmin(ref['rows'][:, 8:10]):.3f}, {np.nanmax(ref['rows'][:, 8:10]):.3f}]")
    assert (diff <= amb[:, :, :ncol]).all(), (tag, diff, amb)
    assert not got["counts"][:, :, ncol:].any()
    f = f_of_counts(got["counts"], N, M)
    for k, col in enumerate(("f", "pa_f")[:ncol // 2]):
        assert np.abs(got["rows"][:, ROW[col]:ROW[col] + 2] - f[:, :, k]).max() <= 1e-6, (tag, col)
    assert np.isnan(got["rows"][:, [10, 11, 14, 15]]).all()
    if not paired:
        assert np.isnan(got["rows"][:, [0, 1, 2, 3, 6, 7, 12, 13]]).all()
    return ref, bounds


# ------------------------------------------------------------------------------------------------ 1. - 3. the kernel against float64
SPECIAL = ("mirrored", "near", "coplanar")
PAIRED_CASES = [(1, 3, None, True), (3, 3, ("mirrored", "near", "generic"), True), (1, 21, None, True), (3, 21, SPECIAL, True), (3, 21, SPECIAL, False),
                (1, 778, None, True), (3, 778, SPECIAL, True), (1, 255, None, True), (3, 256, None, True), (1, 257, None, True), (1, 257, None, False),
                (1, 1023, None, True), (1, 1024, None, True), (3, 1025, None, True)]


@pytest.mark.parametrize("B,N,kinds,with_root", PAIRED_CASES)
def test_paired_shapes_vs_float64(B, N, kinds, with_root):
    case = draw_case(B, N, N, 2000 + 7 * N + B, kinds, with_root=with_root)
    center = 0 if N == 21 else (2 if N == 3 else -1)
    got = _kernel(case, center)
    ref, bounds = _check(f"({B},{N},{N}{'' if with_root else ',no root'})", case, got, center)
    if kinds and N > 3:                                     # mirrored: a reflection, not the best proper rotation
        print(f"mirrored ({N}): pa_epe {got['rows'][0, 2]:.3e}  proper-rotation fit {ref['pa_epe_proper'][0]:.3e}")
        assert got["rows"][0, 2] < 0.1 * ref["pa_epe_proper"][0]
    # `aligned`, recovered through pa_epe and the aligned scan, is the one ab_procrustes_loss forms
    from artiboost_amd import kernels as K
    pred, targ, root = case
    zroot = root if root is not None else np.zeros((B, 3), np.float32)
    al = K.procrustes_loss(_dev(pred), _dev(targ), _dev(zroot), want_grad=False, want_aligned=True)["aligned"].cpu().numpy()
    G = targ.astype(F64) + zroot.astype(F64)[:, None]
    pa_epe = np.linalg.norm(al.astype(F64) - G, axis=2).mean(1)
    err = np.abs(pa_epe - got["rows"][:, 2]).max()
    print(f"aligned of ab_procrustes_loss ({B},{N}): pa_epe differs by {err:.3e}  bound {bounds['pa_epe'][0]:.3e}")
    assert err <= bounds["pa_epe"][0]
    for b in range(B):
        D = np.sqrt(((al[b].astype(F64)[:, None] - G[b][None]) ** 2).sum(-1))
        for name, d in (("pa_d_pg", D.min(1)), ("pa_d_gp", D.min(0))):
            assert np.abs(d - got[name][b]).max() <= bounds[name][0], (name, b)


@pytest.mark.parametrize("B,N,M", [(3, 257, 63), (3, 1, 300), (1, 63, 1025)])
def test_unpaired_shapes_vs_float64(B, N, M):
    from artiboost_amd import kernels as K
    case = draw_case(B, N, M, 3000 + N + M)
    got = _kernel(case, flags=K.MM_NN)
    _check(f"({B},{N},{M})", case, got)


def test_a_cloud_padded_by_repetition_counts_every_duplicate():
    pred, targ, root = draw_case(2, 300, 300, 77)
    targ[:, 200:], pred[:, 200:] = targ[:, :100], pred[:, :100]
    got = _kernel((pred, targ, root))
    _check("padded (2,300,300)", (pred, targ, root), got)
    for name in DIST:
        assert np.array_equal(got[name][:, 200:], got[name][:, :100]), name
    plain = _kernel((pred[:, :200], targ[:, :200], root), flags=4)
    # the distances of the unpadded clouds, and counts that count the duplicates: first 100 points twice
    assert np.array_equal(plain["d_pg"], got["d_pg"][:, :200]) and np.array_equal(plain["d_gp"], got["d_gp"][:, :200])
    for t, thr in enumerate(THR):
        assert np.array_equal(got["counts"][:, t, 0], (got["d_pg"] < np.float32(thr)).sum(1)) and np.array_equal(got["counts"][:, t, 1], (got["d_gp"] < np.float32(thr)).sum(1))
        assert np.array_equal(got["counts"][:, t, 0], plain["counts"][:, t, 0] + (plain["d_pg"][:, :100] < np.float32(thr)).sum(1))


def test_flag_groups_and_optional_outputs():
    case = draw_case(3, 21, 21, 11, ("generic", "mirrored", "near"))
    full = _kernel(case, 0)
    groups = {1: [0, 1], 2: [2, 3], 4: [4, 5, 8, 9], 3: [0, 1, 2, 3], 5: [0, 1, 4, 5, 8, 9], 6: [2, 3, 4, 5, 6, 7, 8, 9, 12, 13], 7: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]}
    for flags, cols in groups.items():
        got = _kernel(case, 0, flags=flags, want_dist=False)
        assert sorted(got) == ["counts", "rows"]
        assert np.array_equal(np.isfinite(got["rows"]).nonzero()[1].reshape(3, -1)[0], cols), flags
        assert np.array_equal(got["rows"][:, cols], full["rows"][:, cols]), flags                       # the same bits as the full call
        want = full["counts"].copy()
        if not flags & 4:
            want[:] = 0
        elif not flags & 2:
            want[:, :, 2:] = 0
        assert np.array_equal(got["counts"], want), flags
    assert np.isnan(_kernel(case, -1, flags=1, want_dist=False)["rows"][:, 1]).all()                  # no centre: no root-relative error
    for omit in DIST:                                                                                  # every optional output NULL in turn
        got = _kernel(case, 0, want_dist=[k for k in DIST if k != omit])
        assert omit not in got and all(np.array_equal(got[k], full[k], equal_nan=True) for k in got)
    none = _kernel(case, 0, thresholds=())                                                             # T = 0: no counts, no F
    assert none["counts"].shape == (3, 0, 4) and np.isnan(none["rows"][:, 8:]).all() and np.array_equal(none["rows"][:, :8], full["rows"][:, :8])
    four = _kernel(case, 0, thresholds=(0.005, 0.015, 0.002, 1.0))
    assert np.array_equal(four["counts"][:, :2], full["counts"]) and np.isfinite(four["rows"]).all()
    assert (four["counts"][:, 3] == 21).all() and (four["rows"][:, [11, 15]] == 1.0).all()


# ------------------------------------------------------------------------------------------------ 4. determinism, batch independence
def test_two_calls_give_the_same_bits_and_a_sample_does_not_depend_on_its_batch():
    for N, M, flags in ((778, 778, 7), (257, 63, 4)):
        case = draw_case(3, N, M, 21 + N, KINDS5[1:4] if N == M else None)
        a, b = _kernel(case, flags=flags), _kernel(case, flags=flags)
        keys = [k for k in a if flags == 7 or not k.startswith("pa_")]
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)
        for s in range(3):
            alone = _kernel([x[s:s + 1] for x in case], flags=flags)
            for k in keys:
                assert np.array_equal(alone[k][0], a[k][s], equal_nan=True), (k, s, N)


# ------------------------------------------------------------------------------------------------ 5. the classes and the evaluator
def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def test_metric_classes_on_hip_tensors_match_their_cpu_route():
    from artiboost_amd.metrics import Evaluator
    batches = [batch_dicts(3, 50), batch_dicts(5, 60)]
    want = expected_measures(batches)
    out = {}
    for dev in ("cpu", "cuda"):
        ev = Evaluator({}, build_metrics())
        for p, t in batches:
            ev.feed_all(_to(p, dev), _to(t, dev))
        out[dev] = ev.get_measures_all()
    assert set(out["cuda"]) == set(out["cpu"]) == MEASURES
    floor = 1000 * 16 * 2.0 ** -24 * 0.6                                      # mm; no coordinate of these batches reaches 0.6 m
    for k, v in want.items():
        e_cpu, e_dev = abs(out["cpu"][k] - v), abs(out["cuda"][k] - v)
        if "_f" in k.rsplit("abs", 1)[1]:
            bound = 0.01                                                        # at most 1 % of a cloud's points are ambiguous (test 3's cap)
        else:
            bound = max(4 * e_cpu, floor) if "_pa_" in k else floor
        print(f"{k}: device {e_dev:.3e}  cpu {e_cpu:.3e}  bound {bound:.3e}")
        assert e_dev <= bound, (k, e_dev, bound)
    # the deferred read-back and the blocking one
    lag = []
    for max_lag in (1, 0):
        ev = Evaluator({}, build_metrics(), max_lag=max_lag)
        for p, t in batches + batches[:1]:
            ev.feed_all(_to(p, "cuda"), _to(t, "cuda"))
        lag.append(ev.get_measures_all())
    assert lag[0] == lag[1]


def test_feed_device_reads_nothing_back_and_makes_one_call_per_key(monkeypatch):
    from artiboost_amd import kernels as K
    from artiboost_amd.metrics import Evaluator
    calls = []
    real = K.mesh_metrics
    monkeypatch.setattr(K, "mesh_metrics", lambda *a, **k: (calls.append(a[0].shape[1]), real(*a, **k))[1])
    p, t = (_to(d, "cuda") for d in batch_dicts(2, 70))
    ev = Evaluator({}, build_metrics(), max_lag=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m in ev._metrics_list:
            tensors, names = m.feed_device(p, t, memo={})
            assert len(tensors) == len(names) and all(x.is_cuda and x.shape == (2,) and x.dtype == torch.float32 for x in tensors)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    calls.clear()
    ev.feed_all(p, t)
    assert sorted(calls) == [21, 300, 778]
    assert set(ev.get_measures_all()) == MEASURES


# ------------------------------------------------------------------------------------------------ 6. the dispatcher op's refusals
def test_dispatcher_op_refusals():
    from artiboost_amd import _lib as L
    L.lib()
    op = torch.ops.artiboost_hip.mesh_metrics
    B, N, M, T = 2, 5, 5, 2
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    ws = torch.zeros(int(torch.ops.artiboost_hip.mesh_metrics_workspace(B, N, M)), dtype=torch.uint8, device="cuda")
    thr = torch.tensor([0.005, 0.015, 0.02, 0.03, 0.04])

    def args(**kw):
        a = dict(pred=z(B, N, 3), targ=z(B, M, 3), root=z(B, 3), B=B, N=N, M=M, center_idx=-1, thresholds_host=thr, T=T, flags=7, rows=z(B, 16),
                 counts=torch.zeros(B, 5, 4, dtype=torch.int32, device="cuda"), d_pg=None, d_gp=None, pa_d_pg=None, pa_d_gp=None, workspace=ws)
        a.update(kw)
        return list(a.values())
    op(*args())                                                                  # the well-formed call goes through
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        op(*args(pred=torch.zeros(B, N, 3)))
    with pytest.raises(RuntimeError, match="'pred' holds"):
        op(*args(pred=z(B * N * 3 - 1)))
    with pytest.raises(RuntimeError, match="'d_gp' holds"):
        op(*args(d_gp=z(B, M - 1)))
    with pytest.raises(RuntimeError, match="bytes"):
        op(*args(workspace=ws[:-1]))
    with pytest.raises(RuntimeError, match="HOST"):
        op(*args(thresholds_host=thr.cuda()))
    ws2 = torch.zeros(int(torch.ops.artiboost_hip.mesh_metrics_workspace(B, N, 7)), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="argument error"):                    # PROCRUSTES with N != M
        op(*args(targ=z(B, 7, 3), M=7, flags=2, workspace=ws2))
    op(*args(targ=z(B, 7, 3), M=7, flags=4, workspace=ws2))                      # ... the scan alone takes it
    with pytest.raises(RuntimeError, match="argument error"):                    # T > 4
        op(*args(T=5))
    with pytest.raises(RuntimeError, match="argument error"):                    # the alignment of two points
        op(*args(pred=z(B, 2, 3), targ=z(B, 2, 3), N=2, M=2, flags=2))
    with pytest.raises(RuntimeError, match="argument error"):
        op(*args(center_idx=N))
    with pytest.raises(RuntimeError, match="argument error"):
        op(*args(flags=0))
    torch.cuda.synchronize()
    from artiboost_amd import kernels as K
    with pytest.raises(RuntimeError, match="device tensors"):
        K.mesh_metrics(torch.zeros(B, N, 3), torch.zeros(B, M, 3))


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_honet_forward_through_the_yaml_evaluator():
    import yaml
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import kernels as K
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import Evaluator
    from test_gpu_honet import ARCH, PRESET, _batch
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_meshmetrics_mi355x.yaml")))
    torch.manual_seed(0)
    model = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32"), preset_cfg=PRESET)[0]
    model.eval()
    batch = _batch(2, 31, N=30)
    batch.update(obj_id=torch.tensor([1, 2]), persp_id=torch.tensor([0, 1]), grasp_id=torch.tensor([3, 4]), is_synth=torch.tensor([1, 1]))
    with torch.no_grad():
        preds = model(batch)
    assert preds["hand_verts_3d_abs"].is_cuda and preds["obj_verts_3d_abs"].shape == (2, 30, 3)
    ev = Evaluator(cfg, R.build_evaluator_metric_list(cfg["EVALUATOR"], cfg["DATA_PRESET"]))
    ev.feed_all(preds, batch, losses={})
    got = ev.get_measures_all()
    new = ["joints_3d_abs_pa_mepe", "hand_verts_3d_abs_pa_mepe", "hand_verts_3d_abs_f5", "hand_verts_3d_abs_f15", "hand_verts_3d_abs_pa_f5",
           "hand_verts_3d_abs_pa_f15", "obj_verts_3d_abs_adds"]
    print({k: got[k] for k in new})
    assert all(np.isfinite(got[k]) for k in new) and all(0.0 <= got[k] <= 1.0 for k in new if "_f" in k.rsplit("abs", 1)[1])
    # the alignment is a least-squares optimum: per sample mean |P' - G| <= rms |P' - G| <= rms |P - G|
    P = preds["hand_verts_3d_abs"].detach().float()
    Gd = (batch["hand_verts_3d"] + batch["root_joint"][:, None]).cuda()
    al = K.procrustes_loss(P.contiguous(), batch["hand_verts_3d"].cuda().contiguous(), batch["root_joint"].cuda().contiguous(), want_grad=False,
                           want_aligned=True)["aligned"]
    rms = lambda d: d.double().pow(2).sum(-1).mean(1).sqrt()      # noqa: E731
    rms_pa, rms_raw = rms(al - Gd).cpu().numpy(), rms(P - Gd).cpu().numpy()
    print(f"rms aligned {rms_pa}  rms unaligned {rms_raw}")
    assert (rms_pa <= rms_raw * (1 + 1e-6)).all()
    assert got["hand_verts_3d_abs_pa_mepe"] <= 1000 * rms_raw.mean() * (1 + 1e-6)


def test_print_the_largest_aligned_ratio():
    """(last: the largest kernel / torch-CPU error ratio of an aligned quantity seen above, for DESIGN.md section 23)"""
    print(f"largest aligned-quantity ratio against the fp32 torch-CPU route: {WORST['ratio']:.2f}")
