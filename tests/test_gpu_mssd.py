"""ab_mssd (csrc/mssd.hip) on the device against the float64 true-set restatement of tests/test_mssd_host.py, its determinism and
independence properties, and the metric routes (AR, ValMetricAR2, Evaluator) on HIP tensors against tests/golden/mssd.npz.

Bound: 2e-6 m (tests/test_gpu_honet.py's bound on positions).  Sizes at 6 cm spread and 0.5 - 1 m depth: rigid mode works on residuals of a
few cm (fp32 spacing 4e-9 m), points mode subtracts positions of about 1 m (spacing 6e-8 .. 1.2e-7 m, a handful of roundings).
Every case prints its measured maximum.  Measured on an MI355X over every case below: rigid mode 3.2e-08 m, points mode 8.3e-08 m."""
import json

import numpy as np
import pytest
import torch

from test_mssd_host import (AR_TAGS, TOL_M, _eval_batches, cfg_for, check_golden_measures, eval_metric_list, golden, mssd_f64, same_measures,
                            true_sets)

pytestmark = pytest.mark.gpu
TILE = 1024             # SYM_TILE of csrc/mssd.hip: vertices staged per round


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def case(B, V, obj_ids, seed, exact=()):
    """Seeded inputs as numpy fp32: 6 cm spread, depths 0.5 - 1 m, predictions a random rotation and 1 cm off (samples in `exact`: the
    ground truth itself), predicted points = the rigid image + 4 mm noise, a centre offset of a few cm."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    can = f(rng.uniform(-1, 1, size=(B, V, 3)) * np.array([0.03, 0.045, 0.06]))
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pR, pt = np.zeros((B, 3, 3), np.float32), np.zeros((B, 1, 3), np.float32)
    for b in range(B):
        T[b, :3, :3], T[b, :3, 3] = _rot(rng), [rng.normal() * 0.05, rng.normal() * 0.05, rng.uniform(0.5, 1.0)]
        d = rng.normal(size=3)
        pR[b], pt[b, 0] = (T[b, :3, :3], T[b, :3, 3]) if b in exact else (_rot(rng), T[b, :3, 3] + 0.01 * d / np.linalg.norm(d))
    pts = np.einsum("bij,bvj->bvi", pR.astype(np.float64), can) + pt
    pts += rng.normal(size=pts.shape) * 0.004 * np.array([b not in exact for b in range(B)])[:, None, None]
    return dict(can=can, obj_transf=T, obj_idx=np.asarray(obj_ids, np.int64), pred_R=pR, pred_t=pt, pred_pts=f(pts), center=f(rng.normal(size=(B, 3)) * 0.04))


def base_for(step=0.25, ycb=0):
    import artiboost_amd.metrics as M
    return M._MSSDBase(**cfg_for(golden()[3], ycb=ycb, step=step))


def run(c, base, mode, center, out=None):
    from artiboost_amd import kernels as K
    d = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    tab = (base.R.cuda(), base.t.cuda(), base.sym_count.cuda())
    kw = dict(pred_pts=d["pred_pts"]) if mode == "points" else dict(pred_R=d["pred_R"], pred_t=d["pred_t"])
    return K.mssd(d["can"], d["obj_transf"], d["obj_idx"], *tab, center=d["center"] if center else None, out=out, **kw)


def want(c, sets, mode, center, ycb=False):
    kw = dict(pred_pts=c["pred_pts"]) if mode == "points" else dict(pred_R=c["pred_R"], pred_t=c["pred_t"])
    return mssd_f64(c["can"], c["obj_transf"], c["obj_idx"], sets, center=c["center"] if center else None, ycb=ycb, **kw)


def check_all_modes(c, base, sets, label, ycb=False):
    for mode in ("rigid", "points"):
        for center in (False, True):
            got = run(c, base, mode, center).double().cpu().numpy()
            err = float(np.abs(got - want(c, sets, mode, center, ycb)).max())
            print(f"{label} {mode}{' + centre' if center else ''}: max |kernel - float64| = {err:.3e} m")
            assert np.isfinite(got).all() and err <= TOL_M, (label, mode, center, err)


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("V", [1, 8, 157, 513, TILE + 6])
def test_kernel_matches_float64_true_sets(B, V):
    """Sets of 1, 2, 12 and 24 mixed in one batch; rigid and points mode, with and without the centre offset; an obj_idx below and above the
    table (clamped to its first / last row); sample 0: a perfect prediction of an identity-containing set, 0 within the bound."""
    base = base_for()
    sets = true_sets(base)
    rng = np.random.default_rng(100 * B + V)
    ids = [2] + [int(x) for x in rng.integers(1, 5, size=B - 1)]
    if B >= 5:
        ids[1:5] = [3, 0, 9, 4]
    c = case(B, V, ids, seed=B * 7919 + V, exact=(0,))
    check_all_modes(c, base, sets, f"B={B} V={V}")
    for mode in ("rigid", "points"):
        assert float(run(c, base, mode, False)[0]) <= TOL_M


def test_sets_of_314_and_628_cross_the_chunk_boundary():
    """MAX_SYM_DISC_STEP = 0.01: 314 = 4 * 64 + 58 and 628 = 9 * 64 + 52 symmetries, a partial last chunk each, and chunks past the
    shorter set's count that must write nothing the result depends on."""
    base = base_for(step=0.01)
    assert base.sym_count.tolist() == [1, 2, 314, 628]
    check_all_modes(case(2, 157, [3, 4], seed=5), base, true_sets(base), "K=314,628")
    check_all_modes(case(2, 8, [4, 1], seed=6), base, true_sets(base), "K=628,1")


def test_use_ho3d_ycb_is_the_sign_folded_table():
    plain, folded = base_for(), base_for(ycb=1)
    c = case(5, 157, [1, 2, 3, 4, 3], seed=11)
    check_all_modes(c, folded, true_sets(plain), "ycb", ycb=True)


def test_bits_do_not_depend_on_the_call_the_batch_the_padding_or_unread_table_entries():
    import artiboost_amd.metrics as M
    base = base_for()
    c = case(5, 157, [3, 4, 2, 1, 4], seed=21)
    for mode in ("rigid", "points"):
        first = run(c, base, mode, True)
        assert torch.equal(first, run(c, base, mode, True))
        # a sample alone equals the same sample inside the batch
        for b in (1, 3):
            alone = {k: v[b:b + 1] for k, v in c.items()}
            assert torch.equal(run(alone, base, mode, True), first[b:b + 1]), (mode, b)
        # vertices padded from 157 to 300 by repetition, as ho_collate pads them
        idx = np.arange(300) % 157
        padded = dict(c, can=np.ascontiguousarray(c["can"][:, idx]), pred_pts=np.ascontiguousarray(c["pred_pts"][:, idx]))
        assert torch.equal(run(padded, base, mode, True), first), mode
        # garbage past sym_count is never read
        dirty = M._MSSDBase(**cfg_for(golden()[3]))
        for i, n in enumerate(dirty.sym_count.tolist()):
            dirty.R[i, n:], dirty.t[i, n:] = float("nan"), float("nan")
        assert torch.equal(run(c, dirty, mode, True), first), mode
    # `out` is written in full and returned
    out = torch.full((5,), -1.0, device="cuda")
    assert run(c, base, "rigid", False, out=out) is out and (out > 0).all()


@pytest.mark.parametrize("route", ["kernel", "torch"])
def test_metrics_on_hip_tensors_reproduce_the_reference(route, monkeypatch):
    """AR and ValMetricAR2 through ab_mssd and through AB_MSSD_TORCH=1, each against the reference's recorded results."""
    from artiboost_amd import kernels as K
    calls = []
    real = K.mssd
    monkeypatch.setattr(K, "mssd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    if route == "torch":
        monkeypatch.setenv("AB_MSSD_TORCH", "1")
    else:
        monkeypatch.delenv("AB_MSSD_TORCH", raising=False)
    g, p, t, info = golden()
    p, t = {k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in t.items()}
    worst = check_golden_measures(g, p, t, info, f"hip/{route} ")
    print(f"hip/{route}: max error {worst:.3e} m (bound {TOL_M:.1e})")
    assert bool(calls) == (route == "kernel")                         # the route under test is the one that ran
    assert len(AR_TAGS) == 8


def test_deferred_and_blocking_evaluators_end_with_identical_measures():
    import artiboost_amd.metrics as M
    info, batches = _eval_batches()
    batches = [({k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in t.items()}) for p, t in batches]
    evs = [M.Evaluator({}, eval_metric_list(info), max_lag=lag) for lag in (1, 0)]
    for p, t in batches:
        for ev in evs:
            ev.feed_all(p, t, {})
    assert not evs[1]._inflight
    a, b = (ev.get_measures_all() for ev in evs)
    same_measures(a, b)
    assert a["MSSD"] > 0 and len(a["mssd"]) > 0 and a["epe_mean_all"] > 0 and json.dumps(sorted(map(str, a)))
