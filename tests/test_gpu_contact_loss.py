"""ab_contact_loss (csrc/contact_loss.hip) on the device against `criterions.contact_loss_torch` in float64 on the same
inputs (run on the device's float64 units, as tests/test_gpu_interaction.py does): every shape at which the kernel takes another path, the
compaction boundary, samples that contribute nothing, AB_CL_SCAN_ALL, determinism and independence of the batch around a sample, the call
without gradients, the dispatcher op's refusals, `ContactLoss` on HIP tensors and two eager HoNet training steps.  Nothing here captures a graph.

Bounds (none is a recorded figure; every figure is printed before it is asserted):
  |sdf|, rep, att, loss     the larger of 4 x the error of the fp32 torch-CPU route against float64 on that case and
                            16 x 2^-24 x max |coordinate| of the case (the rule of section 24).
  g_hand, g_rot, g_tsl      max |got - ref| / max |ref|, bounded by the larger of 4 x the fp32 torch-CPU route's error and
                            16 x 2^-24 x max |coordinate| / d_min, d_min the smallest float64 distance among the compared contributing vertices.
  inside flags, n_inside,   equal to float64's.
  zone winners
Left out, decided on the float64 side only: a vertex whose o w lies within 1e-3 of 0.5; one whose distance to the surface or to a face
plane of the box is below the distance bound; one with d < 1e-4 m (gradient direction only); one for which a triangle within 1e-6 m of
the best distance has its closest point more than 1e-4 m from the best one (a medial-axis tie); a zone whose two smallest exterior
distances differ by less than the distance bound.  At most 1 % of a case's vertices, and none of the stand-in case's zones: asserted on
the float64 side."""
import os

import numpy as np
import pytest
import torch

from test_contact_loss_host import ALPHA, RHO, class_batch, run_cl
from test_interaction_host import HI, LO, box_mesh, table_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
WORST = {}
OUT = ("loss", "rep", "att", "counts", "sdf", "g_hand", "g_rot", "g_tsl")


def zones_for(Nh, Z, seed):
    """About a third of the vertices in Z zones, the others in none."""
    rng = np.random.default_rng(seed)
    zone = np.full(Nh, -1, np.int32)
    if Z:
        pick = rng.permutation(Nh)[:max(Nh // 3, min(Nh, Z))]
        zone[pick] = rng.integers(0, Z, len(pick))
    return zone


def small(B, Nh, seed, rows, Z=3, far=()):
    from test_gpu_interaction import small_case
    c = small_case(B, Nh, seed, rows=rows, far=far)
    return dict(table=c["table"], hand=c["hand"], rows=np.asarray(c["rows"]), rot=c["rot"], tsl=c["tsl"], zone=zones_for(Nh, Z, seed + 1) if Z else None, Z=Z)


def _call(case, kernel, dtype=None, device="cuda", **kw):
    c = dict(case)
    out = run_cl(c["table"], c["hand"], c["zone"], c["Z"], c["rows"], c["rot"], c["tsl"], mask=c.get("mask"),
                 dtype=dtype or (torch.float32 if kernel else torch.float64), device=device, kernel=kernel, **kw)
    if kernel:
        torch.cuda.synchronize()
    return out


def _take(case, idx):
    return {k: (v[list(idx)] if k in ("hand", "rows", "rot", "tsl", "mask") and v is not None else v) for k, v in case.items()}


def check(tag, case, stand_in=False, **kw):
    """One kernel call against float64 (device) and the fp32 torch-CPU route; every figure printed before it is asserted.  -> (got, ref)"""
    table, hand = case["table"], case["hand"]
    B, Nh, Z = hand.shape[0], hand.shape[1], case["Z"]
    got = _call(case, True, want_sdf=True, **kw)
    ref = _call(case, False, want_sdf=True, want_diag=True, medial=(1e-6, 1e-4), **kw)
    cpu = _call(case, False, dtype=torch.float32, device="cpu", want_sdf=True, **kw)
    D = ref["diag"]
    big = max(np.abs(hand).max(), np.abs(case["tsl"]).max() + np.abs(table.verts).max() * 1.8)
    cand = ~np.isnan(ref["sdf"])
    d = np.where(cand, np.abs(ref["sdf"]), np.inf)
    coord = 16 * 2.0 ** -24 * big
    amb_w = cand & ~np.isnan(D["wind"]) & (np.abs(D["wind"] - 0.5) < 1e-3)
    both = cand & ~np.isnan(cpu["sdf"]) & ~np.isnan(got["sdf"])
    e_cpu_d = float(np.abs(np.abs(cpu["sdf"].astype(F64)) - d)[both].max()) if both.any() else 0.0
    bound_d = max(4 * e_cpu_d, coord)
    near = (cand & (d < bound_d)) | (D["box_margin"] < bound_d)                        # on the surface, or on a face plane of the box
    out = amb_w | near | (cand & D["medial"])
    out_g = out | (cand & (d < 1e-4))
    live = np.isfinite(D["box_margin"]).any(1)                                         # samples that were looked at at all
    assert out_g.sum() <= 0.01 * max(live.sum() * Nh, 1) or out_g.sum() == 0, (tag, int(out_g.sum()))      # the cap, on the float64 side
    # the zones whose two smallest exterior distances are closer than the bound
    zone = np.full(Nh, -1) if case["zone"] is None else np.where((case["zone"] >= 0) & (case["zone"] < Z), case["zone"], -1)
    zone_out = np.zeros((B, max(Z, 1)), bool)
    for b in range(B):
        for z in range(Z):
            dz = np.sort(d[b][(zone == z) & cand[b] & ~D["inside"][b]])
            zone_out[b, z] = (len(dz) >= 2 and dz[1] - dz[0] < bound_d) or (out[b] & (zone == z)).any()
    assert not (stand_in and zone_out.any()), (tag, zone_out)
    # ---- sdf, flags, counts
    keep = cand & ~out
    assert np.array_equal(np.isnan(got["sdf"])[~near], ~cand[~near]), tag              # the candidates are float64's, but for vertices on the box
    err_d = float(np.abs(np.abs(got["sdf"].astype(F64)) - d)[keep].max()) if keep.any() else 0.0
    print(f"{tag} |sdf|: kernel {err_d:.3e}  cpu-fp32 {e_cpu_d:.3e}  bound {bound_d:.3e}  candidates {got['counts'][:, 1].tolist()} of {Nh}  inside {got['counts'][:, 0].tolist()}  left out {int(out_g.sum())}")
    assert err_d <= bound_d, (tag, err_d, bound_d)
    in_k = np.nan_to_num(got["sdf"], nan=1.0) < 0
    assert np.array_equal(in_k[keep], D["inside"][keep]) and np.array_equal(got["counts"][:, 0], in_k.sum(1)), tag
    assert (np.abs(got["counts"][:, 0] - ref["counts"][:, 0]) <= out.sum(1)).all() and (np.abs(got["counts"][:, 1] - ref["counts"][:, 1]) <= near.sum(1)).all(), tag
    # ---- rep, att, loss: float64 distances under the device's flags where a vertex was left out
    lr, la = kw.get("lambda_r", 0.5), kw.get("lambda_a", 0.5)
    rep_want = np.where(in_k & cand, RHO * np.tanh(np.where(cand, d, 0.0) / RHO), 0.0).sum(1) / Nh
    clean = ~out.any(1)
    err_rep, err_att = np.abs(got["rep"] - rep_want).max(), np.abs(got["att"] - ref["att"])[clean].max() if clean.any() else 0.0
    e_cpu_v = max(np.abs(cpu["rep"] - ref["rep"])[clean].max(), np.abs(cpu["att"] - ref["att"])[clean].max()) if clean.any() else 0.0
    bound_v = max(4 * e_cpu_v, coord)
    print(f"{tag} rep {err_rep:.3e}  att {err_att:.3e}  cpu-fp32 {e_cpu_v:.3e}  bound {bound_v:.3e}  rep {got['rep'].tolist()}  att {got['att'].tolist()}")
    assert err_rep <= bound_v and err_att <= bound_v, (tag, err_rep, err_att)
    if clean.all():
        err_l = abs(float(got["loss"][0]) - float(ref["loss"][0]))
        print(f"{tag} loss {float(got['loss'][0]):.9f}  float64 {float(ref['loss'][0]):.9f}  error {err_l:.3e}")
        assert err_l <= (abs(lr) + abs(la)) * bound_v, (tag, err_l)
    # ---- winners and gradients
    contrib = np.abs(ref["g_hand"]).sum(-1) > 0
    winners_k = (np.abs(got["g_hand"]).sum(-1) > 0) & ~in_k
    for b in range(B):
        for z in range(Z):
            w = D["winner"][b, z]
            if not zone_out[b, z] and w >= 0 and la != 0 and d[b, w] > 0:
                assert winners_k[b, w] and winners_k[b][zone == z].sum() == 1, (tag, b, z)      # float64's winner, and no other vertex of the zone
    cmp = contrib & ~out_g
    for b in range(B):
        for z in range(Z):
            if zone_out[b, z] and D["winner"][b, z] >= 0:
                cmp[b, zone == z] &= D["inside"][b][zone == z]
    assert not (np.abs(got["g_hand"]).sum(-1) > 0)[~contrib & ~out_g & ~(zone_out[:, zone.clip(0)] & (zone >= 0))].any(), tag      # every other vertex: exactly 0
    if cmp.any():
        d_min = d[cmp].min()
        ref_max = np.abs(ref["g_hand"][cmp]).max()
        err_g = np.abs(got["g_hand"].astype(F64) - ref["g_hand"])[cmp].max() / ref_max
        e_cpu_g = np.abs(cpu["g_hand"].astype(F64) - ref["g_hand"])[cmp].max() / ref_max
        bound_g = max(4 * e_cpu_g, coord / d_min)
        print(f"{tag} g_hand: kernel {err_g:.3e}  cpu-fp32 {e_cpu_g:.3e}  bound {bound_g:.3e}  d_min {d_min:.3e}  compared {int(cmp.sum())}")
        assert err_g <= bound_g, (tag, err_g, bound_g)
        W = WORST.setdefault(tag, {})
        W.update(sdf=err_d, sdf_cpu=e_cpu_d, g_hand=err_g, g_hand_cpu=e_cpu_g)
        whole = np.array([not (contrib[b] & out_g[b]).any() and not zone_out[b].any() for b in range(B)]) & contrib.any(1)
        if whole.any():                                                                 # the pose sums of the samples in which nothing was left out
            dm = d[contrib & whole[:, None]].min()
            for k in ("g_rot", "g_tsl"):
                rm = np.abs(ref[k][whole]).max()
                e_k, e_c = np.abs(got[k].astype(F64) - ref[k])[whole].max() / rm, np.abs(cpu[k].astype(F64) - ref[k])[whole].max() / rm
                b_k = max(4 * e_c, coord / dm)
                print(f"{tag} {k}: kernel {e_k:.3e}  cpu-fp32 {e_c:.3e}  bound {b_k:.3e}  samples {int(whole.sum())}")
                assert e_k <= b_k, (tag, k, e_k, b_k)
                W[k], W[k + "_cpu"] = e_k, e_c
    else:
        assert not got["g_hand"].any() or out_g.any() or zone_out.any(), tag
    return got, ref


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
def test_one_vertex_against_a_box():
    got, _ = check("(1,1,box)", small(1, 1, 1, rows=[1], Z=1))
    assert got["counts"].tolist() == [[1, 1]] and got["rep"][0] > 0 and got["att"][0] == 0.0


def test_one_past_a_wave():
    got, _ = check("(2,65,{1280,box})", small(2, 65, 167, rows=[4, 1]))
    assert got["counts"][:, 0].max() > 0 and (got["att"] > 0).all()


@pytest.mark.parametrize("Nh,seed", [(255, 355), (257, 358)])      # seeds at which the cap on the vertices left out holds (checked on the host)
def test_around_a_chunk_with_three_tiles(Nh, seed):
    got, _ = check(f"(3,{Nh},{{20,1280,tri}})", small(3, Nh, seed, rows=[2, 4, 0]))
    assert got["counts"][:2, 0].max() > 0 and got["counts"][2, 0] == 0                  # one open triangle encloses nothing


def stand_in(B, seed, rows):
    from artiboost_amd.criterions import ContactLoss
    from test_gpu_interaction import stand_in_case
    c = stand_in_case(B, seed, obj_rows=rows)
    zone, Z = ContactLoss().zone_ids(778)
    return dict(table=c["table"], hand=c["hand"], rows=np.asarray(c["rows"]), rot=c["rot"], tsl=c["tsl"], zone=zone, Z=Z)


def test_stand_in_hand_and_object():
    case = stand_in(2, 36, [2, 1])                                                       # a seed at which the cap on the vertices left out holds (checked on the host)
    assert case["hand"].shape == (2, 778, 3) and (case["table"].face_off[1:] - case["table"].face_off[:-1]).tolist() == [3968] * 4 and case["Z"] == 5
    got, ref = check("(2,778,HO3D)", case, stand_in=True)
    assert (got["counts"][:, 1] < 778).all() and (got["counts"][:, 1] > 0).all() and got["counts"][:, 0].max() > 10


def boundary_case(n_in, Nh=600):
    """Exactly n_in vertices inside the object's box (a box mesh: they are inside the object), the others a centimetre or more outside it; no zones."""
    rng = np.random.default_rng(n_in)
    half = (HI - LO) / 2
    inside = rng.uniform(-0.9, 0.9, (n_in, 3)) * half
    u = rng.standard_normal((Nh - n_in, 3))
    outside = (u / np.abs(u / half).max(1, keepdims=True)) * rng.uniform(1.5, 2.5, (Nh - n_in, 1))      # on the box scaled by 1.5 - 2.5
    can = np.concatenate([inside, outside])[rng.permutation(Nh)]
    from test_interaction_host import rotation
    R, t = rotation(n_in), np.array([0.02, -0.01, 0.5])
    tb = table_of([box_mesh(LO, HI)], box_mesh(LO / 2, HI / 2))
    return dict(table=tb, hand=(can @ R.T + t)[None].astype(np.float32), rows=np.array([0]), rot=R[None].astype(np.float32), tsl=t[None].astype(np.float32), zone=None, Z=0)


@pytest.mark.parametrize("n_in", [256, 257])
def test_candidate_count_of_exactly_one_chunk_and_one_more(n_in):
    got, ref = check(f"(1,600,{n_in} candidates)", boundary_case(n_in))
    assert got["counts"].tolist() == [[n_in, n_in]] == ref["counts"].tolist() and (~np.isnan(got["sdf"])).sum() == n_in


def test_a_sample_off_its_object_without_zones_has_no_candidate():
    case = small(1, 65, 31, rows=[1], Z=0, far=(0,))
    got, _ = check("(1,65,far,Z=0)", case)
    assert got["loss"][0] == 0.0 and got["counts"].tolist() == [[0, 0]] and np.isnan(got["sdf"]).all()
    assert not got["g_hand"].any() and not got["g_rot"].any() and not got["g_tsl"].any() and got["rep"][0] == 0.0 and got["att"][0] == 0.0


def test_the_same_sample_with_zones_is_attracted_from_a_distance():
    case = small(1, 65, 31, rows=[1], Z=3, far=(0,))
    got, ref = check("(1,65,far,Z=3)", case)
    assert got["counts"][0, 0] == 0 and got["counts"][0, 1] == (case["zone"] >= 0).sum() and got["rep"][0] == 0.0
    assert abs(got["att"][0] - ALPHA) <= 1e-6 and ref["diag"]["d"][0][case["zone"] >= 0].min() > 0.15      # tanh has saturated


def test_an_unknown_object_and_a_masked_sample_contribute_nothing():
    case = small(4, 65, 80, rows=[4, 1, 3, 1])                                           # a seed at which nothing is left out (checked on the host)
    case["rows"] = np.array([4, -1, 3, 1])
    case["mask"] = np.array([1.0, 1.0, 0.0, 1.0], np.float32)
    got, ref = check("(4,65,unknown+masked)", case)
    for b in (1, 2):
        assert got["rep"][b] == 0 and got["att"][b] == 0 and got["counts"][b].tolist() == [0, 0] and np.isnan(got["sdf"][b]).all()
        assert not got["g_hand"][b].any() and not got["g_rot"][b].any() and not got["g_tsl"][b].any()
    two = _call(_take(case, [0, 3]), True)
    assert abs(got["loss"][0] - two["loss"][0] / 2) <= 1e-7 and np.array_equal(got["rep"][[0, 3]], two["rep"])      # they count in B
    past = dict(case, rows=np.array([4, 5, 3, 1]), mask=None)                                              # a row past the table's five
    assert _call(past, True)["counts"][1].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 2. determinism, the flag, batch independence
def test_scan_all_and_a_second_call_give_the_same_bits():
    from artiboost_amd import kernels as K
    for case in (small(3, 257, 358, rows=[2, 4, 0]), stand_in(2, 5, [1, 3]), small(2, 65, 31, rows=[1, 4], Z=0, far=(0,))):
        a, b = _call(case, True, want_sdf=True), _call(case, True, want_sdf=True)
        s = _call(case, True, want_sdf=True, flags=K.CL_SCAN_ALL)
        assert sorted(a) == sorted(OUT)
        for k in OUT:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
            assert np.array_equal(a[k], s[k], equal_nan=True), k
        assert (a["counts"][:, 1] < case["hand"].shape[1]).any()                        # the flag did scan more than the candidates


def test_a_sample_does_not_depend_on_its_batch():
    case = small(4, 257, 77, rows=[4, 2, 1, 3])
    full = _call(case, True, want_sdf=True)
    per = ("rep", "att", "counts", "sdf")
    grads = ("g_hand", "g_rot", "g_tsl")
    for s in range(4):
        alone = _call(_take(case, [s]), True, want_sdf=True)
        second = _call(_take(case, [(s + 1) % 4, s]), True, want_sdf=True)
        for k in per:
            assert np.array_equal(alone[k][0], full[k][s], equal_nan=True) and np.array_equal(second[k][1], full[k][s], equal_nan=True), (k, s)
        for k in grads:                                                                 # gradients carry 1 / B: compared x B
            assert np.array_equal(alone[k][0], full[k][s] * np.float32(4)) and np.array_equal(second[k][1] * np.float32(2), full[k][s] * np.float32(4)), (k, s)
        assert full["g_hand"][s].any()
    for r in range(1, 4):                                                               # every sample at each position of four
        order = [(p - r) % 4 for p in range(4)]
        rolled = _call(_take(case, order), True, want_sdf=True)
        for k in per + grads:
            assert np.array_equal(rolled[k], full[k][order], equal_nan=True), (k, r)


def test_only_the_loss_with_null_gradient_pointers():
    case = small(3, 65, 55, rows=[3, 4, 1])
    a, b = _call(case, True, want_sdf=True), _call(case, True, grad=None)
    assert sorted(b) == ["att", "counts", "loss", "rep"] and all(np.array_equal(a[k], b[k]) for k in b) and a["loss"][0] > 0


# ------------------------------------------------------------------------------------------------ 3. the dispatcher op's refusals
def test_dispatcher_op_refusals():
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    from test_gpu_interaction import small_table
    L.lib()
    op = torch.ops.artiboost_hip.contact_loss
    tb = small_table().on("cuda")
    B, Nh = 2, 5
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    ws = torch.zeros(int(torch.ops.artiboost_hip.contact_loss_workspace(B, Nh)), dtype=torch.uint8, device="cuda")
    eye = torch.eye(3, device="cuda").repeat(B, 1, 1).contiguous()

    def args(**kw):
        a = dict(hand_verts=z(B, Nh, 3), zone_id=torch.zeros(Nh, dtype=torch.int32, device="cuda"), Nh=Nh, Z=1, obj_verts=tb["obj_verts"], obj_faces=tb["obj_faces"],
                 vert_off=tb["vert_off"], face_off=tb["face_off"], obj_orient=tb["obj_orient"], obj_box=tb["obj_box"], n_obj=5,
                 obj_row=torch.tensor([1, 4], device="cuda"), rot=eye, tsl=z(B, 3), mask=None, B=B, rho=0.02, alpha=0.01, lambda_r=0.5, lambda_a=0.5, flags=0,
                 loss=z(1), rep=z(B), att=z(B), counts=torch.zeros(B, 2, dtype=torch.int32, device="cuda"), sdf=None, g_hand=z(B, Nh, 3), g_rot=z(B, 9),
                 g_tsl=z(B, 3), workspace=ws)
        a.update(kw)
        return list(a.values())
    op(*args())                                                                  # the well-formed call goes through
    op(*args(g_hand=None, g_rot=None, g_tsl=None, zone_id=None, Z=0))
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        op(*args(hand_verts=torch.zeros(B, Nh, 3)))
    with pytest.raises(RuntimeError, match="'hand_verts' holds"):
        op(*args(hand_verts=z(B * Nh * 3 - 1)))
    with pytest.raises(RuntimeError, match="'zone_id' holds"):
        op(*args(zone_id=torch.zeros(Nh - 1, dtype=torch.int32, device="cuda")))
    with pytest.raises(RuntimeError, match="'obj_box' holds"):
        op(*args(obj_box=tb["obj_box"][:4].contiguous()))
    with pytest.raises(RuntimeError, match="'g_hand' holds"):
        op(*args(g_hand=z(B, Nh - 1, 3)))
    with pytest.raises(RuntimeError, match="'sdf' holds"):
        op(*args(sdf=z(B, Nh - 1)))
    with pytest.raises(RuntimeError, match="bytes"):
        op(*args(workspace=ws[:-1]))
    for bad in (dict(flags=2), dict(rho=0.0), dict(alpha=-1.0), dict(Z=17), dict(Z=-1), dict(zone_id=None), dict(g_rot=None), dict(g_hand=None, g_rot=None),
                dict(loss=None), dict(rho=float("inf"))):
        with pytest.raises(RuntimeError, match="argument error"):
            op(*args(**bad))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="obj_row"):
        K.contact_loss(z(B, Nh, 3), None, 0, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], tb["obj_box"],
                       torch.tensor([1, 4], device="cuda", dtype=torch.int32), eye, z(B, 3))
    with pytest.raises(ValueError, match="n_zones"):
        K.contact_loss(z(B, Nh, 3), None, 17, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], tb["obj_box"],
                       torch.tensor([1, 4], device="cuda"), eye, z(B, 3))


# ------------------------------------------------------------------------------------------------ 4. the class on HIP tensors
def test_class_on_hip_tensors_matches_the_class_on_cpu_float64(monkeypatch):
    from artiboost_amd import kernels as K
    from artiboost_amd.criterions import ContactLoss
    tb, preds, targs = class_batch(3, 21)
    calls = []
    real = K.contact_loss
    monkeypatch.setattr(K, "contact_loss", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    out = {}
    for dev, dt in (("cpu", torch.float64), ("cuda", torch.float32)):
        loss = ContactLoss().set_obj_meshes(tb)
        p = {k: v.detach().clone().to(dev).to(dt).requires_grad_(True) for k, v in preds.items()}
        total, d = loss(p, {k: v.to(dev) for k, v in targs.items()})
        (2.0 * total.sum()).backward()
        out[dev] = ({k: float(v.detach()) for k, v in d.items()}, {k: v.grad.detach().cpu().double().numpy() for k, v in p.items()})
    assert calls == [(3, 778, 3)]                                                       # ONE kernel call for forward and backward
    for k, v in out["cpu"][0].items():
        print(f"{k}: cpu float64 {v:.9f}  device {out['cuda'][0][k]:.9f}")
        assert abs(out["cuda"][0][k] - v) <= 1e-6, k
    for k, g in out["cpu"][1].items():
        err = np.abs(out["cuda"][1][k] - g).max() / np.abs(g).max()
        print(f"grad {k}: relative error {err:.3e}")
        assert out["cuda"][1][k].shape == g.shape and err <= 1e-3, k


# ------------------------------------------------------------------------------------------------ 5. two eager training steps of HoNetHIP
def _train(with_loss, use_graph=False, steps=2):
    import random
    import yaml
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    from artiboost_amd.train import TrainStep
    from test_gpu_honet import ARCH, PRESET, _batch
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_contact_mi355x.yaml")))
    cfgc, lambdas = (cfg["CRITERION"], cfg["LAMBDAS"]) if with_loss else (cfg["CRITERION"][:-1], cfg["LAMBDAS"][:-1])
    random.seed(3); torch.manual_seed(3); np.random.seed(3)
    arch = dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32")
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=PRESET))
    crit = Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(cfgc, preset_cfg=PRESET, LAMBDAS=lambdas))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=3e-4, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    batch = {k: v.cuda() for k, v in _batch(4, 8, N=30).items()}
    batch["obj_idx"] = torch.tensor([9, 12, 5, 11], device="cuda")
    ts = TrainStep(model, crit, opt, batch, use_graph=use_graph)
    seen = []
    for _ in range(steps):
        _, total, losses = ts()
        torch.cuda.synchronize()
        seen.append(({k: float(v.detach()) for k, v in losses.items() if v is not None}, model.model_list[0].store.grad.detach().cpu().clone()))
    return ts, seen


def test_two_eager_honet_steps_with_the_loss_and_no_capture(monkeypatch):
    from artiboost_amd import kernels as K
    capturing = []
    real = K.contact_loss
    monkeypatch.setattr(K, "contact_loss", lambda *a, **k: (capturing.append(torch.cuda.is_current_stream_capturing()), real(*a, **k))[1])
    ts, with_loss = _train(True, use_graph=True)                                         # such a list never captures: it goes down the eager route
    assert ts.fused is None and not ts.use_graph and ts.g_fwd_bwd is None and capturing == [False, False]
    _, without = _train(False)
    for i, (losses, grad) in enumerate(with_loss):
        print(i, losses)
        assert {"contact_loss", "repulsion_loss", "attraction_loss", "final_loss"} <= set(losses) and all(np.isfinite(v) for v in losses.values())
        assert torch.isfinite(grad).all() and not torch.equal(grad, without[i][1]), i
    assert "contact_loss" not in without[0][0]


def test_print_the_error_table():
    """(last: the measured kernel errors beside the fp32 torch-CPU route's, for DESIGN.md section 26)"""
    for tag, w in WORST.items():
        print(tag + ": " + "  ".join(f"{k} {w[k]:.2e} (cpu {w[k + '_cpu']:.2e})" for k in ("sdf", "g_hand", "g_rot", "g_tsl") if k in w))
