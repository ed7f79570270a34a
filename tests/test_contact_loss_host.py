"""The contact loss on the host: the float64 torch expression (`criterions.contact_loss_torch`) against the analytic
signed distance of a box and its analytic gradient, its autograd gradient against central finite differences, the closed-form gradient of
the definitions against that autograd gradient, the zone rules, samples that contribute nothing, `ContactLoss` from a config on CPU tensors
and inside one forward + backward of the torch HoNet, and the header contract with its generated op.  The helpers are shared with
tests/test_gpu_contact_loss.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_interaction_host import HI, LO, ONE_TRI, box_mesh, icosphere, rotation, stand_in_assets, table_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64
RHO, ALPHA = 0.02, 0.01
TINY_HAND = box_mesh([-1, -1, -1], [1, 1, 1])


def run_cl(table, hand, zone, Z, rows, rot, tsl, mask=None, dtype=torch.float64, device="cpu", kernel=False, grad="closed", **kw):
    """One call of the torch expression (or of the kernel) on numpy inputs -> dict of numpy arrays.  grad: "closed" (the closed form of the
    definitions / the kernel's buffers), "autograd" (the torch expression differentiated by autograd) or None."""
    from artiboost_amd import kernels as K
    from artiboost_amd.criterions import contact_loss_torch
    tb = table.on(device)
    t = lambda a, d=dtype: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=d).contiguous()      # noqa: E731
    B = len(hand)
    hv, R, tt = t(hand), t(np.asarray(rot).reshape(B, 3, 3)), t(np.asarray(tsl).reshape(B, 3))
    zi = None if zone is None else t(zone, torch.int32)
    args = (zi, Z, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], tb["obj_box"], t(rows, torch.int64))
    m = None if mask is None else t(mask)
    if kernel:
        o = K.contact_loss(hv, *args, R, tt, mask=m, want_grad=grad is not None, **kw)
    else:
        if grad == "autograd":
            for x in (hv, R, tt):
                x.requires_grad_(True)
        o = contact_loss_torch(hv, *args, R, tt, mask=m, want_grad=grad == "closed", **kw)
        if grad == "autograd":
            o["loss"].sum().backward()
            z = lambda x: torch.zeros_like(x) if x.grad is None else x.grad      # noqa: E731
            o["g_hand"], o["g_rot"], o["g_tsl"] = z(hv), z(R), z(tt)
    diag = o.pop("diag", None)
    out = {k: v.detach().cpu().numpy() for k, v in o.items()}
    if diag is not None:
        out["diag"] = {k: v.cpu().numpy() for k, v in diag.items()}
    return out


def box_case(seed=4):
    """Points inside and outside the box [LO, HI], away from its edges, corners' bisectors and medial planes, under a general pose; the
    outside points are one zone each.  -> (table, hand [1,N,3], zone, Z, R, t, canonical points, analytic d, analytic unit n', inside)"""
    q = np.array([[0.02, 0.005, 0.01], [-0.025, -0.004, 0.03], [0.001, 0.016, -0.02], [0.004, -0.003, -0.046],          # inside: nearest face +x, -x, +y, -z
                  [0.05, 0.003, 0.01], [-0.004, 0.035, 0.02], [0.05, 0.04, 0.004], [-0.04, 0.001, 0.07], [0.05, 0.03, 0.08]], F64)
    lo, hi = LO, HI
    e = np.maximum(np.maximum(lo - q, q - hi), 0)                                      # outside: the vector from the box to q
    inside = (e == 0).all(1)
    d_out = np.linalg.norm(e, axis=1)
    face = np.minimum(q - lo, hi - q)                                                  # inside: distance to each pair's nearer face
    ax = face.argmin(1)
    d = np.where(inside, face.min(1), d_out)
    n = np.where(inside[:, None], 0.0, e * np.sign(q - (lo + hi) / 2) / np.maximum(d_out, 1e-300)[:, None])
    for i in np.nonzero(inside)[0]:                                                    # r' = q' - cp' points from the face into the box
        n[i, ax[i]] = -1.0 if hi[ax[i]] - q[i, ax[i]] < q[i, ax[i]] - lo[ax[i]] else 1.0
    zone = np.full(len(q), -1, np.int32)
    zone[~inside] = np.arange((~inside).sum())
    R, t = rotation(seed), np.array([0.03, -0.02, 0.5])
    tb = table_of([box_mesh(LO, HI)], TINY_HAND)
    return tb, (q @ R.T + t)[None], zone, int((~inside).sum()), R[None], t[None], q, d, n, inside


# ------------------------------------------------------------------------------------------------ 1. analytic values and gradient on a box
def test_box_signed_distance_loss_and_gradient_are_analytic():
    tb, hand, zone, Z, R, t, q, d, n, inside = box_case()
    N = len(q)
    lr, la = 0.7, 0.3
    got = run_cl(tb, hand, zone, Z, [0], R, t, lambda_r=lr, lambda_a=la, want_sdf=True, want_diag=True)
    want_sdf = np.where(inside, -d, d)
    print("sdf error", np.abs(got["sdf"][0] - want_sdf).max(), "counts", got["counts"].tolist())
    assert np.abs(got["sdf"][0] - want_sdf).max() <= 1e-15 and got["counts"].tolist() == [[int(inside.sum()), N]]
    assert np.array_equal(got["diag"]["inside"][0], inside) and np.abs(got["diag"]["wind"][0][inside] - 1).max() <= 1e-12
    rep = (RHO * np.tanh(d[inside] / RHO)).sum() / N
    att = (ALPHA * np.tanh(d[~inside] / ALPHA)).sum() / Z
    assert abs(got["rep"][0] - rep) <= 1e-15 and abs(got["att"][0] - att) <= 1e-15 and abs(got["loss"][0] - (lr * rep + la * att)) <= 1e-15
    wgt = np.where(inside, lr / N, la / Z)
    g = (wgt / np.cosh(d / np.where(inside, RHO, ALPHA)) ** 2)[:, None] * (n @ R[0].T)
    cp = q - n * d[:, None]
    for how in ("closed", "autograd"):
        o = run_cl(tb, hand, zone, Z, [0], R, t, lambda_r=lr, lambda_a=la, grad=how)
        scale = np.abs(g).max()
        errs = [np.abs(o["g_hand"][0] - g).max() / scale, np.abs(o["g_tsl"][0] + g.sum(0)).max() / scale,
                np.abs(o["g_rot"][0] + np.einsum("ij,ik->jk", g, cp)).max() / np.abs(np.einsum("ij,ik->jk", g, cp)).max()]
        print(how, "relative gradient errors (hand, tsl, rot)", errs)
        assert max(errs) <= 1e-10, (how, errs)


# ------------------------------------------------------------------------------------------------ 2. autograd, finite differences, closed form
def generic_case(seed, B=2, N=24):
    """Points around a posed icosphere (80 faces) and the box, three zones; generic positions."""
    rng = np.random.default_rng(seed)
    tb = table_of([icosphere(0.04, 1), box_mesh(LO, HI)], TINY_HAND)
    R = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    t = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.03, 0.03, (B, 3))
    can = rng.uniform(-0.055, 0.055, (B, N, 3))
    hand = np.einsum("bij,bnj->bni", R, can) + t[:, None]
    zone = np.full(N, -1, np.int32)
    zone[rng.permutation(N)[:12]] = np.arange(12) % 3
    return tb, hand, zone, 3, np.arange(B) % 2, R, t


@pytest.mark.parametrize("seed", [1, 2])
def test_closed_form_gradient_equals_autograd(seed):
    tb, hand, zone, Z, rows, R, t = generic_case(seed)
    a = run_cl(tb, hand, zone, Z, rows, R, t, grad="autograd", want_diag=True)
    c = run_cl(tb, hand, zone, Z, rows, R, t, grad="closed")
    assert a["counts"][:, 0].min() > 0 and (a["diag"]["winner"] >= 0).all()           # both terms are present in every sample
    for k in ("g_hand", "g_rot", "g_tsl"):
        err = np.abs(a[k] - c[k]).max() / np.abs(a[k]).max()
        print(seed, k, "closed form vs autograd", err)
        assert err <= 1e-10, (k, err)
    assert np.count_nonzero(np.abs(c["g_hand"]).sum(-1)) == a["counts"][:, 0].sum() + (a["diag"]["winner"] >= 0).sum()      # the two sets are disjoint


def _skew(k):
    return np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])


@pytest.mark.parametrize("seed", [1, 2])
def test_autograd_gradient_against_central_differences(seed):
    from scipy.linalg import expm
    tb, hand, zone, Z, rows, R, t = generic_case(seed)
    a = run_cl(tb, hand, zone, Z, rows, R, t, grad="autograd")
    rng = np.random.default_rng(100 + seed)
    L = lambda h, r, tt: float(run_cl(tb, h, zone, Z, rows, r, tt, grad=None)["loss"][0])      # noqa: E731
    eps = 1e-6
    for trial in range(3):
        uh, ut, k = rng.standard_normal(hand.shape), rng.standard_normal(t.shape), rng.standard_normal((len(R), 3))
        fd_h = (L(hand + eps * uh, R, t) - L(hand - eps * uh, R, t)) / (2 * eps)
        fd_t = (L(hand, R, t + eps * ut) - L(hand, R, t - eps * ut)) / (2 * eps)
        Rp = np.stack([r @ expm(eps * _skew(x)) for r, x in zip(R, k)]); Rm = np.stack([r @ expm(-eps * _skew(x)) for r, x in zip(R, k)])
        fd_r = (L(hand, Rp, t) - L(hand, Rm, t)) / (2 * eps)
        an_h, an_t = (a["g_hand"] * uh).sum(), (a["g_tsl"] * ut).sum()
        an_r = sum((a["g_rot"][b] * (R[b] @ _skew(k[b]))).sum() for b in range(len(R)))
        print(seed, trial, "hand", fd_h, an_h, "tsl", fd_t, an_t, "rot", fd_r, an_r)
        for fd, an in ((fd_h, an_h), (fd_t, an_t), (fd_r, an_r)):
            assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-3), (fd, an)


# ------------------------------------------------------------------------------------------------ 3. zone rules
I3, Z3 = np.eye(3)[None], np.zeros((1, 3))


def test_zone_rules():
    from artiboost_amd.criterions import ContactLoss, tip_zones
    tb = table_of([box_mesh(LO, HI)], TINY_HAND)
    inside_pts = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.01]])
    # all vertices of a zone inside: the zone contributes 0; the other zone's exterior vertex counts
    hand = np.concatenate([inside_pts, [[0.05, 0.0, 0.0]]])[None]
    o = run_cl(tb, hand, [0, 0, 1], 2, [0], I3, Z3, want_diag=True)
    assert o["diag"]["winner"].tolist() == [[-1, 2]] and abs(o["att"][0] - ALPHA * math.tanh((0.05 - HI[0]) / ALPHA) / 2) <= 1e-15 and o["counts"][0, 0] == 2
    assert np.abs(o["g_hand"][0, 2]).max() > 0 and np.abs(o["g_hand"][0, :2]).max() > 0          # repulsion on the inside ones, attraction on the winner
    # empty Z: no attraction, and a vertex outside the box is no candidate at all
    o = run_cl(tb, hand, None, 0, [0], I3, Z3, want_sdf=True)
    assert o["att"][0] == 0.0 and o["counts"].tolist() == [[2, 2]] and np.isnan(o["sdf"][0, 2]) and not o["g_hand"][0, 2].any()
    # a tie: two exterior vertices of one zone at the same distance; the lowest index wins, whichever comes first
    for pts in ([[0.05, 0.0, 0.0], [-0.05, 0.0, 0.0]], [[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]]):
        o = run_cl(tb, np.array([pts + [[0.0, 0.06, 0.0]]], F64), [0, 0, 0], 1, [0], I3, Z3, want_diag=True)
        assert o["diag"]["d"][0, 0] == o["diag"]["d"][0, 1] < o["diag"]["d"][0, 2] and o["diag"]["winner"].tolist() == [[0]]
        assert o["g_hand"][0, 0].any() and not o["g_hand"][0, 1:].any()
    # a vertex in two tip spheres goes to the lower zone
    v = np.array([[0.0, 0, 0], [0.012, 0, 0], [0.006, 0, 0], [0.03, 0, 0]])
    assert tip_zones(v, (1, 0), 0.01).tolist() == [1, 0, 0, -1]
    assert tip_zones(v, (0, 1), 0.01).tolist() == [0, 1, 0, -1]
    assert ContactLoss(ZONES=[[3, 2], [2, 1]]).zone_ids(4)[0].tolist() == [-1, 1, 0, 0]
    # the shipped zones on the hand model: five zones, each holding its tip
    zone, Z = ContactLoss().zone_ids(778)
    assert Z == 5 and [int(zone[i]) for i in ContactLoss.TIPS] == [0, 1, 2, 3, 4] and (zone >= 0).sum() >= 5 and zone.min() == -1


def test_masked_and_unknown_samples_contribute_nothing_and_count_in_the_batch():
    tb, hand, zone, Z, R, t, *_ = box_case()
    one = run_cl(tb, hand, zone, Z, [0], R, t, want_sdf=True)
    h3, R3, t3 = np.repeat(hand, 3, 0), np.repeat(R, 3, 0), np.repeat(t, 3, 0)
    o = run_cl(tb, h3, zone, Z, [0, -1, 0], R3, t3, mask=[1.0, 1.0, 0.0], want_sdf=True)
    assert abs(o["loss"][0] - one["loss"][0] / 3) <= 1e-16 and o["rep"][1:].tolist() == [0, 0] and o["att"][1:].tolist() == [0, 0]
    assert o["counts"][1:].tolist() == [[0, 0], [0, 0]] and np.isnan(o["sdf"][1:]).all() and not o["g_hand"][1:].any() and not o["g_rot"][1:].any()
    assert np.allclose(o["g_hand"][0] * 3, one["g_hand"][0], rtol=1e-14, atol=0) and np.array_equal(o["sdf"][0], one["sdf"][0])
    big = run_cl(tb, hand, zone, Z, [7], R, t)                                          # a row past the table
    assert big["loss"][0] == 0.0 and not big["g_hand"].any()


# ------------------------------------------------------------------------------------------------ 4. the class: config, registry, KeyErrors
def class_batch(B=3, seed=21, dtype=torch.float64):
    """(table, preds, targs): 778 "hand" points around posed stand-in objects, some inside."""
    from artiboost_amd.metrics import ObjectMeshTable
    rng = np.random.default_rng(seed)
    tb = ObjectMeshTable.from_assets(stand_in_assets())
    ids = rng.choice(tb.obj_ids, B)
    R = np.stack([rotation(int(s)) for s in rng.integers(0, 1000, B)])
    t = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.02, 0.02, (B, 3))
    hand = rng.uniform(-0.04, 0.04, (B, 778, 3)) + (t + rng.uniform(-0.03, 0.03, (B, 3)))[:, None]
    T = np.tile(np.eye(4), (B, 1, 1)); T[:, :3, :3], T[:, :3, 3] = R, t
    tt = lambda a: torch.as_tensor(a).to(dtype)      # noqa: E731
    return tb, {"hand_verts_3d_abs": tt(hand), "box_rot_rotmat": tt(R), "boxroot_3d_abs": tt(t).reshape(B, 1, 3)}, {"obj_idx": torch.as_tensor(ids), "obj_transf": tt(T)}


def test_config_parsing_registry_lookup_and_key_errors():
    import yaml
    from anakin.criterions.contactloss import ContactLoss as Alias
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import ContactLoss
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_contact_mi355x.yaml")))
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_mi355x.yaml")))
    assert cfg["CRITERION"][:-1] == base["CRITERION"] and cfg["LAMBDAS"] == base["LAMBDAS"] + [1.0]
    assert {k: v for k, v in cfg.items() if k not in ("CRITERION", "LAMBDAS")} == {k: v for k, v in base.items() if k not in ("CRITERION", "LAMBDAS")}
    loss = R.build_criterion_loss_list(cfg["CRITERION"], preset_cfg=cfg["DATA_PRESET"], LAMBDAS=cfg["LAMBDAS"])[-1]
    assert type(loss) is ContactLoss is Alias and loss.table.row_of == {9: 0, 12: 1, 5: 2, 11: 3} and loss.output_key == "contact_loss_output"
    assert (loss.lambda_repulsion, loss.lambda_attraction, loss.rho, loss.alpha, loss.zone_radius, loss.obj_pose, loss.zones) == (0.5, 0.5, 0.02, 0.01, 0.01, "pred", "tips")
    d = ContactLoss()
    assert (d.lambda_repulsion, d.lambda_attraction, d.rho, d.alpha, d.hand_key, d.rot_key, d.tsl_key, d.obj_pose, d.table) == \
        (0.5, 0.5, 0.02, 0.01, "hand_verts_3d_abs", "box_rot_rotmat", "boxroot_3d_abs", "pred", None)
    for bad in (dict(REPULSE_MM=0), dict(ATTRACT_MM=-1), dict(OBJ_POSE="both"), dict(ZONES="palm"), dict(ZONES=[[0]] * 17), dict(OBJ_MESHES={"SOURCE": "files"})):
        with pytest.raises(ValueError):
            ContactLoss(**bad)
    tb, preds, targs = class_batch()
    with pytest.raises(RuntimeError, match="no object meshes"):
        ContactLoss()(preds, targs)
    loss = ContactLoss().set_obj_meshes(tb)
    with pytest.raises(KeyError, match="obj_idx"):
        loss(preds, {})
    for k in preds:
        with pytest.raises(KeyError, match=k):
            loss({kk: v for kk, v in preds.items() if kk != k}, targs)
    gt = ContactLoss(OBJ_POSE="gt").set_obj_meshes(tb)
    with pytest.raises(KeyError, match="obj_transf"):
        gt(preds, {"obj_idx": targs["obj_idx"]})
    # the values, the None conventions, and where the gradient goes
    p = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    total, d = loss(p, targs)
    assert set(d) == {"contact_loss", "repulsion_loss", "attraction_loss", "contact_loss_output"} and d["repulsion_loss"] > 0 and d["attraction_loss"] > 0
    assert abs(float(d["contact_loss"].detach()) - 0.5 * float(d["repulsion_loss"]) - 0.5 * float(d["attraction_loss"])) <= 1e-15
    total.sum().backward()
    assert all(v.grad is not None and v.grad.abs().max() > 0 for v in p.values()) and p["boxroot_3d_abs"].grad.shape == (3, 1, 3)
    p2 = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    total2, d2 = gt(p2, targs)                                                          # the same pose from the annotation: the same value, no pose gradient
    total2.sum().backward()
    assert float(d2["contact_loss"]) == float(d["contact_loss"]) and torch.equal(p2["hand_verts_3d_abs"].grad, p["hand_verts_3d_abs"].grad)
    assert p2["box_rot_rotmat"].grad is None and p2["boxroot_3d_abs"].grad is None
    off = ContactLoss(LAMBDA_REPULSION=0.0, LAMBDA_ATTRACTION=0.0)(preds, targs)[1]
    assert off["contact_loss"] is None and off["repulsion_loss"] is None and off["attraction_loss"] is None
    half = ContactLoss(LAMBDA_ATTRACTION=0.0).set_obj_meshes(tb)(preds, targs)[1]
    assert half["attraction_loss"] is None and half["repulsion_loss"] is not None and abs(float(half["contact_loss"]) - 0.5 * float(d["repulsion_loss"])) <= 1e-15
    unknown = loss(preds, {"obj_idx": torch.tensor([400, 9, 7])})[1]                    # two ids the table lacks: they count in B
    one = loss({k: v[1:2] for k, v in preds.items()}, {"obj_idx": torch.tensor([9])})[1]
    assert abs(float(unknown["contact_loss"]) - float(one["contact_loss"]) / 3) <= 1e-15


def test_class_on_cpu_tensors_inside_one_forward_and_backward_of_the_torch_honet():
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from test_gpu_honet import ARCH, CRIT, PRESET, _batch
    torch.manual_seed(0)
    model = R.build_arch_model_list(ARCH, preset_cfg=PRESET)[0]
    model.train()
    cfgc = CRIT + [{"TYPE": "ContactLoss", "ATTRACT_MM": 1000, "OBJ_MESHES": {"SOURCE": "assets", "DATASET": "HO3D"}}]
    crit = Criterion({"LAMBDAS": [1.0, 1.0, 1.0]}, R.build_criterion_loss_list(cfgc, preset_cfg=PRESET, LAMBDAS=[1.0, 1.0, 1.0]))
    batch = _batch(2, 31, N=30)
    batch["obj_idx"] = torch.tensor([9, 11])
    preds = model(batch)
    for k in ("hand_verts_3d_abs", "box_rot_rotmat", "boxroot_3d_abs"):
        preds[k].retain_grad()
    total, losses = crit.compute_losses(preds, batch)
    assert {"contact_loss", "repulsion_loss", "attraction_loss", "hand_verts_3d_loss", "final_loss"} <= set(losses) and torch.isfinite(total).all()
    assert float(losses["attraction_loss"]) > 0
    total.sum().backward()
    assert preds["box_rot_rotmat"].grad.abs().max() > 0 and preds["boxroot_3d_abs"].grad.abs().max() > 0
    g = torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])
    assert torch.isfinite(g).all() and g.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 5. the box, the header contract, the generated op
def test_object_box_is_the_exact_fp32_box_of_the_canonical_vertices():
    tb = table_of([ONE_TRI, box_mesh(LO, HI), icosphere(0.04, 1)], TINY_HAND)
    assert tb.box.dtype == np.float32 and tb.box.shape == (3, 6) and tuple(tb.on("cpu")["obj_box"].shape) == (3, 6)
    for r in range(3):
        v = tb.verts[tb.vert_off[r]:tb.vert_off[r + 1]]
        assert np.array_equal(tb.box[r], np.concatenate([v.min(0), v.max(0)]))


def test_header_contract_and_generated_op():
    from artiboost_amd import _lib as L
    from artiboost_amd import gen_torch_ops, kernels
    txt = open(gen_torch_ops.HEADER).read()
    assert re.search(r"@check\s+ab_contact_loss:", txt) and re.search(r"\bint\s+ab_contact_loss\s*\(", txt) and re.search(r"\blong\s+ab_contact_loss_workspace\s*\(", txt)
    assert {"ab_contact_loss", "ab_contact_loss_workspace"} <= set(L.declared_symbols())
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    cons = gen_torch_ops.contracts()["ab_contact_loss"]
    assert any("ab_contact_loss_workspace(B,Nh)" in c for c in cons)
    src = open(gen_torch_ops.OUT).read()
    _, schema, body = gen_torch_ops.schema_and_wrapper("int", "ab_contact_loss", decl["ab_contact_loss"], cons)
    assert body in src and f'm.def("{schema}");' in src                         # the committed source is what the generator writes
    assert kernels.CL_SCAN_ALL == 1 and re.search(r"#define AB_CL_SCAN_ALL 1\b", txt)
    block = txt[txt.index("Contact loss: hand-object repulsion"):txt.index("long ab_contact_loss_workspace")]
    assert re.search(r"not captured in a hipGraph", block) and "o w(q) > 0.5" in block
    hip = open(os.path.join(ROOT, "artiboost_amd", "csrc", "contact_loss.hip")).read()
    assert "never captured in a hipGraph" in hip and "atomic" not in hip.replace("No atomics", "") and '#include "ia_tile.h"' in hip
    assert '#include "ia_tile.h"' in open(os.path.join(ROOT, "artiboost_amd", "csrc", "interact.hip")).read()


def test_capture_refuses_a_step_that_holds_the_loss_before_touching_the_device(monkeypatch):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.train import TrainStep
    from test_mesh_losses_device_host import _Arch, _NoCuda, _Opt, _Store
    for k in ("AB_FAKE_COMM", "AB_DDP_SINGLE_RANK", "AB_DDP_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    cfgc = [{"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}, {"TYPE": "ContactLoss"}]
    crit = Criterion({"LAMBDAS": [1.0, 1.0]}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=[1.0, 1.0]))
    hb = type("Model", (), dict(store=_Store(), ncomps=15, inp_res=[64, 64], center_idx=0))()
    batch = {"root_joint": torch.zeros(2, 3), "joints_3d": torch.zeros(2, 21, 3)}
    ts = TrainStep(_Arch(hb), crit, _Opt(), batch, use_graph=True, fused_criterion=False)
    assert ts.use_graph and ts.fused is None            # the one construction that reaches _capture with such a list
    monkeypatch.setattr(torch, "cuda", _NoCuda())
    with pytest.raises(NotImplementedError, match="ContactLoss runs on the eager route only"):
        ts._capture()
    with pytest.raises(NotImplementedError, match="eager route only"):
        ts()
