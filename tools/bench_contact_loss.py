#!/usr/bin/env python
"""Times the contact loss on the device, ab_contact_loss against the torch expression, and prints / writes one JSON document.

  B = 64, Nh = 778: the stand-in hand posed by ab_mano_lbs at the assets' grasps against the stand-in HO3D table (4 objects of 3 968
  faces), the fingertip zones of `ContactLoss` (the inputs of tools/bench_interaction.py).
    "hip_culled" / "hip_scan_all":   one kernels.contact_loss call with its gradients, scanning the candidates / every vertex
                                     (AB_CL_SCAN_ALL; the outputs have the same bits, which is checked here too)
    "hip_culled_no_grad":            the same call with the gradient pointers NULL
    "class_fwd_bwd":                 ContactLoss on HIP tensors, forward + backward through torch.autograd
    "torch_fwd_bwd":                 criterions.contact_loss_torch (the route of CPU tensors) on the SAME device tensors, fp32, forward + backward
    "honet_step_base" / "honet_step_with_loss":   the eager HoNetHIP training step of tools/bench_honet.py without and with the loss in
                                     its criterion list (the criterion of config/ho3dv2_honet_contact_mi355x.yaml)
  The routes are measured as alternating rounds in one process, each sample the device-event time of `--inner` back-to-back repetitions
  (the torch expression: one) followed by a synchronise, after a warm-up; median and range over `--pairs` rounds.  Also the mean
  candidate fraction and the loss by both routes.  Nothing here captures a graph.

Usage: python tools/bench_contact_loss.py [--pairs 7] [--inner 5] [--out profiles/contact_loss_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = 64


def _honet_step(with_loss, ids):
    import yaml
    import artiboost_amd.honet  # noqa: F401
    import bench_honet as BH
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    from artiboost_amd.train import TrainStep
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_contact_mi355x.yaml")))
    arch = dict(cfg["ARCH"], DEVICE="cuda")
    preset = {"IMAGE_SIZE": list(BH.SIZE), "HEATMAP_SIZE": [16, 16], "CENTER_IDX": 0}
    crit_cfg, lambdas = (cfg["CRITERION"], cfg["LAMBDAS"]) if with_loss else (cfg["CRITERION"][:-1], cfg["LAMBDAS"][:-1])
    torch.manual_seed(0)
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=preset))
    crit = Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(crit_cfg, preset_cfg=preset, LAMBDAS=lambdas))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=1e-4, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    hst, ost, K, joints, verts, can, ccan = BH._inputs(B, 300, seed=1)
    g = torch.Generator().manual_seed(2)
    batch = {"image": (torch.rand(B, 3, BH.SIZE[1], BH.SIZE[0], generator=g) - 0.5).cuda(), "cam_intr": K, "corners_can": ccan, "obj_verts_can": can,
             "root_joint": torch.tensor([0.0, 0.0, 0.5]).repeat(B, 1).cuda(), "joints_3d": joints, "hand_verts_3d": verts,
             "obj_verts_3d": can + 0.05, "corners_3d": ccan + 0.05, "obj_idx": ids.clone()}
    ts = TrainStep(model, crit, opt, batch, use_graph=False)
    assert ts.fused is None and not ts.use_graph
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contact_loss needs a HIP device")
    from artiboost_amd import kernels as K
    from artiboost_amd import metrics as MT
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.criterions import ContactLoss, contact_loss_torch
    from bench_interaction import _case, _event_ms, _stats
    assets = SceneAssets("HO3D", seed=1)
    table = MT.ObjectMeshTable.from_assets(assets)
    hand, ids, rot, tsl = _case(assets, table)
    tb = table.on(hand.device)
    loss = ContactLoss().set_obj_meshes(table)
    zone, Z = loss._zone_on(778, hand.device)
    args = (zone, Z, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], tb["obj_box"], table.rows(ids))
    kw = dict(rho=loss.rho, alpha=loss.alpha, lambda_r=loss.lambda_repulsion, lambda_a=loss.lambda_attraction)
    preds = {"hand_verts_3d_abs": hand.clone().requires_grad_(True), "box_rot_rotmat": rot.clone().requires_grad_(True),
             "boxroot_3d_abs": tsl.reshape(B, 1, 3).clone().requires_grad_(True)}
    leaves = [hand.clone().requires_grad_(True), rot.clone().requires_grad_(True), tsl.clone().requires_grad_(True)]

    def run_class():
        loss(preds, {"obj_idx": ids})[0].sum().backward()

    def run_torch():
        contact_loss_torch(leaves[0], *args, leaves[1], leaves[2], **kw)["loss"].sum().backward()

    routes = {"hip_culled": lambda: K.contact_loss(hand, *args, rot, tsl, **kw),
              "hip_scan_all": lambda: K.contact_loss(hand, *args, rot, tsl, flags=K.CL_SCAN_ALL, **kw),
              "hip_culled_no_grad": lambda: K.contact_loss(hand, *args, rot, tsl, want_grad=False, **kw),
              "class_fwd_bwd": run_class, "torch_fwd_bwd": run_torch}
    if not a.no_step:
        routes["honet_step_base"], routes["honet_step_with_loss"] = _honet_step(False, ids), _honet_step(True, ids)
    culled = {k: v.clone() for k, v in K.contact_loss(hand, *args, rot, tsl, want_sdf=True, **kw).items()}
    scan_all = K.contact_loss(hand, *args, rot, tsl, want_sdf=True, flags=K.CL_SCAN_ALL, **kw)
    same_bits = all(torch.equal(culled[k].view(torch.int32) if culled[k].dtype == torch.float32 else culled[k],
                                scan_all[k].view(torch.int32) if scan_all[k].dtype == torch.float32 else scan_all[k]) for k in culled)
    torch_loss = float(contact_loss_torch(hand, *args, rot, tsl, **kw)["loss"])
    inner = {k: (1 if k.startswith("torch") else a.inner) for k in routes}
    for k, fn in routes.items():
        _event_ms(fn, 1 if k.startswith("torch") else 3)
    ms = {k: [] for k in routes}
    for _ in range(a.pairs):
        for k, fn in routes.items():
            if k.startswith("torch") and len(ms[k]) >= 3:      # the torch expression takes long per call: three rounds
                continue
            ms[k].append(_event_ms(fn, inner[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    cnt = culled["counts"].double().cpu().numpy()
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "inner": a.inner, "B": B, "Nh": 778, "faces_per_object": int(table.face_off[1]), "zones": Z,
           **{k + "_ms": _stats(v) for k, v in ms.items()},
           "scan_all_over_culled": round(med["hip_scan_all"] / med["hip_culled"], 3),
           "torch_over_class": round(med["torch_fwd_bwd"] / med["class_fwd_bwd"], 1),
           "scan_all_has_the_bits_of_culled": bool(same_bits),
           "mean_candidate_fraction": round(float(cnt[:, 1].mean() / 778), 4), "mean_inside_fraction": round(float(cnt[:, 0].mean() / 778), 4),
           "loss_hip": float(culled["loss"]), "loss_torch_fp32_on_device": torch_loss,
           "repulsion_mean": float(culled["rep"].mean()), "attraction_mean": float(culled["att"].mean())}
    if not a.no_step:
        out["loss_cost_in_the_eager_step_ms"] = round(med["honet_step_with_loss"] - med["honet_step_base"], 5)
        out["loss_share_of_the_eager_step"] = round((med["honet_step_with_loss"] - med["honet_step_base"]) / med["honet_step_with_loss"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
