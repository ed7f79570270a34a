#!/usr/bin/env python
"""Times the hand-object interaction measures of the evaluator on the device, ab_interaction against the torch expression, and prints /
writes one JSON document.

  B = 64, Nh = 778: the stand-in hand posed by ab_mano_lbs at the assets' grasps, objects at 0.45 - 0.55 m depth.
    "hip_<table>_verts" / "hip_<table>_both":   one kernels.interaction call without / with the intersection volume, <table> = ho3d (4
                        stand-in objects of 3 968 faces) or dexycb (21 stand-in objects of 16 128 faces)
    "torch_<table>_verts" / "torch_ho3d_both":  metrics.interaction_values_torch (the route of CPU tensors) on the SAME device tensors, fp32
                        (the DexYCB table with the volume is left out: minutes per call)
    "evaluator_base" / "evaluator_with_interaction":  feed_all of the EVALUATOR list of config/ho3dv2_honet_meshmetrics_mi355x.yaml and of
                        config/ho3dv2_honet_interaction_mi355x.yaml (the same list + InteractionMetric)
  The routes are measured as alternating rounds in one process, each sample the device-event time of `--inner` back-to-back repetitions
  (the torch expression: one) followed by a synchronise, after a warm-up; median and range over `--pairs` rounds.  Also the measures of
  the batch by both routes.  Nothing here captures a graph.

  --epoch-report: instead, ArtiBoostLoader.prepare() on the stand-in assets once without a refiner and once with the REFINER block the
  tests use (no checkpoint: the seeded stand-in weights of tools/bench_refiner.py), and the measures of the epoch's own grasps (the epoch's hand vertices and object poses) printed for both.  A print-out;
  nothing asserts its values.

Usage: python tools/bench_interaction.py [--pairs 7] [--inner 5] [--out profiles/interaction_bench.json] [--epoch-report [--samples 256]]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
B = 64


def _rotations(rng, n):
    q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def _case(assets, table, seed=0):
    """Device tensors (hand [B,778,3], obj_idx [B] class ids, rot [B,3,3], tsl [B,3]) of a batch of stand-in grasps."""
    from artiboost_amd.assets import make_grasps
    from artiboost_amd.synth import ManoLayerHIP
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, table.n_obj, B)
    pose, shape, tsl = make_grasps(table.n_obj, 50, seed=6)
    g = rng.integers(0, 50, B)
    verts = ManoLayerHIP(assets.hand)(torch.from_numpy(pose[rows, g]).cuda(), torch.from_numpy(shape[rows, g]).cuda())[0] + torch.from_numpy(tsl[rows, g]).cuda()[:, None]
    R = torch.from_numpy(_rotations(rng, B).astype(np.float32)).cuda()
    t = torch.from_numpy(np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.45, 0.55, B)], 1).astype(np.float32)).cuda()
    hand = (verts @ R.transpose(1, 2) + t[:, None]).contiguous()
    return hand, torch.tensor([table.obj_ids[r] for r in rows]).cuda(), R.contiguous(), t.contiguous()


def _event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def _measures(val):
    rows, cnt = val["rows"].double().cpu().numpy(), val["counts"].cpu().numpy()
    ok = cnt[:, 3] == 0
    return {"pen_depth_mm": 1e3 * rows[:, 0].mean(), "pen_mean_mm": 1e3 * rows[:, 1].mean(), "min_dist_mm": 1e3 * rows[:, 2].mean(), "inside_frac": rows[:, 3].mean(),
            "contact_ratio": rows[:, 4].mean(), "inter_vol_cm3": float(1e6 * rows[ok, 5].mean()) if ok.any() and not np.isnan(rows[ok, 5]).any() else None,
            "capped": int((~ok).sum()), "n_lattice_mean": float(cnt[:, 1].mean())}


def epoch_report(samples):
    import copy
    import yaml
    from artiboost_amd import metrics as MT
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.synth import ArtiBoostLoader
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_clasbased_artiboost_mi355x.yaml")))
    assets = SceneAssets("HO3D", seed=1)
    table = MT.ObjectMeshTable.from_assets(assets)
    metric = MT.InteractionMetric().set_obj_meshes(table)
    out = {}
    for name in ("no_refiner", "refiner_stand_in"):
        mcfg = copy.deepcopy(cfg["MANAGER"])
        if name != "no_refiner":
            mcfg["REFINER"] = {"TYPE": "hand_obj", "PRETRAINED": "", "ITERS": 3, "ALLOW_RANDOM_INIT": True}
        loader = ArtiBoostLoader.from_assets(assets, mcfg, cfg["DATA_PRESET"], 64, samples, compute_dtype=torch.float32, random_seed=3)
        if loader.refiner is not None:
            from bench_refiner import random_state_dict
            loader.refiner.load_state_dict(random_state_dict(4))      # GrabNet's refinenet.pt is a download: seeded stand-in weights
        loader.prepare()
        ep = loader.epoch_poses
        pose = ep["obj_pose"].float()
        ids = torch.as_tensor(assets.obj_idx)[torch.as_tensor(np.asarray(ep["obj_id"])).long()].cuda()
        vals = [metric.values(ep["hand_verts"][s:s + 64].float(), pose[s:s + 64, :3, :3], pose[s:s + 64, :3, 3], ids[s:s + 64]) for s in range(0, samples, 64)]
        out[name] = _measures({k: torch.cat([v[k] for v in vals]) for k in ("rows", "counts")})
        print(f"{name:>18}: " + "  ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in out[name].items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--epoch-report", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interaction_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interaction needs a HIP device")
    if a.epoch_report:
        epoch_report(a.samples)
        return
    import yaml
    from artiboost_amd import kernels as K
    from artiboost_amd import metrics as MT
    from artiboost_amd import registry as R
    from artiboost_amd.assets import SceneAssets
    from bench_mesh_metrics import _batch
    routes, values, faces = {}, {}, {}
    for name in ("ho3d", "dexycb"):
        assets = SceneAssets("HO3D" if name == "ho3d" else "DexYCB", seed=1)
        table = MT.ObjectMeshTable.from_assets(assets)
        faces[name] = int(table.face_off[1])
        hand, ids, rot, tsl = _case(assets, table)
        tb = table.on(hand.device)
        args = (hand, tb["hand_faces"], table.hand_orient, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], table.rows(ids), rot, tsl)
        for what, flags in (("verts", K.IA_VERTS), ("both", K.IA_VERTS | K.IA_VOLUME)):
            routes[f"hip_{name}_{what}"] = lambda args=args, flags=flags: K.interaction(*args, flags=flags)
            if name == "ho3d" or what == "verts":
                routes[f"torch_{name}_{what}"] = lambda args=args, flags=flags: MT.interaction_values_torch(*args, flags=flags)
        if name == "ho3d":
            ho3d = (hand, ids, rot, tsl)
    # the HoNet evaluator lists on a validation batch that carries the stand-in grasps
    preds, targs = _batch()
    hand, ids, rot, tsl = ho3d
    preds.update(hand_verts_3d_abs=hand, box_rot_rotmat=rot, boxroot_3d_abs=tsl.reshape(B, 1, 3))
    targs.update(hand_verts_3d=hand - targs["root_joint"][:, None] + 0.004 * torch.randn(B, 778, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1)), obj_idx=ids)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_interaction_mi355x.yaml")))
    base_cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_meshmetrics_mi355x.yaml")))
    build = lambda c: MT.Evaluator(cfg, R.build_evaluator_metric_list(c, cfg["DATA_PRESET"]))      # noqa: E731
    ev_base, ev_with = build(base_cfg["EVALUATOR"]), build(cfg["EVALUATOR"])
    routes["evaluator_base"] = lambda: ev_base.feed_all(preds, targs, losses={})
    routes["evaluator_with_interaction"] = lambda: ev_with.feed_all(preds, targs, losses={})
    inner = {k: (1 if k.startswith("torch") else a.inner) for k in routes}
    for k, fn in routes.items():
        values[k] = fn()
        _event_ms(fn, 1 if k.startswith("torch") else 3)
    ms = {k: [] for k in routes}
    for _ in range(a.pairs):
        for k, fn in routes.items():
            if k.startswith("torch") and len(ms[k]) >= 3:      # the torch expression takes seconds per call: three rounds
                continue
            ms[k].append(_event_ms(fn, inner[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "inner": a.inner, "B": B, "Nh": 778, "faces_per_object": faces,
           **{k + "_ms": _stats(v) for k, v in ms.items()},
           **{f"torch_over_hip_{k[4:]}": round(med["torch_" + k[4:]] / med[k], 1) for k in med if k.startswith("hip_") and "torch_" + k[4:] in med},
           "interaction_cost_in_the_evaluator_ms": round(med["evaluator_with_interaction"] - med["evaluator_base"], 5),
           "measures_hip": {k[4:]: _measures(values[k]) for k in values if k.startswith("hip_") and k.endswith("both")},
           "measures_torch_fp32_on_device": {"ho3d_both": _measures(values["torch_ho3d_both"])},
           "evaluator_measures": {k: v for k, v in ev_with.get_measures_all().items() if k in MT.IA_MEASURES}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
