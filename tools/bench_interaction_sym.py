#!/usr/bin/env python
"""Times the reverse direction of the interaction measures on the device, ab_interaction_sym (the object's vertices against the hand mesh)
beside ab_interaction's vertex scan and the torch expression of the new route, and prints / writes one JSON document.

  B = 64, Nh = 778: the stand-in hand posed by ab_mano_lbs at the assets' grasps, objects at 0.45 - 0.55 m depth (the batch of
  tools/bench_interaction.py), <table> = ho3d (4 stand-in objects of 2 048 vertices / 3 968 faces) or dexycb (21 of 8 192 / 16 128).
    "hip_sym_<table>"     one kernels.interaction_sym call (no optional outputs)
    "hip_verts_<table>"   one kernels.interaction call with the vertex flag only, in the same rounds
    "torch_sym_<table>"   metrics.interaction_sym_values_torch (the route of CPU tensors) on the SAME device tensors, fp32
  The routes are measured as alternating rounds in one process, each sample the device-event time per call of `--inner` back-to-back
  calls (the torch expression: one) followed by a synchronise, after a warm-up; median and range over `--pairs` rounds (the torch
  expression: three).  pairs/s counts (query, triangle) pairs: B x No x Fh for the new scan, B x Nh x F for the one-sided one.  Also the
  measures of the batch by both routes.  Nothing here captures a graph.

  --epoch-report: instead, ArtiBoostLoader.prepare() on the stand-in assets once without a refiner and once with the REFINER block the
  tests use (the seeded stand-in weights of tools/bench_refiner.py), and the symmetric measures of the epoch's own grasps printed for
  both.  A print-out; nothing asserts its values.

Usage: python tools/bench_interaction_sym.py [--pairs 7] [--inner 5] [--out profiles/interaction_sym_bench.json] [--epoch-report [--samples 256]]"""
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
from bench_interaction import B, _case, _event_ms, _stats  # noqa: E402  (the same batch and the same timing protocol)


def _measures(one, sym):
    o, s = one["rows"].double().cpu().numpy(), sym["rows"].double().cpu().numpy()
    return {"obj_pen_depth_mm": 1e3 * s[:, 0].mean(), "obj_pen_mean_mm": 1e3 * s[:, 1].mean(), "obj_min_dist_mm": 1e3 * s[:, 2].mean(), "obj_inside_frac": s[:, 3].mean(),
            "sym_pen_depth_mm": 1e3 * np.maximum(o[:, 0], s[:, 0]).mean(), "sym_contact_ratio": np.maximum(o[:, 4], s[:, 4]).mean(),
            "pen_depth_mm": 1e3 * o[:, 0].mean(), "contact_ratio": o[:, 4].mean(), "n_obj_inside_mean": float(sym["counts"][:, 0].double().mean())}


def epoch_report(samples):
    import copy
    import yaml
    from artiboost_amd import metrics as MT
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.synth import ArtiBoostLoader
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_clasbased_artiboost_mi355x.yaml")))
    assets = SceneAssets("HO3D", seed=1)
    table = MT.ObjectMeshTable.from_assets(assets)
    metric = MT.InteractionMetric(VOLUME=False, SYMMETRIC=True).set_obj_meshes(table)
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
        batches = [(ep["hand_verts"][s:s + 64].float(), pose[s:s + 64, :3, :3], pose[s:s + 64, :3, 3], ids[s:s + 64]) for s in range(0, samples, 64)]
        one, sym = [metric.values(*b) for b in batches], [metric.values_sym(*b) for b in batches]
        cat = lambda vals: {k: torch.cat([v[k] for v in vals]) for k in ("rows", "counts")}      # noqa: E731
        out[name] = _measures(cat(one), cat(sym))
        print(f"{name:>18}: " + "  ".join(f"{k} {v:.4g}" for k, v in out[name].items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--epoch-report", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interaction_sym_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interaction_sym needs a HIP device")
    if a.epoch_report:
        epoch_report(a.samples)
        return
    from artiboost_amd import kernels as K
    from artiboost_amd import metrics as MT
    from artiboost_amd.assets import SceneAssets
    routes, pairs, shapes = {}, {}, {}
    for name in ("ho3d", "dexycb"):
        assets = SceneAssets("HO3D" if name == "ho3d" else "DexYCB", seed=1)
        table = MT.ObjectMeshTable.from_assets(assets)
        hand, ids, rot, tsl = _case(assets, table)
        tb = table.on(hand.device)
        rows = table.rows(ids)
        Fh, F, No = int(tb["hand_faces"].shape[0]), int(table.face_off[1]), int(table.vert_off[1])
        shapes[name] = {"No": No, "F": F, "Fh": Fh, "no_max": table.no_max}
        sym_args = (hand, tb["hand_faces"], table.hand_orient, tb["obj_verts"], tb["vert_off"], rows, rot, tsl, table.no_max)
        one_args = (hand, tb["hand_faces"], table.hand_orient, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], rows, rot, tsl)
        routes[f"hip_sym_{name}"] = lambda args=sym_args: K.interaction_sym(*args)
        routes[f"hip_verts_{name}"] = lambda args=one_args: K.interaction(*args, flags=K.IA_VERTS)
        routes[f"torch_sym_{name}"] = lambda args=sym_args: MT.interaction_sym_values_torch(*args)
        pairs[f"hip_sym_{name}"], pairs[f"hip_verts_{name}"] = B * No * Fh, B * hand.shape[1] * F
    inner = {k: (1 if k.startswith("torch") else a.inner) for k in routes}
    values = {}
    for k, fn in routes.items():
        values[k] = fn()
        _event_ms(fn, 1 if k.startswith("torch") else 3)
    ms = {k: [] for k in routes}
    for _ in range(a.pairs):
        for k, fn in routes.items():
            if k.startswith("torch") and len(ms[k]) >= 3:      # the torch expression takes a long time per call: three rounds
                continue
            ms[k].append(_event_ms(fn, inner[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rate = {k: pairs[k] / (med[k] * 1e-3) for k in pairs}
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "inner": a.inner, "B": B, "Nh": 778, "shapes": shapes,
           **{k + "_ms": _stats(v) for k, v in ms.items()},
           "pairs_per_call": pairs, "pairs_per_s": {k: float(f"{v:.4g}") for k, v in rate.items()},
           **{f"sym_over_verts_rate_{n}": round(rate[f"hip_sym_{n}"] / rate[f"hip_verts_{n}"], 3) for n in shapes},
           **{f"torch_over_hip_sym_{n}": round(med[f"torch_sym_{n}"] / med[f"hip_sym_{n}"], 1) for n in shapes},
           "measures_hip": {n: _measures(values[f"hip_verts_{n}"], values[f"hip_sym_{n}"]) for n in shapes},
           "measures_torch_fp32_on_device": {n: _measures(values[f"hip_verts_{n}"], values[f"torch_sym_{n}"]) for n in shapes}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
