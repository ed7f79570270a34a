#!/usr/bin/env python
"""Times the leaderboard mesh metrics of the evaluator on the device, ab_mesh_metrics against the torch expression, and prints / writes one
JSON document.

  B = 64; a validation batch of HoNet: 21 joints, 778 hand vertices, 300 object vertices (MANAGER.MESH_QUERIES of the shipped configs).
    "hip_feed_all":     one Evaluator.feed_all of MeanAlignedEPE [joints_3d_abs, hand_verts_3d_abs], MeshFScore [hand_verts_3d_abs] and
                        MeanSurfaceDist [obj_verts_3d_abs] on HIP tensors (kernels.mesh_metrics: one call per key)
    "torch_feed_all":   the same feed_all with metrics.mesh_values_torch (the route of CPU tensors) on the SAME device tensors
    "hip_kernel_<n>":   one kernels.mesh_metrics call alone, all groups, per key
    "torch_values_<n>": one mesh_values_torch call alone on the same device tensors, per key
    "evaluator_base" / "evaluator_with_mesh":  feed_all of the EVALUATOR list of config/ho3dv2_honet_mi355x.yaml and of
                        config/ho3dv2_honet_meshmetrics_mi355x.yaml (the same list + the three metrics)
  The routes are measured as alternating rounds in one process, each sample the device-event time of `--inner` back-to-back repetitions
  followed by a synchronise, after a warm-up; median and range over `--pairs` rounds.  Also, per measure, the difference of the kernel route from the torch
  expression on the device and from the CPU-tensor route on copies of the batch, and the peak allocation of one feed_all of each.  Nothing here captures a graph.

Usage: python tools/bench_mesh_metrics.py [--pairs 11] [--inner 10] [--out profiles/mesh_metrics_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 64
KEYS = (("joints_3d", 21), ("hand_verts_3d", 778), ("obj_verts_3d", 300))


def _batch(seed=0):
    """(preds, targs) on the device: clouds of a hand-sized box at half a metre, predictions 4 mm off."""
    g = torch.Generator().manual_seed(seed)
    root = torch.stack([0.05 * torch.randn(B, generator=g), 0.05 * torch.randn(B, generator=g), 0.5 + 0.1 * torch.rand(B, generator=g)], 1)
    preds, targs = {}, {"root_joint": root.cuda()}
    for key, n in KEYS:
        rel = (torch.rand(B, n, 3, generator=g) - 0.5) * torch.tensor([0.18, 0.10, 0.03])
        targs[key] = rel.cuda()
        preds[key + "_abs"] = (rel + root.unsqueeze(1) + 0.004 * torch.randn(B, n, 3, generator=g)).cuda()
    preds["corners_3d_abs"] = (0.05 * torch.randn(B, 8, 3, generator=g) + root.unsqueeze(1)).cuda()
    targs["corners_3d"] = (preds["corners_3d_abs"].cpu() - root.unsqueeze(1) + 0.004 * torch.randn(B, 8, 3, generator=g)).cuda()
    for k in ("obj_id", "persp_id", "grasp_id"):
        targs[k] = torch.randint(0, 20, (B,), generator=g).cuda()
    targs["is_synth"] = torch.ones(B, dtype=torch.int64).cuda()
    return preds, targs


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


def _peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_metrics needs a HIP device")
    import yaml
    from artiboost_amd import kernels as K
    from artiboost_amd import metrics as MT
    from artiboost_amd import registry as R
    preds, targs = _batch()
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_meshmetrics_mi355x.yaml")))
    base_cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_mi355x.yaml")))
    mesh_cfg = [c for c in cfg["EVALUATOR"] if c["TYPE"] in ("MeanAlignedEPE", "MeshFScore", "MeanSurfaceDist")]
    build = lambda c: MT.Evaluator(cfg, R.build_evaluator_metric_list(c, cfg["DATA_PRESET"]))      # noqa: E731
    ev_hip, ev_torch, ev_base, ev_with = build(mesh_cfg), build(mesh_cfg), build(base_cfg["EVALUATOR"]), build(cfg["EVALUATOR"])
    hip_kernel = K.mesh_metrics

    def torch_route(*args, **kw):                       # mesh_values_torch under the kernel's name: what _mesh_values calls for HIP tensors
        return MT.mesh_values_torch(*args, **kw)

    def feed(ev, route):
        def fn():
            K.mesh_metrics = route
            try:
                ev.feed_all(preds, targs, losses={})
            finally:
                K.mesh_metrics = hip_kernel
        return fn

    routes = {"hip_feed_all": feed(ev_hip, hip_kernel), "torch_feed_all": feed(ev_torch, torch_route),
              "evaluator_base": feed(ev_base, hip_kernel), "evaluator_with_mesh": feed(ev_with, hip_kernel)}
    thr = (0.005, 0.015)
    for key, n in KEYS:
        p, t, r = preds[key + "_abs"], targs[key], targs["root_joint"]
        c = 0 if n == 21 else -1
        routes[f"hip_kernel_{n}"] = lambda p=p, t=t, r=r, c=c: hip_kernel(p, t, r, center_idx=c, thresholds=thr, flags=7)
        routes[f"torch_values_{n}"] = lambda p=p, t=t, r=r, c=c: MT.mesh_values_torch(p, t, r, center_idx=c, thresholds=thr, flags=7)
    peak = {k: _peak_mb(routes[k]) for k in ("hip_feed_all", "torch_feed_all")}
    for fn in routes.values():
        _event_ms(fn, 3)
    ms = {k: [] for k in routes}
    for _ in range(a.pairs):
        for k, fn in routes.items():
            ms[k].append(_event_ms(fn, a.inner))
    mh, mt = ev_hip.get_measures_all(), ev_torch.get_measures_all()
    ev_cpu = build(mesh_cfg)                            # the route of CPU tensors on copies of the batch: the third opinion
    ev_cpu.feed_all({k: v.cpu() for k, v in preds.items()}, {k: v.cpu() for k, v in targs.items()}, losses={})
    mc = ev_cpu.get_measures_all()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "inner": a.inner, "B": B, "points": dict(KEYS),
           **{k + "_ms": _stats(v) for k, v in ms.items()},
           "torch_feed_all_over_hip_feed_all": round(med["torch_feed_all"] / med["hip_feed_all"], 2),
           **{f"torch_over_hip_{n}": round(med[f"torch_values_{n}"] / med[f"hip_kernel_{n}"], 2) for _, n in KEYS},
           "mesh_metrics_cost_in_the_evaluator_ms": round(med["evaluator_with_mesh"] - med["evaluator_base"], 5),
           "peak_allocation_of_one_feed_all_mb": peak,
           "measures_hip": {k: round(v, 6) for k, v in mh.items()},
           "measure_difference_hip_vs_torch_on_device": {k: abs(mh[k] - mt[k]) for k in mh},
           "measure_difference_hip_vs_cpu_route": {k: abs(mh[k] - mc[k]) for k in mh}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert set(mh) == set(mt) and all(v == v for v in mh.values())


if __name__ == "__main__":
    main()
