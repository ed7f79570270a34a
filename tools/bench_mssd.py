#!/usr/bin/env python
"""Times the evaluator's MSSD on the device, the torch expression against ab_mssd, and prints / writes one JSON document.

  B = 64 samples of one object whose symmetry set has K transforms, V model points, (K, V) = (1, 8), (314, 8), (1, 4000), (314, 4000):
  K = 1 an object without symmetries, K = 314 one continuous axis at the default MAX_SYM_DISC_STEP = 0.01; V = 8 the corners
  (MSSD_USE_CORNERS: points mode), V = 4000 the full surface (rigid mode).
    "torch":  metrics._MSSDBase.values with AB_MSSD_TORCH=1 -- the eager expression with its [B, K, V, 3] temporaries
    "hip":    the same call on the default route (kernels.mssd: ab_mssd, two launches)
  measured as alternating pairs in one process (torch, hip, torch, hip, ...), each sample the device-event time of `--inner` back-to-back
  repetitions; median and range over `--pairs` pairs.  Per route also the peak of allocated device bytes above the inputs during one
  call, and per shape the largest difference between the two routes' values.  The counted work (`pairs`, `flops`: 9 fused multiply-adds
  for the residual and 5 flops for its squared length per (sample, symmetry, point); `input_bytes`) comes from the shapes.

Usage: python tools/bench_mssd.py [--pairs 15] [--inner 20] [--out profiles/mssd_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 64
SHAPES = ((1, 8), (314, 8), (1, 4000), (314, 4000))


def _rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)
    q[:, :, 0] *= torch.linalg.det(q).unsqueeze(1)
    return q


def _case(K, V, seed=0):
    import artiboost_amd.metrics as M
    info = {"1": {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]} if K > 1 else {}}
    corners = V == 8
    base = M._MSSDBase(USE_MSSD=True, MODEL_INFO=info, MAX_SYM_DISC_STEP=0.01, MSSD_USE_CORNERS=corners)
    assert base.sym_count.tolist() == [K], base.sym_count.tolist()
    g = torch.Generator().manual_seed(seed)
    can = (torch.rand(B, V, 3, generator=g) * 2 - 1) * torch.tensor([0.03, 0.045, 0.06])
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, :3, :3] = _rotations(B, g)
    T[:, :3, 3] = torch.stack([0.05 * torch.randn(B, generator=g), 0.05 * torch.randn(B, generator=g), 0.5 + 0.5 * torch.rand(B, generator=g)], 1)
    pR = _rotations(B, g)
    pt = (T[:, :3, 3] + 0.01 * torch.randn(B, 3, generator=g)).unsqueeze(1)
    targs = {"corners_can" if corners else "obj_verts_can": can.cuda(), "obj_transf": T.cuda(), "obj_idx": torch.ones(B, dtype=torch.int64).cuda()}
    preds = {"box_rot_rotmat": pR.cuda(), "boxroot_3d_abs": pt.cuda()}
    if corners:
        preds["corners_3d_abs"] = ((pR @ can.transpose(1, 2)).transpose(1, 2) + pt + 0.004 * torch.randn(B, V, 3, generator=g)).cuda()
    return base, preds, targs


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


def _peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def bench(K, V, pairs, inner):
    base, preds, targs = _case(K, V)

    def route(torch_route):
        def fn():
            if torch_route:
                os.environ["AB_MSSD_TORCH"] = "1"
            else:
                os.environ.pop("AB_MSSD_TORCH", None)
            return base.values(preds, targs)[1]
        return fn

    run_torch, run_hip = route(True), route(False)
    diff = float((run_torch().double() - run_hip().double()).abs().max())
    for fn in (run_torch, run_hip):
        _event_ms(fn, 5)
    peak = {"torch": _peak_bytes(run_torch), "hip": _peak_bytes(run_hip)}
    t, h = [], []
    for _ in range(pairs):
        t.append(_event_ms(run_torch, inner))
        h.append(_event_ms(run_hip, inner))
    n = B * K * V
    return {"K": K, "V": V, "mode": "points" if V == 8 else "rigid", "torch_ms": _stats(t), "hip_ms": _stats(h),
            "ratio_of_medians": round(statistics.median(t) / statistics.median(h), 2), "peak_allocated_bytes": peak,
            "max_abs_difference_m": diff, "pairs": n, "flops": n * 23,
            "input_bytes": B * V * 12 * (2 if V == 8 else 1) + B * (64 + 8 + 48) + K * 48 + 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mssd_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mssd needs a HIP device")
    keep = os.environ.get("AB_MSSD_TORCH")
    out = {"device": torch.cuda.get_device_name(0), "B": B, "pairs": a.pairs, "inner": a.inner, "shapes": [bench(K, V, a.pairs, a.inner) for K, V in SHAPES]}
    os.environ.pop("AB_MSSD_TORCH", None)
    if keep is not None:
        os.environ["AB_MSSD_TORCH"] = keep
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert np.isfinite([s["max_abs_difference_m"] for s in out["shapes"]]).all()


if __name__ == "__main__":
    main()
