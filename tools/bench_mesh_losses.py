#!/usr/bin/env python
"""Times ChamferLoss and AlignLoss on the device, the HIP kernels against the eager torch expression, and prints / writes one JSON document.

  B = 64; ChamferLoss with N = M = 300 (MANAGER.MESH_QUERIES of the shipped configs) and N = M = 2048; AlignLoss with n = 21.
    "hip_forward":   one kernel call without gradient buffers (kernels.chamfer_rigid / procrustes_loss, want_grad=False)
    "hip_gradient":  one kernel call that also leaves the gradient (want_grad=True): what the autograd Function's forward issues
    "hip_class":     the public class on device tensors, forward + .backward() (the call above, the scaling by the incoming gradient, autograd)
    "torch_class":   the SAME loss as the eager torch expression of the CPU route on the same device tensors, forward + .backward()
                     (ChamferLoss.torch_expression; AlignLoss.procrustes_align + mse_loss: a batched torch.svd)
    "cpu_class":     the public class on CPU copies of the tensors, forward + .backward(), wall clock
  The device routes are measured as alternating rounds in one process (hip_forward, hip_gradient, hip_class, torch_class, ...), each
  sample the device-event time of `--inner` back-to-back repetitions; median and range over `--pairs` rounds.  Per shape also the largest
  relative difference between the two device routes' loss and gradients.  Nothing here captures a graph.

Usage: python tools/bench_mesh_losses.py [--pairs 11] [--inner 10] [--out profiles/mesh_losses_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = 64
MESH_SIZES = (300, 2048)


def _rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g))
    return q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)


def _chamfer_case(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    can = (torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([0.03, 0.045, 0.06])
    root = torch.stack([0.05 * torch.randn(B, generator=g), 0.05 * torch.randn(B, generator=g), 0.5 + 0.1 * torch.rand(B, generator=g)], 1)
    R = _rotations(B, g)
    v3d = ((R @ can.transpose(1, 2)).transpose(1, 2) + 0.002 * torch.randn(B, N, 3, generator=g)).contiguous()
    preds = {"box_rot_rotmat": R + 0.02 * torch.randn(B, 3, 3, generator=g), "boxroot_3d_abs": (root + 0.01 * torch.randn(B, 3, generator=g)).unsqueeze(1)}
    targs = {"obj_verts_can": can, "obj_verts_3d": v3d, "root_joint": root, "corners_vis": torch.ones(B, 8)}
    return preds, targs


def _align_case(seed=1):
    g = torch.Generator().manual_seed(seed)
    j = 0.05 * torch.randn(B, 21, 3, generator=g)
    root = torch.stack([0.05 * torch.randn(B, generator=g), 0.05 * torch.randn(B, generator=g), 0.5 + 0.1 * torch.rand(B, generator=g)], 1)
    return {"joints_3d_abs": j + root.unsqueeze(1) + 0.01 * torch.randn(B, 21, 3, generator=g)}, {"joints_3d": j, "root_joint": root}


def _event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _wall_ms(fn, inner):
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    return (time.perf_counter() - t) * 1e3 / inner


def _stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5), "n": len(v)}


def _leaves(preds, dev):
    return {k: v.to(dev).clone().requires_grad_(True) for k, v in preds.items()}


def _class_route(loss_of, preds, targs, dev):
    """fn() -> (loss value, gradients): forward + backward of `loss_of(preds, targs)` on fresh leaves of `dev`."""
    targs = {k: v.to(dev) for k, v in targs.items()}

    def fn():
        p = _leaves(preds, dev)
        loss = loss_of(p, targs)
        loss.backward()
        return loss.detach(), [p[k].grad for k in sorted(p)]
    return fn


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def bench(name, cls, torch_of, kernel_of, preds, targs, pairs, inner, shape):
    hip_class = _class_route(lambda p, t: cls(p, t)[0].sum(), preds, targs, "cuda")
    torch_class = _class_route(torch_of, preds, targs, "cuda")
    cpu_class = _class_route(lambda p, t: cls(p, t)[0].sum(), preds, targs, "cpu")
    preds, targs = {k: v.contiguous() for k, v in preds.items()}, {k: v.contiguous() for k, v in targs.items()}    # (qr returns column-major factors)
    dp, dt = {k: v.cuda() for k, v in preds.items()}, {k: v.cuda() for k, v in targs.items()}
    routes = {"hip_forward": lambda: kernel_of(dp, dt, False), "hip_gradient": lambda: kernel_of(dp, dt, True), "hip_class": hip_class,
              "torch_class": torch_class}
    (lh, gh), (lt, gt) = hip_class(), torch_class()
    diff = {"loss": _rel(lh, lt), "gradients": max(_rel(a, b) for a, b in zip(gh, gt))}
    for fn in routes.values():
        _event_ms(fn, 3)
    ms = {k: [] for k in routes}
    for _ in range(pairs):
        for k, fn in routes.items():
            ms[k].append(_event_ms(fn, inner))
    cpu_class()
    cpu = [_wall_ms(cpu_class, 1) for _ in range(min(pairs, 5))]
    out = {"loss": name, **shape, **{k + "_ms": _stats(v) for k, v in ms.items()}, "cpu_class_ms": _stats(cpu),
           "torch_class_over_hip_class": round(statistics.median(ms["torch_class"]) / statistics.median(ms["hip_class"]), 2),
           "max_relative_difference_hip_vs_torch": diff}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_losses_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_losses needs a HIP device")
    from artiboost_amd import kernels as K
    from artiboost_amd.criterions import AlignLoss, ChamferLoss
    chamfer, align = ChamferLoss(LAMBDA_CHAMFER=1.0), AlignLoss(LAMBDA_PROCRUSTES_ALIGN=1.0)

    def chamfer_torch(p, t):
        return ChamferLoss.torch_expression(p["box_rot_rotmat"], p["boxroot_3d_abs"], t, p["box_rot_rotmat"].device)

    def chamfer_kernel(p, t, grad):
        return K.chamfer_rigid(t["obj_verts_can"], p["box_rot_rotmat"], p["boxroot_3d_abs"], t["obj_verts_3d"], t["root_joint"], t["corners_vis"],
                               want_grad=grad)

    def align_torch(p, t):
        xyz = t["joints_3d"] + t["root_joint"].unsqueeze(1)
        return F.mse_loss(AlignLoss.procrustes_align(xyz, p["joints_3d_abs"]), xyz)

    def align_kernel(p, t, grad):
        return K.procrustes_loss(p["joints_3d_abs"], t["joints_3d"], t["root_joint"], want_grad=grad)

    shapes = []
    for N in MESH_SIZES:
        preds, targs = _chamfer_case(N)
        shapes.append(bench("ChamferLoss", chamfer, chamfer_torch, chamfer_kernel, preds, targs, a.pairs, a.inner, {"B": B, "N": N, "M": N}))
    preds, targs = _align_case()
    shapes.append(bench("AlignLoss", align, align_torch, align_kernel, preds, targs, a.pairs, a.inner, {"B": B, "n": 21}))
    out = {"device": torch.cuda.get_device_name(0), "pairs": a.pairs, "inner": a.inner, "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert np.isfinite([v for s in shapes for v in s["max_relative_difference_hip_vs_torch"].values()]).all()


if __name__ == "__main__":
    main()
