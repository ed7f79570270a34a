#!/usr/bin/env python
"""Times HoNet's recovery stage and its eager train step on the device and prints one JSON line.

  recover_ms    at B = 64 and N = 1000 / 4000 object vertices, one forward + backward of the recovery stage:
                  "hip":   ab_honet_recover_fwd + ab_honet_recover_bwd (kernels.honet_recover_fwd / _bwd), gradients on every output
                  "torch": the same arithmetic as eager torch device ops with autograd (honet.HoNet.recover_3d_proj, hpregnet._rodrigues,
                           batch_persp_proj2d), the same gradients
                measured as alternating pairs in one process (torch, hip, torch, hip, ...), each sample the device-event time of `--inner`
                back-to-back repetitions; median and range over `--pairs` pairs
  step_ms       the whole eager train step (TrainStep: HoNetHIP forward, ManoLoss + ObjLoss, backward, fused clip + Adam) at B = 64,
                128 x 128, ResNet-18, bf16x3, for both N: median and range over `--steps` steps after `--warmup`

  --fused       instead of the above: the eager train step against the graph-replayed fused one (ARCH.FUSED_MESH_STEP: FusedMeshCriterion,
                two hipGraphs) at B = 64, 128 x 128, ResNet-18, bf16x3, N = 300 and 4000.  Two models and optimizers in one process,
                measured as alternating pairs (eager, fused, eager, fused, ...), each sample the device-event time per step of `--inner`
                back-to-back steps ending in a synchronise; medians with ranges over `--pairs` pairs, the ratio of the medians, and the
                number of kernel launches one replayed step holds (counted by the profiler in a window of its own, after the timing).
                The eager route is the one `step_ms` measures, untouched by the fused one.

Usage: python tools/bench_honet.py [--pairs 15] [--inner 20] [--steps 30] [--warmup 5] [--fused]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FACTORS, SIZE = (100.0, 0.0001), (128, 128)


def _inputs(B, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 400.0 + 200.0 * torch.rand(B, generator=g)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = SIZE[0] / 2, SIZE[1] / 2, 1.0
    hst = torch.cat([1.0 + 9.0 * torch.rand(B, 1, generator=g), 0.3 * torch.randn(B, 2, generator=g)], 1)
    ost = torch.cat([1.0 + 9.0 * torch.rand(B, 1, generator=g), 0.3 * torch.randn(B, 2, generator=g), 0.8 * torch.randn(B, 3, generator=g)], 1)
    r = lambda *s: (0.06 * torch.randn(*s, generator=g)).cuda()      # noqa: E731
    return hst.cuda(), ost.cuda(), K.cuda(), r(B, 21, 3), r(B, 778, 3), r(B, N, 3), r(B, 8, 3)


def _torch_stage(hst, ost, K, joints, verts, can, ccan):
    from artiboost_amd.honet import HoNet
    from artiboost_amd.hpregnet import _rodrigues, batch_persp_proj2d as proj
    B = hst.shape[0]
    place = lambda p, st: HoNet.recover_3d_proj(p, K, st[:, :1].view(B, 1, 1) * FACTORS[1], st[:, 1:3].unsqueeze(1) * FACTORS[0], input_res=SIZE)  # noqa: E731
    j_abs, root = place(joints, hst)
    v_abs = verts + root
    R = _rodrigues(ost[:, 3:])
    o_abs, centre = place(R.bmm(can.transpose(1, 2)).transpose(1, 2), ost)
    c_abs = R.bmm(ccan.transpose(1, 2)).transpose(1, 2) + centre
    return dict(root_joint=root, joints_3d_abs=j_abs, hand_verts_3d_abs=v_abs, joints_2d=proj(j_abs, K), hand_verts_2d=proj(v_abs, K),
                obj_center=centre, box_rot_rotmat=R, obj_verts_3d_abs=o_abs, obj_verts_2d=proj(o_abs, K), corners_3d_abs=c_abs,
                corners_2d=proj(c_abs, K), corners_3d=c_abs - root, obj_verts_3d=o_abs - root)


def _event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def bench_recover(B, N, pairs, inner):
    from artiboost_amd import kernels as Kn
    hst, ost, K, joints, verts, can, ccan = _inputs(B, N)
    ups = {k: torch.randn(v.shape, device=v.device) for k, v in _torch_stage(hst, ost, K, joints, verts, can, ccan).items()}
    leaves = [t.clone().requires_grad_(True) for t in (hst, ost, joints, verts)]

    def run_torch():
        o = _torch_stage(leaves[0], leaves[1], K, leaves[2], leaves[3], can, ccan)
        torch.autograd.grad([o[k] for k in ups], leaves, [ups[k] for k in ups])

    def run_hip():
        Kn.honet_recover_fwd(hst, ost, K, joints, verts, can, ccan, FACTORS, SIZE)
        Kn.honet_recover_bwd(hst, ost, K, joints, verts, can, ccan, FACTORS, SIZE, ups)

    for fn in (run_torch, run_hip):
        _event_ms(fn, 5)
    t, h = [], []
    for _ in range(pairs):
        t.append(_event_ms(run_torch, inner))
        h.append(_event_ms(run_hip, inner))
    return {"torch": _stats(t), "hip": _stats(h), "ratio_of_medians": round(statistics.median(t) / statistics.median(h), 2)}


def _train_step(B, N, fused=False):
    import artiboost_amd.honet  # noqa: F401
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    from artiboost_amd.train import TrainStep
    arch = {"TYPE": "HoNet", "PRETRAINED": "", "PREVIOUS": [], "OBJ_TRANS_FACTOR": 100, "OBJ_SCALE_FACTOR": 0.0001, "DEVICE": "cuda",
            "BACKBONE": {"TYPE": "ResNet18", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
            "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}
    if fused:
        arch["FUSED_MESH_STEP"] = True
    preset = {"IMAGE_SIZE": list(SIZE), "HEATMAP_SIZE": [16, 16], "CENTER_IDX": 0}
    crit_cfg = [{"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_HAND_VERTS_3D": 1.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6},
                {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}]
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=preset))
    crit = Criterion({"LAMBDAS": [1.0, 1.0]}, R.build_criterion_loss_list(crit_cfg, preset_cfg=preset, LAMBDAS=[1.0, 1.0]))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=1e-4, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    hst, ost, K, joints, verts, can, ccan = _inputs(B, N, seed=1)
    g = torch.Generator().manual_seed(2)
    batch = {"image": (torch.rand(B, 3, SIZE[1], SIZE[0], generator=g) - 0.5).cuda(), "cam_intr": K, "corners_can": ccan, "obj_verts_can": can,
             "root_joint": torch.tensor([0.0, 0.0, 0.5]).repeat(B, 1).cuda(), "joints_3d": joints, "hand_verts_3d": verts,
             "obj_verts_3d": can + 0.05, "corners_3d": ccan + 0.05}
    return TrainStep(model, crit, opt, batch, use_graph=True)


def bench_step(B, N, steps, warmup):
    ts = _train_step(B, N)
    for _ in range(warmup):
        ts()
    torch.cuda.synchronize()
    v = [_event_ms(ts, 1) for _ in range(steps)]
    return _stats(v)


def _launches_per_step(ts, steps=3):
    """Kernel launches of one step, counted by the profiler over `steps` steps (None when the profiler reports no device activity)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            ts()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower())
    return round(n / steps, 1) if n else None


def bench_fused(B, N, pairs, inner, warmup):
    eager, fused = _train_step(B, N), _train_step(B, N, fused=True)
    assert eager.fused is None and not eager.use_graph and fused.fused is not None and fused.use_graph
    for ts in (eager, fused):
        for _ in range(warmup):
            ts()
    torch.cuda.synchronize()
    e, f = [], []
    for _ in range(pairs):
        e.append(_event_ms(eager, inner))
        f.append(_event_ms(fused, inner))
    out = {"eager": _stats(e), "fused": _stats(f), "ratio_of_medians": round(statistics.median(e) / statistics.median(f), 3)}
    out["kernel_launches_per_step"] = {"eager": _launches_per_step(eager), "fused": _launches_per_step(fused)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--fused", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_honet needs a HIP device")
    if a.fused:
        out = {"B": 64, "size": list(SIZE), "dtype": "bf16x3", "pairs": a.pairs, "inner": a.inner, "fused_step_ms": {}}
        for N in (300, 4000):
            out["fused_step_ms"][str(N)] = bench_fused(64, N, a.pairs, a.inner, a.warmup)
        print(json.dumps(out))
        return
    out = {"B": 64, "recover_ms": {}, "step_ms": {}}
    for N in (1000, 4000):
        out["recover_ms"][str(N)] = bench_recover(64, N, a.pairs, a.inner)
    if not a.no_step:
        for N in (1000, 4000):
            out["step_ms"][str(N)] = bench_step(64, N, a.steps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
