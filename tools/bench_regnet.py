"""Timing of the regression-based model (HOPRegNet on the HIP kernels, config/ho3dv2_regbased_artiboost_mi355x.yaml) on a seeded synthetic
batch, one GPU:
   train : TrainStep's eager step -- forward + the config's criterion (registry losses through autograd) + backward + clip/Adam;
           --fused: ARCH.FUSED_STEP, the fused criterion kernel and the step replayed as two hipGraphs
   eval  : eval-mode forward (trunk + heads + MANO + the torch-op projections)
One JSON line per (mode, size)."""
import argparse
import json
import os
import sys
import time

import torch
import yaml

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))      # gen_batch: seeded inputs in the reference's batch schema

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=64)
ap.add_argument("--sizes", default="224,256")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dtype", default="bf16x3")
ap.add_argument("--modes", default="train,eval")
ap.add_argument("--fused", action="store_true", help="ARCH.FUSED_STEP: the fused regbased criterion + graph-replayed step")
a = ap.parse_args()

from gen_batch import make_batch
import artiboost_amd.hpregnet  # noqa: F401  (registers HOPRegNet)
from artiboost_amd import registry as R
from artiboost_amd.criterions import Criterion
from artiboost_amd.models import Arch
from artiboost_amd.netutils import build_optimizer
from artiboost_amd.train import TrainStep


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_regbased_artiboost_mi355x.yaml")))
for size in [int(s) for s in a.sizes.split(",")]:
    preset = dict(cfg["DATA_PRESET"], IMAGE_SIZE=[size, size], HEATMAP_SIZE=[size // 8, size // 8])
    arch = dict(cfg["ARCH"], COMPUTE_DTYPE=a.dtype, DEVICE="cuda", INIT_SEED=1, **({"FUSED_STEP": True} if a.fused else {}))
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=preset))
    batch = {k: v.cuda() for k, v in make_batch(a.bs, size, 5).items()}
    for mode in a.modes.split(","):
        if mode == "train":
            crit = Criterion(cfg, R.build_criterion_loss_list(cfg["CRITERION"], preset_cfg=preset, LAMBDAS=cfg["LAMBDAS"]))
            opt = build_optimizer(model.models_params, **cfg["TRAIN"])
            opt.max_norm = cfg["TRAIN"]["GRAD_CLIP"]
            model.train()
            ts = TrainStep(model, crit, opt, batch, use_graph=True)
            assert (ts.fused is not None and ts.use_graph) == a.fused
            dt = timed(ts, a.steps, a.warmup)
        else:
            model.eval()
            with torch.no_grad():
                dt = timed(lambda: model(batch), a.steps, a.warmup)
        print(json.dumps({"mode": mode, "size": size, "bs": a.bs, "dtype": a.dtype, "ms": round(dt * 1e3, 3),
                          "samples_per_s": round(a.bs / dt, 1), **({"fused": True} if a.fused else {})}), flush=True)
