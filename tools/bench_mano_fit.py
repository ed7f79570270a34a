#!/usr/bin/env python
"""Times the hand-mesh fit of the submit pass (artiboost_amd/fitting.py) on the device and prints one JSON line:

  kernel_ms      ab_mano_fit per launch (device events around `--reps` back-to-back launches) at B = 100 (the README's --batch_size)
                 and 64, for 20 steps and for 0 steps (prologue + epilogue alone: the batch-mean pass, whose work grows with B, and the
                 778-vertex skinning), and at B = 1
  iknet_ms       the 7 ab_linear_fused launches of IKNet at the same batch sizes
  submit_s       train/submit_reload.py on the clasbased eval config over --frames seeded frames at --batch_size 100, without and with
                 --postprocess_fit_mesh (wall time the script reports for the pass; two alternating runs each, the lower kept)
  oracle_ms_per_hand   the float64 CPU restatement (tests/fit_oracle.py) per hand: the only baseline there is, the reference needs JAX

Usage: python tools/bench_mano_fit.py [--reps 50] [--frames 400] [--no-submit]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    quat = torch.randn(B, 64, generator=g)
    quat.view(B, 16, 4)[:, :, 0] += 2.0
    pj = 0.03 * torch.randn(B, 21, 3, generator=g) + torch.tensor([0.0, 0.0, 0.6])
    return quat.cuda().contiguous(), pj.cuda().contiguous()


def _time(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _submit(frames, fit):
    cmd = [sys.executable, os.path.join(ROOT, "train", "submit_reload.py"), "--cfg",
           os.path.join(ROOT, "config", "eval_ho3dv2_clasbased_artiboost_mi355x.yaml"), "--ignore_pretrained", "--random_frames",
           str(frames), "--batch_size", "100", "--submit_dump"] + (["--postprocess_fit_mesh"] if fit else [])
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=d)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("submit:")][-1]
    return float(re.search(r"in ([0-9.]+) s", line).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--no-submit", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mano_fit needs a HIP device")
    from artiboost_amd import kernels as K
    from artiboost_amd.fitting import FittingUnit, root_bone_target
    fu = FittingUnit(reload_prefix=None)
    res = {"kernel_ms": {}, "iknet_ms": {}}
    for B in (100, 64, 1):
        quat, pj = _inputs(B)
        for n in (20, 0):
            res["kernel_ms"][f"B{B}_steps{n}"] = round(_time(lambda: K.mano_fit(quat, pj, fu.tables, n_iter=n), a.reps), 4)
        inp = root_bone_target(pj)[2]
        res["iknet_ms"][f"B{B}"] = round(_time(lambda: fu.iknet(inp), a.reps), 4)
    import fit_oracle as fo
    from artiboost_amd.hpregnet import load_hand_model
    quat, pj = _inputs(100)
    t = time.perf_counter()
    fo.fit(quat.cpu().double(), pj.cpu().double(), load_hand_model(None))
    res["oracle_ms_per_hand"] = round((time.perf_counter() - t) * 1e3 / 100, 3)
    if not a.no_submit:
        runs = {False: [], True: []}
        for fit in (False, True, False, True):
            runs[fit].append(_submit(a.frames, fit))
        res["submit_s"] = {"frames": a.frames, "plain": min(runs[False]), "fit_mesh": min(runs[True])}
        res["submit_s"]["ratio"] = round(res["submit_s"]["fit_mesh"] / res["submit_s"]["plain"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
