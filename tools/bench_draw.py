#!/usr/bin/env python
"""Times the drawing path of the submit pass (artiboost_amd/draw.py) on the device and prints one JSON line:

  kernel_ms      ab_draw_meshes per call (device events around `--reps` back-to-back calls) at B = 100 (the README's --batch_size),
                 256 x 256 panels, the fitted-hand stand-in plus one object of about 10^4 faces (a stand-in library object subdivided
                 once: 16384 faces), and the same with no object
  d2h_ms         the one device-to-host copy of the [B, H, 4W, 3] sheet
  host_s         the host half per batch: the two PIL skeleton panels and the PNG encode of B files (wall clock)
  submit_s       train/submit_reload.py on the clasbased eval config over --frames seeded frames at --batch_size 100 with
                 --postprocess_fit_mesh, without and with --postprocess_draw (wall time the script reports for the pass; alternating
                 runs, every value listed: their spread is the run-to-run noise)

Usage: python tools/bench_draw.py [--reps 30] [--frames 400] [--runs 3] [--no-submit]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def _submit(frames, draw):
    cmd = [sys.executable, os.path.join(ROOT, "train", "submit_reload.py"), "--cfg",
           os.path.join(ROOT, "config", "eval_ho3dv2_clasbased_artiboost_mi355x.yaml"), "--ignore_pretrained", "--random_frames",
           str(frames), "--batch_size", "100", "--submit_dump", "--postprocess_fit_mesh"] + (["--postprocess_draw"] if draw else [])
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=d)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("submit:")][-1]
    return float(re.search(r"in ([0-9.]+) s", line).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-submit", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_draw needs a HIP device")
    from artiboost_amd import kernels as K
    from artiboost_amd.assets import SceneAssets, _subdivide
    from artiboost_amd.draw import MeshDrawer, hand_model_faces
    from artiboost_amd.hpregnet import load_hand_model
    B, S = 100, 256
    hm = load_hand_model(None)
    o = SceneAssets("HO3D", seed=1).objects[0]
    ov, of = _subdivide(np.asarray(o["verts"], np.float64), np.asarray(o["faces"], np.int64))
    drawer = MeshDrawer(hand_model_faces(hm), object_library=dict(ids=[0], verts=[ov], faces=[of]), image_size=(S, S))
    rng = np.random.default_rng(0)
    hv = np.asarray(hm["v_template"], np.float32)
    hv = (hv - hv.mean(0))[None] + np.stack([rng.uniform(-0.03, 0.03, B), rng.uniform(-0.03, 0.03, B), rng.uniform(0.4, 0.7, B)], 1)[:, None]
    t = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dt)      # noqa: E731
    hv_d = t(hv)
    Kc = t(np.tile(np.array([[480.0, 0, S / 2], [0, 480.0, S / 2], [0, 0, 1]]), (B, 1, 1)))
    img = torch.rand((B, 3, S, S), device="cuda") - 0.5
    rot = t(np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)]))
    tsl = t(hv.mean(1) + rng.uniform(-0.03, 0.03, (B, 3)))
    out = torch.zeros((B, S, 4 * S, 3), dtype=torch.uint8, device="cuda")
    res = {"B": B, "panel": S, "hand_faces": int(drawer.hand_faces.shape[0]), "object_faces": int(len(of)), "device": torch.cuda.get_device_name(0)}
    for name, oid in (("hand_and_object", 0), ("hand_only", -1)):
        ids = torch.full((B,), oid, dtype=torch.int32, device="cuda")
        res[f"kernel_ms_{name}"] = round(_time(lambda: K.draw_meshes(hv_d, drawer.tables, img, Kc, out, obj_id=ids, obj_rot=rot, obj_tsl=tsl), a.reps), 4)
    res["d2h_ms"] = round(min(_host(lambda: out.cpu()) for _ in range(5)) * 1e3, 3)
    import tempfile as tf
    joints = torch.from_numpy(hv[:, :21].copy())
    with tf.TemporaryDirectory() as d:
        whole = []
        for _ in range(2):
            t0 = time.perf_counter()
            drawer.draw_batch(img, Kc, torch.arange(B), joints, hv_d, rot, tsl, None, _OneObject(ov, of), d, 0)
            whole.append(time.perf_counter() - t0)
    res["draw_batch_s"] = [round(w, 3) for w in whole]
    res["host_s"] = round(min(whole) - (res["kernel_ms_hand_and_object"] + res["d2h_ms"]) * 1e-3, 3)
    if not a.no_submit:
        fit, draw = [], []
        for _ in range(a.runs):
            fit.append(_submit(a.frames, False))
            draw.append(_submit(a.frames, True))
        res["submit_s"] = {"frames": a.frames, "fit": fit, "fit_draw": draw, "ratio_of_minima": round(min(draw) / min(fit), 3)}
    print(json.dumps(res))


def _host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


class _OneObject:
    """The dataset methods the drawer reads its object library from."""
    name = "bench"

    def __init__(self, v, f):
        self.v, self.f = v, f

    def get_obj_idx(self, idx):
        return 0

    def get_obj_verts_can(self, idx):
        return np.asarray(self.v, np.float32), None, None

    def get_obj_faces(self, idx):
        return np.asarray(self.f, np.int32)


if __name__ == "__main__":
    main()
