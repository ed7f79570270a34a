#!/usr/bin/env python
"""Times the BOP average recall of the evaluator (BOPRecall: VSD, MSSD, MSPD) and prints / writes one JSON document.

  B = 64 on 256 x 256 images, the stand-in object meshes of HO3D (4 objects of 3 968 faces) and of DexYCB (21 objects of 16 128 faces) at
  0.45 - 0.55 m; the estimate is the annotation turned by up to 0.3 rad and shifted by up to 1 cm; 300 model points per sample.
    "hip_<table>_vsd" / "_mssd" / "_mspd":  one kernels.vsd / mssd / mspd call
    "hip_<table>_metric":                   BOPRecall.feed_device on device tensors (the three calls + the hit counting), DEPTH_TEST none
    "cpu_<table>_metric":                   the same on CPU tensors (vsd_values_numpy and the torch expressions), on the first --cpu-samples
                                            samples, wall clock, once; also reported per sample
  Device routes: the device-event time of `--inner` back-to-back repetitions followed by a synchronise, after a warm-up; median and range
  over `--rounds`.  Then the measures of the batch by the device route.  Nothing here captures a graph.

Usage: python tools/bench_bop_recall.py [--rounds 7] [--inner 5] [--cpu-samples 8] [--out profiles/bop_recall_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, SIZE, NPTS = 64, 256, 300


def _rotations(rng, n):
    q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def _batch(table, seed=0):
    """(preds, targs) on the host: fp32 tensors of one synthetic validation batch over the table's objects."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, table.n_obj, B)
    Rg = _rotations(rng, B)
    tg = np.stack([rng.uniform(-0.05, 0.05, B), rng.uniform(-0.05, 0.05, B), rng.uniform(0.45, 0.55, B)], 1)
    ax = rng.standard_normal((B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.3, B)
    Kx = np.zeros((B, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    Re = (np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * Kx @ Kx) @ Rg
    te = tg + rng.uniform(-0.01, 0.01, (B, 3))
    T = np.tile(np.eye(4), (B, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = Rg, tg
    K = np.tile(np.array([[435.0 * SIZE / 512, 0, SIZE / 2], [0, 435.0 * SIZE / 512, SIZE / 2], [0, 0, 1]]), (B, 1, 1))
    can = np.stack([table.verts[table.vert_off[r]:table.vert_off[r + 1]][:NPTS] for r in rows])
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))      # noqa: E731
    preds = {"box_rot_rotmat": f(Re), "boxroot_3d_abs": f(te).reshape(B, 1, 3)}
    targs = {"obj_transf": f(T), "obj_idx": torch.tensor([table.obj_ids[r] for r in rows]), "cam_intr": f(K), "obj_verts_can": f(can)}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--cpu-samples", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bop_recall_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bop_recall needs a HIP device")
    import yaml
    from artiboost_amd import kernels as K
    from artiboost_amd import metrics as MT
    from artiboost_amd.assets import SceneAssets
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_bop_mi355x.yaml")))
    mcfg = dict(cfg["EVALUATOR"][-1], DEPTH_TEST="none", DATA_PRESET=dict(cfg["DATA_PRESET"], IMAGE_SIZE=[SIZE, SIZE]))
    mcfg.pop("OBJ_MESHES")
    mcfg.pop("TYPE")
    routes, cpu, measures, faces = {}, {}, {}, {}
    for name in ("ho3d", "dexycb"):
        table = MT.ObjectMeshTable.from_assets(SceneAssets("HO3D" if name == "ho3d" else "DexYCB", seed=1))
        faces[name] = int(table.face_off[1])
        preds, targs = _batch(table)
        dev = lambda d: {k: v.cuda() for k, v in d.items()}      # noqa: E731
        pd, td = dev(preds), dev(targs)
        m = MT.BOPRecall(**mcfg).set_obj_meshes(table)
        m.feed(pd, td)
        measures[name] = {k: v for k, v in m.get_measures().items() if not k.endswith(".ar")}
        tn = m._on(pd["box_rot_rotmat"].device)
        rows = tn["lut"][td["obj_idx"]]
        T = td["obj_transf"]
        rg, tg, te = T[:, :3, :3].contiguous(), T[:, :3, 3].contiguous(), pd["boxroot_3d_abs"].reshape(B, 3).contiguous()
        routes[f"hip_{name}_vsd"] = lambda tn=tn, rows=rows, pd=pd, td=td, rg=rg, tg=tg, te=te, m=m: K.vsd(
            tn["obj_verts"], tn["obj_faces"], tn["vert_off"], tn["face_off"], m.max_obj_verts, rows, pd["box_rot_rotmat"], te, rg, tg, td["cam_intr"], SIZE, SIZE,
            m.delta, m.taus, tn["row_diam"])
        routes[f"hip_{name}_mssd"] = lambda m=m, pd=pd, td=td: m.base.values(pd, td)
        routes[f"hip_{name}_mspd"] = lambda m=m, pd=pd, td=td, te=te: K.mspd(td["obj_verts_can"], td["obj_transf"], td["obj_idx"], m.base.R, m.base.t, m.base.sym_count,
                                                                             td["cam_intr"], pred_R=pd["box_rot_rotmat"], pred_t=te)
        routes[f"hip_{name}_metric"] = lambda m=m, pd=pd, td=td: m.feed_device(pd, td)
        n = a.cpu_samples
        mc = MT.BOPRecall(**mcfg).set_obj_meshes(table)
        t0 = time.perf_counter()
        mc.feed({k: v[:n] for k, v in preds.items()}, {k: v[:n] for k, v in targs.items()})
        cpu[name] = time.perf_counter() - t0
        md = MT.BOPRecall(**mcfg).set_obj_meshes(table)
        md.feed({k: v[:n] for k, v in pd.items()}, {k: v[:n].contiguous() for k, v in td.items()})
        assert torch.equal(md._hits[:, 0].cpu(), mc._hits[:, 0]), "the VSD hits of the device and the CPU route differ"
    for fn in routes.values():
        _event_ms(fn, 3)
    ms = {k: [] for k in routes}
    for _ in range(a.rounds):
        for k, fn in routes.items():
            ms[k].append(_event_ms(fn, a.inner))
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "B": B, "image": [SIZE, SIZE], "model_points": NPTS, "faces_per_object": faces,
           **{k + "_ms": _stats(v) for k, v in ms.items()},
           **{f"cpu_{k}_metric_s": {"samples": a.cpu_samples, "total": round(v, 3), "per_sample": round(v / a.cpu_samples, 4)} for k, v in cpu.items()},
           "measures": measures}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
