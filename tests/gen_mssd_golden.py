"""Writes tests/golden/mssd.npz by running the reference's own MSSD.feed (anakin/metrics/bopAR.py:131-175, through AR) and ValMetricAR2
(anakin/metrics/val_metric.py:145-327) of lixiny/ArtiBoost on seeded inputs -- run by hand, never by a test; the output is committed.

Four objects with symmetry sets of 1, 2, 12 and 24 transforms at MAX_SYM_DISC_STEP = 0.25 (none / one discrete / one continuous axis with
an offset / one discrete + one continuous): BOP's enumeration of a continuous symmetry starts at i = 1, so the sets of objects 3 and 4 do
not contain the identity.  B = 8 samples of objects 1,2,3,4,3,4,2,3; V = 513 canonical points of about 6 cm spread; depths 0.5 - 1 m; even
samples are predicted exactly, odd ones with a random rotation and a 1 cm shift.

Contents:
  model_info                                   the json of the four objects
  t.<key>, p.<key>                             targets / predictions (obj_verts_can [B,513,3], corners_can [B,8,3], obj_transf, obj_idx,
                                               root_joint, the synthetic ids; box_rot_rotmat, boxroot_3d_abs, corners_3d_abs, joints_3d_abs)
  ar.<v|c>.c<0|1>.y<0|1>.keys / .vals          AR.get_measures() of the whole batch: vertices | corners, MSSD_USE_CENTER_IDX, USE_HO3D_YCB
  ar.<v|c>.c<0|1>.y<0|1>.sample [B]            per-sample MSSD in metres (each sample fed alone, read from its object's meter)
  val.<v|c>.y<0|1>.ids / .vals                 ValMetricAR2.get_measures_averaged() (mm), sorted by id

Run:  python tests/gen_mssd_golden.py"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SEED, V, OBJ_IDS, STEP, CENTER_IDX = 23, 513, (1, 2, 3, 4, 3, 4, 2, 3), 0.25, 9
INFO = {"1": {},
        "2": {"symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
        "3": {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [5, -3, 0]}]},
        "4": {"symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 12, 0, 0, 0, 1]],
              "symmetries_continuous": [{"axis": [0, 1, 0], "offset": [0, 0, 0]}]}}


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def inputs():
    rng = np.random.default_rng(SEED)
    B = len(OBJ_IDS)
    can = (rng.uniform(-1, 1, size=(B, V, 3)) * np.array([0.03, 0.045, 0.06])).astype(np.float32)
    ccan = (rng.uniform(-1, 1, size=(B, 8, 3)) * np.array([0.03, 0.045, 0.06])).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    R_pred, t_pred = np.zeros((B, 3, 3), np.float32), np.zeros((B, 1, 3), np.float32)
    for b in range(B):
        T[b, :3, :3] = rotation(rng)
        T[b, :3, 3] = np.array([rng.normal() * 0.05, rng.normal() * 0.05, rng.uniform(0.5, 1.0)])
        if b % 2 == 0:
            R_pred[b], t_pred[b, 0] = T[b, :3, :3], T[b, :3, 3]
        else:
            d = rng.normal(size=3)
            R_pred[b], t_pred[b, 0] = rotation(rng), T[b, :3, 3] + 0.01 * d / np.linalg.norm(d)
    corners_abs = (np.einsum("bij,bnj->bni", R_pred, ccan) + t_pred).astype(np.float32)
    corners_abs[1::2] += (rng.normal(size=(B // 2, 8, 3)) * 0.004).astype(np.float32)      # not a rigid image of the canonical corners
    root = (T[:, :3, 3] + rng.normal(size=(B, 3)) * 0.04).astype(np.float32)
    joints = (root[:, None] + rng.normal(size=(B, 21, 3)) * 0.03).astype(np.float32)
    joints_abs = (joints + rng.normal(size=(B, 21, 3)) * 0.008).astype(np.float32)
    targs = dict(obj_verts_can=can, corners_can=ccan, obj_transf=T, obj_idx=np.asarray(OBJ_IDS, np.int64), root_joint=root,
                 is_synth=np.array([1, 1, 0, 1, 1, 1, 1, 1], bool), obj_id=np.array([0, 1, 2, 3, 2, 3, 3, 2], np.int64),
                 persp_id=np.array([5, 17, 40, 3, 40, 3, 3, 40], np.int64), grasp_id=np.array([1, 2, 3, 4, 3, 4, 4, 3], np.int64))
    # samples 3, 5 (object 4) and 6 (object 2) share a triplet: the reference visits the classes in order, so sample 5 wins, not 6
    preds = dict(box_rot_rotmat=R_pred, boxroot_3d_abs=t_pred, corners_3d_abs=corners_abs, joints_3d_abs=joints_abs)
    return targs, preds


def main():
    import ref_import
    ref_import.load_control_plane()
    from anakin.metrics.bopAR import AR
    from anakin.metrics.val_metric import ValMetricAR2
    targs_np, preds_np = inputs()
    targs = {k: torch.from_numpy(v) for k, v in targs_np.items()}
    preds = {k: torch.from_numpy(v) for k, v in preds_np.items()}
    B = len(OBJ_IDS)
    out = {f"t.{k}": v for k, v in targs_np.items()}
    out.update({f"p.{k}": v for k, v in preds_np.items()})
    out["model_info"] = np.array(json.dumps(INFO))
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(INFO, f)
    base = dict(USE_MSSD=True, MODEL_INFO_PATH=f.name, MAX_SYM_DISC_STEP=STEP, DATA_PRESET={"CENTER_IDX": CENTER_IDX})
    for pts, corners in (("v", False), ("c", True)):
        for ycb in (0, 1):
            for cen in (0, 1):
                cfg = dict(base, MSSD_USE_CORNERS=corners, MSSD_USE_CENTER_IDX=bool(cen), USE_HO3D_YCB=bool(ycb))
                tag = f"ar.{pts}.c{cen}.y{ycb}"
                a = AR(**cfg)
                assert [len(r) for r in a.mssd.R] == [1, 2, 12, 24]
                a.feed(preds, targs)
                meas = a.get_measures()
                out[f"{tag}.keys"] = np.array(sorted(meas))
                out[f"{tag}.vals"] = np.array([meas[k] for k in sorted(meas)], np.float64)
                per = np.zeros(B, np.float64)
                for b in range(B):
                    a.reset()
                    a.feed({k: v[b:b + 1] for k, v in preds.items()}, {k: v[b:b + 1] for k, v in targs.items()})
                    m = a.mssd.objs_error[OBJ_IDS[b]]
                    assert m.count == 1
                    per[b] = m.sum
                out[f"{tag}.sample"] = per
            v = ValMetricAR2(**dict(base, MSSD_USE_CORNERS=corners, USE_HO3D_YCB=bool(ycb)))
            v.feed(preds, targs)
            avg = v.get_measures_averaged()
            out[f"val.{pts}.y{ycb}.ids"] = np.array(sorted(avg), np.int64)
            out[f"val.{pts}.y{ycb}.vals"] = np.array([avg[k] for k in sorted(avg)], np.float64)
    os.unlink(f.name)
    path = os.path.join(ROOT, "tests", "golden", "mssd.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    for k in ("ar.v.c0.y0.sample", "ar.c.c0.y0.sample", "ar.v.c1.y1.sample"):
        print(k, np.round(out[k], 5))
    print("val.v.y0", out["val.v.y0.ids"].tolist(), np.round(out["val.v.y0.vals"], 3))


if __name__ == "__main__":
    main()
