"""Writes tests/golden/mesh_losses.npz by running the reference's own AlignLoss, ChamferLoss and ObjLoss (anakin/criterions/alignloss.py,
chamferloss.py, honetloss.py of lixiny/ArtiBoost) on seeded inputs -- run by hand, never by a test; the output is committed.

`chamfer_distance` (third party, un-pinned, absent) is bound to a brute-force, gather-based, differentiable stand-in written here:
squared distances to the first nearest neighbour.  Parity is unpinned at exactly that boundary, as for the refiner.

Contents (B = 3 samples; meshes of 300 / 211 / 157 vertices padded by repetition to 300 as hodata_collate does; sample 2 has no
visible corner, so ChamferLoss masks it):
  counts [B]                                       the meshes' own vertex counts
  obj_verts_can, obj_verts_3d [B,300,3], obj_transf [B,4,4], root_joint [B,3], corners_vis [B,8], joints_3d [B,21,3]      targets
  box_rot_rotmat [B,3,3], boxroot_3d_abs [B,1,3], joints_3d_abs [B,21,3], obj_verts_3d_abs [B,300,3]                      predictions
  chamfer_loss, procrustes_aligned_loss, obj_verts_3d_loss, final_<loss>                                                   loss values
  g_box_rot_rotmat, g_boxroot_3d_abs (ChamferLoss), g_joints_3d_abs (AlignLoss), g_obj_verts_3d_abs (ObjLoss)              autograd

Run:  python tests/gen_mesh_loss_golden.py"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
COUNTS, NMAX, SEED = (300, 211, 157), 300, 19


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def inputs():
    rng = np.random.default_rng(SEED)
    B = len(COUNTS)
    can = np.zeros((B, NMAX, 3), np.float32)
    for b, n in enumerate(COUNTS):
        v = (rng.uniform(-1, 1, size=(n, 3)) * np.array([0.05, 0.08, 0.11])).astype(np.float32)
        can[b] = np.concatenate([v] * int(NMAX / n + 1))[:NMAX]
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    root = (rng.normal(size=(B, 3)) * 0.03 + np.array([0.0, 0.0, 0.5])).astype(np.float32)
    R_pred = np.zeros((B, 3, 3), np.float32)
    for b in range(B):
        T[b, :3, :3] = rotation(rng)
        T[b, :3, 3] = root[b] + rng.normal(size=3) * 0.04
        R_pred[b] = rotation(rng) if b == 1 else (T[b, :3, :3] @ _small_rotation(rng, 0.2))      # near the target, and one far off
    v3d = (np.einsum("bij,bnj->bni", T[:, :3, :3], can) + T[:, None, :3, 3] - root[:, None]).astype(np.float32)
    vis = np.ones((B, 8), np.float32)
    vis[0, :3] = 0
    vis[2] = 0
    joints = (rng.normal(size=(B, 21, 3)) * np.array([0.04, 0.05, 0.03])).astype(np.float32)
    d = dict(counts=np.asarray(COUNTS, np.int64), obj_verts_can=can, obj_verts_3d=v3d, obj_transf=T, root_joint=root, corners_vis=vis,
             joints_3d=joints, box_rot_rotmat=R_pred,
             boxroot_3d_abs=(T[:, None, :3, 3] + rng.normal(size=(B, 1, 3)) * 0.01).astype(np.float32),
             joints_3d_abs=(joints + root[:, None] + rng.normal(size=(B, 21, 3)) * 0.008).astype(np.float32),
             obj_verts_3d_abs=(v3d + root[:, None] + rng.normal(size=(B, NMAX, 3)) * 0.005).astype(np.float32))
    d["joints_3d_abs"][1] = d["joints_3d_abs"][1] * np.array([-1.0, 1.0, 1.0], np.float32)      # a mirrored hand: the reflection case
    return d


def _small_rotation(rng, angle):
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * angle
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) / angle * K + (1 - np.cos(angle)) / angle ** 2 * K @ K).astype(np.float32)


class ChamferDistance:
    def __call__(self, x, y):
        with torch.no_grad():
            d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
            i, j = d.argmin(2), d.argmin(1)
        g = lambda t, idx: torch.gather(t, 1, idx[..., None].expand(-1, -1, 3))      # noqa: E731
        return ((x - g(y, i)) ** 2).sum(-1), ((g(x, j) - y) ** 2).sum(-1), i, j


def main():
    import ref_import
    ref_import.load()
    cd = types.ModuleType("chamfer_distance")
    cd.ChamferDistance = ChamferDistance
    sys.modules["chamfer_distance"] = cd
    from anakin.criterions.alignloss import AlignLoss
    from anakin.criterions.chamferloss import ChamferLoss
    from anakin.criterions.honetloss import ObjLoss
    d = inputs()
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    targs = {k: t[k] for k in ("obj_verts_can", "obj_verts_3d", "obj_transf", "root_joint", "corners_vis", "joints_3d")}
    preds = {k: t[k].clone().requires_grad_(True) for k in ("box_rot_rotmat", "boxroot_3d_abs", "joints_3d_abs", "obj_verts_3d_abs")}
    out = dict(d)
    for loss, key in ((ChamferLoss(LAMBDA_CHAMFER=0.7), "chamfer_loss"), (AlignLoss(LAMBDA_PROCRUSTES_ALIGN=0.3), "procrustes_aligned_loss"),
                      (ObjLoss(LAMBDA_OBJ_VERTS_3D=0.5), "obj_verts_3d_loss")):
        final, losses = loss(preds, targs)
        final.sum().backward()
        out[key] = losses[key].detach().numpy()
        out["final_" + type(loss).__name__] = final.detach().numpy()
        assert set(losses) >= {key}
        out["keys_" + type(loss).__name__] = np.array(sorted(losses))
    for k, p in preds.items():
        out["g_" + k] = p.grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "mesh_losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: float(out[k]) for k in ("chamfer_loss", "procrustes_aligned_loss", "obj_verts_3d_loss")})


if __name__ == "__main__":
    main()
