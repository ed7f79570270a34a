"""Writes tests/golden/bop_recall.npz by running the reference's own BOP error functions (anakin/utils/bop_toolkit of lixiny/ArtiBoost:
bop_pose_error.vsd / mssd / mspd, bop_misc.calc_pts_diameter / get_symmetry_transformations) on seeded inputs -- run by hand, never by a
test; the output is committed.  The reference ships no depth renderer: `vsd` gets a stub whose render_object returns the depth image of the
stage contract (tests/bop_raster_ref.py), and K, delta, taus and the diameters are the fp32 values ab_vsd receives, cast to float64.

Two objects at MAX_SYM_DISC_STEP = 0.25: id 1 a box without symmetries, id 2 an icosphere of 320 faces with one continuous axis (12
transforms, none the identity).  B = 6 samples on a 48 x 40 image at about half a metre; lengths in metres.

Contents:
  model_info                      the json of the two objects (no diameters: the metric's fallback is under test)
  verts.<r>, faces.<r>            the meshes of table rows 0, 1 (fp32 / int32); obj_ids their ids
  obj_idx, rot_est, tsl_est, rot_gt, tsl_gt, cam_intr, depth_test, W, H, delta, taus, image_size
  diameter [2]                    calc_pts_diameter of each mesh (float64 of the fp32 vertices)
  vsd [B,T], union [B], inter [B] vsd's errors, and the two counts recomputed beside it with the reference's own functions
  mssd [B], mspd [B]              float64, the model points the meshes' vertices
  recall.<AR|AR_VSD|AR_MSSD|AR_MSPD>, recall.vsd / .mssd / .mspd [10]      the BOP19 recalls of these errors (strict <)

Run:  python tests/gen_bop_recall_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
W, H, STEP, SEED = 48, 40, 0.25, 41
INFO = {"1": {}, "2": {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
OBJ_IDX = (1, 2, 2, 1, 2, 1)


def inputs():
    from test_interaction_host import box_mesh, icosphere, rotation
    rng = np.random.default_rng(SEED)
    B = len(OBJ_IDX)
    meshes = [box_mesh([-0.03, -0.02, -0.045], [0.03, 0.02, 0.045]), icosphere(0.04, 2)]
    meshes = [(np.asarray(v, np.float32), np.asarray(f, np.int32)) for v, f in meshes]
    Rg = np.stack([rotation(int(s)) for s in rng.integers(0, 10 ** 6, B)])
    tg = np.stack([rng.uniform(-0.02, 0.02, B), rng.uniform(-0.02, 0.02, B), rng.uniform(0.45, 0.55, B)], 1)
    Re, te = Rg.copy(), tg.copy()
    for b, (ang, shift) in enumerate(((0.05, 0.002), (0.3, 0.004), (0.0, 0.0), (0.0, 0.02), (0.6, 0.01), (0.1, 0.0))):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Re[b] = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx) @ Rg[b]
        d = rng.normal(size=3)
        te[b] = tg[b] + shift * d / np.linalg.norm(d)
    tg[4, 0], te[4, 0] = 0.07, 0.072                      # straddles the right border
    te[5, 0] = 0.6                                        # the estimate is off-screen
    K = np.tile(np.array([[150.0, 0, 23.5], [0, 148.0, 19.25], [0, 0, 1]]), (B, 1, 1))
    K[:, 0, 2] += rng.uniform(-1, 1, B)
    K[:, 1, 2] += rng.uniform(-1, 1, B)
    f32 = lambda a: np.asarray(a, np.float32)      # noqa: E731
    depth = np.zeros((B, H, W), np.float32)
    depth[1, :, :24] = np.float32(tg[1, 2])               # a fronto-parallel plane through the object's centre over the left half
    depth[2] = 1.0                                        # a wall behind everything
    depth[4, ::2] = np.float32(tg[4, 2] - 0.1)            # every other row in front of the object
    return dict(meshes=meshes, obj_idx=np.asarray(OBJ_IDX, np.int64), rot_est=f32(Re), tsl_est=f32(te), rot_gt=f32(Rg), tsl_gt=f32(tg), cam_intr=f32(K),
                depth_test=depth, delta=np.float32(0.015), taus=np.arange(0.05, 0.51, 0.05).astype(np.float32))


def main():
    import ref_import
    ref_import.load()
    from anakin.utils.bop_toolkit import bop_misc, bop_pose_error, visibility
    import bop_raster_ref as RR
    inp = inputs()
    meshes, B = inp["meshes"], len(OBJ_IDX)
    f64 = lambda a: np.asarray(a, np.float64)      # noqa: E731
    diam = np.array([bop_misc.calc_pts_diameter(f64(v)) for v, _ in meshes])
    diam32 = diam.astype(np.float32)
    syms = []
    for i in (1, 2):
        s = bop_misc.get_symmetry_transformations(INFO[str(i)], STEP)
        syms.append([{"R": x["R"], "t": x["t"] / 1000.0} for x in s])
    assert [len(s) for s in syms] == [1, 12]

    class Stub:
        def render_object(self, obj_id, R, t, fx, fy, cx, cy):
            v, f = meshes[obj_id]
            K = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)
            return {"depth": RR.render_depth(v, f, np.asarray(R, np.float32), np.asarray(t, np.float32).reshape(3), K, W, H)}

    taus = [float(t) for t in inp["taus"]]
    delta = float(inp["delta"])
    vsd, union, inter, mssd, mspd = np.zeros((B, len(taus))), np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B), np.zeros(B)
    for b in range(B):
        r = OBJ_IDX[b] - 1
        K = f64(inp["cam_intr"][b])
        Re, te, Rg, tg = f64(inp["rot_est"][b]), f64(inp["tsl_est"][b]).reshape(3, 1), f64(inp["rot_gt"][b]), f64(inp["tsl_gt"][b]).reshape(3, 1)
        bop_misc.Precomputer.K, bop_misc.Precomputer.depth_im_shape = None, None
        vsd[b] = bop_pose_error.vsd(Re, te, Rg, tg, inp["depth_test"][b], K, delta, taus, True, float(diam32[r]), Stub(), r, "step")
        # the two counts, recomputed beside vsd with the reference's own functions
        de, dg = Stub().render_object(r, Re, te, K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"], Stub().render_object(r, Rg, tg, K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
        Lt, Lg, Le = (bop_misc.depth_im_to_dist_im_fast(d, K) for d in (inp["depth_test"][b], dg, de))
        vg = visibility.estimate_visib_mask_gt(Lt, Lg, delta, visib_mode="bop19")
        ve = visibility.estimate_visib_mask_est(Lt, Le, vg, delta, visib_mode="bop19")
        union[b], inter[b] = np.logical_or(vg, ve).sum(), np.logical_and(vg, ve).sum()
        pts = f64(meshes[r][0])
        mssd[b] = bop_pose_error.mssd(Re, te, Rg, tg, pts, syms[r])
        mspd[b] = bop_pose_error.mspd(Re, te, Rg, tg, K, pts, syms[r])
    th = np.arange(0.05, 0.51, 0.05)
    rr = W / 640.0
    rec_vsd = np.array([(vsd < t).mean() for t in th])
    rec_mssd = np.array([(mssd < t * diam[np.asarray(OBJ_IDX) - 1]).mean() for t in th])
    rec_mspd = np.array([(mspd < t).mean() for t in [rr * k for k in range(5, 51, 5)]])
    out = {f"verts.{r}": v for r, (v, _) in enumerate(meshes)}
    out.update({f"faces.{r}": f for r, (_, f) in enumerate(meshes)})
    out.update({k: inp[k] for k in ("obj_idx", "rot_est", "tsl_est", "rot_gt", "tsl_gt", "cam_intr", "depth_test", "delta", "taus")})
    out.update(model_info=np.array(json.dumps(INFO)), obj_ids=np.array([1, 2]), W=W, H=H, step=STEP, diameter=diam, vsd=vsd, union=union, inter=inter, mssd=mssd,
               mspd=mspd)
    out.update({"recall.vsd": rec_vsd, "recall.mssd": rec_mssd, "recall.mspd": rec_mspd, "recall.AR_VSD": rec_vsd.mean(), "recall.AR_MSSD": rec_mssd.mean(),
                "recall.AR_MSPD": rec_mspd.mean(), "recall.AR": (rec_vsd.mean() + rec_mssd.mean() + rec_mspd.mean()) / 3.0})
    path = os.path.join(ROOT, "tests", "golden", "bop_recall.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    print("union", union, "inter", inter)
    print("vsd", np.round(vsd, 4))
    print("mssd", np.round(mssd, 5), "mspd", np.round(mspd, 3), "diam", diam)
    print({k: np.round(v, 4) for k, v in out.items() if k.startswith("recall.")})


if __name__ == "__main__":
    main()
