"""TEST INFRASTRUCTURE -- writes tests/golden/real_mesh.npz: what the REAL reference reader (anakin/datasets/ho3d.py: class HO3D, SPLIT_MODE
"paper") returns from the getters a real frame's mesh queries are defined by, for every train and test frame of the
miniature HO3D v2 tree of tests/ho3d_fake_tree.py (seed 7):
  <split>.<i>.obj_verts_can     get_obj_verts_can(i)[0]      (ho3d.py:376-385)
  <split>.<i>.obj_verts_transf  get_obj_verts_transf(i)      (:401-413)
  <split>.<i>.hand_verts_3d     get_hand_verts_3d(i)         (:253-262)
  <split>.<i>.joints_3d         get_joints_3d(i)
  <split>.n, hand_seed
Run by hand, never by a test; the output is committed.  The recipe is oracle/gen_ho3d_reader_golden.py's (oracle/ref_import.py unchanged;
cv2.Rodrigues -> scipy's rotation vectors, trimesh.load -> the `v` / `f` lines of the file).  One more third-party boundary is crossed here:
`manotorch.manolayer.ManoLayer`, which HOdata.__init__ builds (hodata.py:129-135: rot_mode "axisang", use_pca False, flat_hand_mean True,
center_idx None) and get_hand_verts_3d calls, is absent and needs the licensed MANO model; it is bound to a stand-in that evaluates
oracle/pose_oracle.mano_lbs on artiboost_amd.assets.make_hand_model(hand_seed) in float64.  Parity is UNPINNED at exactly that call, as for
the refiner's and HoNet's goldens: everything around it (the annotation substitution of evaluation frames :171-175, handTrans, cam_extr, the
cast) is the reference's own code.

Run:  python tests/gen_real_mesh_golden.py"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
HAND_SEED = 1


def main():
    import torch
    from scipy.spatial.transform import Rotation
    import ho3d_fake_tree as T
    import pose_oracle as po
    import ref_import
    from artiboost_amd.assets import make_hand_model
    ref_import.load_control_plane()
    hand = make_hand_model(HAND_SEED)

    class MANOOutput:
        def __init__(self, verts, joints):
            self.verts, self.joints = verts, joints

    class ManoLayer:
        def __init__(self, rot_mode="axisang", use_pca=False, mano_assets_root=None, center_idx=None, flat_hand_mean=True, **kw):
            assert rot_mode == "axisang" and not use_pca and center_idx is None and flat_hand_mean and not kw

        def __call__(self, pose_coeffs, betas):
            v, j, _ = po.mano_lbs(hand, pose_coeffs.double().numpy(), betas.double().numpy())
            return MANOOutput(torch.from_numpy(v), torch.from_numpy(j))

    ml = types.ModuleType("manotorch.manolayer")
    ml.ManoLayer, ml.MANOOutput = ManoLayer, MANOOutput
    sys.modules["manotorch.manolayer"] = ml
    cv2 = sys.modules["cv2"]
    cv2.Rodrigues = lambda r: (Rotation.from_rotvec(np.asarray(r, np.float64).reshape(3)).as_matrix(), None)
    trimesh = sys.modules["trimesh"]

    def load(path, process=False):
        v, f = [], []
        for line in open(path):
            if line.startswith("v "):
                v.append([float(t) for t in line.split()[1:4]])
            elif line.startswith("f "):
                f.append([int(t.split("/")[0]) - 1 for t in line.split()[1:4]])
        return types.SimpleNamespace(vertices=np.asarray(v), faces=np.asarray(f), bounding_box_oriented=types.SimpleNamespace(vertices=np.zeros((8, 3))))
    trimesh.load = load
    dep, sph = types.ModuleType("deprecated"), types.ModuleType("deprecated.sphinx")
    sph.deprecated = lambda **k: (lambda fn: fn)
    dep.sphinx = sph
    sys.modules.setdefault("deprecated", dep)
    sys.modules.setdefault("deprecated.sphinx", sph)
    if not hasattr(np, "asfarray"):                                      # removed in NumPy 2 (ho3dutils.py:28, ho3d.py:385)
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)
    import anakin.datasets.hodata  # noqa
    from anakin.datasets.ho3d import HO3D
    root = tempfile.mkdtemp(prefix="ho3d_fake_")
    T.build(root, seed=7)
    os.chdir(tempfile.mkdtemp(prefix="ho3d_cache_"))                       # the reference writes common/cache/... relative to the cwd
    out = {"hand_seed": np.int64(HAND_SEED)}
    for split in ("train", "test"):
        ds = HO3D(DATA_ROOT=root, DATA_SPLIT=split, SPLIT_MODE="paper", AUG=False, AUG_PARAM=None, MINI_FACTOR=1.0,
                  DATA_PRESET={"USE_CACHE": False, "FILTER_NO_CONTACT": False, "FILTER_THRESH": 0.0, "BBOX_EXPAND_RATIO": 1.2, "FULL_IMAGE": False,
                               "IMAGE_SIZE": [224, 224], "CENTER_IDX": 0, "CROP_MODEL": "hand_obj"})
        assert isinstance(ds.mano_layer, ManoLayer)
        out[f"{split}.n"] = np.int64(len(ds))
        for i in range(len(ds)):
            pre = f"{split}.{i}."
            out[pre + "obj_verts_can"] = ds.get_obj_verts_can(i)[0]
            out[pre + "obj_verts_transf"] = ds.get_obj_verts_transf(i)
            out[pre + "hand_verts_3d"] = ds.get_hand_verts_3d(i)
            out[pre + "joints_3d"] = ds.get_joints_3d(i)
    path = os.path.join(ROOT, "tests", "golden", "real_mesh.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
