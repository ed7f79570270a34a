"""Writes tests/golden/mano_fit.npz by running the reference's own fitting module (anakin/postprocess/iknet/fittingunit.py, model.py,
utils.py, manolayer.py of lixiny/ArtiBoost) -- run by hand, never by a test; the output is committed.

The module loads under shims: `jax.numpy` -> numpy (so the reference's objective runs in float64), `jax.jit` -> identity,
`jax.grad` / `jax.experimental.optimizers` -> placeholders (the loop is not run here: the fit's step is pinned through its
objective and gradient), `cv2.Rodrigues` (the layer's loader, on the all-zero rest pose only), `opendr.*` and `transforms3d` (the
drawing code, unused), and a MANO_RIGHT.pkl written from the seeded stand-in hand model into a temporary assets/mano_v1_2/models/.

Contents (16 hands, seeded):
  iknet_in [B,21,3], iknet_quat [B,16,4], iknet_so3 [B,48]  the reference IKNet (torch.manual_seed(IKNET_SEED) init, eval BatchNorm
                                                           statistics set as below) in float64 on the normalised joints
  so3_init [B,48], root [B,1,3], bone [B], target [B,21,3]  the inputs of `residuals` (fittingunit.py:157-163,190)
  params [B,59]                                            points (so3 | beta | bone) at which the objective is evaluated
  residuals [B]                                            `residuals` at those points, float64
  fd_grad [B,59]                                           central differences (h = 1e-6) of `residuals`, float64; the points
                                                           are chosen away from the |.| and clip kinks
  mano_de_verts [B,778,3], mano_de_joints [B,21,3]         `mano_de(params, root, bone)`

Run:  python tests/gen_mano_fit_golden.py <root of a lixiny/ArtiBoost checkout>"""
import importlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
IKNET_SEED, B, SEED = 0, 16, 5


def _rodrigues(v):
    from scipy.spatial.transform import Rotation
    return (Rotation.from_rotvec(np.asarray(v, dtype=np.float64).reshape(3)).as_matrix(),)


def _install_shims(ref_root):
    jax = types.ModuleType("jax")
    jax.jit = lambda f, *a, **k: f
    jax.grad = lambda f, *a, **k: None
    jnp = types.ModuleType("jax.numpy")
    jnp.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    jax.numpy = jnp
    exp = types.ModuleType("jax.experimental")
    opt = types.ModuleType("jax.experimental.optimizers")
    opt.adam = lambda *a, **k: (None, None, None)
    exp.optimizers = opt
    cv2 = types.ModuleType("cv2")
    cv2.Rodrigues = _rodrigues
    mods = {"jax": jax, "jax.numpy": jnp, "jax.experimental": exp, "jax.experimental.optimizers": opt, "cv2": cv2,
            "transforms3d": types.ModuleType("transforms3d")}
    for name in ("opendr", "opendr.camera", "opendr.renderer", "opendr.lighting"):
        m = types.ModuleType(name)
        m.ProjectPoints = m.ColoredRenderer = m.LambertianPointLight = None
        mods[name] = m
    # the reference's package path (model.py / utils.py import `anakin.postprocess.iknet`) -- not this repository's alias package
    for name, sub in (("anakin", "anakin"), ("anakin.postprocess", "anakin/postprocess"), ("anakin.postprocess.iknet", "anakin/postprocess/iknet")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref_root, sub)]
        mods[name] = m
    sys.modules.update(mods)


def write_mano_pkl(hm, root):
    import scipy.sparse as sp
    os.makedirs(os.path.join(root, "assets", "mano_v1_2", "models"))
    parents = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
    dd = {"hands_components": np.eye(45), "hands_mean": np.asarray(hm["hands_mean"], np.float64),
          "shapedirs": np.asarray(hm["shapedirs"], np.float64), "posedirs": np.asarray(hm["posedirs"], np.float64),
          "v_template": np.asarray(hm["v_template"], np.float64), "J_regressor": sp.csc_matrix(np.asarray(hm["J_regressor"], np.float64)),
          "weights": np.asarray(hm["weights"], np.float64), "f": np.asarray(hm["faces"], np.int64),
          "kintree_table": np.stack([np.asarray(parents, np.int64) % (2 ** 32), np.arange(16)]), "bs_type": "lrotmin"}
    with open(os.path.join(root, "assets", "mano_v1_2", "models", "MANO_RIGHT.pkl"), "wb") as f:
        pickle.dump(dd, f, protocol=2)


def seeded_iknet(IKNet):
    """The golden's IKNet: torch.manual_seed(IKNET_SEED) init, then BatchNorm running statistics from a second seeded generator."""
    import torch
    torch.manual_seed(IKNET_SEED)
    net = IKNet()
    g = torch.Generator().manual_seed(IKNET_SEED + 1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(0.2 * torch.rand(m.num_features, generator=g) - 0.1)
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net.double().eval()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_root = sys.argv[1]
    import torch
    from artiboost_amd.hpregnet import load_hand_model
    import fit_oracle as fo
    hm = load_hand_model(None)
    tmp = tempfile.mkdtemp(prefix="ab_fit_")
    write_mano_pkl(hm, tmp)
    _install_shims(ref_root)
    cwd = os.getcwd()
    os.chdir(tmp)                                        # fittingunit.py builds its layer from assets/mano_v1_2 at import
    try:
        fu = importlib.import_module("anakin.postprocess.iknet.fittingunit")
    finally:
        os.chdir(cwd)
    g = torch.Generator().manual_seed(SEED)
    pj = 0.03 * torch.randn(B, 21, 3, generator=g, dtype=torch.float64) + torch.tensor([0.0, 0.0, 0.6], dtype=torch.float64)
    root = pj[:, 9:10]
    joint_ = pj - root
    bone = torch.norm(joint_[:, 0] - joint_[:, 9], dim=1)
    target = joint_ / bone[:, None, None]
    net = seeded_iknet(fu.IKNet)
    with torch.no_grad():
        so3, quat = net(target)
    so3_init = so3.numpy()
    # evaluation points: the IKNet pose moved a little, some shape, the bone scaled; kept away from the kinks
    mano = fo.Mano(hm)
    rng = np.random.default_rng(SEED)
    params = np.zeros((B, 59))
    for b in range(B):
        while True:
            p = np.concatenate([so3_init[b] + 0.1 * rng.standard_normal(48), 0.3 * rng.standard_normal(10),
                                [bone[b].item() * (1 + 0.1 * rng.standard_normal())]])
            if not bool(fo.near_kink(torch.from_numpy(p[None]), root[b:b + 1], target[b:b + 1], mano, rel=1e-3)[0]):
                break
        params[b] = p

    def res(b, p):
        d = {"so3": p[:48], "beta": p[48:58], "bone": np.array([[[p[58]]]])}
        return float(fu.residuals(d, so3_init, np.zeros(10), root[b:b + 1].numpy(), target[b].numpy(), np.zeros((1, 21, 4))))
    r = np.array([res(b, params[b]) for b in range(B)])
    h = 1e-6
    fd = np.zeros((B, 59))
    for b in range(B):
        for k in range(59):
            e = np.zeros(59)
            e[k] = h
            fd[b, k] = (res(b, params[b] + e) - res(b, params[b] - e)) / (2 * h)
    vs, js = [], []
    for b in range(B):
        v, j = fu.mano_de({"so3": params[b, :48], "beta": params[b, 48:58]}, root[b:b + 1].numpy(), bone[b:b + 1, None, None].numpy())
        vs.append(np.asarray(v))
        js.append(np.asarray(j))
    out = os.path.join(ROOT, "tests", "golden", "mano_fit.npz")
    np.savez_compressed(out, iknet_seed=np.int64(IKNET_SEED), iknet_in=target.numpy(), iknet_quat=quat.numpy(), iknet_so3=so3_init,
                        so3_init=so3_init, root=root.numpy(), bone=bone.numpy(), target=target.numpy(), params=params, residuals=r,
                        fd_grad=fd, mano_de_verts=np.stack(vs), mano_de_joints=np.stack(js))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
