"""CPU: ChamferLoss / AlignLoss / ObjLoss -- registry and alias surface, the torch routes against the reference's own values
(tests/golden/mesh_losses.npz, written by tests/gen_mesh_loss_golden.py) and the padded collate."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mesh_losses.npz"), allow_pickle=False))


def _split(g, dtype=torch.float32):
    t = lambda k: torch.from_numpy(g[k]).to(dtype) if g[k].dtype.kind == "f" else torch.from_numpy(g[k])      # noqa: E731
    targs = {k: t(k) for k in ("obj_verts_can", "obj_verts_3d", "obj_transf", "root_joint", "corners_vis", "joints_3d")}
    preds = {k: t(k).clone().requires_grad_(True) for k in ("box_rot_rotmat", "boxroot_3d_abs", "joints_3d_abs", "obj_verts_3d_abs")}
    return preds, targs


def test_loss_types_and_aliases_resolve():
    from artiboost_amd import registry as R
    import artiboost_amd.criterions as C
    for name in ("ChamferLoss", "AlignLoss", "ObjLoss"):
        assert R.LOSS.get(name) is getattr(C, name)
    losses = R.build_criterion_loss_list([{"TYPE": "ChamferLoss", "LAMBDA_CHAMFER": 1.0}, {"TYPE": "AlignLoss"},
                                          {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}], preset_cfg={})
    assert [type(l).__name__ for l in losses] == ["ChamferLoss", "AlignLoss", "ObjLoss"]
    assert losses[1].lambda_procrustes_align == 1.0 and losses[1].lambda_st_align == 0.0 and losses[0].output_key == "chamfer_loss_output"
    from anakin.criterions import (AlignLoss, ChamferLoss, Criterion, HandOrdLoss, JointsLoss, ManoLoss, ObjLoss, SceneOrdLoss,  # noqa: F401
                                   SymCornerLoss)
    from anakin.criterions.alignloss import AlignLoss as A2
    from anakin.criterions.chamferloss import ChamferLoss as C2
    from anakin.criterions.honetloss import ObjLoss as O2
    assert (A2, C2, O2) == (C.AlignLoss, C.ChamferLoss, C.ObjLoss)
    from anakin.datasets.hoquery import Queries
    assert (Queries.OBJ_VERTS_CAN, Queries.OBJ_VERTS_3D, Queries.OBJ_VERTS_2D) == ("obj_verts_can", "obj_verts_3d", "obj_verts_2d")


def test_torch_routes_reproduce_the_reference(golden):
    from artiboost_amd.criterions import AlignLoss, ChamferLoss, ObjLoss
    preds, targs = _split(golden)
    for loss, key in ((ChamferLoss(LAMBDA_CHAMFER=0.7), "chamfer_loss"), (AlignLoss(LAMBDA_PROCRUSTES_ALIGN=0.3), "procrustes_aligned_loss"),
                      (ObjLoss(LAMBDA_OBJ_VERTS_3D=0.5), "obj_verts_3d_loss")):
        final, losses = loss(preds, targs)
        final.sum().backward()
        name = type(loss).__name__
        assert sorted(losses) == list(golden["keys_" + name]), name
        np.testing.assert_allclose(losses[key].detach().numpy(), golden[key], rtol=2e-6, err_msg=key)
        np.testing.assert_allclose(final.detach().numpy(), golden["final_" + name], rtol=2e-6, err_msg=name)
    for k, p in preds.items():
        ref = golden["g_" + k]
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=1e-5, atol=2e-6 * np.abs(ref).max(), err_msg=k)


def test_none_conventions_and_errors(golden):
    from artiboost_amd.criterions import AlignLoss, ChamferLoss, ObjLoss
    preds, targs = _split(golden)
    _, l = ChamferLoss(LAMBDA_CHAMFER=0.0)(preds, targs)
    assert l["chamfer_loss"] is None
    f, l = AlignLoss(LAMBDA_PROCRUSTES_ALIGN=0.0)(preds, targs)
    assert l["procrustes_aligned_loss"] is None and l["st_aligned_loss"] is None and float(f) == 0.0
    with pytest.raises(NotImplementedError):
        AlignLoss(LAMBDA_ST_ALIGN=1.0)(preds, targs)
    _, l = ObjLoss(LAMBDA_OBJ_VERTS_3D=1.0)(preds, {k: v for k, v in targs.items() if k != "obj_verts_3d"})
    assert l["obj_verts_3d_loss"] is None
    bare = {k: v for k, v in targs.items() if not k.startswith("obj_verts")}
    with pytest.raises(KeyError, match="obj_verts_can"):
        ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, bare)


def test_masked_sample_counts_in_the_mean_and_mirrored_hand_aligns_by_reflection(golden):
    """The reference multiplies both clouds by any(corners_vis): a masked sample contributes distance 0 and no gradient but stays in the
    mean; it applies no determinant correction: an exactly mirrored hand aligns with loss 0."""
    from artiboost_amd.criterions import AlignLoss, ChamferLoss
    preds, targs = _split(golden, torch.float64)
    f, l = ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, targs)
    f.sum().backward()
    assert not preds["box_rot_rotmat"].grad[2].any() and not preds["boxroot_3d_abs"].grad[2].any()
    two = {k: v[:2] for k, v in targs.items()}
    _, l2 = ChamferLoss(LAMBDA_CHAMFER=1.0)({k: v[:2] for k, v in preds.items()}, two)
    np.testing.assert_allclose(float(l["chamfer_loss"].detach()) * 3, float(l2["chamfer_loss"].detach()) * 2, rtol=1e-12)
    xyz = targs["joints_3d"] + targs["root_joint"][:, None]
    mirrored = {"joints_3d_abs": xyz * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64)}
    _, l = AlignLoss()(mirrored, targs)
    # not to float64 rounding: the reference adds 1e-8 to both norms (~0.25 here), a 4e-8 relative scale mismatch on 0.1 m coordinates
    assert float(l["procrustes_aligned_loss"]) < (0.1 * 1e-7) ** 2


def test_ho_collate_pads_meshes_by_repetition():
    from artiboost_amd.datasets import ho_collate
    from artiboost_amd.registry import Queries
    rng = np.random.default_rng(0)
    ns = (5, 7, 3)
    samples = [{Queries.OBJ_VERTS_CAN: rng.normal(size=(n, 3)).astype(np.float32), Queries.OBJ_VERTS_3D: rng.normal(size=(n, 3)).astype(np.float32),
                Queries.OBJ_VERTS_2D: rng.normal(size=(n, 2)).astype(np.float32), Queries.ROOT_JOINT: np.zeros(3, np.float32), "obj_idx": n}
               for n in ns]
    keep = [{k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in s.items()} for s in samples]
    out = ho_collate(samples)
    for q in (Queries.OBJ_VERTS_CAN, Queries.OBJ_VERTS_3D, Queries.OBJ_VERTS_2D):
        assert out[q].shape[:2] == (3, 7)
        for b, n in enumerate(ns):
            np.testing.assert_array_equal(out[q][b].numpy(), keep[b][q][np.arange(7) % n])
    assert out[Queries.PADDING_MASK].tolist() == [[1] * 5 + [0] * 2, [1] * 7, [1] * 3 + [0] * 4]
    assert out["obj_idx"].tolist() == list(ns)
    # a batch without mesh queries: exactly the former result (stacked per key, no mask)
    plain = [{Queries.ROOT_JOINT: rng.normal(size=3).astype(np.float32), Queries.JOINTS_3D: rng.normal(size=(21, 3)), "obj_idx": i} for i in range(3)]
    out = ho_collate(plain)
    assert set(out) == {Queries.ROOT_JOINT, Queries.JOINTS_3D, "obj_idx"}
    for k in (Queries.ROOT_JOINT, Queries.JOINTS_3D):
        np.testing.assert_array_equal(out[k].numpy(), np.stack([p[k] for p in plain]))
        assert out[k].dtype == torch.from_numpy(plain[0][k]).dtype
