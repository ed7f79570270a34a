"""ChamferLoss / AlignLoss on the device, eager route (csrc/mesh_align.hip): the public classes on the tensors of
tests/golden/mesh_losses.npz; ab_chamfer_rigid and ab_procrustes_loss against float64 at the shapes where a path changes; determinism and
independence of the batch around a sample; an eager HybridBaseline step that holds both losses.  Nothing here captures a graph.

Bounds (none is a recorded figure): for every compared quantity the error is max |got - ref64| / max |ref64|, ref64 this project's classes
(or their numpy restatement) in float64 on the same fp32 inputs.  The kernel may be off by at most 4 x the error of the fp32 CPU torch route
measured the same way (the kernel sums in another order and the CPU route's error on one seeded input is a single draw), and not less than
sqrt(L) 2^-24 with L the longest sum that feeds the quantity.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

from test_mesh_losses_device_host import procrustes_closed_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = np.float64


def _rel(got, ref):
    ref = np.asarray(ref, F64)
    return float(np.abs(np.asarray(got, F64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _check(what, got, ref64, cpu32, L):
    """got within max(4 x the CPU fp32 route's error, sqrt(L) 2^-24) of ref64; -> (kernel error, CPU route error)."""
    e_cpu, e_got = _rel(cpu32, ref64), _rel(got, ref64)
    bound = max(4.0 * e_cpu, np.sqrt(L) * 2.0 ** -24)
    print(f"{what}: kernel {e_got:.3e}  cpu-fp32 {e_cpu:.3e}  ratio {e_got / max(e_cpu, 1e-300):.2f}  bound {bound:.3e}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert e_got <= bound, (what, e_got, bound, e_cpu)
    return e_got, e_cpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. golden, through the public classes
@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mesh_losses.npz"), allow_pickle=False))


PRED_KEYS = ("box_rot_rotmat", "boxroot_3d_abs", "joints_3d_abs")
TARG_KEYS = ("obj_verts_can", "obj_verts_3d", "obj_transf", "root_joint", "corners_vis", "joints_3d")


def _split(g, dtype, dev):
    targs = {k: torch.from_numpy(g[k]).to(dtype).to(dev) for k in TARG_KEYS}
    preds = {k: torch.from_numpy(g[k]).to(dtype).to(dev).requires_grad_(True) for k in PRED_KEYS}
    return preds, targs


def _run_classes(g, dtype, dev):
    from artiboost_amd.criterions import AlignLoss, ChamferLoss
    preds, targs = _split(g, dtype, dev)
    out = {}
    for loss, key in ((ChamferLoss(LAMBDA_CHAMFER=0.7), "chamfer_loss"), (AlignLoss(LAMBDA_PROCRUSTES_ALIGN=0.3), "procrustes_aligned_loss")):
        final, losses = loss(preds, targs)
        final.sum().backward()
        name = type(loss).__name__
        out["keys_" + name] = sorted(losses)
        out[key] = losses[key].detach().cpu().numpy()
        out["final_" + name] = final.detach().cpu().numpy()
        out["none_" + name] = [k for k, v in losses.items() if v is None]
    for k, p in preds.items():
        out["g_" + k] = p.grad.cpu().numpy()
    return out


def test_public_classes_on_the_device_reproduce_the_reference(golden):
    ref, cpu, got = _run_classes(golden, torch.float64, "cpu"), _run_classes(golden, torch.float32, "cpu"), _run_classes(golden, torch.float32, "cuda")
    B, N = golden["obj_verts_can"].shape[:2]
    for name in ("ChamferLoss", "AlignLoss"):
        assert got["keys_" + name] == list(golden["keys_" + name]) and got["none_" + name] == cpu["none_" + name], name
        assert got["final_" + name].shape == golden["final_" + name].shape == (1,)
    assert got["chamfer_loss"].shape == () and got["procrustes_aligned_loss"].shape == ()
    for k, L in (("chamfer_loss", B * N), ("final_ChamferLoss", B * N), ("g_box_rot_rotmat", N), ("g_boxroot_3d_abs", N),
                 ("procrustes_aligned_loss", 63), ("final_AlignLoss", 63), ("g_joints_3d_abs", 63)):
        _, e_cpu = _check(k, got[k], ref[k], cpu[k], L)
        # ... and against the reference's own fp32 values: the same bound plus the error those carry against float64 themselves
        e_gold, to_gold = _rel(golden[k], ref[k]), _rel(got[k], golden[k])
        bound = max(4.0 * e_cpu, np.sqrt(L) * 2.0 ** -24) + e_gold
        print(f"{k} vs golden: kernel {to_gold:.3e}  golden vs float64 {e_gold:.3e}  bound {bound:.3e}")
        assert to_gold <= bound, (k, to_gold, bound)
    # sample 2 is masked: no gradient at all
    assert not got["g_box_rot_rotmat"][2].any() and not got["g_boxroot_3d_abs"][2].any()
    assert got["g_box_rot_rotmat"][:2].any() and got["g_joints_3d_abs"].any()


def test_none_conventions_and_errors_on_the_device(golden):
    from artiboost_amd.criterions import AlignLoss, ChamferLoss
    preds, targs = _split(golden, torch.float32, "cuda")
    _, l = ChamferLoss(LAMBDA_CHAMFER=0.0)(preds, targs)
    assert l["chamfer_loss"] is None
    f, l = AlignLoss(LAMBDA_PROCRUSTES_ALIGN=0.0)(preds, targs)
    assert l["procrustes_aligned_loss"] is None and l["st_aligned_loss"] is None and float(f) == 0.0
    with pytest.raises(NotImplementedError):
        AlignLoss(LAMBDA_ST_ALIGN=1.0)(preds, targs)
    with pytest.raises(KeyError, match="obj_verts_can"):
        ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, {k: v for k, v in targs.items() if not k.startswith("obj_verts")})
    with torch.no_grad():                                    # no gradient buffers are asked for, the value is the same
        a = ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, targs)[1]["chamfer_loss"]
    b = ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, targs)[1]["chamfer_loss"]
    assert not a.requires_grad and b.requires_grad and torch.equal(a, b.detach())


def test_chamfer_rigid_op_refuses_an_undersized_gradient_buffer():
    from artiboost_amd import _lib as L
    L.lib()
    B, N, M = 2, 5, 7
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    ws = torch.zeros(int(torch.ops.artiboost_hip.chamfer_rigid_workspace(B, N, M)), dtype=torch.uint8, device="cuda")
    args = [z(B, N, 3), z(B, 9), z(B, 3), z(B, M, 3), z(B, 3), z(B, 8), B, N, M, z(1), None, None, None, None, z(B * 9 - 1), z(B, 3), ws]
    with pytest.raises(RuntimeError, match="'g_rot' holds"):
        torch.ops.artiboost_hip.chamfer_rigid(*args)
    args[14], args[16] = z(B, 9), ws[:-1]
    with pytest.raises(RuntimeError, match="bytes"):
        torch.ops.artiboost_hip.chamfer_rigid(*args)
    args[16] = ws
    args[15] = None                                         # g_rot without g_tsl: the entry point's own argument error
    with pytest.raises(RuntimeError, match="argument error"):
        torch.ops.artiboost_hip.chamfer_rigid(*args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. / 3. kernel forms against float64
def _chamfer_case(B, N, M, seed, masked=()):
    """Two different random clouds (no duplicates) of an object-sized box at 0.5 m depth; the rotation is a rotation plus noise (its nine
    entries are free variables); a visible sample has zeros among its corners_vis as well."""
    rng = np.random.default_rng(seed)
    can = 0.06 * rng.standard_normal((B, N, 3))
    rot = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)]) + 0.01 * rng.standard_normal((B, 3, 3))
    root = [0.0, 0.0, 0.5] + 0.05 * rng.standard_normal((B, 3))
    tsl = root + 0.02 * rng.standard_normal((B, 3))
    targ = 0.06 * rng.standard_normal((B, M, 3)) + 0.02 * rng.standard_normal((B, 1, 3))
    vis = (rng.random((B, 8)) > 0.4).astype(np.float32)
    vis[:, 0] = 1.0
    vis[list(masked)] = 0.0
    return [a.astype(np.float32) for a in (can, rot.reshape(B, 9), tsl, targ, root, vis)]


def _chamfer_f64(can, rot, tsl, targ, root, vis):
    can, rot, tsl, targ, root = (np.asarray(a, F64) for a in (can, rot, tsl, targ, root))
    B, N, M = can.shape[0], can.shape[1], targ.shape[1]
    keep = (np.asarray(vis) != 0).any(1).astype(F64)
    x = (np.einsum("bij,bnj->bni", rot.reshape(B, 3, 3), can) + tsl[:, None]) * keep[:, None, None]
    y = (targ + root[:, None]) * keep[:, None, None]
    o = dict(dist_xy=np.zeros((B, N)), dist_yx=np.zeros((B, M)), idx_xy=np.zeros((B, N), np.int64), idx_yx=np.zeros((B, M), np.int64),
             g_rot=np.zeros((B, 3, 3)), g_tsl=np.zeros((B, 3)), sure_xy=np.zeros((B, N), bool), sure_yx=np.zeros((B, M), bool))
    for b in range(B):
        d = ((x[b][:, None] - y[b][None]) ** 2).sum(-1)
        for tag, dd in (("xy", d), ("yx", d.T)):
            i = dd.argmin(1)
            best = dd[np.arange(len(i)), i]
            o["dist_" + tag][b], o["idx_" + tag][b] = best, i
            if dd.shape[1] > 1 and keep[b]:                 # (a masked sample ties everywhere, exactly: index 0 by the first-minimum rule)
                second = np.partition(dd, 1, axis=1)[:, 1]
                o["sure_" + tag][b] = (second - best) > 1e-6 * best
            else:
                o["sure_" + tag][b] = True
        gx = (2.0 / (B * N)) * (x[b] - y[b][o["idx_xy"][b]])
        np.add.at(gx, o["idx_yx"][b], (2.0 / (B * M)) * (x[b][o["idx_yx"][b]] - y[b]))
        o["g_tsl"][b], o["g_rot"][b] = keep[b] * gx.sum(0), keep[b] * (gx.T @ can[b])
    o["loss"] = o["dist_xy"].mean() + o["dist_yx"].mean()
    return o


def _chamfer_cpu_route(case, dtype):
    """The CPU torch route of the class: loss and gradients through ChamferLoss itself, the distances through its own expression."""
    from artiboost_amd.criterions import ChamferLoss, chamfer_distance_torch
    can, rot, tsl, targ, root, vis = (torch.from_numpy(a).to(dtype) for a in case)
    B = can.shape[0]
    preds = {"box_rot_rotmat": rot.reshape(B, 3, 3).clone().requires_grad_(True), "boxroot_3d_abs": tsl.reshape(B, 1, 3).clone().requires_grad_(True)}
    targs = {"obj_verts_can": can, "obj_verts_3d": targ, "root_joint": root, "corners_vis": vis}
    final, losses = ChamferLoss(LAMBDA_CHAMFER=1.0)(preds, targs)
    final.sum().backward()
    with torch.no_grad():
        keep = torch.any(vis != 0, dim=1).to(dtype)
        pred = torch.einsum("bij,b->bij", torch.matmul(preds["box_rot_rotmat"], can.permute(0, 2, 1)).permute(0, 2, 1) + preds["boxroot_3d_abs"], keep)
        dxy, dyx, _, _ = chamfer_distance_torch(pred, torch.einsum("bij,b->bij", targ + root.unsqueeze(1), keep))
    return dict(loss=losses["chamfer_loss"].detach().numpy(), dist_xy=dxy.numpy(), dist_yx=dyx.numpy(),
                g_rot=preds["box_rot_rotmat"].grad.numpy(), g_tsl=preds["boxroot_3d_abs"].grad.reshape(B, 3).numpy())


def _chamfer_kernel(case, want_grad=True):
    from artiboost_amd import kernels as K
    o = K.chamfer_rigid(*[_dev(a) for a in case], want_grad=want_grad, want_dist=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("B,N,M,masked", [(1, 1, 1, ()), (2, 65, 127, ()), (2, 127, 65, ()), (3, 1025, 300, (1,)), (2, 300, 2049, ())])
def test_chamfer_rigid_kernel_vs_float64(B, N, M, masked):
    case = _chamfer_case(B, N, M, 100 + N + M, masked)
    ref, got = _chamfer_f64(*case), _chamfer_kernel(case)
    cpu, cls64 = _chamfer_cpu_route(case, torch.float32), _chamfer_cpu_route(case, torch.float64)
    for k in ("loss", "dist_xy", "dist_yx", "g_rot", "g_tsl"):          # the numpy restatement is the class's arithmetic
        np.testing.assert_allclose(np.asarray(ref[k]).reshape(cls64[k].shape), cls64[k], rtol=1e-9, atol=1e-14 * max(np.abs(cls64[k]).max(), 1e-30), err_msg=k)
    assert got["loss"].shape == (1,) and got["g_rot"].shape == (B, 3, 3) and got["idx_xy"].dtype == np.int32
    for k, L in (("loss", B * max(N, M)), ("dist_xy", 3), ("dist_yx", 3), ("g_rot", max(N, M)), ("g_tsl", max(N, M))):
        _check(f"chamfer ({B},{N},{M}) {k}", got[k].reshape(np.shape(ref[k])), ref[k], cpu[k].reshape(np.shape(ref[k])), L)
    for tag in ("xy", "yx"):
        sure = ref["sure_" + tag]
        frac = sure.mean()
        print(f"chamfer ({B},{N},{M}) idx_{tag}: {frac:.4f} of the points have a float64 gap above 1e-6 of the best")
        assert frac >= 0.99
        assert np.array_equal(got["idx_" + tag][sure], ref["idx_" + tag][sure]), tag
        assert got["idx_" + tag].min() >= 0 and got["idx_" + tag].max() < (M if tag == "xy" else N)
    for b in masked:                                                     # zero distances, indices and gradients, exactly
        for k in ("dist_xy", "dist_yx", "idx_xy", "idx_yx", "g_rot", "g_tsl"):
            assert not got[k][b].any(), (k, b)
    # without the gradient buffers: the same loss and distances, bit for bit
    plain = _chamfer_kernel(case, want_grad=False)
    assert "g_rot" not in plain and all(np.array_equal(plain[k], got[k]) for k in plain)


def test_chamfer_first_minimum_wins_on_exact_ties():
    """A mesh padded by repetition (what ho_collate builds): every duplicate ties exactly, the lowest index wins as in argmin, and the
    gradient equals that of the float64 restatement, which resolves the ties the same way."""
    case = _chamfer_case(2, 40, 40, 7)
    for a in (case[0], case[3]):
        a[:, 25:] = a[:, :15]
    ref, got = _chamfer_f64(*case), _chamfer_kernel(case)
    cpu = _chamfer_cpu_route(case, torch.float32)
    assert got["idx_xy"].max() < 25 and got["idx_yx"].max() < 25
    assert np.array_equal(got["idx_xy"][:, 25:], got["idx_xy"][:, :15]) and np.array_equal(got["dist_yx"][:, 25:], got["dist_yx"][:, :15])
    for k in ("loss", "g_rot", "g_tsl"):
        _check("padded " + k, got[k].reshape(np.shape(ref[k])), ref[k], cpu[k].reshape(np.shape(ref[k])), 2 * 40)


def _procrustes_case(B, n, seed, kind="generic"):
    rng = np.random.default_rng(seed)
    targ = 0.05 * rng.standard_normal((B, n, 3))
    root = [0.0, 0.0, 0.5] + 0.05 * rng.standard_normal((B, 3))
    xyz = targ + root[:, None]
    if kind == "near":                                                    # within 1e-4 m of the target
        pred = xyz + rng.uniform(-5e-5, 5e-5, (B, n, 3))
    else:                                                                 # a rotated, scaled, shifted and noisy copy
        q = np.stack([np.linalg.qr(np.eye(3) + 0.3 * rng.standard_normal((3, 3)))[0] for _ in range(B)])
        q *= np.sign(np.linalg.det(q))[:, None, None]
        pred = (1.0 + 0.1 * rng.standard_normal((B, 1, 1))) * np.einsum("bij,bnj->bni", q, targ) + root[:, None] + 0.01 * rng.standard_normal((B, n, 3))
        if kind == "mirrored":
            pred[0] = (xyz[0] - xyz[0].mean(0)) * [-1.0, 1.0, 1.0] + xyz[0].mean(0)
        if kind == "coplanar":
            pred[..., 2] = 0.5
    return pred.astype(np.float32), targ.astype(np.float32), root.astype(np.float32)


def _procrustes_cpu_route(case, dtype, backward=True):
    from artiboost_amd.criterions import AlignLoss
    pred, targ, root = (torch.from_numpy(a).to(dtype) for a in case)
    pred.requires_grad_(backward)
    final, losses = AlignLoss(LAMBDA_PROCRUSTES_ALIGN=1.0)({"joints_3d_abs": pred}, {"joints_3d": targ, "root_joint": root})
    o = {"loss": losses["procrustes_aligned_loss"].detach().numpy()}
    if backward:
        final.sum().backward()
        o["g_pred"] = pred.grad.numpy()
    with torch.no_grad():
        xyz = targ + root.unsqueeze(1)
        o["aligned"] = AlignLoss.procrustes_align(xyz, pred.detach()).numpy()
        o["sample_loss"] = ((torch.from_numpy(o["aligned"]) - xyz) ** 2).mean((1, 2)).numpy()
    return o


def _procrustes_kernel(case, want_grad=True):
    from artiboost_amd import kernels as K
    o = K.procrustes_loss(*[_dev(a) for a in case], want_grad=want_grad, want_aligned=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("B,n,kind", [(1, 21, "generic"), (67, 21, "generic"), (1, 3, "generic"), (67, 3, "generic"), (5, 21, "mirrored"),
                                      (67, 21, "near"), (5, 21, "coplanar")])
def test_procrustes_kernel_vs_float64(B, n, kind):
    case = _procrustes_case(B, n, 300 + B + n, kind)
    grads = n > 3 and kind != "coplanar"              # a rank-deficient correlation: the gradient is unspecified, the numbers stay finite
    ref, cpu = _procrustes_cpu_route(case, torch.float64, grads), _procrustes_cpu_route(case, torch.float32, grads)
    got = _procrustes_kernel(case)
    loss64, sample64, g64 = procrustes_closed_form(*case)                # the closed form is the classes' arithmetic
    np.testing.assert_allclose(sample64, ref["sample_loss"], rtol=1e-6, atol=1e-9 * ref["sample_loss"].max())
    if grads:
        np.testing.assert_allclose(g64, ref["g_pred"], rtol=1e-6, atol=1e-6 * np.abs(ref["g_pred"]).max())
    assert got["loss"].shape == (1,) and got["sample_loss"].shape == (B,) and got["g_pred"].shape == (B, n, 3)
    assert all(np.isfinite(v).all() for v in got.values())
    tag = f"procrustes ({B},{n},{kind}) "
    _check(tag + "loss", got["loss"][0], ref["loss"], cpu["loss"], 3 * n)
    _check(tag + "sample_loss", got["sample_loss"], ref["sample_loss"], cpu["sample_loss"], 3 * n)
    _check(tag + "aligned", got["aligned"], ref["aligned"], cpu["aligned"], 3 * n)
    if grads:
        _check(tag + "g_pred", got["g_pred"], ref["g_pred"], cpu["g_pred"], 3 * n)
    if kind == "mirrored":                                               # no determinant correction: the mirrored hand aligns by a reflection
        assert got["sample_loss"][0] < (0.1 * 1e-5) ** 2 and ref["sample_loss"][0] < (0.1 * 1e-7) ** 2
    plain = _procrustes_kernel(case, want_grad=False)
    assert "g_pred" not in plain and all(np.array_equal(plain[k], got[k]) for k in plain)


# ------------------------------------------------------------------------------------------------ 4. determinism, batch independence
def test_two_calls_give_the_same_bits():
    case = _chamfer_case(3, 1025, 300, 5, masked=(1,))
    a, b = _chamfer_kernel(case), _chamfer_kernel(case)
    assert sorted(a) == ["dist_xy", "dist_yx", "g_rot", "g_tsl", "idx_xy", "idx_yx", "loss"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    case = _procrustes_case(67, 21, 6)
    a, b = _procrustes_kernel(case), _procrustes_kernel(case)
    assert sorted(a) == ["aligned", "g_pred", "loss", "sample_loss"] and all(np.array_equal(a[k], b[k]) for k in a)


def test_a_sample_does_not_depend_on_the_batch_around_it():
    """Alone (B = 1), second of two and at every position of four: distances, indices and per-sample losses are the same bits, and so are
    the gradients taken x B (1 / B is a power of two)."""
    full = _chamfer_case(4, 300, 257, 9)
    whole = _chamfer_kernel(full)
    for b in range(4):
        for rows in ([b], [(b + 1) % 4, b]):
            sub = _chamfer_kernel([a[rows] for a in full])
            Bs = len(rows)
            for k in ("dist_xy", "dist_yx", "idx_xy", "idx_yx"):
                assert np.array_equal(sub[k][-1], whole[k][b]), (k, b, Bs)
            for k in ("g_rot", "g_tsl"):
                assert np.array_equal(sub[k][-1] * np.float32(Bs), whole[k][b] * np.float32(4)), (k, b, Bs)
    full = _procrustes_case(4, 21, 10)
    whole = _procrustes_kernel(full)
    for b in range(4):
        for rows in ([b], [(b + 1) % 4, b]):
            sub = _procrustes_kernel([a[rows] for a in full])
            Bs = len(rows)
            for k in ("sample_loss", "aligned"):
                assert np.array_equal(sub[k][-1], whole[k][b]), (k, b, Bs)
            assert np.array_equal(sub["g_pred"][-1] * np.float32(Bs), whole["g_pred"][b] * np.float32(4)), (b, Bs)


# ------------------------------------------------------------------------------------------------ 5. end to end, eager
N_MESH = 32
_ASSETS = []


def _eager_run(steps=2):
    import random
    import yaml
    from artiboost_amd import registry as R
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.models import Arch
    from artiboost_amd.optim import FusedClipAdam
    from artiboost_amd.synth import ArtiBoostLoader
    from artiboost_amd.train import TrainStep
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_clasbased_meshloss_mi355x.yaml")))
    cfg["DATA_PRESET"]["IMAGE_SIZE"], cfg["DATA_PRESET"]["HEATMAP_SIZE"] = [64, 64], [8, 8]
    if not _ASSETS:
        _ASSETS.append(SceneAssets("HO3D", seed=1))
    random.seed(9); torch.manual_seed(9); np.random.seed(9)
    arch = dict(cfg["ARCH"], COMPUTE_DTYPE="f32", INIT_SEED=3, BACKBONE=dict(cfg["ARCH"]["BACKBONE"], TYPE="ResNet18"))
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=cfg["DATA_PRESET"]))
    hb = model.model_list[0]
    crit_cfg = [c for c in cfg["CRITERION"] if c["TYPE"] in ("JointsLoss", "ChamferLoss", "AlignLoss")]
    lambdas = [1.0, 0.5, 0.5]
    crit = Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(crit_cfg, preset_cfg=cfg["DATA_PRESET"], LAMBDAS=lambdas))
    assert [type(l).__name__ for l in crit.loss_list] == ["JointsLoss", "ChamferLoss", "AlignLoss"]
    opt = FusedClipAdam(model.models_params, lr=1e-3, max_norm=1.0, model=hb)
    model.train()
    loader = ArtiBoostLoader.from_assets(_ASSETS[0], dict(cfg["MANAGER"], MESH_QUERIES=N_MESH, EPOCH=1), cfg["DATA_PRESET"], 4, 4 * steps, device="cuda",
                                         compute_dtype=torch.float32, random_seed=1)
    loader.prepare()
    batches = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()} for b in loader][:steps]
    assert len(batches) == steps and batches[0]["obj_verts_can"].shape == (4, N_MESH, 3) and batches[0]["obj_verts_can"].is_cuda
    ts = TrainStep(model, crit, opt, batches[0], use_graph=False)
    assert ts.fused is None and not ts.use_graph          # a list that names either loss is outside the fused pose/loss kernel
    seen = []
    for b in batches:
        preds, total, losses = ts(b)
        torch.cuda.synchronize()
        seen.append(dict(preds={k: v.detach().cpu() for k, v in preds.items() if torch.is_tensor(v)},
                         batch={k: v.cpu() for k, v in ts.static.items() if torch.is_tensor(v) and not k.startswith("_")},
                         losses={k: v.detach().cpu().numpy() for k, v in losses.items() if v is not None}, grad=hb.store.grad.detach().cpu().clone(),
                         flat=hb.store.flat.detach().cpu().clone()))
    return seen


def test_eager_hybridbaseline_step_with_both_losses():
    from artiboost_amd.criterions import AlignLoss, ChamferLoss
    first, again = _eager_run(), _eager_run()
    for i, s in enumerate(first):
        assert {"chamfer_loss", "procrustes_aligned_loss", "joints_3d_loss", "final_loss"} <= set(s["losses"])
        for cls, key, L in ((ChamferLoss(LAMBDA_CHAMFER=1.0), "chamfer_loss", 4 * N_MESH), (AlignLoss(), "procrustes_aligned_loss", 63)):
            cpu = cls({k: v.float() for k, v in s["preds"].items()}, s["batch"])[1][key].numpy()
            ref = cls({k: v.double() for k, v in s["preds"].items()}, {k: (v.double() if v.is_floating_point() else v) for k, v in s["batch"].items()})[1][key].numpy()
            _check(f"step {i} {key}", s["losses"][key], ref, cpu, L)
        g = s["grad"]
        assert torch.isfinite(g).all() and g.abs().max() > 0, i
    assert not torch.equal(first[0]["flat"], first[1]["flat"])
    for a, b in zip(first, again):                        # the same seed again: the same bits
        assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["flat"], b["flat"])
        assert all(np.array_equal(a["losses"][k], b["losses"][k]) for k in a["losses"])
