"""Loss plugin classes with the reference's names, config keys and RNG behaviour
(anakin/criterions/criterion.py:8-67, jointloss.py:14-67, ordinal.py:17-306, symcornerloss.py:18-102).

The ordinal losses draw from the same global RNGs in the same order as the reference (torch.rand for the virtual
view vectors, random.shuffle for the pair subsets), so seeding `random` and `torch` identically reproduces the
reference's loss values.  Tensors here are tiny ((B,21,3)-sized); the arithmetic runs as device torch ops."""
import ctypes
import os
import random
from itertools import combinations, product
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .registry import CONST, LOSS, Queries, camel_to_snake


class TensorLoss(object):
    def __init__(self):
        self.output_key = f"{camel_to_snake(type(self).__name__)}_output"

    def __call__(self, preds: Dict, targs: Dict, **kwargs) -> Tuple[torch.Tensor, Dict]:
        dev = None
        for v in preds.values():
            if isinstance(v, torch.Tensor):
                dev = v.device
                break
        if dev is None:
            raise RuntimeError("Cannot found valid Tensor with device")
        return torch.zeros(1, dtype=torch.float32, device=dev), {}


class Criterion(TensorLoss):
    def __init__(self, cfg: Dict, loss_list: List[TensorLoss]) -> None:
        super().__init__()
        self._loss_list = loss_list
        lambdas = list(cfg["LAMBDAS"])
        self._loss_lambdas = {type(l).__name__: lambdas[i] for i, l in enumerate(loss_list)}
        # predictions that come straight from the HIP model carry a link to its raw outputs; with it compute_losses runs
        # the fused pose/loss kernel instead of the registry losses' torch ops.  FUSED_CRITERION: false / AB_FUSED_CRITERION=0: off
        self.fused_route = bool(cfg.get("FUSED_CRITERION", os.environ.get("AB_FUSED_CRITERION", "1") != "0"))

    @property
    def loss_list(self):
        return self._loss_list

    @property
    def loss_lambdas(self):
        return self._loss_lambdas

    def draw(self, dev):
        """Refresh the random draws of every loss (host RNG, reference order) into their device buffers.  On a GPU the
        draws of all losses are packed into one pinned staging tensor and shipped with a single H2D copy."""
        dev = torch.device(dev)
        arena = None
        if dev.type == "cuda":
            arena = getattr(self, "_draw_arena", None)
            if arena is None:
                arena = self._draw_arena = _DrawArena()
            arena.begin()
        for loss in self.loss_list:
            if hasattr(loss, "draw"):
                if hasattr(loss, "draws"):
                    loss.draws.arena = arena
                loss.draw(dev)
        if arena is not None:
            arena.flush(dev)
            for loss in self.loss_list:          # a loss called on its own (not through this method) copies directly
                if hasattr(loss, "draws"):
                    loss.draws.arena = None

    def freeze_draws(self, frozen=True):
        for loss in self.loss_list:
            if hasattr(loss, "draws"):
                loss.draws.frozen = frozen

    # ---- the fused route of the reference-shaped loop ----------------------------------------------------------------
    _FUSED_TARGETS = (Queries.ROOT_JOINT, Queries.CAM_INTR, Queries.CORNERS_CAN, Queries.JOINTS_3D, Queries.CORNERS_3D,
                      Queries.JOINTS_VIS, Queries.CORNERS_VIS)

    def _fused_for(self, link):
        """FusedPoseCriterion of this loss list for the model geometry in `link`, or None when a loss is outside the kernel."""
        key = (tuple(link["inp_res"]), link["center_idx"])
        cache = self.__dict__.setdefault("_fused_cache", {})
        if key not in cache:
            cache[key] = fused_or_none(FusedPoseCriterion, self, link["inp_res"], link["center_idx"])
        return cache[key]

    def _compute_losses_fused(self, link, targs):
        """One HIP kernel (csrc/pose_loss.hip) for pose assembly + all losses + their gradients, behind `compute_losses`:
        the ~350 small torch kernels per step of the registry losses and of their autograd backward disappear, and the
        update becomes deterministic (the autograd backward of index_select accumulates with float atomics)."""
        fused = self._fused_for(link)
        if fused is None:
            return None
        kp3d, box6d = link["kp3d"], link["box6d"]
        dev = kp3d.device
        t = {}
        for k in self._FUSED_TARGETS:
            v = targs[k]
            if not torch.is_tensor(v):
                return None
            t[k] = v.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        if fused.sym is not None:                            # SymCornerLoss: the object's class index and pose
            for k, dt in ((Queries.OBJ_IDX, torch.int64), (Queries.OBJ_TRANSF, torch.float32)):
                v = targs.get(k)
                if not torch.is_tensor(v):
                    return None
                t[k] = v.to(device=dev, dtype=dt, non_blocking=True).contiguous()
        if not all(l.draws.frozen for l in self.loss_list if hasattr(l, "draws")):
            self.draw(dev)                                   # reference RNG order: the losses' draws in list order
        total, vals, sym = _FusedLossFn.apply(kp3d, box6d, fused, t)
        out = {}
        for loss in self.loss_list:                          # the entries each registry class reports
            if isinstance(loss, JointsLoss):
                out["joints_3d_loss"] = vals[0] if loss.lambda_joints_3d else None
                out["corners_3d_loss"] = vals[1] if loss.lambda_corners_3d else None
                out[loss.output_key] = loss.lambda_joints_3d * vals[0] + loss.lambda_corners_3d * vals[1]
            elif isinstance(loss, HandOrdLoss):
                out["joint_ord_loss"], out["part_ord_loss"] = vals[2], vals[3]
                out[loss.output_key] = loss.lambda_joint_lev * vals[2] + loss.lambda_part_lev * vals[3]
            elif isinstance(loss, SceneOrdLoss):
                out["scene_ord_loss"] = vals[4]
            elif isinstance(loss, SymCornerLoss):
                out["sym_corners_3d_loss"] = sym[0] if loss.lambda_sym_corners_3d else None
                out[loss.output_key] = loss.lambda_sym_corners_3d * sym[0]
        out["final_loss"] = total
        return total, out

    def compute_losses(self, preds: Dict, targs: Dict, **kwargs):
        link = getattr(preds.get("joints_3d_abs"), "_ab_fuse", None) if self.fused_route else None
        if link is not None and torch.is_grad_enabled():
            r = self._compute_losses_fused(link, targs)
            if r is not None:
                return r
        total, out = super().__call__(preds, targs, **kwargs)
        for loss in self.loss_list:
            fl, d = loss(preds, targs, **kwargs)
            total = total + self.loss_lambdas[type(loss).__name__] * fl
            out.update(d)
        assert "final_loss" not in out
        out["final_loss"] = total
        return total, out


def _abs_masked(preds, targs, dev):
    root = targs[Queries.ROOT_JOINT].to(dev)
    jv = targs[Queries.JOINTS_VIS].to(dev)[..., None]
    cv = targs[Queries.CORNERS_VIS].to(dev)[..., None]
    jt = (targs[Queries.JOINTS_3D].to(dev) + root[:, None]) * jv
    ct = (targs[Queries.CORNERS_3D].to(dev) + root[:, None]) * cv
    return preds["joints_3d_abs"] * jv, jt, preds["corners_3d_abs"] * cv, ct


@LOSS.register_module
class JointsLoss(TensorLoss):
    def __init__(self, **cfg):
        super().__init__()
        self.lambda_joints_3d = cfg.get("LAMBDA_JOINTS_3D", 0.0)
        self.lambda_corners_3d = cfg.get("LAMBDA_CORNERS_3D", 0.0)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        jp, jt, cp, ct = _abs_masked(preds, targs, final_loss.device)
        lj = F.mse_loss(jp, jt) if self.lambda_joints_3d else None
        lc = F.mse_loss(cp, ct) if self.lambda_corners_3d else None
        if lj is not None:
            final_loss = final_loss + self.lambda_joints_3d * lj
        if lc is not None:
            final_loss = final_loss + self.lambda_corners_3d * lc
        losses["joints_3d_loss"] = lj
        losses["corners_3d_loss"] = lc
        losses[self.output_key] = final_loss
        return final_loss, losses


@LOSS.register_module
class ManoLoss(TensorLoss):
    """anakin/criterions/honetloss.py:12-73: MANO shape / pose regularisers and (optional) joint / vertex supervision of the
    regression-based model (config_eval/eval_ho3dv2_regbased_artiboost.yaml)."""

    def __init__(self, **cfg):
        super().__init__()
        self.lambda_joints_3d = float(cfg["LAMBDA_JOINTS_3D"])
        self.lambda_hand_verts_3d = float(cfg["LAMBDA_HAND_VERTS_3D"])
        self.lambda_shape_reg = float(cfg["LAMBDA_SHAPE_REG"])
        self.lambda_pose_reg = float(cfg["LAMBDA_POSE_REG"])

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        shape_reg = pose_reg = lj = lv = None
        if self.lambda_shape_reg:
            shape_reg = preds["mano_shape"].pow(2).mean()
            final_loss = final_loss + self.lambda_shape_reg * shape_reg
        if self.lambda_pose_reg:
            pose_reg = preds["mano_pca_pose"][:, 3:].pow(2).mean()            # the root rotation is not regularised
            final_loss = final_loss + self.lambda_pose_reg * pose_reg
        if self.lambda_joints_3d and Queries.JOINTS_3D in targs:
            p = preds["joints_3d_abs"]
            lj = F.mse_loss(p, targs[Queries.JOINTS_3D].to(p.device) + targs[Queries.ROOT_JOINT].to(p.device).unsqueeze(1))
            final_loss = final_loss + self.lambda_joints_3d * lj
        if self.lambda_hand_verts_3d and "hand_verts_3d" in targs:
            p = preds["hand_verts_3d_abs"]
            lv = F.mse_loss(p, targs["hand_verts_3d"].to(p.device) + targs[Queries.ROOT_JOINT].to(p.device).unsqueeze(1))
            final_loss = final_loss + self.lambda_hand_verts_3d * lv
        losses.update(mano_shape=shape_reg, mano_pca_pose=pose_reg, joints_3d_loss=lj, hand_verts_3d_loss=lv)
        return final_loss, losses


def sample_view_vectors(n_virtual_views=20):
    """ordinal.py:59-71 (CPU draws from the global torch RNG: rand(n) for theta, then rand(n) for u)."""
    cam_vec = torch.Tensor([0.0, 0.0, 1.0]).unsqueeze(0)
    theta = torch.rand(n_virtual_views) * 2.0 * np.pi
    u = torch.rand(n_virtual_views)
    s = torch.sqrt(1.0 - u ** 2)
    nv = torch.cat([(s * torch.cos(theta)).unsqueeze(1), (s * torch.sin(theta)).unsqueeze(1), u.unsqueeze(1)], dim=1)
    return torch.cat([cam_vec, nv], dim=0)


def _shuffled_third(n):
    idx = list(range(n))
    random.shuffle(idx)
    return idx[: n // 3]


class _DrawArena:
    """One persistent device byte buffer for every per-step draw of a Criterion: `add` records (owner, name, cpu tensor) in
    call order, `flush` packs them (16-byte aligned slots, layout fixed by the first step), pins the pack and issues ONE
    async H2D copy; the owners' `bufs[name]` are typed views into the device buffer (stable addresses for hipGraphs)."""

    def __init__(self):
        self.items, self.layout, self.dev_buf = [], None, None

    def begin(self):
        self.items = []

    def add(self, owner, name, cpu_tensor):
        self.items.append((owner, name, cpu_tensor.contiguous()))

    def flush(self, dev):
        sig = tuple((id(o), n, tuple(t.shape), t.dtype) for o, n, t in self.items)
        if self.layout is None or self.layout[0] != sig:
            offs, off = [], 0
            for _, _, t in self.items:
                offs.append(off)
                off += (t.numel() * t.element_size() + 15) // 16 * 16
            self.layout = (sig, offs, off)
            self.dev_buf = torch.empty(max(off, 16), dtype=torch.uint8, device=dev)
            self.views = [self.dev_buf[b:b + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for (_, _, t), b in zip(self.items, offs)]
        for (o, n, _), v in zip(self.items, self.views):      # (re)bind every step: a loss called on its own in between
            o.bufs[n] = v                                       # (registry route) works on private buffers, see _Draws.put
        _, offs, total = self.layout
        pack = torch.empty(max(total, 16), dtype=torch.uint8)
        for (_, _, t), b in zip(self.items, offs):
            nb = t.numel() * t.element_size()
            pack[b:b + nb] = t.reshape(-1).view(torch.uint8)
        self.dev_buf.copy_(pack.pin_memory(), non_blocking=True)      # a fresh pinned block per step: no reuse hazard


class _Draws:
    """Per-call random draws of the ordinal losses, kept in persistent device buffers so that the arithmetic can be
    captured in a hipGraph: `draw()` (host RNG, same order as the reference) refreshes the buffers with async H2D
    copies OUTSIDE the graph; the captured ops only read them."""

    def __init__(self):
        self.dev = None
        self.bufs = {}
        self.frozen = False     # True while a captured graph owns the call: __call__ must not draw
        self.arena = None       # set by Criterion.draw: pack all draws of the step into one H2D copy

    def put(self, name, cpu_tensor, dev):
        if self.arena is not None:
            self.arena.add(self, name, cpu_tensor)
            return None
        b = self.bufs.get(name)
        # buffers are persistent (a captured hipGraph holds their addresses) -- but never a view of the arena here: the
        # arena's views share one version counter, and an in-place refresh of one would invalidate what autograd saved of another
        if b is None or b.shape != cpu_tensor.shape or b._base is not None:
            b = torch.empty(cpu_tensor.shape, dtype=cpu_tensor.dtype, device=dev)
            self.bufs[name] = b
        src = cpu_tensor.pin_memory() if dev.type == "cuda" else cpu_tensor
        b.copy_(src, non_blocking=True)
        return b


def _ord(a, b, views):      # jointlevel_ordinal_relation (ordinal.py:39-56)
    return torch.einsum("bpk,vk->bpv", a - b, views)


@LOSS.register_module
class HandOrdLoss(TensorLoss):
    def __init__(self, **cfg):
        super().__init__()
        self.lambda_part_lev = float(cfg.get("LAMBDA_PART_LEVEL", 1.0))
        self.lambda_joint_lev = float(cfg.get("LAMBDA_JOINTS_LEVEL", 1.0))
        self.n_virtual_views = int(cfg.get("N_VIRTUAL_VIEWS", 20))
        self.joint_pairs_idx = list(combinations(range(CONST.NUM_JOINTS), 2))
        self.parts_pairs_idx = list(combinations(range(CONST.NUM_JOINTS - 1), 2))
        self.draws = _Draws()

    def draw(self, dev):
        """RNG order of the reference (ordinal.py:159,165-166,202-203): views, joint-pair shuffle, part-pair shuffle."""
        d = self.draws
        d.put("views", sample_view_vectors(self.n_virtual_views), dev)
        sel = _shuffled_third(len(self.joint_pairs_idx))
        d.put("j0", torch.tensor([self.joint_pairs_idx[i][0] for i in sel]), dev)
        d.put("j1", torch.tensor([self.joint_pairs_idx[i][1] for i in sel]), dev)
        sel = _shuffled_third(len(self.parts_pairs_idx))
        d.put("p0", torch.tensor([self.parts_pairs_idx[i][0] for i in sel]), dev)
        d.put("p1", torch.tensor([self.parts_pairs_idx[i][1] for i in sel]), dev)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        dev = final_loss.device
        jp, jt, _, _ = _abs_masked(preds, targs, dev)
        if not self.draws.frozen:
            self.draw(dev)
        b = self.draws.bufs
        views, i0, i1 = b["views"], b["j0"], b["j1"]
        gt = _ord(jt.index_select(1, i0), jt.index_select(1, i1), views)
        pr = _ord(jp.index_select(1, i0), jp.index_select(1, i1), views)
        joint_ord_loss = torch.log(1.0 + F.relu(-1.0 * torch.sign(gt) * pr)).mean()
        final_loss = final_loss + self.lambda_joint_lev * joint_ord_loss
        losses["joint_ord_loss"] = joint_ord_loss

        def parts(j):   # joints_2_part_pairs (ordinal.py:98-121)
            return (j - j[:, CONST.JOINTS_IDX_PARENTS])[:, 1:]

        pp, pt = parts(jp), parts(jt)
        a0, a1 = b["p0"], b["p1"]
        gt = torch.einsum("bpk,vk->bpv", torch.cross(pt.index_select(1, a0), pt.index_select(1, a1), dim=-1), views)
        pr = torch.einsum("bpk,vk->bpv", torch.cross(pp.index_select(1, a0), pp.index_select(1, a1), dim=-1), views)
        part_ord_loss = F.relu(-1.0 * torch.sign(gt) * pr).mean()
        final_loss = final_loss + self.lambda_part_lev * part_ord_loss
        losses["part_ord_loss"] = part_ord_loss
        losses[self.output_key] = final_loss
        return final_loss, losses


@LOSS.register_module
class SceneOrdLoss(TensorLoss):
    def __init__(self, **cfg):
        super().__init__()
        self.lambda_scene_lev = float(cfg.get("LAMBDA_SCENE_LEVEL", 1.0))
        self.n_virtual_views = int(cfg.get("N_VIRTUAL_VIEWS", 40))
        self.ho_pairs_idx = list(product(range(CONST.NUM_JOINTS), range(CONST.NUM_CORNERS)))
        self.draws = _Draws()

    def draw(self, dev):
        d = self.draws
        d.put("views", sample_view_vectors(self.n_virtual_views), dev)
        sel = _shuffled_third(len(self.ho_pairs_idx))
        d.put("i0", torch.tensor([self.ho_pairs_idx[i][0] for i in sel]), dev)
        d.put("i1", torch.tensor([self.ho_pairs_idx[i][1] for i in sel]), dev)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        dev = final_loss.device
        jp, jt, cp, ct = _abs_masked(preds, targs, dev)
        if not self.draws.frozen:
            self.draw(dev)
        b = self.draws.bufs
        views, i0, i1 = b["views"], b["i0"], b["i1"]
        gt = _ord(jt.index_select(1, i0), ct.index_select(1, i1), views)
        pr = _ord(jp.index_select(1, i0), cp.index_select(1, i1), views)
        scene_ord_loss = torch.log(1.0 + F.relu(-1.0 * torch.sign(gt) * pr)).mean()
        final_loss = final_loss + self.lambda_scene_lev * scene_ord_loss
        losses["scene_ord_loss"] = scene_ord_loss
        return final_loss, losses


def get_symmetry_transformations(model_info, max_sym_disc_step):
    """anakin/utils/bop_toolkit/bop_misc.py:18-65 (BOP toolkit): discrete x discretised-continuous symmetries."""
    trans_disc = [{"R": np.eye(3), "t": np.array([[0, 0, 0]]).T}]
    for sym in model_info.get("symmetries_discrete", []):
        s = np.reshape(sym, (4, 4))
        trans_disc.append({"R": s[:3, :3], "t": s[:3, 3].reshape((3, 1))})
    trans_cont = []
    for sym in model_info.get("symmetries_continuous", []):
        axis = np.array(sym["axis"], dtype=np.float64)
        offset = np.array(sym["offset"], dtype=np.float64).reshape((3, 1))
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        axis_n = axis / np.linalg.norm(axis)
        for i in range(1, steps):
            a = i * step
            K_ = np.array([[0, -axis_n[2], axis_n[1]], [axis_n[2], 0, -axis_n[0]], [-axis_n[1], axis_n[0], 0]])
            R = np.cos(a) * np.eye(3) + (1 - np.cos(a)) * np.outer(axis_n, axis_n) + np.sin(a) * K_
            trans_cont.append({"R": R, "t": -R.dot(offset) + offset})
    trans = []
    for td in trans_disc:
        if trans_cont:
            for tc in trans_cont:
                trans.append({"R": tc["R"].dot(td["R"]), "t": tc["R"].dot(td["t"]) + tc["t"]})
        else:
            trans.append(td)
    return trans


@LOSS.register_module
class SymCornerLoss(TensorLoss):
    def __init__(self, **cfg):
        super().__init__()
        self.lambda_sym_corners_3d = cfg.get("LAMBDA_SYM_CORNERS_3D", 0.0)
        info = cfg.get("MODEL_INFO")
        if info is None:
            import json
            info = json.load(open(cfg["MODEL_INFO_PATH"], "r"))
        step = cfg.get("MAX_SYM_DISC_STEP", 0.01)
        if cfg.get("USE_HO3D_YCB", False):
            raise NotImplementedError("USE_HO3D_YCB")
        syms = [get_symmetry_transformations(info[str(i)], step) for i in range(1, len(info) + 1)]
        kmax = max(len(s) for s in syms)
        R = np.tile(np.eye(3), (len(syms), kmax, 1, 1))
        t = np.zeros((len(syms), kmax, 3, 1))
        for i, s in enumerate(syms):
            for k, tr in enumerate(s):
                R[i, k] = tr["R"]
                t[i, k] = tr["t"] / 1000.0
        self.R = torch.Tensor(R)
        self.t = torch.Tensor(t)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        dev = final_loss.device
        loss = None
        if self.lambda_sym_corners_3d:
            obj = (targs[Queries.OBJ_IDX] - 1).long().to(dev)
            Rs, ts = self.R.to(dev)[obj], self.t.to(dev)[obj]
            T = targs[Queries.OBJ_TRANSF].to(dev)
            can = targs[Queries.CORNERS_CAN].to(dev).permute(0, 2, 1)[:, None]
            sym_can = torch.matmul(Rs, can) + ts
            gt = (torch.matmul(T[:, None, :3, :3], sym_can) + T[:, None, :3, 3:]).permute(0, 1, 3, 2)
            vis = targs[Queries.CORNERS_VIS].to(dev)
            pred = (preds["corners_3d_abs"] * vis[..., None])[:, None]
            gt = gt * vis[:, None, :, None]
            loss = ((gt - pred) ** 2).mean(-1).mean(-1).min(dim=-1)[0].mean()
            final_loss = final_loss + self.lambda_sym_corners_3d * loss
        losses["sym_corners_3d_loss"] = loss
        losses[self.output_key] = final_loss
        return final_loss, losses


class _FusedLossFn(torch.autograd.Function):
    """final_loss as a function of the network's raw outputs; the kernel has already produced its gradient."""

    @staticmethod
    def forward(ctx, kp3d, box6d, fused, targs):
        o = fused(kp3d.detach().contiguous(), box6d.detach().contiguous(), box6d.shape[-1], targs, backward=True)
        vals, sym = o["losses"].clone(), o["sym_loss"].clone()
        ctx.save_for_backward(o["g_kp3d"].clone(), o["g_box6d"].clone())
        ctx.mark_non_differentiable(vals, sym)
        return vals[5].clone(), vals, sym

    @staticmethod
    def backward(ctx, g_total, g_vals, g_sym):
        gk, gb = ctx.saved_tensors
        return gk * g_total, gb * g_total, None, None


def fused_or_none(cls, *args):
    """cls(*args), or None when the criterion holds a loss outside that kernel: the registry losses then run through autograd."""
    try:
        return cls(*args)
    except NotImplementedError:
        return None


class _FusedCriterion:
    """What the fused criteria share: each wraps a `Criterion` (self.crit), leaves its kernel's outputs in self.out and reports the
    kernel's loss vector (LOSS_WIDTH floats) under the registry route's keys."""
    LOSS_WIDTH = 8           # floats of the kernel's loss vector
    _last = None             # the slots of the last call, where they depend on that call's targets

    def draw(self, dev):
        self.crit.draw(dev)

    def _set_keys(self, key_slots):
        """key_slots: key -> slot of the loss vector (None: the registry route reports None), in the registry's own update order.
        LOSS_KEYS is the vector's layout: the dict key each slot is reported under (None: not an entry of the loss dict)."""
        self.key_slots, by_slot = key_slots, {s: k for k, s in key_slots.items()}
        self.LOSS_KEYS = tuple(by_slot.get(i) for i in range(self.LOSS_WIDTH))

    def losses_dict(self):
        """Host view of the loss scalars of the last call under the keys of Criterion.compute_losses (synchronises)."""
        v = self.out["losses"].cpu()
        return {k: (None if s is None else v[s]) for k, s in (self._last or self.key_slots).items()}

    def _ordinal_args(self):
        """The ordinal-draw arguments of ab_pose_loss_sym / ab_reg_pose_loss: hand views, nvh, j0, j1, count, p0, p1, count, scene
        views, nvs, i0, i1, count (null / 0 without that loss)."""
        from . import _lib as L
        hb = self.hand.draws.bufs if self.hand is not None else {}
        sb = self.scene.draws.bufs if self.scene is not None else {}
        n = lambda b, k: L.i(b[k].numel() if b else 0)   # noqa: E731
        return (L.ptr(hb.get("views")), L.i(hb["views"].shape[0] if hb else 0), L.ptr(hb.get("j0")), L.ptr(hb.get("j1")), n(hb, "j0"),
                L.ptr(hb.get("p0")), L.ptr(hb.get("p1")), n(hb, "p0"),
                L.ptr(sb.get("views")), L.i(sb["views"].shape[0] if sb else 0), L.ptr(sb.get("i0")), L.ptr(sb.get("i1")), n(sb, "i0"))


class FusedPoseCriterion(_FusedCriterion):
    """Pose assembly + JointsLoss + HandOrdLoss + SceneOrdLoss + per-sample EPE + backward in ONE HIP kernel
    (csrc/pose_loss.hip).  Built from a `Criterion` whose loss list is [JointsLoss, HandOrdLoss, SceneOrdLoss] (any
    subset); uses that criterion's draw buffers so the RNG behaviour is the reference's."""

    def __init__(self, criterion: Criterion, inp_res, center_idx=0):
        self.crit = criterion
        self.inp_res = inp_res
        self.center_idx = center_idx
        w = [0.0] * 8
        self.hand = self.scene = self.sym = None
        self.sym_weight = 0.0
        self._sym_dev = None
        for loss in criterion.loss_list:
            lam = criterion.loss_lambdas[type(loss).__name__]
            if isinstance(loss, JointsLoss):
                w[0], w[1], w[5] = float(loss.lambda_joints_3d), float(loss.lambda_corners_3d), float(lam)
            elif isinstance(loss, HandOrdLoss):
                w[2], w[3], w[6] = loss.lambda_joint_lev, loss.lambda_part_lev, float(lam)
                self.hand = loss
            elif isinstance(loss, SceneOrdLoss):
                w[4], w[7] = loss.lambda_scene_lev, float(lam)
                self.scene = loss
            elif isinstance(loss, SymCornerLoss):
                self.sym = loss
                self.sym_weight = float(lam)
            else:
                raise NotImplementedError(f"{type(loss).__name__} is not part of the fused criterion")
        self.weights = (ctypes.c_float * 8)(*w)
        self.out = None

    def _alloc(self, B, dev):
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        self.out = dict(joints_3d_abs=z(B, 21, 3), corners_3d_abs=z(B, 8, 3), box_rot_rotmat=z(B, 3, 3),
                        uvd2d=z(B, 30, 3), sample_part=z(B, 8), losses=z(8), g_kp3d=z(B, 22, 3), g_box6d=z(B, 6),
                        sym_loss=torch.zeros(1, dtype=torch.float32, device=dev))

    def __call__(self, kp3d, box6d_buf, box_stride, targs, backward=True):
        """kp3d [B,22,3] f32; box6d_buf: f32 buffer whose rows (pitch box_stride) start with the 6-D rotation."""
        from . import _lib as L
        B, dev = kp3d.shape[0], kp3d.device
        if self.out is None or self.out["g_kp3d"].shape[0] != B:
            self._alloc(B, dev)
        o = self.out
        t = lambda k: targs[k]   # noqa: E731
        symp = None
        if self.sym is not None and self.sym.lambda_sym_corners_3d:
            if self._sym_dev is None or self._sym_dev[0].device != dev:
                self._sym_dev = (self.sym.R.to(dev).contiguous(), self.sym.t.to(dev).reshape(self.sym.t.shape[0], -1, 3).contiguous())
            Rd, td = self._sym_dev
            obj = t(Queries.OBJ_IDX)
            if obj.dtype != torch.int64:
                raise TypeError("obj_idx must be int64")
            self._sym_struct = L.SymCorner(L.addr(Rd), L.addr(td), int(Rd.shape[1]), L.addr(obj), L.addr(t(Queries.OBJ_TRANSF)),
                                           float(self.sym.lambda_sym_corners_3d), float(self.sym_weight), L.addr(o["sym_loss"]))
            symp = ctypes.byref(self._sym_struct)
        L.check(L.lib().ab_pose_loss_sym(
            L.ptr(kp3d), L.ptr(box6d_buf), L.i(box_stride), L.ptr(t(Queries.ROOT_JOINT)), L.ptr(t(Queries.CAM_INTR)),
            L.ptr(t(Queries.CORNERS_CAN)), L.ptr(t(Queries.JOINTS_3D)), L.ptr(t(Queries.CORNERS_3D)),
            L.ptr(t(Queries.JOINTS_VIS)), L.ptr(t(Queries.CORNERS_VIS)), *self._ordinal_args(),
            L.i(B), L.i(self.center_idx), L.f(self.inp_res[0]), L.f(self.inp_res[1]), self.weights, symp,
            L.ptr(o["joints_3d_abs"]), L.ptr(o["corners_3d_abs"]), L.ptr(o["box_rot_rotmat"]), L.ptr(o["uvd2d"]),
            L.ptr(o["sample_part"]), L.ptr(o["losses"]), L.ptr(o["g_kp3d"] if backward else None),
            L.ptr(o["g_box6d"] if backward else None), L.stream()), "ab_pose_loss_sym")
        return o

    LOSS_KEYS = ("joints_3d_loss", "corners_3d_loss", "joint_ord_loss", "part_ord_loss", "scene_ord_loss", "final_loss")
    key_slots = {k: i for i, k in enumerate(LOSS_KEYS)}      # (the vector's last two slots are no entries of the loss dict)

    def losses_dict(self):
        d = super().losses_dict()
        if self.sym is not None:
            d["sym_corners_3d_loss"] = self.out["sym_loss"].cpu()[0]
        return d


class FusedRegCriterion(_FusedCriterion):
    """The regression-based model's criterion in ONE HIP kernel (ab_reg_pose_loss, csrc/pose_loss.hip): HOPRegNet's assembly
    (hpregnet.mano_outputs / object_outputs: joints + the target's root, corners = R(transf[3:9]) can + root + transf[0:3]) +
    ManoLoss + JointsLoss + HandOrdLoss + SceneOrdLoss + per-sample EPE + backward down to MANO's joints, the PCA pose, the shape
    and the nine TransHead values.  Built from a `Criterion` whose list is any subset of those four containing ManoLoss; uses that
    criterion's draw buffers, so the host RNG stream is the reference's.  The hand-vertex term needs a `hand_verts_3d` target:
    a batch that carries one under a non-zero LAMBDA_HAND_VERTS_3D is refused (the registry losses then run instead)."""

    LOSS_WIDTH = 16          # floats of the kernel's loss vector

    def __init__(self, criterion: Criterion, ncomps, example_batch=None):
        self.crit = criterion
        self.ncomps = int(ncomps)
        w = [0.0] * 12
        self.mano = self.hand = self.scene = None
        # key -> slot of the loss vector (None: the registry route reports None), in the registry's own update order
        d = {}
        for loss in criterion.loss_list:
            lam = float(criterion.loss_lambdas[type(loss).__name__])
            if isinstance(loss, ManoLoss):
                if self.mano is not None:
                    raise NotImplementedError("two ManoLoss entries")
                self.mano = loss
                w[8], w[9], w[10], w[11] = loss.lambda_shape_reg, loss.lambda_pose_reg, loss.lambda_joints_3d, lam
                d.update(mano_shape=8 if loss.lambda_shape_reg else None, mano_pca_pose=9 if loss.lambda_pose_reg else None,
                         joints_3d_loss=10 if loss.lambda_joints_3d else None, hand_verts_3d_loss=None)
            elif isinstance(loss, JointsLoss):
                w[0], w[1], w[5] = float(loss.lambda_joints_3d), float(loss.lambda_corners_3d), lam
                d.update({"joints_3d_loss": 0 if loss.lambda_joints_3d else None, "corners_3d_loss": 1 if loss.lambda_corners_3d else None,
                          loss.output_key: 11})
            elif isinstance(loss, HandOrdLoss):
                w[2], w[3], w[6] = loss.lambda_joint_lev, loss.lambda_part_lev, lam
                self.hand = loss
                d.update({"joint_ord_loss": 2, "part_ord_loss": 3, loss.output_key: 12})
            elif isinstance(loss, SceneOrdLoss):
                w[4], w[7] = loss.lambda_scene_lev, lam
                self.scene = loss
                d["scene_ord_loss"] = 4
            else:
                raise NotImplementedError(f"{type(loss).__name__} is not part of the fused regbased criterion")
        if self.mano is None:
            raise NotImplementedError("the fused regbased criterion needs ManoLoss in the list")
        if self.mano.lambda_hand_verts_3d and example_batch is not None and "hand_verts_3d" in example_batch:
            raise NotImplementedError("ManoLoss's hand-vertex term (a hand_verts_3d target with LAMBDA_HAND_VERTS_3D != 0)")
        d["final_loss"] = 5
        self._set_keys(d)
        self.weights = (ctypes.c_float * 12)(*[float(x) for x in w])
        self.out = None

    def _alloc(self, B, dev):
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        self.out = dict(joints_3d_abs=z(B, 21, 3), corners_3d_abs=z(B, 8, 3), box_rot_rotmat=z(B, 3, 3), sample_part=z(B, 8),
                        losses=z(self.LOSS_WIDTH), g_joints=z(B, 21, 3), g_pose=z(B, 3 + self.ncomps), g_shape=z(B, 10), g_transf=z(B, 9))

    def __call__(self, joints_3d, mano_pca_pose, mano_shape, transf, targs, backward=True, g_transf=None):
        """joints_3d [B,21,3] (MANO's, root-relative), mano_pca_pose [B,3+ncomps], mano_shape [B,10] f32 contiguous; transf: f32 rows
        whose first nine values are translation | 6-D rotation (any row pitch >= 9).  g_transf: a buffer of transf's pitch to receive
        its gradient (default: the criterion's own [B,9] when transf is [B,9])."""
        from . import _lib as L
        if "hand_verts_3d" in targs and self.mano.lambda_hand_verts_3d:
            raise NotImplementedError("ManoLoss's hand-vertex term (a hand_verts_3d target with LAMBDA_HAND_VERTS_3D != 0)")
        B, dev = joints_3d.shape[0], joints_3d.device
        if mano_pca_pose.shape[1] != 3 + self.ncomps:
            raise ValueError(f"mano_pca_pose has {mano_pca_pose.shape[1]} columns, ncomps = {self.ncomps}")
        if self.out is None or self.out["g_joints"].shape[0] != B or self.out["g_joints"].device != dev:
            self._alloc(B, dev)
        o = self.out
        stride = transf.stride(0)
        gt = g_transf if g_transf is not None else o["g_transf"]
        if backward and (gt.stride(0) != stride or transf.stride(1) != 1 or gt.stride(1) != 1):
            raise ValueError("g_transf must have transf's row pitch")
        t = lambda k: targs[k]   # noqa: E731
        L.check(L.lib().ab_reg_pose_loss(
            L.ptr(joints_3d), L.ptr(mano_pca_pose), L.ptr(mano_shape), L.view_ptr(transf), L.i(stride),
            L.ptr(t(Queries.ROOT_JOINT)), L.ptr(t(Queries.CAM_INTR)), L.ptr(t(Queries.CORNERS_CAN)), L.ptr(t(Queries.JOINTS_3D)),
            L.ptr(t(Queries.CORNERS_3D)), L.ptr(t(Queries.JOINTS_VIS)), L.ptr(t(Queries.CORNERS_VIS)), *self._ordinal_args(),
            L.i(B), L.i(self.ncomps), self.weights,
            L.ptr(o["joints_3d_abs"]), L.ptr(o["corners_3d_abs"]), L.ptr(o["box_rot_rotmat"]), L.ptr(o["sample_part"]), L.ptr(o["losses"]),
            L.ptr(o["g_joints"] if backward else None), L.ptr(o["g_pose"] if backward else None), L.ptr(o["g_shape"] if backward else None),
            L.view_ptr(gt if backward else None), L.stream()), "ab_reg_pose_loss")
        return o


class FusedMeshCriterion(_FusedCriterion):
    """HoNet's criterion in ONE HIP kernel + a finalize pass (ab_honet_loss, csrc/honet_loss.hip): ManoLoss with all four terms -- the
    hand-vertex term included -- + ObjLoss + per-sample EPE + the gradient of final_loss wrt joints_3d_abs, hand_verts_3d_abs,
    obj_verts_3d_abs, mano_pca_pose and mano_shape.  Built from a `Criterion` whose list is [ManoLoss] or [ManoLoss, ObjLoss]; anything else
    raises NotImplementedError (the registry losses then run through autograd).  A term whose target the batch does not carry is dropped, as
    the registry classes drop it (`key in targs`); `example_batch` fixes which ones the loss record reports."""

    _SLOTS = ("mano_shape", "mano_pca_pose", "joints_3d_loss", "hand_verts_3d_loss", "obj_verts_3d_loss", "final_loss")
    _TARGET = {"joints_3d_loss": Queries.JOINTS_3D, "hand_verts_3d_loss": "hand_verts_3d", "obj_verts_3d_loss": Queries.OBJ_VERTS_3D}

    def __init__(self, criterion: Criterion, ncomps, example_batch=None):
        self.crit = criterion
        self.ncomps = int(ncomps)
        self.mano = self.obj = None
        for loss in criterion.loss_list:
            if isinstance(loss, ManoLoss) and self.mano is None and self.obj is None:
                self.mano = loss
            elif isinstance(loss, ObjLoss) and self.mano is not None and self.obj is None:
                self.obj = loss
            else:
                raise NotImplementedError(f"{type(loss).__name__} is not part of the fused mesh criterion ([ManoLoss] or [ManoLoss, ObjLoss])")
        if self.mano is None:
            raise NotImplementedError("the fused mesh criterion needs ManoLoss in the list")
        m, lam = self.mano, criterion.loss_lambdas
        self._on = {"mano_shape": bool(m.lambda_shape_reg), "mano_pca_pose": bool(m.lambda_pose_reg), "joints_3d_loss": bool(m.lambda_joints_3d),
                    "hand_verts_3d_loss": bool(m.lambda_hand_verts_3d)}
        w = [m.lambda_shape_reg, m.lambda_pose_reg, m.lambda_joints_3d, m.lambda_hand_verts_3d, 0.0, lam["ManoLoss"], 0.0]
        if self.obj is not None:
            self._on["obj_verts_3d_loss"] = bool(self.obj.lambda_obj_verts_3d)
            w[4], w[6] = self.obj.lambda_obj_verts_3d, lam["ObjLoss"]
        self.weights = (ctypes.c_float * 7)(*[float(x) for x in w])
        self._set_keys(self._slots_for(example_batch))
        self.out = None

    def _slots_for(self, targs):
        """key -> slot of the loss vector (None: the registry route reports None), in the registry's own update order."""
        d = {}
        for k, on in self._on.items():
            t = self._TARGET.get(k)
            d[k] = self._SLOTS.index(k) if on and (t is None or targs is None or t in targs) else None
        d["final_loss"] = 5
        return d

    def draw(self, dev):
        """No loss of this criterion draws random numbers; kept so that TrainStep treats every fused criterion alike."""

    def _alloc(self, B, N, dev):
        from . import _lib as L
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        self.out = dict(sample_part=z(B, 8), losses=z(self.LOSS_WIDTH), g_joints_3d_abs=z(B, 21, 3), g_hand_verts_3d_abs=z(B, 778, 3),
                        g_obj_verts_3d_abs=z(B, N, 3) if N else None, g_mano_pca_pose=z(B, 3 + self.ncomps), g_mano_shape=z(B, 10),
                        workspace=torch.empty((L.lib().ab_honet_loss_workspace(L.i(B), L.i(N)),), dtype=torch.uint8, device=dev))
        self._shape = (B, N, dev)

    def __call__(self, joints_3d_abs, hand_verts_3d_abs, obj_verts_3d_abs, corners_3d_abs, mano_pca_pose, mano_shape, targs, backward=True):
        """The model's absolute predictions (fp32, contiguous; corners_3d_abs may be None; obj_verts_3d_abs is not read without ObjLoss)
        and the batch.  -> dict: losses [8], sample_part [B,8] and, with backward, the five g_* tensors (persistent buffers)."""
        from . import _lib as L
        B, dev = joints_3d_abs.shape[0], joints_3d_abs.device
        if mano_pca_pose.shape[1] != 3 + self.ncomps:
            raise ValueError(f"mano_pca_pose has {mano_pca_pose.shape[1]} columns, ncomps = {self.ncomps}")
        if self.obj is None:
            obj_verts_3d_abs = None
        N = obj_verts_3d_abs.shape[1] if obj_verts_3d_abs is not None else 0
        if self.out is None or self._shape != (B, N, dev):
            self._alloc(B, N, dev)
        o = self.out
        self._last = self._slots_for(targs)
        t = lambda k: targs[self._TARGET[k]] if self._last[k] is not None else None   # noqa: E731
        tc = targs.get(Queries.CORNERS_3D) if corners_3d_abs is not None else None
        g = lambda k: o[k] if backward else None   # noqa: E731
        L.check(L.lib().ab_honet_loss(
            L.ptr(joints_3d_abs), L.ptr(hand_verts_3d_abs), L.ptr(obj_verts_3d_abs), L.ptr(corners_3d_abs if tc is not None else None),
            L.ptr(mano_pca_pose), L.ptr(mano_shape), L.ptr(targs[Queries.ROOT_JOINT]),
            # (the joint target also feeds the EPE: it is passed whenever the batch has it, the weight decides the loss term)
            L.ptr(targs.get(Queries.JOINTS_3D)), L.ptr(t("hand_verts_3d_loss")),
            L.ptr(t("obj_verts_3d_loss") if self.obj is not None else None), L.ptr(tc), L.i(B), L.i(N), L.i(self.ncomps), self.weights,
            L.ptr(o["sample_part"]), L.ptr(o["losses"]), L.ptr(g("g_joints_3d_abs")), L.ptr(g("g_hand_verts_3d_abs")),
            L.ptr(g("g_obj_verts_3d_abs")), L.ptr(g("g_mano_pca_pose")), L.ptr(g("g_mano_shape")), L.ptr(o["workspace"]), L.stream()),
            "ab_honet_loss")
        return o


# ---- mesh-level losses --------------------------------------------------------------------------------------------
class _ChamferRigidFn(torch.autograd.Function):
    """ab_chamfer_rigid (csrc/mesh_align.hip): ONE call in forward leaves the loss and its gradient with respect to the rotation entries and
    the translation; backward scales the kept buffers by the incoming gradient."""

    @staticmethod
    def forward(ctx, rot, tsl, can, targ, root, corners_vis):
        from . import kernels as K
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        o = K.chamfer_rigid(can, rot, tsl, targ, root, corners_vis, want_grad=want)
        ctx.shapes = (rot.shape, tsl.shape)
        if want:
            ctx.save_for_backward(o["g_rot"], o["g_tsl"])
        return o["loss"].reshape(())

    @staticmethod
    def backward(ctx, g):
        g_rot, g_tsl = ctx.saved_tensors
        return (g_rot * g).reshape(ctx.shapes[0]), (g_tsl * g).reshape(ctx.shapes[1]), None, None, None, None


class _ProcrustesLossFn(torch.autograd.Function):
    """ab_procrustes_loss (csrc/mesh_align.hip): ONE call in forward leaves the loss and its gradient with respect to the predicted joints."""

    @staticmethod
    def forward(ctx, pred, targ, root):
        from . import kernels as K
        o = K.procrustes_loss(pred, targ, root, want_grad=ctx.needs_input_grad[0])
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(o["g_pred"])
        return o["loss"].reshape(())

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None, None


def _dev_f32(t, dev):
    return t.to(device=dev, dtype=torch.float32).contiguous()


def chamfer_distance_torch(x, y):
    """Brute-force, gather-based, differentiable stand-in for chamfer_distance.ChamferDistance (the un-pinned CUDA extension of
    chamferloss.py:17): x [B,N,3], y [B,M,3] -> squared distances dist_xy [B,N], dist_yx [B,M] and the indices.  One sample at a time:
    the [N,M] distance matrix of one sample is the only large temporary."""
    dxy, dyx, ixy, iyx = [], [], [], []
    for xb, yb in zip(x, y):
        with torch.no_grad():
            d = ((xb[:, None, :] - yb[None, :, :]) ** 2).sum(-1)
            i, j = d.argmin(1), d.argmin(0)
        dxy.append(((xb - yb[i]) ** 2).sum(-1)); dyx.append(((xb[j] - yb) ** 2).sum(-1))
        ixy.append(i); iyx.append(j)
    return torch.stack(dxy), torch.stack(dyx), torch.stack(ixy), torch.stack(iyx)


@LOSS.register_module
class ChamferLoss(TensorLoss):
    """anakin/criterions/chamferloss.py:11-52.  The predicted cloud is R_pred can + boxroot, the target obj_verts_3d + root_joint (the
    reference's padded [B,N,3] batch, datasets.ho_collate); both are multiplied by any(corners_vis) and compared by the two-way squared
    nearest-neighbour distance.  CPU tensors: torch ops over chamfer_distance_torch.  HIP tensors: ab_chamfer_rigid (csrc/mesh_align.hip),
    loss and rigid gradient in one call; the eager route only (TrainStep refuses to capture a step that holds this loss)."""

    def __init__(self, **cfg):
        super().__init__()
        self.lambda_chamfer = cfg.get("LAMBDA_CHAMFER", 0.0)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        chamfer_loss = None
        if self.lambda_chamfer:
            dev = final_loss.device
            rot, tsl = preds["box_rot_rotmat"], preds["boxroot_3d_abs"]
            if dev.type == "cuda":      # one ab_chamfer_rigid call; the mask is formed in the kernel (eager only)
                t = lambda k: _dev_f32(targs[k], dev)   # noqa: E731
                chamfer_loss = _ChamferRigidFn.apply(_dev_f32(rot, dev), _dev_f32(tsl, dev), t(Queries.OBJ_VERTS_CAN), t(Queries.OBJ_VERTS_3D),
                                                     t(Queries.ROOT_JOINT), t(Queries.CORNERS_VIS))
            else:
                chamfer_loss = self.torch_expression(rot, tsl, targs, dev)
            final_loss = final_loss + self.lambda_chamfer * chamfer_loss
        losses["chamfer_loss"] = chamfer_loss
        losses[self.output_key] = final_loss
        return final_loss, losses

    @staticmethod
    def torch_expression(rot, tsl, targs, dev):
        """The route of CPU tensors: the reference's torch ops (tools/bench_mesh_losses.py times the same expression on device tensors)."""
        keep = torch.any(targs[Queries.CORNERS_VIS].to(dev) != 0, dim=1).to(rot.dtype)
        can = targs[Queries.OBJ_VERTS_CAN].to(dev)
        v3d, root = targs[Queries.OBJ_VERTS_3D].to(dev), targs[Queries.ROOT_JOINT].to(dev)
        pred = torch.matmul(rot, can.permute(0, 2, 1)).permute(0, 2, 1) + tsl
        pred = torch.einsum("bij,b->bij", pred, keep)
        targ = torch.einsum("bij,b->bij", v3d + root.unsqueeze(1), keep)
        dist_xy, dist_yx, _, _ = chamfer_distance_torch(pred, targ)
        return torch.mean(dist_xy) + torch.mean(dist_yx)


@LOSS.register_module
class AlignLoss(TensorLoss):
    """anakin/criterions/alignloss.py:12-80.  CPU tensors: the reference's torch ops (batched torch.svd under autograd).  HIP tensors:
    ab_procrustes_loss (csrc/mesh_align.hip), one wave per sample, analytic backward; the eager route only, as for ChamferLoss."""

    def __init__(self, **cfg):
        super().__init__()
        self.lambda_procrustes_align = cfg.get("LAMBDA_PROCRUSTES_ALIGN", 1.0)
        self.lambda_st_align = cfg.get("LAMBDA_ST_ALIGN", 0.0)

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        dev = final_loss.device
        pred = preds["joints_3d_abs"]
        loss = None
        if self.lambda_procrustes_align:
            if dev.type == "cuda":      # one ab_procrustes_loss call, analytic backward (eager only)
                loss = _ProcrustesLossFn.apply(_dev_f32(pred, dev), _dev_f32(targs[Queries.JOINTS_3D], dev), _dev_f32(targs[Queries.ROOT_JOINT], dev))
            else:
                xyz = (targs[Queries.JOINTS_3D] + targs[Queries.ROOT_JOINT].unsqueeze(1)).to(dev)
                loss = F.mse_loss(self.procrustes_align(xyz, pred), xyz)
            final_loss = final_loss + self.lambda_procrustes_align * loss
        losses["procrustes_aligned_loss"] = loss
        if self.lambda_st_align:
            raise NotImplementedError()
        losses["st_aligned_loss"] = None
        losses[self.output_key] = final_loss
        return final_loss, losses

    @staticmethod
    def torch_orthogonal_procrustes(A, B):
        u, w, v = torch.svd(B.transpose(1, 2).bmm(A).transpose(1, 2))
        R = u.bmm(v.transpose(1, 2))
        scale = w.sum(dim=1, keepdim=True).unsqueeze(-1)
        return R, scale

    @staticmethod
    def procrustes_align(xyz, pred_xyz):
        tsl = xyz.mean(1, keepdim=True)
        pred_tsl = pred_xyz.mean(1, keepdim=True)
        xyz_tsl = xyz - tsl
        pred_xyz_tsl = pred_xyz - pred_tsl
        scale = torch.norm(xyz_tsl, dim=(1, 2), keepdim=True) + 1e-8
        xyz_tsl_scale = xyz_tsl / scale
        pred_scale = torch.norm(pred_xyz_tsl, dim=(1, 2), keepdim=True) + 1e-8
        pred_xyz_tsl_scale = pred_xyz_tsl / pred_scale
        R, s = AlignLoss.torch_orthogonal_procrustes(xyz_tsl_scale, pred_xyz_tsl_scale)
        return torch.bmm(pred_xyz_tsl_scale, R.transpose(1, 2)) * s * scale + tsl


@LOSS.register_module
class ObjLoss(TensorLoss):
    """anakin/criterions/honetloss.py:76-97: MSE on the posed object vertices.  Torch ops only: it reads preds["obj_verts_3d_abs"], which
    HoNet produces (honet.HoNet / regnet.HoNetHIP)."""

    def __init__(self, **cfg):
        super().__init__()
        self.lambda_obj_verts_3d = cfg["LAMBDA_OBJ_VERTS_3D"]

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        loss = None
        if self.lambda_obj_verts_3d and Queries.OBJ_VERTS_3D in targs:
            p = preds["obj_verts_3d_abs"]
            loss = F.mse_loss(p, targs[Queries.OBJ_VERTS_3D].to(p.device) + targs[Queries.ROOT_JOINT].to(p.device).unsqueeze(1))
            final_loss = final_loss + self.lambda_obj_verts_3d * loss
        losses["obj_verts_3d_loss"] = loss
        return final_loss, losses


# ---- contact loss: hand-object repulsion and attraction ------------------------------------------------------------------
def contact_loss_torch(hand_verts, zone_id, n_zones, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_box, obj_row, rot, tsl, mask=None,
                       rho=0.02, alpha=0.01, lambda_r=0.5, lambda_a=0.5, flags=0, want_grad=False, want_sdf=False, want_diag=False, medial=None):
    """The definitions of ab_contact_loss (include/artiboost_hip.h) as torch ops in hand_verts' dtype: the route of CPU tensors, in float64
    the reference of the tests, and what tools/bench_contact_loss.py times on device tensors.  Same arguments and the same dict as
    kernels.contact_loss (`flags` is accepted and changes nothing: AB_CL_SCAN_ALL does not change a value).  `loss` [1] is differentiable by
    autograd with respect to hand_verts, rot and tsl: the closest point cp' is found without a graph (the region form's v, w as computed,
    the minimum over faces through gather, one [Q,F] block per sample: metrics._triangle_scan) and held fixed, and the distance is
    stated again as d = |q - (R cp' + t)|.  want_grad: also g_hand, g_rot, g_tsl by the closed form of the header (no autograd).
    want_diag (this route only): `diag` = {wind [B,Nh] (o w, NaN where it was not computed), inside bool [B,Nh], d [B,Nh] (NaN: no
    candidate), winner int64 [B,max(Z,1)] (-1: none), box_margin [B,Nh] (distance of q' to the nearest face plane of the box) and, with
    medial = (tol_d, tol_cp), medial bool [B,Nh]}."""
    from .metrics import _triangle_scan
    hv = hand_verts
    dt, dev = hv.dtype, hv.device
    B, Nh, Z = hv.shape[0], hv.shape[1], int(n_zones)
    n_obj = int(obj_orient.numel())
    R_all, t_all = rot.to(device=dev, dtype=dt).reshape(B, 3, 3), tsl.to(device=dev, dtype=dt).reshape(B, 3)
    vo, fo = [int(x) for x in vert_off.cpu()], [int(x) for x in face_off.cpu()]
    rows, orient = [int(r) for r in obj_row.cpu()], [float(x) for x in obj_orient.cpu()]
    keep = [1.0] * B if mask is None else [float(x) for x in mask.cpu()]
    zone = torch.full((Nh,), -1, dtype=torch.int64, device=dev)
    if Z:
        zi = zone_id.to(dev).long().reshape(Nh)
        zone = torch.where((zi >= 0) & (zi < Z), zi, zone)
    zero = torch.zeros((), dtype=dt, device=dev)
    nan = float("nan")
    rep, att = [], []
    out = {"counts": torch.zeros((B, 2), dtype=torch.int32, device=dev)}
    if want_sdf:
        out["sdf"] = torch.full((B, Nh), nan, dtype=dt, device=dev)
    if want_grad:
        out["g_hand"], out["g_rot"], out["g_tsl"] = hv.new_zeros((B, Nh, 3)), hv.new_zeros((B, 3, 3)), hv.new_zeros((B, 3))
    if want_diag:
        out["diag"] = diag = {"wind": torch.full((B, Nh), nan, dtype=dt, device=dev), "inside": torch.zeros((B, Nh), dtype=torch.bool, device=dev),
                              "d": torch.full((B, Nh), nan, dtype=dt, device=dev), "winner": torch.full((B, max(Z, 1)), -1, dtype=torch.int64, device=dev),
                              "box_margin": torch.full((B, Nh), nan, dtype=dt, device=dev), "medial": torch.zeros((B, Nh), dtype=torch.bool, device=dev)}
    w_rep, w_att = lambda_r / (B * Nh), lambda_a / (B * max(Z, 1))
    for b in range(B):
        r = rows[b]
        if not 0 <= r < n_obj or keep[b] == 0.0:         # m_b = 0: nothing of the sample is scanned
            rep.append(zero); att.append(zero)
            continue
        can = obj_verts[vo[r]:vo[r + 1]].to(device=dev, dtype=dt)
        tri = can[obj_faces[fo[r]:fo[r + 1]].to(dev).long().reshape(-1, 3)]
        R, t, q = R_all[b], t_all[b], hv[b]
        with torch.no_grad():
            qc = (q - t) @ R                                                       # q' = R^T (q - t)
            box = obj_box.reshape(-1, 6)[r].to(device=dev, dtype=dt)
            inbox = ((qc >= box[:3]) & (qc <= box[3:])).all(1)
            idx = (inbox | (zone >= 0)).nonzero()[:, 0]                            # the candidates, ascending
            if want_diag:
                diag["box_margin"][b] = torch.minimum((qc - box[:3]).abs(), (qc - box[3:]).abs()).min(1)[0]
        out["counts"][b, 1] = idx.numel()
        if idx.numel() == 0:
            rep.append(zero); att.append(zero)
            continue
        with torch.no_grad():
            w, d2, cp = _triangle_scan(qc[idx], tri, True, want_cp=True, medial=medial)
            ow = orient[r] * w
            ins = inbox[idx] & (ow > 0.5)
            ds = d2.sqrt()
            cpc = qc[idx] + cp["r"]                                                # cp' = q' - r', r' = -(cp - q')
        diff = q[idx] - (cpc @ R.T + t)                                           # cp' is held fixed: d = |q - (R cp' + t)|
        s2 = (diff * diff).sum(-1)
        nz = s2 > 0
        d = torch.where(nz, torch.where(nz, s2, torch.ones_like(s2)).sqrt(), torch.zeros_like(s2))
        rep.append((rho * torch.tanh(d / rho))[ins].sum() / Nh)
        a, zc, winners = zero, zone[idx], []
        for z in range(Z):
            sel = ((zc == z) & ~ins).nonzero()[:, 0]
            if sel.numel():
                j = sel[ds[sel].min(0)[1]]                                         # the smallest d, the lowest index among equals
                a = a + alpha * torch.tanh(d[j] / alpha)
                winners.append(int(j))
                if want_diag:
                    diag["winner"][b, z] = idx[j]
        att.append(a / max(Z, 1))
        out["counts"][b, 0] = ins.sum().to(torch.int32)
        if want_sdf:
            out["sdf"][b, idx] = torch.where(ins, -d, d).detach()
        if want_diag:
            diag["wind"][b, idx] = torch.where(inbox[idx], ow, torch.full_like(ow, nan))
            diag["inside"][b, idx], diag["d"][b, idx] = ins, ds
            if medial is not None:
                diag["medial"][b, idx] = cp["medial"]
        if want_grad:
            with torch.no_grad():
                wgt, scale = torch.where(ins, torch.full_like(ds, w_rep), torch.zeros_like(ds)), torch.full_like(ds, rho)
                for j in winners:
                    wgt[j], scale[j] = w_att, alpha
                safe = torch.where(ds > 0, ds, torch.ones_like(ds))
                c = torch.where(ds > 0, wgt / torch.cosh(ds / scale) ** 2 / safe, torch.zeros_like(ds))
                g = c[:, None] * ((-cp["r"]) @ R.T)                                # weight s n, n = R r' / d
                out["g_hand"][b, idx] = g
                out["g_tsl"][b] = -g.sum(0)
                out["g_rot"][b] = -(g[:, :, None] * cpc[:, None, :]).sum(0)
    out["rep"], out["att"] = torch.stack(rep), torch.stack(att)
    out["loss"] = ((lambda_r * out["rep"].sum() + lambda_a * out["att"].sum()) / B).reshape(1)
    return out


class _ContactLossFn(torch.autograd.Function):
    """ab_contact_loss (csrc/contact_loss.hip): ONE call in forward leaves the loss and its gradient with respect to the hand vertices, the
    rotation entries and the translation; backward scales the kept buffers by the incoming gradient."""

    @staticmethod
    def forward(ctx, hand, rot, tsl, args, kw):
        from . import kernels as K
        want = any(ctx.needs_input_grad[:3])
        o = K.contact_loss(hand, args[0], args[1], *args[2:], rot, tsl, want_grad=want, **kw)
        ctx.shapes = (hand.shape, rot.shape, tsl.shape)
        if want:
            ctx.save_for_backward(o["g_hand"], o["g_rot"], o["g_tsl"])
        rep, att = o["rep"].mean(), o["att"].mean()
        ctx.mark_non_differentiable(rep, att)
        return o["loss"].reshape(()), rep, att

    @staticmethod
    def backward(ctx, g, g_rep, g_att):
        return tuple((t * g).reshape(s) for t, s in zip(ctx.saved_tensors, ctx.shapes)) + (None, None)


def tip_zones(v_template, tips, radius):
    """zone_id int32 [Nh]: zone z holds the rest-template vertices within `radius` of vertex tips[z]; a vertex in two spheres goes to the
    lower zone; -1 elsewhere."""
    v = np.asarray(v_template, np.float64)
    zone = np.full(len(v), -1, np.int32)
    for z in reversed(range(len(tips))):
        zone[np.linalg.norm(v - v[tips[z]], axis=1) <= radius] = z
    return zone


@LOSS.register_module
class ContactLoss(TensorLoss):
    """The contact loss of Hasson et al. (CVPR 2019) between the predicted hand mesh and the posed object mesh:
    repulsion of the hand vertices inside the object, rho tanh(d / rho) with rho = REPULSE_MM, and attraction of the contact zones that do
    not touch it, alpha tanh(d_z / alpha) with alpha = ATTRACT_MM.  The hand is preds[HAND_KEY]; the object is its canonical mesh
    (OBJ_MESHES, the block of InteractionMetric, or `set_obj_meshes(table)`) chosen by targs[obj_idx] under preds[ROT_KEY] / preds[TSL_KEY]
    (OBJ_POSE: pred) or under targs[obj_transf], which gets no gradient (OBJ_POSE: gt).  ZONES: `tips` (one zone per fingertip vertex
    745, 317, 444, 556, 673 -- anakin/models/mano.py:26-30 -- holding the rest-template vertices within ZONE_RADIUS_MM of it), a list of
    vertex index lists, or [].  MANO_ASSETS_ROOT (assets/mano_v1_2) names the hand model whose rest template the tip zones are cut from;
    SCAN_ALL: true passes AB_CL_SCAN_ALL (every vertex scanned; the same bits).  A sample whose object the table lacks contributes 0 and
    counts in the batch.  HIP tensors: ONE
    ab_contact_loss call, loss and gradients; the eager route only (TrainStep refuses to capture a step that holds this loss).  CPU tensors:
    contact_loss_torch in their dtype."""
    TIPS = (745, 317, 444, 556, 673)

    def __init__(self, **cfg):
        super().__init__()
        self.lambda_repulsion, self.lambda_attraction = float(cfg.get("LAMBDA_REPULSION", 0.5)), float(cfg.get("LAMBDA_ATTRACTION", 0.5))
        self.rho, self.alpha = float(cfg.get("REPULSE_MM", 20)) / 1000.0, float(cfg.get("ATTRACT_MM", 10)) / 1000.0
        self.zone_radius = float(cfg.get("ZONE_RADIUS_MM", 10)) / 1000.0
        if not (self.rho > 0 and self.alpha > 0 and self.zone_radius >= 0):
            raise ValueError("ContactLoss: REPULSE_MM > 0, ATTRACT_MM > 0 and ZONE_RADIUS_MM >= 0")
        self.hand_key = cfg.get("HAND_KEY", "hand_verts_3d_abs")
        self.rot_key, self.tsl_key = cfg.get("ROT_KEY", "box_rot_rotmat"), cfg.get("TSL_KEY", "boxroot_3d_abs")
        self.obj_pose = str(cfg.get("OBJ_POSE", "pred"))
        if self.obj_pose not in ("pred", "gt"):
            raise ValueError(f"ContactLoss: OBJ_POSE must be 'pred' or 'gt', got {self.obj_pose!r}")
        self.zones = cfg.get("ZONES", "tips")
        if not (self.zones == "tips" or (isinstance(self.zones, (list, tuple)) and len(self.zones) <= 16 and
                                          all(isinstance(z, (list, tuple)) for z in self.zones))):
            raise ValueError("ContactLoss: ZONES must be 'tips' or a list of at most 16 vertex index lists")
        self.mano_assets_root = cfg.get("MANO_ASSETS_ROOT", "assets/mano_v1_2")
        self.scan_all = bool(cfg.get("SCAN_ALL", False))
        self.table = None
        src = cfg.get("OBJ_MESHES")
        if src:
            if str(src.get("SOURCE", "assets")) != "assets":
                raise ValueError(f"ContactLoss: OBJ_MESHES.SOURCE must be 'assets' (or call set_obj_meshes), got {src.get('SOURCE')!r}")
            from .assets import SceneAssets
            from .metrics import ObjectMeshTable
            self.table = ObjectMeshTable.from_assets(SceneAssets(src.get("DATASET", "HO3D"), seed=1))
        self._zone = {}

    def set_obj_meshes(self, table):
        if table.hand_faces is None:
            from .hpregnet import load_hand_model
            table.set_hand(load_hand_model(self.mano_assets_root))
        self.table = table
        return self

    def zone_ids(self, Nh):
        """(zone_id int32 [Nh] numpy, Z) of the configured zones for a hand of Nh vertices."""
        if Nh not in self._zone:
            if self.zones == "tips":
                from .hpregnet import load_hand_model
                v = np.asarray(load_hand_model(self.mano_assets_root)["v_template"])
                if len(v) != Nh:
                    raise ValueError(f"ContactLoss: ZONES 'tips' needs the hand model's {len(v)} vertices, got {Nh}")
                self._zone[Nh] = (tip_zones(v, self.TIPS, self.zone_radius), len(self.TIPS))
            else:
                zone = np.full(Nh, -1, np.int32)
                for z in reversed(range(len(self.zones))):
                    ids = np.asarray(self.zones[z], np.int64).reshape(-1)
                    if ids.size and (ids.min() < 0 or ids.max() >= Nh):
                        raise ValueError(f"ContactLoss: zone {z} holds a vertex index outside [0, {Nh})")
                    zone[ids] = z                                                  # a vertex in two zones goes to the lower one
                self._zone[Nh] = (zone, len(self.zones))
        return self._zone[Nh]

    def _zone_on(self, Nh, dev):
        key = (Nh, str(dev))
        if key not in self._zone:
            zone, Z = self.zone_ids(Nh)
            self._zone[key] = (torch.from_numpy(zone).to(dev), Z)
        return self._zone[key]

    def __call__(self, preds, targs, **kwargs):
        final_loss, losses = super().__call__(preds, targs, **kwargs)
        contact = rep = att = None
        if self.lambda_repulsion or self.lambda_attraction:
            if self.table is None:
                raise RuntimeError("ContactLoss: no object meshes (OBJ_MESHES in the config, or set_obj_meshes)")
            if targs.get(Queries.OBJ_IDX) is None:
                raise KeyError(Queries.OBJ_IDX)
            for k in (self.hand_key,) + ((self.rot_key, self.tsl_key) if self.obj_pose == "pred" else ()):
                if preds.get(k) is None:
                    raise KeyError(k)
            hand = preds[self.hand_key]
            dev, B, Nh = hand.device, hand.shape[0], hand.shape[1]
            if self.obj_pose == "pred":
                rot, tsl = preds[self.rot_key], preds[self.tsl_key]
            else:
                if targs.get(Queries.OBJ_TRANSF) is None:
                    raise KeyError(Queries.OBJ_TRANSF)
                T = targs[Queries.OBJ_TRANSF].detach().to(dev)
                rot, tsl = T[:, :3, :3], T[:, :3, 3]
            tb = self.table.on(dev)
            zone, Z = self._zone_on(Nh, dev)
            args = (zone if Z else None, Z, tb["obj_verts"], tb["obj_faces"], tb["vert_off"], tb["face_off"], tb["obj_orient"], tb["obj_box"],
                    self.table.rows(targs[Queries.OBJ_IDX].to(dev)))
            kw = dict(rho=self.rho, alpha=self.alpha, lambda_r=self.lambda_repulsion, lambda_a=self.lambda_attraction)
            if dev.type == "cuda":      # one ab_contact_loss call, analytic backward (eager only)
                from . import kernels as K
                kw["flags"] = K.CL_SCAN_ALL if self.scan_all else 0
                contact, rep, att = _ContactLossFn.apply(_dev_f32(hand, dev), _dev_f32(rot, dev).reshape(B, 3, 3), _dev_f32(tsl, dev).reshape(B, 3), args, kw)
            else:
                o = contact_loss_torch(hand, args[0], args[1], *args[2:], rot.to(hand.dtype).reshape(B, 3, 3), tsl.to(hand.dtype).reshape(B, 3), **kw)
                contact, rep, att = o["loss"].reshape(()), o["rep"].detach().mean(), o["att"].detach().mean()
            final_loss = final_loss + contact
        losses["contact_loss"] = contact
        losses["repulsion_loss"] = rep if self.lambda_repulsion else None
        losses["attraction_loss"] = att if self.lambda_attraction else None
        losses[self.output_key] = final_loss
        return final_loss, losses
