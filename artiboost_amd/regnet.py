"""HOPRegNet (anakin/models/hpregnet.py:18-150, anakin/models/mano.py:46-137) on the HIP kernels: the regression-based model trained and
evaluated on the device.  `hpregnet.HOPRegNet(**cfg)` builds this class when cfg["DEVICE"] names a HIP device (train_artiboost.py passes
it; the GPU eval config sets ARCH.DEVICE) and the torch module otherwise.

  trunk     ResNet-18/34 of hybridnet.HybridNet in its trunk-only layout (ParamStore(reg_heads=ncomps)): the same conv / BatchNorm
            kernels, precisions and explicit backward as HybridBaseline, returning res_layer4_mean [N, 512]
  heads     ManoBranch's MLP (512 -> 512 -> 512, ReLU) -> pose_reg (3 + ncomps) / shape_reg (10), and TransHead (512 -> 256, ReLU -> 9):
            the exact-fp32 linear kernels (ab_linear_fwd / _dgrad / _wgrad) on weights in the same flat buffer, outputs padded with zero
            rows to multiples of ParamStore.REG_PAD
  MANO      ab_mano_pca_fwd / ab_mano_pca_bwd (PCA pose + shape -> centred verts / joints and the exact reverse)

Autograd boundary: ONE torch.autograd.Function (_RegBridge, as models._NetBridge) with inputs (flat_param, image / padded image) and
outputs (mano_pca_pose, mano_shape, hand_verts_3d, joints_3d, mano_full_pose, transf [N, 9]); its backward runs MANO bwd -> head bwd ->
trunk bwd, writes store.grad and hands it to flat_param.grad.  The camera projections and the 6-D rotation of the object stay torch ops
on those outputs (hpregnet.mano_outputs / object_outputs), so the model returns the CPU module's 18 keys and the registry losses and
metrics run unchanged.

HoNetHIP (below) is HoNet (anakin/models/honetMANO.py) on the same trunk, ManoBranch heads and MANO kernels; its camera-frame stage is
one kernel pair (ab_honet_recover_fwd / _bwd) inside its bridge instead of torch ops outside it."""
import os
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
from .honet import HoNet
from .hpregnet import HOPRegNet, combine_outputs, load_hand_model, mano_outputs, object_outputs
from .hybridnet import HybridNet, ParamStore
from .models import BACKBONES, HybridBaseline
from .registry import RUNTIME, Queries, enable_lower_param

HEADS = ("mano_branch.base_layer.0", "mano_branch.base_layer.2", "mano_branch.pose_reg", "mano_branch.shape_reg.0",
         "obj_transfhead.decoder.0", "obj_transfhead.final_layer")


class _RegBridge(torch.autograd.Function):
    """forward: HIP trunk + heads + MANO; backward: MANO bwd -> heads bwd -> trunk bwd into the flat gradient."""

    @staticmethod
    def forward(ctx, flat_param, owner, image, xpad):
        out = owner._run(image, xpad, save=True)
        ctx.owner = owner
        return out

    @staticmethod
    def backward(ctx, g_pose, g_shape, g_verts, g_joints, g_full, g_transf):
        owner = ctx.owner
        owner._backward(g_pose, g_shape, g_verts, g_joints, g_full, g_transf)
        owner.flat_param.grad = owner.store.grad      # the kernels wrote it; no copy, no accumulation
        return None, None, None, None


class HOPRegNetHIP(nn.Module):
    HAS_BOX_HEAD = False             # (TrainStep: no MLP_O box head -- the fused pose/loss kernel is HybridBaseline's assembly)
    CHECKPOINT_NAME = "HOPRegNet"    # checkpoint files are interchangeable with the torch module's
    TORCH_MODULE = HOPRegNet         # the registry's torch module of the same model: its checkpoint cleaning
    REG_MODEL = "HOPRegNet"          # ParamStore(reg_model=...): which head set follows the trunk in the flat buffer

    @enable_lower_param
    def __init__(self, **cfg):
        super().__init__()
        preset = cfg["DATA_PRESET"]
        self.inp_res = preset["IMAGE_SIZE"]
        self.center_idx = preset["CENTER_IDX"]
        if cfg.get("MANO_FHB_ADAPTOR", False):
            raise NotImplementedError("MANO_FHB_ADAPTOR (FPHAB skeleton adaptor, hpregnet.py:41-49)")
        bb, head = cfg["BACKBONE"], cfg["HEAD"]
        if head.get("TYPE", "ManoBranch") != "ManoBranch":
            raise NotImplementedError(f"HOPRegNet head {head.get('TYPE')}: ManoBranch only")
        if not head["USE_PCA"]:
            raise NotImplementedError("ManoBranch with USE_PCA: false (16 x 9 rotation-matrix regression, mano.py:76-79,90-96)")
        if not head.get("USE_SHAPE", True):
            raise NotImplementedError("ManoBranch with USE_SHAPE: false on the HIP model")
        if BACKBONES.get(bb["TYPE"], (None,))[0] != "basic":
            raise NotImplementedError(f"backbone {bb['TYPE']}: ResNet18 / ResNet34 (the registered HOPRegNet backbones)")
        if head["INPUT_DIM"] != 512:
            raise NotImplementedError("ManoBranch INPUT_DIM: 512 (res_layer4_mean of ResNet-18/34)")
        if bb.get("PRETRAINED") is True:
            import warnings
            warnings.warn("BACKBONE.PRETRAINED: true -- ImageNet weights are a torchvision download and are not fetched; "
                          "pass a converted checkpoint through ARCH.PRETRAINED")
        self.ncomps = int(head["NCOMPS"])
        self.P = 3 + self.ncomps
        # ARCH.FUSED_STEP: true -- TrainStep runs this model without autograd (criterions.FusedRegCriterion) and replays the step as hipGraphs
        self.FUSED_STEP = bool(cfg.get("FUSED_STEP", False))
        self._read_cfg(cfg)
        dev = cfg.get("DEVICE", "cuda")
        cd = cfg.get("COMPUTE_DTYPE", "bf16x3")
        self.store = ParamStore(device=dev, layers=BACKBONES[bb["TYPE"]][1], reg_heads=self.ncomps, reg_model=self.REG_MODEL)
        self.store.init_reference_like(seed=int(cfg.get("INIT_SEED", 1)))
        self.net = HybridNet(self.store, image_size=self.inp_res,
                             compute_dtype=(torch.bfloat16 if cd in ("bf16", torch.bfloat16) else
                                            "bf16x3" if cd in ("bf16x3", "x3") else torch.float32))
        self.net.frozen_bn = self.store.frozen_bn = bool(bb.get("FREEZE_BATCHNORM", False))
        RUNTIME["loader_compute_dtype"] = ("u8n" if self.net.x3 and os.environ.get("AB_IMAGE_PLANE", "u8n") == "u8n" else self.net.dtype)
        self.flat_param = nn.Parameter(self.store.flat, requires_grad=True)   # shares storage with the store
        self.flat_param._ab_owner = self                                      # netutils.build_optimizer recognises it
        # MANO tables: the same assets as the torch module (hpregnet.ManoLayerTorch with flat_hand_mean=False)
        hm = load_hand_model(head.get("MANO_ASSETS_ROOT"))
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.store.device)      # noqa: E731
        comps = hm.get("hands_components")
        comps = np.eye(45, dtype=np.float32) if comps is None else np.asarray(comps, np.float32)
        self.mano = {k: f(hm[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")}
        self.mano["comps"] = f(comps[:self.ncomps])
        self.faces = torch.from_numpy(np.asarray(hm["faces"], np.int64))
        self._saved = None
        pretrained = cfg.get("PRETRAINED", "")
        if pretrained:
            if not os.path.isfile(pretrained):
                raise FileNotFoundError(f"=> No {self.CHECKPOINT_NAME} checkpoints file found in {pretrained}")
            ck = torch.load(pretrained, map_location="cpu")
            self.load_state_dict(ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck, strict=True)

    def _read_cfg(self, cfg):
        """Subclass hook, called before the store is built: the model's own config keys and refusals."""

    # --- checkpoints in the reference layout (the torch module's keys: base_net.*, mano_branch.*, obj_transfhead.*)
    def state_dict(self, *a, **k):
        return OrderedDict((k_, v.cpu()) for k_, v in self.store.reference_state_dict().items())

    def load_state_dict(self, sd, strict=True):
        sd = self.TORCH_MODULE.clean_reference_state_dict(sd)
        if strict:
            expected = set(self.store.reference_state_dict().keys())
            unexpected = sorted(set(sd) - expected)
            if unexpected:
                raise KeyError(f"unexpected keys: {unexpected[:5]}... ({len(unexpected)})")
        self.store.load_reference_state_dict(sd, strict=strict)
        self.net._packed = False

    def train(self, mode=True):
        super().train(mode)
        self.net.training = mode
        return self

    def params_updated(self):
        self.net._packed = False

    _plane_of = HybridBaseline._plane_of

    def _replicate_for_data_parallel(self):
        raise RuntimeError(f"{self.CHECKPOINT_NAME} (HIP) cannot be replicated by nn.DataParallel: its parameters live in one device's flat buffer; "
                           "restrict DataParallel to one device (--gpu_id 0 / CUDA_VISIBLE_DEVICES=0)")

    # --- the device computation
    def _w(self, name):
        e = self.store.entries[name + ".weight"]
        return self.store.view(name + ".weight").view(e.kshape[0], -1)

    def _lin(self, x, name, relu=False):
        return K.linear_fwd(x, self._w(name), self.store.view(name + ".bias"), relu=relu)

    def _mano_heads(self, fmean):
        """ManoBranch's heads on res_layer4_mean: -> (h1, h2, mano_pca_pose [N,3+ncomps], mano_shape [N,10])."""
        h1 = self._lin(fmean, HEADS[0], relu=True)
        h2 = self._lin(h1, HEADS[1], relu=True)
        pose = self._lin(h2, HEADS[2])[:, :self.P].contiguous()
        shape = self._lin(h2, HEADS[3])[:, :10].contiguous()
        return h1, h2, pose, shape

    def _run(self, image, xpad, save):
        """-> (mano_pca_pose [N,3+ncomps], mano_shape [N,10], hand_verts_3d [N,778,3], joints_3d [N,21,3], mano_full_pose [N,48], transf [N,9])."""
        fmean = self.net.forward(image=image, xpad=xpad)                    # res_layer4_mean [N, 512] f32
        h1, h2, pose, shape = self._mano_heads(fmean)
        d1 = self._lin(fmean, HEADS[4], relu=True)
        transf = self._lin(d1, HEADS[5])[:, :9].contiguous()
        verts, joints, full = K.mano_pca_fwd(pose, shape, self.mano, self.center_idx)
        self._saved = dict(fmean=fmean, h1=h1, h2=h2, d1=d1, pose=pose, shape=shape) if save else None
        return pose, shape, verts, joints, full, transf

    def _padded(self, name, N, *parts):
        """[N, padded width] zero-filled gradient of a head's output: the sum of the given [N, w] gradients (None: no contribution)
        in its first columns; the padding columns stay zero, so the padding rows of the weights receive zero gradient."""
        g = torch.zeros((N, self.store.entries[name + ".bias"].kshape[0]), dtype=torch.float32, device=self.store.device)
        for t in parts:
            if t is not None:
                g[:, :t.shape[1]] += t
        return g

    def _hand_branch_backward(self, S, g_pose, g_shape, g_verts, g_joints, g_full):
        """MANO bwd -> pose_reg / shape_reg -> ManoBranch's MLP: writes their weight gradients, -> the gradient wrt base_layer.0's
        output (h1), whose data gradient the caller adds to the other branches' at res_layer4_mean."""
        p, dev = self.store, self.store.device
        N = S["fmean"].shape[0]
        c = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
        gvt = c(g_verts) if g_verts is not None else torch.zeros((N, 778, 3), dtype=torch.float32, device=dev)
        gjt = c(g_joints) if g_joints is not None else torch.zeros((N, 21, 3), dtype=torch.float32, device=dev)
        g_pc, g_b = K.mano_pca_bwd(S["pose"], S["shape"], self.mano, gvt, gjt, c(g_full), self.center_idx)
        gp = self._padded(HEADS[2], N, g_pc, c(g_pose))
        gs = self._padded(HEADS[3], N, g_b, c(g_shape))
        gv, gb, wt = self._gv, self._gb, self._wt
        # pose_reg and shape_reg share their input (h2); its gradient is the sum of theirs, pose first
        K.linear_wgrad(gp, S["h2"], gv(HEADS[2]), gb(HEADS[2]))
        K.linear_wgrad(gs, S["h2"], gv(HEADS[3]), gb(HEADS[3]))
        gh2 = K.linear_dgrad(gp, wt(HEADS[2]), act_out=S["h2"]) + K.linear_dgrad(gs, wt(HEADS[3]), act_out=S["h2"])
        K.linear_wgrad(gh2, S["h1"], gv(HEADS[1]), gb(HEADS[1]))
        gh1 = K.linear_dgrad(gh2, wt(HEADS[1]), act_out=S["h1"])
        K.linear_wgrad(gh1, S["fmean"], gv(HEADS[0]), gb(HEADS[0]))
        return gh1

    def _gv(self, n):
        return self.store.gview(n + ".weight").view(self.store.entries[n + ".weight"].kshape[0], -1)

    def _gb(self, n):
        return self.store.gview(n + ".bias")

    def _wt(self, n):
        return self.net.box_t[n + ".weight"]      # ([in][out] copies)

    def _transhead_backward(self, S, g, dec, fin, act):
        """TransHead (decoder.0 + ReLU + final_layer) from g, the padded gradient of its output: writes the weight gradients, -> the
        gradient wrt decoder.0's output."""
        K.linear_wgrad(g, S[act], self._gv(fin), self._gb(fin))
        gd = K.linear_dgrad(g, self._wt(fin), act_out=S[act])
        K.linear_wgrad(gd, S["fmean"], self._gv(dec), self._gb(dec))
        return gd

    def _take_saved(self):
        """The activations of the last grad-mode forward, handed over once."""
        S, self._saved = self._saved, None
        if S is None:
            raise RuntimeError("backward without a grad-mode training forward")
        return S

    def _backward(self, g_pose, g_shape, g_verts, g_joints, g_full, g_transf):
        S = self._take_saved()
        N = S["fmean"].shape[0]
        c = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
        gt = self._padded(HEADS[5], N, c(g_transf))
        wt = self._wt
        gh1 = self._hand_branch_backward(S, g_pose, g_shape, g_verts, g_joints, g_full)
        gd1 = self._transhead_backward(S, gt, HEADS[4], HEADS[5], "d1")
        # res_layer4_mean feeds both branches: hand + object, in that order
        g_mean = K.linear_dgrad(gh1, wt(HEADS[0])) + K.linear_dgrad(gd1, wt(HEADS[4]))
        self.net.backward(g_mean=g_mean)

    def _image_of(self, inputs):
        """-> (image, xpad) of the batch on the device, the trunk's image plane set and the weight copies fresh."""
        dev = self.store.device
        xpad = inputs.get("image_nhwc4_padded")
        image = None
        if xpad is None:
            image = inputs.get(Queries.IMAGE).to(dev, non_blocking=True)
            self.net.image_plane = "f32"
        else:
            self.net.image_plane = self._plane_of(inputs, xpad)
        if not self.net._packed or self.flat_param._version != getattr(self, "_seen_version", -1):
            self.net.pack_weights()      # torch-side update (e.g. torch.optim.Adam); the fused optimizer repacks itself
            self._seen_version = self.flat_param._version
        return image, xpad

    def forward(self, inputs: Dict):
        dev = self.store.device
        image, xpad = self._image_of(inputs)
        if self.training and torch.is_grad_enabled():
            pose, shape, verts, joints, full, transf = _RegBridge.apply(self.flat_param, self, image, xpad)
        else:
            with torch.no_grad():
                pose, shape, verts, joints, full, transf = self._run(image, xpad, save=False)
        mano = {"hand_verts_3d": verts, "joints_3d": joints, "mano_shape": shape, "mano_pca_pose": pose, "mano_full_pose": full}
        return combine_outputs(mano_outputs(mano, inputs, dev), object_outputs(transf, inputs, dev))


class RegRoute:
    """TrainStep's route for a model that declares FUSED_STEP (HOPRegNet built with ARCH.FUSED_STEP): its own fused criterion and two linear
    graphs; the trunk-only layout has no staged backward, so with a process group the all-reduce runs between the two graphs, unsplit."""
    splittable, pipelinable = False, True

    @staticmethod
    def criterion(ts, example_batch):
        from .criterions import FusedRegCriterion, fused_or_none
        return fused_or_none(FusedRegCriterion, ts.crit, ts.hb.ncomps, example_batch)      # (None also for a hand_verts_3d target)

    @staticmethod
    def fwd_bwd(ts):
        """Trunk + heads + MANO -> fused regbased criterion (+backward) -> MANO / heads / trunk backward, no autograd."""
        hb, st = ts.hb, ts.static
        pose, shape, verts, joints, full, transf = hb._run(st.get(Queries.IMAGE), st.get("image_nhwc4_padded"), save=True)
        o = ts.fused(joints, pose, shape, transf, st)
        hb._backward(o["g_pose"], o["g_shape"], None, o["g_joints"], None, o["g_transf"])
        hb.flat_param.grad = hb.store.grad
        bridge = {"hand_verts_3d": verts, "joints_3d": joints, "mano_shape": shape, "mano_pca_pose": pose, "mano_full_pose": full, "transf": transf}
        return bridge, o["losses"], o

    @staticmethod
    def predictions(ts):
        """HOPRegNet's 18 keys from the bridge outputs (the camera projections stay torch ops, as in its forward)."""
        mano = {k: v for k, v in ts.out[0].items() if k != "transf"}
        return combine_outputs(mano_outputs(mano, ts.static, ts.dev), object_outputs(ts.out[0]["transf"], ts.static, ts.dev))


# ------------------------------------------------------------------------------------------------ HoNet
HONET_TRANS = ("mano_transhead.decoder.0", "mano_transhead.final_layer", "obj_transhead.decoder.0", "obj_transhead.final_layer")
# the bridge's outputs after the five of the MANO branch and the two TransHead rows: ab_honet_recover_fwd's, under the model's keys
HONET_GEO = K.HONET_FWD_OUT


class _HoBridge(torch.autograd.Function):
    """forward: HIP trunk + heads + MANO + recovery; backward: recovery bwd -> MANO bwd -> heads bwd -> trunk bwd into the flat gradient."""

    @staticmethod
    def forward(ctx, flat_param, owner, image, xpad, geo):
        out = owner._run(image, xpad, True, geo)
        ctx.owner = owner
        return out

    @staticmethod
    def backward(ctx, *grads):
        owner = ctx.owner
        owner._backward(*grads)
        owner.flat_param.grad = owner.store.grad      # the kernels wrote it; no copy, no accumulation
        return None, None, None, None, None


class HoNetHIP(HOPRegNetHIP):
    """HoNet (anakin/models/honetMANO.py:19-286; the torch module is honet.HoNet) on the HIP kernels: HOPRegNetHIP's trunk, ManoBranch heads
    and MANO kernels, two TransHeads (512 -> 256 -> 3 / 6) on the fp32 linear kernels, and the recovery stage -- placement from the predicted
    scale / translation, Rodrigues, rotation of the canonical object vertices, every projection -- as ab_honet_recover_fwd / _bwd.  One
    autograd Function (_HoBridge) whose outputs are the differentiable entries of the returned dict; the dict is the torch module's, key
    for key.  ARCH.FUSED_MESH_STEP: true -- TrainStep runs the model without autograd (criterions.FusedMeshCriterion on the recovery
    outputs) and replays the step as two hipGraphs; without it TrainStep takes its eager route."""
    CHECKPOINT_NAME = "HoNet"

    TORCH_MODULE = HoNet
    REG_MODEL = "HoNet"

    def _read_cfg(self, cfg):
        if self.FUSED_STEP:
            raise NotImplementedError("HoNet with FUSED_STEP: true -- that key selects HOPRegNet's fused criterion; HoNet's fused mesh "
                                      "criterion and captured step are ARCH.FUSED_MESH_STEP: true (leave ARCH.FUSED_STEP out)")
        self.FUSED_MESH_STEP = bool(cfg.get("FUSED_MESH_STEP", False))
        self.obj_trans_factor, self.obj_scale_factor = float(cfg["OBJ_TRANS_FACTOR"]), float(cfg["OBJ_SCALE_FACTOR"])

    def _geo_of(self, inputs):
        """The batch's geometric inputs of the recovery stage on the device: (cam_intr, obj_verts_can, corners_can | None).  An fp32
        contiguous tensor already on the device is handed on as it is (no copy): a captured step reads TrainStep's static tensors."""
        dev = self.store.device
        f = lambda t: t.to(dev, torch.float32, non_blocking=True).contiguous()      # noqa: E731
        img = inputs.get(Queries.IMAGE)
        if img is not None and (int(img.shape[3]), int(img.shape[2])) != (int(self.inp_res[0]), int(self.inp_res[1])):
            raise ValueError(f"HoNet: image {tuple(img.shape)} does not match DATA_PRESET.IMAGE_SIZE {tuple(self.inp_res)}")
        return (f(inputs[Queries.CAM_INTR]), f(inputs[Queries.OBJ_VERTS_CAN]),
                f(inputs[Queries.CORNERS_CAN]) if Queries.CORNERS_3D in inputs else None)

    def _run(self, image, xpad, save, geo):
        """-> (mano_pca_pose, mano_shape, hand_verts_3d, joints_3d, mano_full_pose, hand_st [N,3], obj_st [N,6], *HONET_GEO)."""
        cam_intr, can, ccan = geo
        fmean = self.net.forward(image=image, xpad=xpad)                    # res_layer4_mean [N, 512] f32
        h1, h2, pose, shape = self._mano_heads(fmean)
        m1 = self._lin(fmean, HONET_TRANS[0], relu=True)
        hst = self._lin(m1, HONET_TRANS[1])[:, :3]                          # rows of the padded output: the kernels take the pitch
        o1 = self._lin(fmean, HONET_TRANS[2], relu=True)
        ost = self._lin(o1, HONET_TRANS[3])[:, :6]
        verts, joints, full = K.mano_pca_fwd(pose, shape, self.mano, self.center_idx)
        o = K.honet_recover_fwd(hst, ost, cam_intr, joints, verts, can, ccan, (self.obj_trans_factor, self.obj_scale_factor), self.inp_res)
        self._saved = dict(fmean=fmean, h1=h1, h2=h2, m1=m1, o1=o1, pose=pose, shape=shape, hst=hst, ost=ost, verts=verts, joints=joints,
                           geo=geo) if save else None
        return (pose, shape, verts, joints, full, hst, ost) + tuple(o[k] for k in HONET_GEO)

    def _backward(self, g_pose, g_shape, g_verts, g_joints, g_full, g_hst, g_ost, *g_geo):
        S = self._take_saved()
        N = S["fmean"].shape[0]
        c = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
        cam_intr, can, ccan = S["geo"]
        # recovery: the kernel overwrites the first 3 / 6 columns of the padded head gradients; direct gradients on the rows are added
        gh, go = self._padded(HONET_TRANS[1], N), self._padded(HONET_TRANS[3], N)
        _, _, g_j, g_v = K.honet_recover_bwd(S["hst"], S["ost"], cam_intr, S["joints"], S["verts"], can, ccan,
                                             (self.obj_trans_factor, self.obj_scale_factor), self.inp_res,
                                             {k: c(g) for k, g in zip(HONET_GEO, g_geo)}, g_hand_st=gh[:, :3], g_obj_st=go[:, :6])
        if g_hst is not None:
            gh[:, :3] += g_hst
        if g_ost is not None:
            go[:, :6] += g_ost
        if g_joints is not None:
            g_j += g_joints
        if g_verts is not None:
            g_v += g_verts
        gh1 = self._hand_branch_backward(S, g_pose, g_shape, g_v, g_j, g_full)
        gm1 = self._transhead_backward(S, gh, HONET_TRANS[0], HONET_TRANS[1], "m1")
        go1 = self._transhead_backward(S, go, HONET_TRANS[2], HONET_TRANS[3], "o1")
        # res_layer4_mean feeds three branches: ManoBranch + hand TransHead + object TransHead, in that order
        wt = self._wt
        g_mean = (K.linear_dgrad(gh1, wt(HEADS[0])) + K.linear_dgrad(gm1, wt(HONET_TRANS[0]))) + K.linear_dgrad(go1, wt(HONET_TRANS[2]))
        self.net.backward(g_mean=g_mean)

    def forward(self, inputs: Dict):
        image, xpad = self._image_of(inputs)
        geo = self._geo_of(inputs)
        if self.training and torch.is_grad_enabled():
            out = _HoBridge.apply(self.flat_param, self, image, xpad, geo)
        else:
            with torch.no_grad():
                out = self._run(image, xpad, False, geo)
        return self._assemble(out)

    def _assemble(self, out):
        """_run's outputs -> the torch module's dict, key for key."""
        pose, shape, verts, joints, full, hst, ost = out[:7]
        B = hst.shape[0]
        res = {"hand_verts_3d": verts, "joints_3d": joints, "mano_shape": shape, "mano_pca_pose": pose, "mano_full_pose": full}
        res.update(zip(HONET_GEO, out[7:]))
        h_scale, h_trans, o_scale, o_trans = hst[:, :1], hst[:, 1:], ost[:, :1], ost[:, 1:3]
        res.update(hand_pred_trans=h_trans, hand_pred_scale=h_scale, hand_trans=h_trans.unsqueeze(1) * self.obj_trans_factor,
                   hand_scale=h_scale.reshape(B, 1, 1) * self.obj_scale_factor, obj_pred_scale=o_scale, obj_pred_trans=o_trans,
                   obj_rot=ost[:, 3:], obj_scale=o_scale.reshape(B, 1, 1) * self.obj_scale_factor,
                   obj_trans=o_trans.unsqueeze(1) * self.obj_trans_factor, boxroot_3d_abs=res["obj_center"])
        return res


class MeshRoute:
    """TrainStep's route for a model that declares FUSED_MESH_STEP (HoNet built with ARCH.FUSED_MESH_STEP): the fused mesh criterion
    (ab_honet_loss) on the recovery outputs and the same two linear graphs as RegRoute.  Its mesh queries are made from the render inputs
    of the batch being learned, which the pipelined modes hold one batch ahead: the step renders and learns in order."""
    splittable, pipelinable = False, False

    @staticmethod
    def criterion(ts, example_batch):
        """A loader with MANAGER.MESH_QUERIES writes the three mesh queries inside the captured region (one ab_mesh_queries launch after
        the render) into tensors allocated here, before the criterion looks at the batch and before any capture."""
        from .criterions import FusedMeshCriterion, fused_or_none
        if getattr(ts.renderer, "mesh_queries", 0) and hasattr(ts.renderer, "mesh_queries_into"):
            ts.renderer.mesh_queries_into(ts.static)
            ts.mesh_queries = True
        return fused_or_none(FusedMeshCriterion, ts.crit, ts.hb.ncomps, ts.static)

    @staticmethod
    def fwd_bwd(ts):
        """Trunk + heads + MANO + recovery -> fused mesh criterion (+backward) -> recovery / MANO / heads / trunk backward, no autograd.
        The recovery stage reads the static batch's own tensors (cam_intr, obj_verts_can, corners_can): fixed addresses."""
        hb, st = ts.hb, ts.static
        out = hb._run(st.get(Queries.IMAGE), st.get("image_nhwc4_padded"), True, hb._geo_of(st))
        rec = dict(zip(HONET_GEO, out[7:]))
        o = ts.fused(rec["joints_3d_abs"], rec["hand_verts_3d_abs"], rec["obj_verts_3d_abs"], rec["corners_3d_abs"], out[0], out[1], st)
        # the five gradients; the TransHead rows (g_hst / g_ost) and the untouched recovery outputs get none
        hb._backward(o["g_mano_pca_pose"], o["g_mano_shape"], None, None, None, None, None, *(o.get("g_" + k) for k in HONET_GEO))
        hb.flat_param.grad = hb.store.grad
        return out, o["losses"], o

    @staticmethod
    def predictions(ts):
        """HoNet's dict from the bridge outputs, as HoNetHIP.forward assembles it."""
        return ts.hb._assemble(ts.out[0])
