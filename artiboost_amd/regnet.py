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
metrics run unchanged."""
import os
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
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
        dev = cfg.get("DEVICE", "cuda")
        cd = cfg.get("COMPUTE_DTYPE", "bf16x3")
        self.store = ParamStore(device=dev, layers=BACKBONES[bb["TYPE"]][1], reg_heads=self.ncomps)
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
                raise FileNotFoundError(f"=> No HOPRegNet checkpoints file found in {pretrained}")
            ck = torch.load(pretrained, map_location="cpu")
            self.load_state_dict(ck["state_dict"] if isinstance(ck, dict) and "state_dict" in ck else ck, strict=True)

    # --- checkpoints in the reference layout (the torch module's keys: base_net.*, mano_branch.*, obj_transfhead.*)
    def state_dict(self, *a, **k):
        return OrderedDict((k_, v.cpu()) for k_, v in self.store.reference_state_dict().items())

    def load_state_dict(self, sd, strict=True):
        sd = HOPRegNet.clean_reference_state_dict(sd)
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
        raise RuntimeError("HOPRegNet (HIP) cannot be replicated by nn.DataParallel: its parameters live in one device's flat buffer; "
                           "restrict DataParallel to one device (--gpu_id 0 / CUDA_VISIBLE_DEVICES=0)")

    # --- the device computation
    def _w(self, name):
        e = self.store.entries[name + ".weight"]
        return self.store.view(name + ".weight").view(e.kshape[0], -1)

    def _lin(self, x, name, relu=False):
        return K.linear_fwd(x, self._w(name), self.store.view(name + ".bias"), relu=relu)

    def _run(self, image, xpad, save):
        """-> (mano_pca_pose [N,3+ncomps], mano_shape [N,10], hand_verts_3d [N,778,3], joints_3d [N,21,3], mano_full_pose [N,48], transf [N,9])."""
        fmean = self.net.forward(image=image, xpad=xpad)                    # res_layer4_mean [N, 512] f32
        h1 = self._lin(fmean, HEADS[0], relu=True)
        h2 = self._lin(h1, HEADS[1], relu=True)
        pose = self._lin(h2, HEADS[2])[:, :self.P].contiguous()
        shape = self._lin(h2, HEADS[3])[:, :10].contiguous()
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

    def _backward(self, g_pose, g_shape, g_verts, g_joints, g_full, g_transf):
        S, p, dev = self._saved, self.store, self.store.device
        if S is None:
            raise RuntimeError("backward without a grad-mode training forward")
        self._saved = None
        N = S["fmean"].shape[0]
        c = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
        gvt = c(g_verts) if g_verts is not None else torch.zeros((N, 778, 3), dtype=torch.float32, device=dev)
        gjt = c(g_joints) if g_joints is not None else torch.zeros((N, 21, 3), dtype=torch.float32, device=dev)
        g_pc, g_b = K.mano_pca_bwd(S["pose"], S["shape"], self.mano, gvt, gjt, c(g_full), self.center_idx)
        gp = self._padded(HEADS[2], N, g_pc, c(g_pose))
        gs = self._padded(HEADS[3], N, g_b, c(g_shape))
        gt = self._padded(HEADS[5], N, c(g_transf))
        gv = lambda n: p.gview(n + ".weight").view(p.entries[n + ".weight"].kshape[0], -1)      # noqa: E731
        gb = lambda n: p.gview(n + ".bias")                                                       # noqa: E731
        wt = lambda n: self.net.box_t[n + ".weight"]                                              # noqa: E731  ([in][out] copies)
        # hand branch: pose_reg and shape_reg share their input (h2); its gradient is the sum of theirs, pose first
        K.linear_wgrad(gp, S["h2"], gv(HEADS[2]), gb(HEADS[2]))
        K.linear_wgrad(gs, S["h2"], gv(HEADS[3]), gb(HEADS[3]))
        gh2 = K.linear_dgrad(gp, wt(HEADS[2]), act_out=S["h2"]) + K.linear_dgrad(gs, wt(HEADS[3]), act_out=S["h2"])
        K.linear_wgrad(gh2, S["h1"], gv(HEADS[1]), gb(HEADS[1]))
        gh1 = K.linear_dgrad(gh2, wt(HEADS[1]), act_out=S["h1"])
        K.linear_wgrad(gh1, S["fmean"], gv(HEADS[0]), gb(HEADS[0]))
        # object branch
        K.linear_wgrad(gt, S["d1"], gv(HEADS[5]), gb(HEADS[5]))
        gd1 = K.linear_dgrad(gt, wt(HEADS[5]), act_out=S["d1"])
        K.linear_wgrad(gd1, S["fmean"], gv(HEADS[4]), gb(HEADS[4]))
        # res_layer4_mean feeds both branches: hand + object, in that order
        g_mean = K.linear_dgrad(gh1, wt(HEADS[0])) + K.linear_dgrad(gd1, wt(HEADS[4]))
        self.net.backward(g_mean=g_mean)

    def forward(self, inputs: Dict):
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
        if self.training and torch.is_grad_enabled():
            pose, shape, verts, joints, full, transf = _RegBridge.apply(self.flat_param, self, image, xpad)
        else:
            with torch.no_grad():
                pose, shape, verts, joints, full, transf = self._run(image, xpad, save=False)
        mano = {"hand_verts_3d": verts, "joints_3d": joints, "mano_shape": shape, "mano_pca_pose": pose, "mano_full_pose": full}
        return combine_outputs(mano_outputs(mano, inputs, dev), object_outputs(transf, inputs, dev))
