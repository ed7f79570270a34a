"""Torch restatement of the reference's hand-mesh fit, for the tests of ab_mano_fit (float64, or float32 for the spread an fp32
implementation has): anakin/postprocess/iknet/fittingunit.py:43-225 (geo, residuals, mano_de, the loop), utils.py:13-41
(quaternion -> axis-angle), manolayer.py:134-276 (the JAX MANO layer: Rodrigues through a quaternion with +1e-8 in both norms,
centred on joint 9), and jax.experimental.optimizers.adam(0.03, b1=0.5, b2=0.5) with the loop's step index i = n = 1..20.

Every hand is fitted independently but the pose regulariser takes the mean over the WHOLE batch of IKNet poses (`so3_init` is the
batch, fittingunit.py:190).  The two non-smooth terms take JAX's gradients: d|t|/dt = sign(t), 0 at 0; d min(S, 0)/dS = 1 where
S < 0, 1/2 at S == 0 (lax.min splits a tie), 0 where S > 0 -- the same rule as the kernel."""
import numpy as np
import torch

PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
TIPS = [745, 317, 444, 556, 673]
REORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
LR, B1, B2, EPS = 0.03, 0.5, 0.5, 1e-8


def quat_to_aa(q):
    """utils.normalize_quaternion + quaternion_to_angle_axis, literally: q [..., 4] -> [..., 3]."""
    q = torch.nn.functional.normalize(q, p=2, dim=-1, eps=1e-12)
    q1, q2, q3 = q[..., 1], q[..., 2], q[..., 3]
    s2 = q1 * q1 + q2 * q2 + q3 * q3
    s, c = torch.sqrt(s2), q[..., 0]

    def my_atan2(y, x):
        pi = torch.tensor(np.pi, dtype=y.dtype)
        a = torch.atan(y / x)
        a = torch.where((y > 0) & (x < 0), a + pi, a)
        return torch.where((y < 0) & (x < 0), a + pi, a)
    two_theta = 2.0 * torch.where(c < 0.0, my_atan2(-s, -c), my_atan2(s, c))
    k = torch.where(s2 > 0.0, two_theta / s, 2.0 * torch.ones_like(s))
    return q[..., 1:] * k.unsqueeze(-1)


class Mano:
    """manolayer.ManoLayer(center_idx=9, use_pca=False, flat_hand_mean=True).__call__ over [N,48] axis-angle and [N,10] betas ->
    (verts [N,778,3], joints [N,21,3]), both minus joint 9."""

    def __init__(self, hand_model, dtype=torch.float64):
        t = lambda k: torch.as_tensor(np.asarray(hand_model[k], np.float64), dtype=dtype)     # noqa: E731
        self.v_template, self.shapedirs, self.posedirs = t("v_template"), t("shapedirs"), t("posedirs")
        self.J_regressor, self.weights, self.dtype = t("J_regressor"), t("weights"), dtype

    def __call__(self, so3, beta):
        N, dt = so3.shape[0], self.dtype
        aa = so3.reshape(N * 16, 3)
        n = torch.linalg.norm(aa + 1e-8, dim=1, keepdim=True)
        quat = torch.cat([torch.cos(n * 0.5), torch.sin(n * 0.5) * (aa / n)], 1)
        quat = quat / torch.linalg.norm(quat + 1e-8, dim=1, keepdim=True)
        w, x, y, z = quat.unbind(1)
        R = torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                         2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                         2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1).reshape(N, 16, 3, 3)
        pose_map = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(N, 135)
        v_shaped = self.v_template + torch.einsum("vcl,nl->nvc", self.shapedirs, beta)
        J = torch.einsum("jv,nvc->njc", self.J_regressor, v_shaped)
        v_posed = v_shaped + torch.einsum("vcp,np->nvc", self.posedirs, pose_map)
        bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dt).expand(N, 1, 4)
        G = [None] * 16
        for j in range(16):
            par = PARENTS[j]
            t = J[:, j] if par < 0 else J[:, j] - J[:, par]
            L = torch.cat([torch.cat([R[:, j], t[:, :, None]], 2), bottom], 1)
            G[j] = L if par < 0 else G[par] @ L
        G = torch.stack(G, 1)[:, :, :3]                                           # [N,16,3,4]
        t2 = G[..., 3] - torch.einsum("njrc,njc->njr", G[..., :3], J)
        G2 = torch.cat([G[..., :3], t2[..., None]], 3)
        T = torch.einsum("vj,njrc->nvrc", self.weights, G2)
        verts = torch.einsum("nvrc,nvc->nvr", T[..., :3], v_posed) + T[..., 3]
        jtr = torch.cat([G[..., 3], verts[:, TIPS]], 1)[:, REORDER]
        c = jtr[:, 9:10]
        return verts - c, jtr - c


def _min0(S):
    """min(S, 0) with JAX's gradient (1/2 at a tie)."""
    zero = torch.zeros_like(S)
    return torch.where(S < 0, S, zero) + torch.where(S == 0, 0.5 * S, zero)


def geo(J):
    """fittingunit.py:43-60 per hand: J [N,21,3] -> [N]."""
    pa, pb, pc, pd = J[:, 1:21:4], J[:, 2:21:4], J[:, 3:21:4], J[:, 4:21:4]
    vab, vbc, vcd = pa - pb, pb - pc, pc - pd
    c1 = torch.cross(vab, vbc, dim=-1)
    loss_1 = (c1 * vcd).sum(-1).abs().mean(-1)
    loss_2 = -_min0((c1 * torch.cross(vbc, vcd, dim=-1)).sum((-1, -2)))
    return 10000 * loss_1 + 100000 * loss_2


def prepare(quat, pred_joints, dtype=torch.float64):
    """quat [B,64] raw IKNet output, pred_joints [B,21,3] -> so3_init [B,48], root [B,1,3], bone [B], target [B,21,3]."""
    quat, pj = quat.to(dtype), pred_joints.to(dtype)
    so3_init = quat_to_aa(quat.reshape(-1, 16, 4)).reshape(-1, 48)
    root = pj[:, 9:10]
    jc = pj - root
    bone = torch.linalg.norm(jc[:, 0] - jc[:, 9], dim=1)
    return so3_init, root, bone, jc / bone[:, None, None]


def residuals(params, so3_init, root, target, mano):
    """fittingunit.py:63-80 for every hand at once: params [N,59] (so3 | beta | bone) -> err [N]; so3_init [B,48] is the batch."""
    so3, beta, bone = params[:, :48], params[:, 48:58], params[:, 58]
    _, jm = mano(so3, beta)
    bp = torch.linalg.norm(jm[:, 0] - jm[:, 9], dim=1)
    reg = ((so3[:, None, :] - so3_init[None]) ** 2).mean((1, 2))
    reg_beta = (beta ** 2).sum(1)
    u = jm / bp[:, None, None]
    errkp = ((u - target) ** 2).mean((1, 2))
    return 0.01 * reg + 0.01 * reg_beta + errkp + 100 * geo(u * bone[:, None, None] + root)


def grad(params, so3_init, root, target, mano):
    p = params.detach().clone().requires_grad_(True)
    err = residuals(p, so3_init, root, target, mano)
    g, = torch.autograd.grad(err.sum(), p)
    return g, err.detach()


def adam_step(x, g, m, v, n):
    """jax.experimental.optimizers.adam update(i = n) with b1 = b2 = 0.5."""
    m = (1 - B1) * g + B1 * m
    v = (1 - B2) * g * g + B2 * v
    mhat = m / (1 - B1 ** (n + 1))
    vhat = v / (1 - B2 ** (n + 1))
    return x - LR * mhat / (torch.sqrt(vhat) + EPS), m, v


def mano_de(params, root, bone, mano):
    """fittingunit.py:83-97 with the PREDICTED bone -> verts [N,778,3], joints [N,21,3]."""
    verts, jm = mano(params[:, :48], params[:, 48:58])
    bp = torch.linalg.norm(jm[:, 0] - jm[:, 9], dim=1)[:, None, None]
    s = bone[:, None, None]
    return verts / bp * s + root, jm / bp * s + root


def fit(quat, pred_joints, hand_model, n_iter=20, dtype=torch.float64):
    """The whole fit of one batch -> dict verts, joints, traj (list of (params, m, v, grad, err) BEFORE each step n = 1..n_iter)."""
    mano = Mano(hand_model, dtype)
    so3_init, root, bone, target = prepare(quat, pred_joints, dtype)
    B = so3_init.shape[0]
    x = torch.cat([so3_init, torch.zeros((B, 10), dtype=dtype), bone[:, None]], 1)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    traj = []
    for n in range(1, n_iter + 1):
        g, err = grad(x, so3_init, root, target, mano)
        traj.append((x, m, v, g, err))
        x, m, v = adam_step(x, g, m, v, n)
    verts, joints = mano_de(x, root, bone, mano)
    return {"verts": verts, "joints": joints, "params": x, "traj": traj, "so3_init": so3_init, "root": root, "bone": bone,
            "target": target, "mano": mano}


def near_kink(params, root, target, mano, rel=1e-4):
    """[N] bool: the hand's objective sits within `rel` (relative) of one of its kinks -- a finger's triple product t_f near 0 or the
    clipped sum S near 0 -- where fp32 rounding can flip a sign of the gradient."""
    with torch.no_grad():
        so3, beta, bone = params[:, :48], params[:, 48:58], params[:, 58]
        _, jm = mano(so3, beta)
        bp = torch.linalg.norm(jm[:, 0] - jm[:, 9], dim=1)
        J = jm / bp[:, None, None] * bone[:, None, None] + root
        pa, pb, pc, pd = J[:, 1:21:4], J[:, 2:21:4], J[:, 3:21:4], J[:, 4:21:4]
        vab, vbc, vcd = pa - pb, pb - pc, pc - pd
        c1, c2 = torch.cross(vab, vbc, dim=-1), torch.cross(vbc, vcd, dim=-1)
        t = (c1 * vcd).sum(-1)
        tscale = vab.norm(dim=-1) * vbc.norm(dim=-1) * vcd.norm(dim=-1)
        S = (c1 * c2).sum((-1, -2))
        sscale = (c1.norm(dim=-1) * c2.norm(dim=-1)).sum(-1)
        return (t.abs() <= rel * tscale).any(1) | (S.abs() <= rel * sscale)
