"""Tensor-level wrappers over the C ABI (include/artiboost_hip.h).  No autograd here: every function launches HIP
kernels on the current stream and returns device tensors.  Layouts: activations NHWC, weights OHWI / IHWO."""
import ctypes

import torch

from . import _lib as L


def _empty(shape, like, dtype=None):
    return torch.empty(shape, dtype=dtype or like.dtype, device=like.device)


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def conv2d_fwd(x, w_ohwi, stride, pad, bias=None, want_stats=False, relu=False):
    """x [N,H,W,Cin], w [Cout,kh,kw,Cin] -> y [N,Ho,Wo,Cout] (+ per-tile BN partials)."""
    N, H, W, Cin = x.shape
    Cout, kh, kw, _ = w_ohwi.shape
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    y = _empty((N, Ho, Wo, Cout), x)
    lib = L.lib()
    stats = None
    if want_stats:
        nt = lib.ab_conv2d_stat_rows(L.i(L.dt(x)), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.i(0))
        stats = torch.empty((nt, Cout, 2), dtype=torch.float32, device=x.device)
    L.check(lib.ab_conv2d_fwd(L.ptr(x), L.ptr(w_ohwi), L.ptr(y), L.i(L.dt(x)), L.i(N), L.i(H), L.i(W), L.i(Cin),
                              L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(bias), L.ptr(stats),
                              L.i(1 if relu else 0), L.stream()), "ab_conv2d_fwd")
    return (y, stats) if want_stats else y


def conv2d_stem_fwd(xpad, w_stem, H, W, want_stats=False):
    """xpad [N,H+6,W+8,4], w_stem [Cout,7,8,4] -> y [N,H/2,W/2,Cout]."""
    N = xpad.shape[0]
    Cout = w_stem.shape[0]
    y = _empty((N, H // 2, W // 2, Cout), xpad)
    lib = L.lib()
    stats = None
    if want_stats:
        nt = lib.ab_conv2d_stat_rows(L.i(L.dt(xpad)), L.i(N), L.i(H), L.i(W), L.i(4), L.i(Cout), L.i(7), L.i(7), L.i(2), L.i(3), L.i(1))
        stats = torch.empty((nt, Cout, 2), dtype=torch.float32, device=xpad.device)
    L.check(lib.ab_conv2d_stem_fwd(L.ptr(xpad), L.ptr(w_stem), L.ptr(y), L.i(L.dt(xpad)), L.i(N), L.i(H), L.i(W),
                                   L.i(Cout), L.ptr(stats), L.stream()), "ab_conv2d_stem_fwd")
    return (y, stats) if want_stats else y


def conv2d_dgrad(dy, w_ihwo, in_hw, stride, pad, addend=None, bn=None, want_stats=False):
    """dy [N,Ho,Wo,Cout], w [Cin,kh,kw,Cout] -> dx [N,H,W,Cin]  (== ConvTranspose2d forward when x:=dy).
    want_stats (transposed-conv forward): returns (dx, part) with the BatchNorm partial sums [rows, Cin, 2] of dx written by
    the kernel's epilogue, or by a col_stats pass where the shape has no fused path.
    bn=(bn_y, bn_out_or_None, bnp): also try to fuse the BatchNorm-backward reduction of the layer that produced this
    conv's input into the epilogue (ab_conv2d_dgrad_bnstats); returns (dx, part) with part=None when the shape has no
    fused path."""
    N, Ho, Wo, Cout = dy.shape
    Cin, kh, kw, _ = w_ihwo.shape
    H, W = in_hw
    dx = _empty((N, H, W, Cin), dy)
    if bn is not None:
        lib = L.lib()
        rows = lib.ab_conv2d_dgrad_bnstats_rows(L.i(L.dt(dy)), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw),
                                                L.i(stride), L.i(pad))
        if rows > 0:
            bn_y, bn_out, bnp = bn
            part = torch.empty((rows, Cin, 2), dtype=torch.float32, device=dy.device)
            L.check(lib.ab_conv2d_dgrad_bnstats(L.ptr(dy), L.ptr(w_ihwo), L.ptr(dx), L.i(L.dt(dy)), L.i(N), L.i(H), L.i(W),
                                                L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(addend),
                                                L.ptr(bn_y), L.ptr(bn_out), L.ptr(bnp), L.ptr(part), L.stream()),
                    "ab_conv2d_dgrad_bnstats")
            return dx, part
    part = None
    if want_stats and addend is None:
        rows = L.lib().ab_conv2d_dgrad_stat_rows(L.i(L.dt(dy)), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw),
                                                 L.i(stride), L.i(pad))
        if rows > 0:
            part = torch.empty((rows, Cin, 2), dtype=torch.float32, device=dy.device)
    L.check(L.lib().ab_conv2d_dgrad(L.ptr(dy), L.ptr(w_ihwo), L.ptr(dx), L.i(L.dt(dy)), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                    L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(addend), L.ptr(part),
                                    L.stream()), "ab_conv2d_dgrad")
    if want_stats:
        return dx, (part if part is not None else col_stats(dx))
    return (dx, None) if bn is not None else dx


_ws = {}


def _workspace(nbytes, device):
    """Scratch for the slab-writing kernels.  Eager: one growing buffer per (device, stream) -- stream order makes the reuse safe.
    Under hipGraph capture: a fresh allocation from the capturing graph's own pool every time.  A cached buffer would be shared by
    every graph captured on torch's (global) capture stream, and replacing it when a later call needs more frees memory that
    an EARLIER graph still replays into."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    w = _ws.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = w
    return w


class PendingReductions:
    """Slab reductions recorded by deferred weight-gradient calls (`defer=`), run in one launch by flush().  Each deferred
    call gets its own slab workspace, kept alive here until the batched reduction has been enqueued."""

    def __init__(self):
        self.descs, self.keep = [], []

    def new(self, nbytes, device):
        ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
        d = L.WgradReduceDesc()
        self.keep.append(ws)
        self.descs.append(d)
        return ws, d

    def flush(self):
        live = [d for d in self.descs if d.nslices > 0]
        if live:
            arr = (L.WgradReduceDesc * len(live))(*live)
            L.check(L.lib().ab_wgrad_reduce_batch(arr, L.i(len(live)), L.stream()), "ab_wgrad_reduce_batch")
        self.descs, self.keep = [], []


def conv2d_wgrad(x, dy, kh, kw, stride, pad, out=None, accumulate=False, defer=None):
    """x [N,H,W,Cin], dy [N,Ho,Wo,Cout] -> dw float32 [Cout,kh,kw,Cin].  defer: a PendingReductions that receives the final
    slab reduction instead of it being launched here (dw is complete only after defer.flush())."""
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    lib = L.lib()
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    nbytes = lib.ab_conv2d_wgrad_workspace(L.i(M), L.i(Cout), L.i(kh * kw * Cin))
    dw = out if out is not None else torch.empty((Cout, kh, kw, Cin), dtype=torch.float32, device=x.device)
    if defer is not None:
        ws, d = defer.new(nbytes, x.device)
        L.check(lib.ab_conv2d_wgrad_deferred(L.ptr(x), L.ptr(dy), L.ptr(dw), L.i(L.dt(x)), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                             L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(ws),
                                             L.i(1 if accumulate else 0), ctypes.byref(d), L.stream()), "ab_conv2d_wgrad_deferred")
        return dw
    ws = _workspace(nbytes, x.device)
    L.check(lib.ab_conv2d_wgrad(L.ptr(x), L.ptr(dy), L.ptr(dw), L.i(L.dt(x)), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(ws),
                                L.i(1 if accumulate else 0), L.stream()), "ab_conv2d_wgrad")
    return dw


def conv2d_stem_wgrad(xpad, dy, H, W, out=None, defer=None):
    N = xpad.shape[0]
    Cout = dy.shape[3]
    lib = L.lib()
    nbytes = lib.ab_conv2d_stem_wgrad_workspace(L.i(N), L.i(H), L.i(W), L.i(Cout))
    dw = out if out is not None else torch.empty((Cout, 7, 8, 4), dtype=torch.float32, device=xpad.device)
    if defer is not None:
        ws, d = defer.new(nbytes, xpad.device)
        L.check(lib.ab_conv2d_stem_wgrad_deferred(L.ptr(xpad), L.ptr(dy), L.ptr(dw), L.i(L.dt(xpad)), L.i(N), L.i(H), L.i(W),
                                                  L.i(Cout), L.ptr(ws), ctypes.byref(d), L.stream()), "ab_conv2d_stem_wgrad_deferred")
        return dw
    ws = _workspace(nbytes, xpad.device)
    L.check(lib.ab_conv2d_stem_wgrad(L.ptr(xpad), L.ptr(dy), L.ptr(dw), L.i(L.dt(xpad)), L.i(N), L.i(H), L.i(W),
                                     L.i(Cout), L.ptr(ws), L.stream()), "ab_conv2d_stem_wgrad")
    return dw


def col_stats(x2d):
    M, C = x2d.shape[:-1].numel(), x2d.shape[-1]
    lib = L.lib()
    part = torch.empty((lib.ab_col_stats_nparts(L.l(M)), C, 2), dtype=torch.float32, device=x2d.device)
    L.check(lib.ab_col_stats(L.ptr(x2d), L.i(L.dt(x2d)), L.l(M), L.i(C), L.ptr(part), L.stream()), "ab_col_stats")
    return part


def bn_finalize(part, count, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, out=None):
    C = gamma.numel()
    bnp = out if out is not None else torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    L.check(L.lib().ab_bn_finalize(L.ptr(part), L.i(part.shape[0]), L.i(C), L.l(count), L.ptr(gamma), L.ptr(beta),
                                   L.f(eps), L.f(momentum), L.ptr(running_mean), L.ptr(running_var), L.ptr(bnp),
                                   L.stream()), "ab_bn_finalize")
    return bnp


def bn_eval_params(gamma, beta, rm, rv, eps=1e-5):
    C = gamma.numel()
    bnp = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    L.check(L.lib().ab_bn_eval_params(L.i(C), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.f(eps), L.ptr(bnp),
                                      L.stream()), "ab_bn_eval_params")
    return bnp


def bn_eval_params_batch(flat, stats, desc_dev, n, max_c, out, eps=1e-5):
    """Eval-mode (scale, shift, mean, invstd) of n BatchNorms in one launch; desc_dev int32 [n,6] (see the header)."""
    L.check(L.lib().ab_bn_eval_params_batch(L.ptr(flat), L.ptr(stats), L.ptr(desc_dev), L.i(n), L.i(max_c), L.f(eps), L.ptr(out), L.stream()),
            "ab_bn_eval_params_batch")
    return out


def bn_apply(y, bnp, res=None, relu=True, out=None):
    C = y.shape[-1]
    M = y.numel() // C
    o = out if out is not None else torch.empty_like(y)
    L.check(L.lib().ab_bn_apply(L.ptr(y), L.ptr(res), L.ptr(bnp), L.i(L.dt(y)), L.l(M), L.i(C), L.i(1 if relu else 0),
                                L.ptr(o), L.stream()), "ab_bn_apply")
    return o


def bn_bwd(dout, out, y, bnp, dgamma, dbeta, relu=True, want_dz=False, dy_out=None, part=None):
    """-> dy (grad wrt the conv output y) [, dz = dout*relu_mask].
    part: per-tile sums from conv2d_dgrad(..., bn=...) -- skips the reduction pass.
    relu: False (no activation), True (mask from the stored activation `out`; required when a residual was added before
    the ReLU) or "recompute" (mask from y*scale+shift, `out` is not read)."""
    C = y.shape[-1]
    M = y.numel() // C
    lib = L.lib()
    bwdp = torch.empty((2, C), dtype=torch.float32, device=y.device)
    dy = dy_out if dy_out is not None else torch.empty_like(y)
    dz = torch.empty_like(y) if want_dz else None
    if part is not None:       # first pass already done in the epilogue of the conv that produced `dout`
        L.check(lib.ab_bn_bwd_apply(L.ptr(dout), L.ptr(out if relu is True else None), L.ptr(y), L.ptr(bnp), L.i(L.dt(y)),
                                    L.l(M), L.i(C), L.i(2 if relu == "recompute" else 1 if relu else 0), L.ptr(part),
                                    L.i(part.shape[0]), L.ptr(bwdp), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dy), L.ptr(dz),
                                    L.stream()), "ab_bn_bwd_apply")
        return (dy, dz) if want_dz else dy
    part = torch.empty((lib.ab_col_stats_nparts(L.l(M)), C, 2), dtype=torch.float32, device=y.device)
    L.check(lib.ab_bn_bwd(L.ptr(dout), L.ptr(out if relu is True else None), L.ptr(y), L.ptr(bnp), L.i(L.dt(y)), L.l(M), L.i(C),
                          L.i(2 if relu == "recompute" else 1 if relu else 0), L.ptr(part), L.ptr(bwdp), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dy),
                          L.ptr(dz), L.stream()), "ab_bn_bwd")
    return (dy, dz) if want_dz else dy


def add(a, b, out=None):
    o = out if out is not None else torch.empty_like(a)
    L.check(L.lib().ab_add(L.ptr(a), L.ptr(b), L.i(L.dt(a)), L.l(a.numel()), L.ptr(o), L.stream()), "ab_add")
    return o


def maxpool_fwd(x, want_idx=True):
    N, H, W, C = x.shape
    o = _empty((N, H // 2, W // 2, C), x)
    idx = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=x.device) if want_idx else None
    L.check(L.lib().ab_maxpool3x3s2_fwd(L.ptr(x), L.i(L.dt(x)), L.i(N), L.i(H), L.i(W), L.i(C), L.ptr(o), L.ptr(idx),
                                        L.stream()), "ab_maxpool3x3s2_fwd")
    return (o, idx) if want_idx else o


def bn_relu_maxpool_fwd(y, bnp):
    """maxpool3x3/2(relu(bn(y))) in one pass -> (pooled, idx); the full-resolution activation is never written."""
    N, H, W, C = y.shape
    o = _empty((N, H // 2, W // 2, C), y)
    idx = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=y.device)
    L.check(L.lib().ab_bn_relu_maxpool3x3s2_fwd(L.ptr(y), L.ptr(bnp), L.i(L.dt(y)), L.i(N), L.i(H), L.i(W), L.i(C),
                                                L.ptr(o), L.ptr(idx), L.stream()), "ab_bn_relu_maxpool3x3s2_fwd")
    return o, idx


def bn_relu_maxpool_fwd_x3(y, bnp, want_win=False, want_f32=True):
    """bn_relu_maxpool_fwd on fp32 -> (pooled fp32 with its (hi, lo) planes as `_ab_split`, idx): the planes come from the
    pooling pass itself instead of a separate split pass over the pooled tensor.  want_win: also the raw conv output at every
    window's winner (-> (pooled, idx, ywin)), which bn_relu_maxpool_bwd_x3(ywin=...) reduces instead of the full-resolution y."""
    N, H, W, C = y.shape
    o = torch.empty((N, H // 2, W // 2, C), dtype=torch.float32, device=y.device)
    pl = torch.empty((2, N, H // 2, W // 2, C), dtype=torch.bfloat16, device=y.device)
    idx = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=y.device)
    if want_win and C % 8 == 0:
        ywin = torch.empty_like(o)
        if not want_f32:      # the pooled activation as planes only (its consumers read planes: conv1, the residual, the weight gradient)
            o = None
        L.check(L.lib().ab_bn_relu_maxpool3x3s2_fwd_x3w(L.ptr(y), L.ptr(bnp), L.i(N), L.i(H), L.i(W), L.i(C), L.ptr(o), L.ptr(pl[0]),
                                                        L.ptr(pl[1]), L.ptr(idx), L.ptr(ywin), L.stream()), "ab_bn_relu_maxpool3x3s2_fwd_x3w")
        if o is None:
            return pl, idx, ywin
        o._ab_split = pl
        return o, idx, ywin
    L.check(L.lib().ab_bn_relu_maxpool3x3s2_fwd_x3(L.ptr(y), L.ptr(bnp), L.i(N), L.i(H), L.i(W), L.i(C), L.ptr(o), L.ptr(pl[0]),
                                                   L.ptr(pl[1]), L.ptr(idx), L.stream()), "ab_bn_relu_maxpool3x3s2_fwd_x3")
    o._ab_split = pl
    return (o, idx, None) if want_win else (o, idx)


def bn_relu_maxpool_bwd(dpool, idx, y, bnp, dgamma, dbeta):
    """Backward of bn_relu_maxpool_fwd -> dy (gradient wrt the conv output y)."""
    N, H, W, C = y.shape
    lib = L.lib()
    part = torch.empty((lib.ab_col_stats_nparts(L.l(N * H * W)), C, 2), dtype=torch.float32, device=y.device)
    bwdp = torch.empty((2, C), dtype=torch.float32, device=y.device)
    dy = torch.empty_like(y)
    L.check(lib.ab_bn_relu_maxpool_bwd(L.ptr(dpool), L.ptr(idx), L.ptr(y), L.ptr(bnp), L.i(L.dt(y)), L.i(N), L.i(H), L.i(W),
                                       L.i(C), L.ptr(part), L.ptr(bwdp), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dy),
                                       L.stream()), "ab_bn_relu_maxpool_bwd")
    return dy


def bn_relu_maxpool_bwd_x3(dpool, idx, y, bnp, dgamma, dbeta, ywin=None):
    """Backward of bn_relu_maxpool_fwd on fp32 tensors -> dy as split planes [2, *y.shape], or None when the shape is not handled:
    the max-pool backward pass also masks and reduces (no separate BatchNorm-backward reduction over the full-size tensors).
    ywin (bn_relu_maxpool_fwd_x3(want_win=True)): the reduction runs over the pooled elements only."""
    N, H, W, C = y.shape
    lib = L.lib()
    if ywin is not None:
        part = torch.empty((lib.ab_col_stats_nparts(L.l(N * (H // 2) * (W // 2))), C, 2), dtype=torch.float32, device=y.device)
        bwdp = torch.empty((2, C), dtype=torch.float32, device=y.device)
        dy = torch.empty((2,) + tuple(y.shape), dtype=torch.bfloat16, device=y.device)
        L.check(lib.ab_bn_relu_maxpool_bwd_x3w(L.ptr(dpool), L.ptr(idx), L.ptr(ywin), L.ptr(y), L.ptr(bnp), L.i(N), L.i(H), L.i(W),
                                               L.i(C), L.ptr(part), L.ptr(bwdp), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dy[0]),
                                               L.ptr(dy[1]), L.stream()), "ab_bn_relu_maxpool_bwd_x3w")
        return dy
    np_ = lib.ab_bn_relu_maxpool_bwd_x3_nparts(L.i(N), L.i(H), L.i(W), L.i(C))
    if np_ <= 0:
        return None
    part = torch.empty((np_, C, 2), dtype=torch.float32, device=y.device)
    bwdp = torch.empty((2, C), dtype=torch.float32, device=y.device)
    dz = torch.empty_like(y)
    dy = torch.empty((2,) + tuple(y.shape), dtype=torch.bfloat16, device=y.device)
    L.check(lib.ab_bn_relu_maxpool_bwd_x3(L.ptr(dpool), L.ptr(idx), L.ptr(y), L.ptr(bnp), L.i(N), L.i(H), L.i(W), L.i(C),
                                          L.ptr(part), L.ptr(bwdp), L.ptr(dgamma), L.ptr(dbeta), L.ptr(dz), L.ptr(dy[0]),
                                          L.ptr(dy[1]), L.stream()), "ab_bn_relu_maxpool_bwd_x3")
    return dy


def maxpool_bwd(idx, dout, in_hw):
    N, Ho, Wo, C = dout.shape
    H, W = in_hw
    dx = _empty((N, H, W, C), dout)
    L.check(L.lib().ab_maxpool3x3s2_bwd(L.ptr(idx), L.ptr(dout), L.i(L.dt(dout)), L.i(N), L.i(H), L.i(W), L.i(C),
                                        L.ptr(dx), L.stream()), "ab_maxpool3x3s2_bwd")
    return dx


def avgpool_fwd(x):
    N, H, W, C = x.shape
    o = torch.empty((N, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().ab_avgpool_fwd(L.ptr(x), L.i(L.dt(x)), L.i(N), L.i(H * W), L.i(C), L.ptr(o), L.stream()),
            "ab_avgpool_fwd")
    return o


def avgpool_bwd(g, dx, accumulate):
    N, H, W, C = dx.shape
    L.check(L.lib().ab_avgpool_bwd(L.ptr(g), L.i(L.dt(dx)), L.i(N), L.i(H * W), L.i(C), L.ptr(dx),
                                   L.i(1 if accumulate else 0), L.stream()), "ab_avgpool_bwd")
    return dx


def cast_bf16(src_f32, dst_bf16):
    L.check(L.lib().ab_cast_f32_bf16(L.ptr(src_f32), L.l(src_f32.numel()), L.ptr(dst_bf16), L.stream()),
            "ab_cast_f32_bf16")
    return dst_bf16


def transpose_oki(src_f32_oki, dst):
    O, K, I = src_f32_oki.shape
    L.check(L.lib().ab_transpose_oki(L.ptr(src_f32_oki), L.i(O), L.i(K), L.i(I), L.i(L.dt(dst)), L.ptr(dst),
                                     L.stream()), "ab_transpose_oki")
    return dst


def linear_fwd(x, w, bias=None, relu=False):
    """fp32 x [M,K] @ w[N,K]^T (+bias) (+ReLU) -> [M,N]   (ab_linear_fwd; the box-rotation MLP)."""
    M, Kd = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    L.check(L.lib().ab_linear_fwd(L.ptr(x), L.ptr(w), L.ptr(bias), L.i(M), L.i(N), L.i(Kd), L.i(1 if relu else 0), L.ptr(y),
                                  L.stream()), "ab_linear_fwd")
    return y


def linear_dgrad(g, wt, act_out=None):
    """fp32 g [M,N] @ W[N,K] -> [M,K] given wt = W^T [K,N]; zeroed where act_out <= 0 (the ReLU that fed this layer)."""
    M, N = g.shape
    Kd = wt.shape[0]
    gx = torch.empty((M, Kd), dtype=torch.float32, device=g.device)
    L.check(L.lib().ab_linear_dgrad(L.ptr(g), L.ptr(wt), L.ptr(act_out), L.i(M), L.i(N), L.i(Kd), L.ptr(gx), L.stream()),
            "ab_linear_dgrad")
    return gx


def linear_wgrad(g, x, dw, db=None):
    """dw[N,K] = g[M,N]^T @ x[M,K], db[N] = sum_m g (written in place into the flat gradient views)."""
    M, N = g.shape
    Kd = x.shape[1]
    L.check(L.lib().ab_linear_wgrad(L.ptr(g), L.ptr(x), L.i(M), L.i(N), L.i(Kd), L.ptr(dw), L.ptr(db), L.stream()),
            "ab_linear_wgrad")


def transpose_plan(pairs):
    """pairs: [(src f32 [O,K,I], dst [I,K,O])] -> (device descriptor table, n, total_tiles, dtype code) for
    transpose_oki_batch; None when a shape does not fit the 16-byte vector tiles."""
    import numpy as np
    rec = np.zeros(len(pairs), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("O", "<i4"), ("K", "<i4"), ("I", "<i4"),
                                               ("tile_begin", "<i4")]))
    tiles = 0
    for n, (src, dst) in enumerate(pairs):
        O, Kk, I = src.shape
        if I % 4 or O % 8 or not src.is_contiguous() or not dst.is_contiguous() or dst.dtype != pairs[0][1].dtype:
            return None
        rec[n] = (src.data_ptr(), dst.data_ptr(), O, Kk, I, tiles)
        tiles += ((O + 63) // 64) * Kk * ((I + 63) // 64)
    dev = torch.from_numpy(rec.view(np.uint8).copy()).to(pairs[0][0].device)
    return dev, len(pairs), tiles, L.dt(pairs[0][1])


def transpose_oki_batch(plan):
    dev, n, tiles, dt = plan
    L.check(L.lib().ab_transpose_oki_batch(L.ptr(dev), L.i(n), L.l(tiles), L.i(dt), L.stream()), "ab_transpose_oki_batch")


def transpose_oki_batch_x3(plan, lo_offset_elems):
    """transpose_oki_batch with bf16 destinations written as split planes (lo plane `lo_offset_elems` behind the hi plane)."""
    dev, n, tiles, dt = plan
    assert dt == L.DT_BF16
    L.check(L.lib().ab_transpose_oki_batch_x3(L.ptr(dev), L.i(n), L.l(tiles), L.l(lo_offset_elems), L.stream()), "ab_transpose_oki_batch_x3")


def image_pad_nhwc4(img_nchw_f32, dtype):
    N, C, H, W = img_nchw_f32.shape
    assert C == 3
    out = torch.empty((N, H + 6, W + 8, 4), dtype=dtype, device=img_nchw_f32.device)
    L.check(L.lib().ab_image_pad_nhwc4(L.ptr(img_nchw_f32), L.i(L.dt(out)), L.i(N), L.i(H), L.i(W), L.ptr(out),
                                       L.stream()), "ab_image_pad_nhwc4")
    return out


def relu_bwd(dout, out):
    dz = torch.empty_like(dout)
    L.check(L.lib().ab_relu_bwd(L.ptr(dout), L.ptr(out), L.i(L.dt(dout)), L.l(dout.numel()), L.ptr(dz), L.stream()),
            "ab_relu_bwd")
    return dz


def col_sum(x, out):
    C = x.shape[-1]
    M = x.numel() // C
    lib = L.lib()
    part = torch.empty((lib.ab_col_stats_nparts(L.l(M)), C, 2), dtype=torch.float32, device=x.device)
    L.check(lib.ab_col_sum(L.ptr(x), L.i(L.dt(x)), L.l(M), L.i(C), L.ptr(part), L.ptr(out), L.stream()), "ab_col_sum")
    return out


# ---------------------------------------------------------------- split-bf16 ("bf16x3") convolutions
# A split tensor is a bf16 tensor [2, ...]: plane 0 = bf16(v), plane 1 = bf16(v - plane0) (include/artiboost_hip.h).

def split(x_f32, out=None):
    """fp32 tensor -> split planes [2, *x.shape] bf16 (ab_split_f32)."""
    if x_f32.dtype != torch.float32:
        raise TypeError("split() takes a float32 tensor")
    sp = out if out is not None else torch.empty((2,) + tuple(x_f32.shape), dtype=torch.bfloat16, device=x_f32.device)
    L.check(L.lib().ab_split_f32(L.ptr(x_f32), L.l(x_f32.numel()), L.ptr(sp[0]), L.ptr(sp[1]), L.stream()), "ab_split_f32")
    return sp


def _planes(t):
    """(hi, lo) of a split tensor, or of the planes cached on an fp32 tensor by its producer; splits on the fly otherwise."""
    if isinstance(t, tuple):
        return t
    if t.dtype == torch.bfloat16:
        return t[0], t[1]
    sp = getattr(t, "_ab_split", None)
    if sp is None:
        # NOT cached on the tensor: a persistent buffer (the static image of a replayed step) changes its contents between
        # calls, and a cached split would silently keep serving the first image.  Producers attach `_ab_split` to the FRESH
        # tensors they allocate; whoever feeds the same fp32 tensor to two convolutions splits it once itself.
        sp = split(t)
    return sp[0], sp[1]


def conv2d_fwd_x3(x, w_split, stride, pad, bias=None, want_stats=False, relu=False):
    """x: fp32 [N,H,W,Cin] or split [2,N,H,W,Cin]; w_split [2,Cout,kh,kw,Cin] -> y fp32 [N,Ho,Wo,Cout] (+ BN partials)."""
    xh, xl = _planes(x)
    N, H, W, Cin = xh.shape
    _, Cout, kh, kw, _ = w_split.shape
    if Cin % 32:        # the kernels read 32-channel chunks: zero planes up to the next chunk add exactly nothing to any output
        padc = -Cin % 32
        zpad = torch.nn.functional.pad
        xh, xl, w_split = zpad(xh, (0, padc)), zpad(xl, (0, padc)), zpad(w_split, (0, padc))
        Cin += padc
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    y = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=xh.device)
    lib = L.lib()
    stats = None
    if want_stats:
        nt = lib.ab_conv2d_x3_stat_rows(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad))
        stats = torch.empty((nt, Cout, 2), dtype=torch.float32, device=xh.device)
    L.check(lib.ab_conv2d_fwd_x3(L.ptr(xh), L.ptr(xl), L.ptr(w_split[0]), L.ptr(w_split[1]), L.ptr(y), L.i(N), L.i(H), L.i(W),
                                 L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(bias), L.ptr(stats),
                                 L.i(1 if relu else 0), L.stream()), "ab_conv2d_fwd_x3")
    return (y, stats) if want_stats else y


def conv1x1_sam_fwd_x3_ok(x, w_split, C, D, DP):
    """True when ab_conv1x1_sam_fwd_x3 takes the final layer's shape (DEPTH_PITCH 32, Cin % 64 == 0, <= 256, H * W % 64 == 0)."""
    xh, _ = _planes(x) if x.dtype == torch.bfloat16 else (x, None)
    N, H, W, Cin = xh.shape
    return DP == 32 and tuple(w_split.shape[1:]) == (C * 32, 1, 1, Cin) and \
        bool(L.lib().ab_conv1x1_sam_fwd_x3_ok(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(C), L.i(D)))


def conv1x1_sam_fwd_x3(x, w_split, bias, C, D):
    """Final layer + soft-argmax stage 1 (ab_conv1x1_sam_fwd_x3): x fp32 / split [.., N,H,W,Cin], w_split [2, C*32, 1, 1, Cin] ->
    (logits fp32 [N,H,W,C*32], part fp32 [N, H*W/64, C, 8])."""
    xh, xl = _planes(x)
    N, H, W, Cin = xh.shape
    y = torch.empty((N, H, W, C * 32), dtype=torch.float32, device=xh.device)
    part = torch.empty((N, H * W // 64, C, 8), dtype=torch.float32, device=xh.device)
    L.check(L.lib().ab_conv1x1_sam_fwd_x3(L.ptr(xh), L.ptr(xl), L.ptr(w_split[0]), L.ptr(w_split[1]), L.ptr(bias), L.ptr(y), L.i(N), L.i(H),
                                          L.i(W), L.i(Cin), L.i(C), L.i(D), L.ptr(part), L.stream()), "ab_conv1x1_sam_fwd_x3")
    return y, part


def conv2d_fwd_x3_evalbn_ok(x, w_split):
    xh = x[0] if x.dtype == torch.bfloat16 else x
    N, H, W, Cin = xh.shape
    _, Cout, kh, kw, _ = w_split.shape
    return (kh, kw) == (3, 3) and bool(L.lib().ab_conv2d_fwd_x3_evalbn_ok(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout)))


def conv2d_fwd_x3_evalbn(x, w_split, bnp, res=None, relu=True, want_f32=False):
    """Eval-mode 3x3/s1 convolution + the BatchNorm after it (+ residual, ReLU) in one launch -> split planes [2,N,H,W,Cout]
    (want_f32: the fp32 tensor with the planes cached on it, as bn_apply_x3 returns).  res: split planes, fp32 tensor or None."""
    xh, xl = _planes(x)
    N, H, W, Cin = xh.shape
    Cout = w_split.shape[1]
    sp = torch.empty((2, N, H, W, Cout), dtype=torch.bfloat16, device=xh.device)
    o = torch.empty((N, H, W, Cout), dtype=torch.float32, device=xh.device) if want_f32 else None
    rh = rl = rf = None
    if res is not None:
        if res.dtype == torch.bfloat16:
            rh, rl = res[0], res[1]
        else:
            rf = res
    L.check(L.lib().ab_conv2d_fwd_x3_evalbn(L.ptr(xh), L.ptr(xl), L.ptr(w_split[0]), L.ptr(w_split[1]), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                            L.i(Cout), L.ptr(bnp), L.ptr(rh), L.ptr(rl), L.ptr(rf), L.i(1 if relu else 0), L.ptr(sp[0]),
                                            L.ptr(sp[1]), L.ptr(o), L.stream()), "ab_conv2d_fwd_x3_evalbn")
    if o is None:
        return sp
    o._ab_split = sp
    return o


def conv2d_fwd_x3_affine(x, w_split, bnp, stride, pad, relu=True, planes=True):
    """Eval-mode generic convolution + following BatchNorm (+ ReLU) in the epilogue -> split planes [2,N,Ho,Wo,Cout] or fp32 [N,Ho,Wo,Cout]."""
    xh, xl = _planes(x)
    N, H, W, Cin = xh.shape
    _, Cout, kh, kw, _ = w_split.shape
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    sp = torch.empty((2, N, Ho, Wo, Cout), dtype=torch.bfloat16, device=xh.device) if planes else None
    o = None if planes else torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=xh.device)
    L.check(L.lib().ab_conv2d_fwd_x3_affine(L.ptr(xh), L.ptr(xl), L.ptr(w_split[0]), L.ptr(w_split[1]), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout),
                                            L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(bnp[0]), L.ptr(bnp[1]), L.i(1 if relu else 0), L.ptr(o),
                                            L.ptr(sp[0] if planes else None), L.ptr(sp[1] if planes else None), L.stream()), "ab_conv2d_fwd_x3_affine")
    return sp if planes else o


def conv2d_dgrad_x3_affine(dy, wt_split, in_hw, stride, pad, bnp, relu=True):
    """Eval-mode transposed convolution (data-gradient form) + following BatchNorm (+ ReLU) -> split planes [2,N,H,W,Cin]."""
    dh, dl = _planes(dy)
    N, Ho, Wo, Cout = dh.shape
    _, Cin, kh, kw, _ = wt_split.shape
    H, W = in_hw
    sp = torch.empty((2, N, H, W, Cin), dtype=torch.bfloat16, device=dh.device)
    L.check(L.lib().ab_conv2d_dgrad_x3_affine(L.ptr(dh), L.ptr(dl), L.ptr(wt_split[0]), L.ptr(wt_split[1]), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                              L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(bnp[0]), L.ptr(bnp[1]), L.i(1 if relu else 0),
                                              L.ptr(None), L.ptr(sp[0]), L.ptr(sp[1]), L.stream()), "ab_conv2d_dgrad_x3_affine")
    return sp


def _relu_mask(bn_out):
    """The ReLU mask of the fused BatchNorm-backward epilogues: the hi plane of the stored activation `bn_out` (split planes, or an fp32
    tensor that carries them as `_ab_split`) -> (mask, True); (None, True) when there is no activation to mask with (the epilogue
    recomputes relu(bn(y))); (None, False) when the activation was kept without its planes and the epilogue cannot be used."""
    if bn_out is None:
        return None, True
    sp = bn_out if bn_out.dtype == torch.bfloat16 else getattr(bn_out, "_ab_split", None)
    return (None, False) if sp is None else (sp[0], True)


def conv2d_dgrad_x3(dy, wt_split, in_hw, stride, pad, addend=None, want_stats=False, bn=None):
    """dy: fp32 / split [.., N,Ho,Wo,Cout]; wt_split [2,Cin,kh,kw,Cout] -> dx fp32 [N,H,W,Cin] (+ BN partials of dx).

    bn=(bn_y, bn_out_or_None, bnp): dx is the gradient arriving at relu(bn(bn_y) [+ residual]).  Returns (dx, part): where the
    kernel can, dx is already MASKED (dz) and `part` holds the BatchNorm-backward partial sums of its epilogue (pass it to
    bn_bwd_x3(part=..., premasked=True)); otherwise part is None and dx the raw gradient."""
    dh, dl = _planes(dy)
    N, Ho, Wo, Cout = dh.shape
    _, Cin, kh, kw, _ = wt_split.shape
    H, W = in_hw
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dh.device)
    lib = L.lib()
    part = None
    if bn is not None:
        bn_y, bn_out, bnp = bn
        rows = lib.ab_conv2d_dgrad_x3_bn_rows(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad))
        mask, has_mask = _relu_mask(bn_out)
        if rows > 0 and has_mask:
            part = torch.empty((rows, Cin, 2), dtype=torch.float32, device=dh.device)
            L.check(lib.ab_conv2d_dgrad_x3_bn(L.ptr(dh), L.ptr(dl), L.ptr(wt_split[0]), L.ptr(wt_split[1]), L.ptr(dx), L.i(N),
                                              L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad),
                                              L.ptr(addend), L.ptr(bn_y), L.ptr(mask), L.ptr(bnp), L.ptr(part), L.stream()),
                    "ab_conv2d_dgrad_x3_bn")
            return dx, part
    if want_stats and addend is None:
        rows = lib.ab_conv2d_dgrad_x3_stat_rows(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad))
        if rows > 0:
            part = torch.empty((rows, Cin, 2), dtype=torch.float32, device=dh.device)
    L.check(lib.ab_conv2d_dgrad_x3(L.ptr(dh), L.ptr(dl), L.ptr(wt_split[0]), L.ptr(wt_split[1]), L.ptr(dx), L.i(N), L.i(H), L.i(W),
                                   L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(addend), L.ptr(part),
                                   L.stream()), "ab_conv2d_dgrad_x3")
    if want_stats:
        return dx, (part if part is not None else col_stats(dx))
    return (dx, None) if bn is not None else dx


def conv2d_dgrad_x3_pair(dy, wt_split, dy2, wt2_split, in_hw, pad, addend=None, bn=None):
    """dx = dgrad(dy, wt; k x k / stride 2) + dgrad(dy2, wt2; 1x1 / stride 2 / pad 0) [+ addend] in one launch: the conv1 and
    downsample branches of a down-sampling block (anakin/models/resnet.py:85-101 backwards).

    bn=(bn_y, bn_out_or_None, bnp) (no addend): dx is the gradient arriving at relu(bn(bn_y) [+ residual]), the output of the stage below.
    Returns (dx, part) as conv2d_dgrad_x3(bn=...) does: masked dx + the BatchNorm-backward partial rows where the kernel can, else (dx, None)."""
    dh, dl = _planes(dy)
    eh, el = _planes(dy2)
    N, Ho, Wo, Cout = dh.shape
    _, Cin, kh, kw, _ = wt_split.shape
    assert tuple(eh.shape) == tuple(dh.shape) and tuple(wt2_split.shape[1:]) == (Cin, 1, 1, Cout)
    H, W = in_hw
    dx = torch.empty((N, H, W, Cin), dtype=torch.float32, device=dh.device)
    lib = L.lib()
    if bn is not None and addend is None:
        bn_y, bn_out, bnp = bn
        rows = lib.ab_conv2d_dgrad_x3_pair_bn_rows(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(pad))
        mask, has_mask = _relu_mask(bn_out)
        if rows > 0 and has_mask:
            part = torch.empty((rows, Cin, 2), dtype=torch.float32, device=dh.device)
            L.check(lib.ab_conv2d_dgrad_x3_pair_bn(L.ptr(dh), L.ptr(dl), L.ptr(wt_split[0]), L.ptr(wt_split[1]), L.ptr(eh), L.ptr(el),
                                                   L.ptr(wt2_split[0]), L.ptr(wt2_split[1]), L.ptr(dx), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                                   L.i(Cout), L.i(kh), L.i(kw), L.i(pad), L.ptr(bn_y), L.ptr(mask), L.ptr(bnp), L.ptr(part),
                                                   L.stream()), "ab_conv2d_dgrad_x3_pair_bn")
            return dx, part
    L.check(lib.ab_conv2d_dgrad_x3_pair(L.ptr(dh), L.ptr(dl), L.ptr(wt_split[0]), L.ptr(wt_split[1]), L.ptr(eh), L.ptr(el),
                                        L.ptr(wt2_split[0]), L.ptr(wt2_split[1]), L.ptr(dx), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                        L.i(Cout), L.i(kh), L.i(kw), L.i(pad), L.ptr(addend), L.stream()),
            "ab_conv2d_dgrad_x3_pair")
    return (dx, None) if bn is not None else dx


def conv2d_wgrad_x3(x, dy, kh, kw, stride, pad, out=None, accumulate=False, defer=None):
    """x, dy: fp32 or split -> dw fp32 [Cout,kh,kw,Cin].  defer: see conv2d_wgrad."""
    xh, xl = _planes(x)
    dh, dl = _planes(dy)
    N, H, W, Cin = xh.shape
    Cout = dh.shape[3]
    lib = L.lib()
    nbytes = lib.ab_conv2d_wgrad_x3_workspace(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad))
    if nbytes <= 0:
        raise RuntimeError(f"conv2d_wgrad_x3: shape not handled (Cin {Cin}, Cout {Cout}, {kh}x{kw})")
    dw = out if out is not None else torch.empty((Cout, kh, kw, Cin), dtype=torch.float32, device=xh.device)
    if defer is not None:
        ws, d = defer.new(nbytes, xh.device)
        L.check(lib.ab_conv2d_wgrad_x3_deferred(L.ptr(xh), L.ptr(xl), L.ptr(dh), L.ptr(dl), L.ptr(dw), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                                L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(ws), L.i(1 if accumulate else 0),
                                                ctypes.byref(d), L.stream()), "ab_conv2d_wgrad_x3_deferred")
        return dw
    ws = _workspace(nbytes, xh.device)
    L.check(lib.ab_conv2d_wgrad_x3(L.ptr(xh), L.ptr(xl), L.ptr(dh), L.ptr(dl), L.ptr(dw), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                   L.i(Cout), L.i(kh), L.i(kw), L.i(stride), L.i(pad), L.ptr(ws), L.i(1 if accumulate else 0),
                                   L.stream()), "ab_conv2d_wgrad_x3")
    return dw


WGRAD_GROUP_MAX = 8


def conv2d_wgrad_x3_group_ok(x, dy, G):
    """True when ab_conv2d_wgrad_x3_group takes G layers of this shape (3x3 / stride 1 / pad 1 on wgrad3x3.hip's map sizes)."""
    xh, dh = _planes(x)[0], _planes(dy)[0]
    N, H, W, Cin = xh.shape
    return dh.shape[:3] == xh.shape[:3] and 1 <= G <= WGRAD_GROUP_MAX and \
        L.lib().ab_conv2d_wgrad_x3_group_workspace(L.i(G), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(dh.shape[3])) > 0


def conv2d_wgrad_x3_group(items, accumulate=False):
    """items: [(x, dy, out)] of ONE shape (3x3 / stride 1 / pad 1; x, dy fp32 or split; out fp32 [Cout,3,3,Cin]) -> the G weight gradients
    from one slab launch + one reduction launch (ab_conv2d_wgrad_x3_group)."""
    G = len(items)
    planes = [(_planes(x), _planes(dy), out) for x, dy, out in items]
    (xh, _), (dh, _), _ = planes[0]
    N, H, W, Cin = xh.shape
    Cout = dh.shape[3]
    lib = L.lib()
    nbytes = lib.ab_conv2d_wgrad_x3_group_workspace(L.i(G), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout))
    if nbytes <= 0:
        raise RuntimeError(f"conv2d_wgrad_x3_group: shape not handled ({G} x [{N},{H},{W},{Cin}] -> {Cout})")
    arr = (L.WgradGroupItem * G)()
    for i, ((a, b), (c, d), out) in enumerate(planes):
        assert a.shape == xh.shape and c.shape == dh.shape and out.dtype == torch.float32 and out.numel() == Cout * 9 * Cin and out.is_contiguous()
        arr[i].x_hi, arr[i].x_lo, arr[i].dy_hi, arr[i].dy_lo, arr[i].dw = a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), out.data_ptr()
    ws = _workspace(nbytes, xh.device)
    L.check(lib.ab_conv2d_wgrad_x3_group(arr, L.i(G), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.ptr(ws), L.i(1 if accumulate else 0),
                                         L.stream()), "ab_conv2d_wgrad_x3_group")
    return [out for _, _, out in planes]


def bn_apply_x3(y, bnp, res=None, relu=True, want_f32=False, res_bnp=None):
    """fp32 y -> split planes [2, *y.shape] of relu(bn(y) + res); want_f32: also the fp32 tensor (returned, with the planes
    cached on it as `_ab_split`) -- needed where the activation is a residual input or a ReLU mask in the backward.
    res_bnp: `res` is the raw output of the downsample conv and the residual is its BatchNorm (scale, shift) applied on the fly."""
    C = y.shape[-1]
    M = y.numel() // C
    sp = torch.empty((2,) + tuple(y.shape), dtype=torch.bfloat16, device=y.device)
    o = torch.empty_like(y) if want_f32 else None
    if res is not None and res.dtype == torch.bfloat16:      # the residual as (hi, lo) planes
        assert res_bnp is None
        L.check(L.lib().ab_bn_apply_x3_respl(L.ptr(y), L.ptr(res[0]), L.ptr(res[1]), L.ptr(bnp), L.l(M), L.i(C), L.i(1 if relu else 0),
                                             L.ptr(o), L.ptr(sp[0]), L.ptr(sp[1]), L.stream()), "ab_bn_apply_x3_respl")
    elif res_bnp is not None:
        L.check(L.lib().ab_bn_apply_x3_resbn(L.ptr(y), L.ptr(res), L.ptr(bnp), L.ptr(res_bnp), L.l(M), L.i(C), L.i(1 if relu else 0),
                                             L.ptr(o), L.ptr(sp[0]), L.ptr(sp[1]), L.stream()), "ab_bn_apply_x3_resbn")
    else:
        L.check(L.lib().ab_bn_apply_x3(L.ptr(y), L.ptr(res), L.ptr(bnp), L.l(M), L.i(C), L.i(1 if relu else 0), L.ptr(o),
                                       L.ptr(sp[0]), L.ptr(sp[1]), L.stream()), "ab_bn_apply_x3")
    if o is None:
        return sp
    o._ab_split = sp
    return o


def bn_fin_apply_x3_ok(part, C):
    """True when ab_bn_fin_apply_x3 takes this BatchNorm (few partial rows, C % 64 == 0): finalize and apply in one launch."""
    return part is not None and bool(L.lib().ab_bn_fin_apply_x3_ok(L.i(part.shape[0]), L.i(C)))


def bn_fin_apply_x3(y, part, count, gamma, beta, running_mean=None, running_var=None, res=None, relu=True, want_f32=False, res_bnp=None,
                    eps=1e-5, momentum=0.1):
    """bn_finalize + bn_apply_x3 in ONE launch (see ab_bn_fin_apply_x3) -> (activation as bn_apply_x3 returns it, bnp [4, C])."""
    C = y.shape[-1]
    M = y.numel() // C
    bnp = torch.empty((4, C), dtype=torch.float32, device=y.device)
    sp = torch.empty((2,) + tuple(y.shape), dtype=torch.bfloat16, device=y.device)
    o = torch.empty_like(y) if want_f32 else None
    rh = rl = rf = None
    if res is not None and res.dtype == torch.bfloat16:
        assert res_bnp is None
        rh, rl = res[0], res[1]
    else:
        rf = res
    L.check(L.lib().ab_bn_fin_apply_x3(L.ptr(part), L.i(part.shape[0]), L.l(count), L.ptr(gamma), L.ptr(beta), L.f(eps), L.f(momentum),
                                       L.ptr(running_mean), L.ptr(running_var), L.ptr(bnp), L.ptr(y), L.ptr(rf), L.ptr(rh), L.ptr(rl),
                                       L.ptr(res_bnp), L.l(M), L.i(C), L.i(1 if relu else 0), L.ptr(o), L.ptr(sp[0]), L.ptr(sp[1]), L.stream()),
            "ab_bn_fin_apply_x3")
    if o is None:
        return sp, bnp
    o._ab_split = sp
    return o, bnp


def bn_bwd_x3(dout, out, y, bnp, dgamma, dbeta, relu=True, want_dz=False, part=None, premasked=False):
    """As bn_bwd on fp32 tensors, with dy returned as split planes [2, *y.shape] (-> dy [, dz fp32]).
    premasked (with part): `dout` is already the masked gradient dz and `part` its reduction (conv2d_dgrad_x3(bn=...))."""
    if premasked:
        assert part is not None
        dy = bn_bwd_x3(dout, None, y, bnp, dgamma, dbeta, relu=False, part=part)
        return (dy, dout) if want_dz else dy
    C = y.shape[-1]
    M = y.numel() // C
    lib = L.lib()
    bwdp = torch.empty((2, C), dtype=torch.float32, device=y.device)
    dy = torch.empty((2,) + tuple(y.shape), dtype=torch.bfloat16, device=y.device)
    dz = torch.empty_like(y) if want_dz else None
    given = 0
    if part is None:
        part = torch.empty((lib.ab_col_stats_nparts(L.l(M)), C, 2), dtype=torch.float32, device=y.device)
    else:
        given = part.shape[0]
    mask, is_hi = (out if relu is True else None), 0
    if mask is not None and mask.dtype == torch.bfloat16:
        mask, is_hi = mask[0], 1                     # the activation exists only as planes
    elif mask is not None and getattr(mask, "_ab_split", None) is not None:
        mask, is_hi = mask._ab_split[0], 1          # sign of the hi plane == sign of the activation; half the bytes
    L.check(lib.ab_bn_bwd_x3(L.ptr(dout), L.ptr(mask), L.i(is_hi), L.ptr(y), L.ptr(bnp), L.l(M), L.i(C),
                             L.i(2 if relu == "recompute" else 1 if relu else 0), L.ptr(part), L.i(given), L.ptr(bwdp),
                             L.ptr(dgamma), L.ptr(dbeta), L.ptr(dy[0]), L.ptr(dy[1]), L.ptr(dz), L.stream()), "ab_bn_bwd_x3")
    return (dy, dz) if want_dz else dy


def _image_planes(xpad):
    """(hi, lo) planes of the padded image, or (plane, None) for the integer plane 2 v - 255 the loaders write with AB_DT_U8N
    (bf16 [N, H+6, W+8, 4]: the network input is plane / 510; ab_conv2d_stem_*_x3 take it with xpad_lo = NULL)."""
    if xpad.dtype == torch.bfloat16 and xpad.dim() == 4:
        return xpad, None
    return _planes(xpad)


def conv2d_stem_fwd_x3(xpad, w_split, H, W, want_stats=False):
    """xpad fp32 / split [.., N,H+6,W+8,4] / integer plane (see _image_planes), w_split [2,64,7,8,4] -> y fp32 [N,H/2,W/2,64] (+ BN partials)."""
    xh, xl = _image_planes(xpad)
    N = xh.shape[0]
    Cout = w_split.shape[1]
    y = torch.empty((N, H // 2, W // 2, Cout), dtype=torch.float32, device=xh.device)
    lib = L.lib()
    stats = None
    if want_stats:
        stats = torch.empty((lib.ab_conv2d_stem_x3_stat_rows(L.i(N), L.i(H), L.i(W)), Cout, 2), dtype=torch.float32, device=xh.device)
    L.check(lib.ab_conv2d_stem_fwd_x3(L.ptr(xh), L.ptr(xl), L.ptr(w_split[0]), L.ptr(w_split[1]), L.ptr(y), L.i(N), L.i(H), L.i(W),
                                      L.i(Cout), L.ptr(stats), L.stream()), "ab_conv2d_stem_fwd_x3")
    return (y, stats) if want_stats else y


def conv2d_stem_wgrad_x3(xpad, dy, H, W, out=None, defer=None):
    xh, xl = _image_planes(xpad)
    dh, dl = _planes(dy)
    N = xh.shape[0]
    Cout = dh.shape[3]
    lib = L.lib()
    nbytes = lib.ab_conv2d_stem_wgrad_workspace(L.i(N), L.i(H), L.i(W), L.i(Cout))
    dw = out if out is not None else torch.empty((Cout, 7, 8, 4), dtype=torch.float32, device=xh.device)
    if defer is not None:
        ws, d = defer.new(nbytes, xh.device)
        L.check(lib.ab_conv2d_stem_wgrad_x3_deferred(L.ptr(xh), L.ptr(xl), L.ptr(dh), L.ptr(dl), L.ptr(dw), L.i(N), L.i(H), L.i(W),
                                                     L.i(Cout), L.ptr(ws), ctypes.byref(d), L.stream()), "ab_conv2d_stem_wgrad_x3_deferred")
        return dw
    ws = _workspace(nbytes, xh.device)
    L.check(lib.ab_conv2d_stem_wgrad_x3(L.ptr(xh), L.ptr(xl), L.ptr(dh), L.ptr(dl), L.ptr(dw), L.i(N), L.i(H), L.i(W), L.i(Cout),
                                        L.ptr(ws), L.stream()), "ab_conv2d_stem_wgrad_x3")
    return dw


def col_sum_x3(x_split, out):
    """Column sums of a split tensor [2, ..., C] (hi + lo) -> out fp32 [C]."""
    C = x_split.shape[-1]
    M = x_split[0].numel() // C
    lib = L.lib()
    part = torch.empty((lib.ab_col_stats_nparts(L.l(M)), C, 2), dtype=torch.float32, device=x_split.device)
    L.check(lib.ab_col_sum_x3(L.ptr(x_split[0]), L.ptr(x_split[1]), L.l(M), L.i(C), L.ptr(part), L.ptr(out), L.stream()), "ab_col_sum_x3")
    return out


def pose_assemble(kp3d, box6d, root_joint, cam_intr, corners_can, center_idx, inp_res):
    """hybridbaseline.py:49-96 in one launch (eval-mode forwards): kp3d [B,22,3] f32, box6d [B,>=6] (row-pitched view allowed),
    -> dict of the module's geometric outputs."""
    B, dev = kp3d.shape[0], kp3d.device
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
    o = dict(joints_3d_abs=z(B, 21, 3), corners_3d_abs=z(B, 8, 3), box_rot_rotmat=z(B, 3, 3), uvd2d=z(B, 30, 3), joints_3d=z(B, 21, 3),
             corners_3d=z(B, 8, 3), boxroot_3d_abs=z(B, 1, 3))
    L.check(L.lib().ab_pose_assemble(L.ptr(kp3d), L.view_ptr(box6d), L.i(box6d.stride(0)), L.ptr(root_joint), L.ptr(cam_intr), L.ptr(corners_can),
                                     L.i(B), L.i(center_idx), L.f(inp_res[0]), L.f(inp_res[1]), L.ptr(o["joints_3d_abs"]),
                                     L.ptr(o["corners_3d_abs"]), L.ptr(o["box_rot_rotmat"]), L.ptr(o["uvd2d"]), L.ptr(o["joints_3d"]),
                                     L.ptr(o["corners_3d"]), L.ptr(o["boxroot_3d_abs"]), L.stream()), "ab_pose_assemble")
    return o


def _mano_tables(t):
    """t: dict of the MANO tables on the device (fp32, contiguous) -> the pointer arguments shared by the ab_mano_pca_* launches."""
    return (L.ptr(t["comps"]), L.ptr(t["hands_mean"]), L.ptr(t["v_template"]), L.ptr(t["shapedirs"]), L.ptr(t["posedirs"]),
            L.ptr(t["J_regressor"]), L.ptr(t["weights"]))


def mano_pca_fwd(pose_coeffs, betas, tables, center_idx=None):
    """MANO from PCA coefficients (ab_mano_pca_fwd): pose_coeffs [B,3+ncomps], betas [B,10] fp32; tables: comps [ncomps,45],
    hands_mean [45], v_template, shapedirs, posedirs, J_regressor, weights -> verts [B,778,3], joints [B,21,3] (minus joint
    center_idx unless None), full_pose [B,48]."""
    B, P = pose_coeffs.shape
    dev = pose_coeffs.device
    verts = torch.empty((B, 778, 3), dtype=torch.float32, device=dev)
    joints = torch.empty((B, 21, 3), dtype=torch.float32, device=dev)
    full = torch.empty((B, 48), dtype=torch.float32, device=dev)
    L.check(L.lib().ab_mano_pca_fwd(L.ptr(pose_coeffs), L.ptr(betas), *_mano_tables(tables), L.i(P - 3),
                                    L.i(-1 if center_idx is None else center_idx), L.i(B), L.ptr(verts), L.ptr(joints), L.ptr(full),
                                    L.stream()), "ab_mano_pca_fwd")
    return verts, joints, full


def mano_pca_bwd(pose_coeffs, betas, tables, g_verts, g_joints, g_full_pose=None, center_idx=None):
    """Reverse of mano_pca_fwd (ab_mano_pca_bwd): -> g_pose_coeffs [B,3+ncomps], g_betas [B,10] (fixed-order reductions: bit-reproducible)."""
    B, P = pose_coeffs.shape
    dev = pose_coeffs.device
    g_pc = torch.empty((B, P), dtype=torch.float32, device=dev)
    g_b = torch.empty((B, 10), dtype=torch.float32, device=dev)
    L.check(L.lib().ab_mano_pca_bwd(L.ptr(pose_coeffs), L.ptr(betas), *_mano_tables(tables), L.i(P - 3),
                                    L.i(-1 if center_idx is None else center_idx), L.i(B), L.ptr(g_verts), L.ptr(g_joints),
                                    L.ptr(g_full_pose), L.ptr(g_pc), L.ptr(g_b), L.stream()), "ab_mano_pca_bwd")
    return g_pc, g_b


HONET_FWD_OUT = ("root_joint", "joints_3d_abs", "hand_verts_3d_abs", "joints_2d", "hand_verts_2d", "obj_center", "box_rot_rotmat",
                 "obj_verts_3d_abs", "obj_verts_2d", "corners_3d_abs", "corners_2d", "corners_3d", "obj_verts_3d")


def _honet_rows(t, w, what):
    """A [B, >= w] fp32 view whose rows are addressed through their pitch: -> the pitch in floats."""
    if t.dim() != 2 or t.shape[1] < w or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what} must be fp32 rows of at least {w} unit-stride columns, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0)


def _honet_inputs(hand_st, obj_st, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, factors, image_size, off_z):
    B, N = obj_verts_can.shape[0], obj_verts_can.shape[1]
    for t, shp, what in ((cam_intr, (B, 3, 3), "cam_intr"), (joints_3d, (B, 21, 3), "joints_3d"), (hand_verts_3d, (B, 778, 3), "hand_verts_3d"),
                         (obj_verts_can, (B, N, 3), "obj_verts_can"), (corners_can, (B, 8, 3), "corners_can")):
        if t is not None and (t.numel() != shp[0] * shp[1] * shp[2] or t.dtype != torch.float32):
            raise ValueError(f"honet_recover: {what} must be fp32 {shp}, got {t.dtype} {tuple(t.shape)}")
    if hand_st.shape[0] != B or obj_st.shape[0] != B or N < 1:
        raise ValueError(f"honet_recover: {hand_st.shape[0]} / {obj_st.shape[0]} head rows for {B} samples of {N} vertices")
    hp, op = _honet_rows(hand_st, 3, "hand_st"), _honet_rows(obj_st, 6, "obj_st")
    return B, N, (L.view_ptr(hand_st), L.i(hp), L.view_ptr(obj_st), L.i(op), L.ptr(cam_intr), L.ptr(joints_3d), L.ptr(hand_verts_3d),
                  L.ptr(obj_verts_can), L.ptr(corners_can), L.i(B), L.i(N), L.f(factors[0]), L.f(factors[1]), L.f(image_size[0]),
                  L.f(image_size[1]), L.f(off_z))


def honet_recover_fwd(hand_st, obj_st, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, factors, image_size, off_z=0.4,
                      want_rel_verts=True):
    """HoNet's recovery stage (ab_honet_recover_fwd).  hand_st [B, >= 3] / obj_st [B, >= 6]: fp32 row views (any row pitch) of the
    TransHeads' outputs; cam_intr [B,3,3]; joints_3d [B,21,3], hand_verts_3d [B,778,3]; obj_verts_can [B,N,3]; corners_can [B,8,3] or
    None; factors (OBJ_TRANS_FACTOR, OBJ_SCALE_FACTOR); image_size (width, height).  -> dict of HONET_FWD_OUT (the model's key names;
    root_joint / obj_center [B,1,3], box_rot_rotmat [B,3,3]); the corner entries are None without corners_can, obj_verts_3d without
    want_rel_verts."""
    B, N, args = _honet_inputs(hand_st, obj_st, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, factors, image_size, off_z)
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=obj_verts_can.device)      # noqa: E731
    cz = (lambda *s: z(*s)) if corners_can is not None else (lambda *s: None)
    o = dict(root_joint=z(B, 1, 3), joints_3d_abs=z(B, 21, 3), hand_verts_3d_abs=z(B, 778, 3), joints_2d=z(B, 21, 2), hand_verts_2d=z(B, 778, 2),
             obj_center=z(B, 1, 3), box_rot_rotmat=z(B, 3, 3), obj_verts_3d_abs=z(B, N, 3), obj_verts_2d=z(B, N, 2), corners_3d_abs=cz(B, 8, 3),
             corners_2d=cz(B, 8, 2), corners_3d=cz(B, 8, 3), obj_verts_3d=z(B, N, 3) if want_rel_verts else None)
    L.check(L.lib().ab_honet_recover_fwd(*args, *(L.ptr(o[k]) for k in HONET_FWD_OUT), L.stream()), "ab_honet_recover_fwd")
    return o


def honet_recover_bwd(hand_st, obj_st, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, factors, image_size, grads, off_z=0.4,
                      g_hand_st=None, g_obj_st=None):
    """Reverse of honet_recover_fwd (ab_honet_recover_bwd).  grads: {HONET_FWD_OUT name: gradient or None / absent = zero}.
    g_hand_st / g_obj_st: optional fp32 row views to write the (scale, trans) / (scale, trans, axis-angle) gradients into (their first
    3 / 6 columns; the rest is not touched); allocated dense when None.  -> (g_hand_st, g_obj_st, g_joints_3d [B,21,3],
    g_hand_verts_3d [B,778,3]).  Fixed-order reductions: bit-reproducible."""
    B, N, args = _honet_inputs(hand_st, obj_st, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, factors, image_size, off_z)
    dev = obj_verts_can.device
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    g_hand_st = z(B, 3) if g_hand_st is None else g_hand_st
    g_obj_st = z(B, 6) if g_obj_st is None else g_obj_st
    if g_hand_st.shape[0] != B or g_obj_st.shape[0] != B:
        raise ValueError("honet_recover_bwd: g_hand_st / g_obj_st need one row per sample")
    ghp, gop = _honet_rows(g_hand_st, 3, "g_hand_st"), _honet_rows(g_obj_st, 6, "g_obj_st")
    gs = []
    for k in HONET_FWD_OUT:
        g = grads.get(k)
        if g is not None:
            want = B * {"root_joint": 3, "obj_center": 3, "box_rot_rotmat": 9, "joints_3d_abs": 63, "joints_2d": 42, "hand_verts_3d_abs": 2334,
                        "hand_verts_2d": 1556, "obj_verts_3d_abs": 3 * N, "obj_verts_3d": 3 * N, "obj_verts_2d": 2 * N, "corners_3d_abs": 24,
                        "corners_3d": 24, "corners_2d": 16}[k]
            if g.numel() != want or g.dtype != torch.float32:
                raise ValueError(f"honet_recover_bwd: gradient of {k} must be fp32 with {want} elements, got {g.dtype} {tuple(g.shape)}")
            if corners_can is None and k.startswith("corners"):
                raise ValueError(f"honet_recover_bwd: a gradient of {k} without corners_can")
        gs.append(L.ptr(g))
    g_j, g_v = z(B, 21, 3), z(B, 778, 3)
    ws = torch.empty((L.lib().ab_honet_recover_workspace(L.i(B), L.i(N)),), dtype=torch.uint8, device=dev)
    L.check(L.lib().ab_honet_recover_bwd(*args, *gs, L.view_ptr(g_hand_st), L.i(ghp), L.view_ptr(g_obj_st), L.i(gop), L.ptr(g_j), L.ptr(g_v),
                                         L.ptr(ws), L.stream()), "ab_honet_recover_bwd")
    return g_hand_st, g_obj_st, g_j, g_v


def mesh_queries(table, obj_id, obj_transf, root_joint, hand_verts, samples, pose_offset, out=None):
    """ab_mesh_queries: synth.add_mesh_queries in one capturable launch.  table [n_obj,n,3] f32, obj_id int64 [B], obj_transf [B,4,4],
    root_joint [B,3], hand_verts [B,778,3] f32; samples: the uint8 [B, pitch] render records, whose `obj_pose` field at byte pose_offset is
    read in place.  out: (obj_verts_can [B,n,3], obj_verts_3d [B,n,3], hand_verts_3d [B,778,3]) to write into (allocated when None)."""
    B, n = obj_id.shape[0], table.shape[1]
    if samples.dtype != torch.uint8 or samples.dim() != 2 or samples.shape[0] != B or obj_id.dtype != torch.int64:
        raise ValueError(f"mesh_queries: samples must be uint8 [{B}, pitch] and obj_id int64, got {samples.dtype} {tuple(samples.shape)} / {obj_id.dtype}")
    for t, numel, what in ((table, table.shape[0] * n * 3, "table"), (obj_transf, B * 16, "obj_transf"), (root_joint, B * 3, "root_joint"),
                           (hand_verts, B * 778 * 3, "hand_verts")):
        if t.dtype != torch.float32 or t.numel() != numel:
            raise ValueError(f"mesh_queries: {what} must be fp32 with {numel} elements, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=table.device)      # noqa: E731
        out = (z(B, n, 3), z(B, n, 3), z(B, 778, 3))
    can, v3d, hv = out
    if tuple(can.shape) != (B, n, 3) or tuple(v3d.shape) != (B, n, 3) or tuple(hv.shape) != (B, 778, 3) or any(t.dtype != torch.float32 for t in out):
        raise ValueError(f"mesh_queries: outputs must be fp32 [{B},{n},3], [{B},{n},3], [{B},778,3]")
    L.check(L.lib().ab_mesh_queries(L.ptr(table), L.i(table.shape[0]), L.i(n), L.ptr(obj_id), L.ptr(obj_transf), L.ptr(root_joint),
                                    L.ptr(hand_verts), L.ptr(samples), L.l(samples.stride(0)), L.l(pose_offset), L.i(B), L.ptr(can), L.ptr(v3d),
                                    L.ptr(hv), L.stream()), "ab_mesh_queries")
    return out


def real_mesh_queries(table, row, obj_map, hand_map, mano_verts, out=None):
    """ab_real_mesh_queries: the mesh queries of REAL frames in one launch (realdata.RealBatcher).  table [n_rows,n,3]
    f32 (datasets.HO3D.mesh_vertex_table), row int64 [B] (clamped into the table), obj_map / hand_map [B,3,4] f32 (realdata.real_mesh_maps),
    mano_verts [B,778,3] f32 (ab_mano_lbs).  out: (obj_verts_can [B,n,3], obj_verts_3d [B,n,3], hand_verts_3d [B,778,3]) to write into
    (allocated when None).  B == 0: nothing is launched."""
    B, n = row.shape[0], table.shape[1]
    if row.dtype != torch.int64 or row.dim() != 1:
        raise ValueError(f"real_mesh_queries: row must be int64 [B], got {row.dtype} {tuple(row.shape)}")
    for t, numel, what in ((table, table.shape[0] * n * 3, "table"), (obj_map, B * 12, "obj_map"), (hand_map, B * 12, "hand_map"),
                           (mano_verts, B * 778 * 3, "mano_verts")):
        if t.dtype != torch.float32 or t.numel() != numel:
            raise ValueError(f"real_mesh_queries: {what} must be fp32 with {numel} elements, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=table.device)      # noqa: E731
        out = (z(B, n, 3), z(B, n, 3), z(B, 778, 3))
    can, v3d, hv = out
    if tuple(can.shape) != (B, n, 3) or tuple(v3d.shape) != (B, n, 3) or tuple(hv.shape) != (B, 778, 3) or any(t.dtype != torch.float32 for t in out):
        raise ValueError(f"real_mesh_queries: outputs must be fp32 [{B},{n},3], [{B},{n},3], [{B},778,3]")
    L.check(L.lib().ab_real_mesh_queries(L.ptr(table), L.i(table.shape[0]), L.i(n), L.ptr(row), L.ptr(obj_map), L.ptr(hand_map),
                                         L.ptr(mano_verts), L.i(B), L.ptr(can), L.ptr(v3d), L.ptr(hv), L.stream()), "ab_real_mesh_queries")
    return out


def mssd(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, pred_R=None, pred_t=None, pred_pts=None, center=None, out=None):
    """ab_mssd: per-sample maximum symmetry-aware surface distance in metres, min over the object's TRUE symmetry set of the max over the
    points.  can [B,V,3], obj_transf [B,4,4] f32; obj_idx int64 [B] (1-based, clamped into the table); sym_R [n_obj,Kmax,3,3] / sym_t
    [n_obj,Kmax,3(,1)] f32 in metres, sym_count int32 [n_obj] (table entries past a row's count are never read).  Rigid mode: pred_R [B,3,3]
    and pred_t [B,(1,)3]; points mode: pred_pts [B,V,3] instead.  center [B,3] or None (zero).  -> mssd [B] f32 (`out` when given)."""
    B, V = can.shape[0], can.shape[1]
    n_obj, Kmax = sym_R.shape[0], sym_R.shape[1]
    if obj_idx.dtype != torch.int64 or sym_count.dtype != torch.int32:
        raise ValueError(f"mssd: obj_idx must be int64 and sym_count int32, got {obj_idx.dtype} / {sym_count.dtype}")
    if (pred_pts is None) == (pred_R is None) or (pred_R is None) != (pred_t is None):
        raise ValueError("mssd: pass either pred_R and pred_t (rigid mode) or pred_pts (points mode)")
    for t, numel, what in ((can, B * V * 3, "can"), (obj_transf, B * 16, "obj_transf"), (obj_idx, B, "obj_idx"), (sym_R, n_obj * Kmax * 9, "sym_R"),
                           (sym_t, n_obj * Kmax * 3, "sym_t"), (sym_count, n_obj, "sym_count"), (pred_R, B * 9, "pred_R"), (pred_t, B * 3, "pred_t"),
                           (pred_pts, B * V * 3, "pred_pts"), (center, B * 3, "center")):
        if t is not None and (t.numel() != numel or (t.dtype != torch.float32 and what not in ("obj_idx", "sym_count"))):
            raise ValueError(f"mssd: {what} must hold {numel} elements (fp32 but for the indices), got {t.dtype} {tuple(t.shape)}")
    if out is None:
        out = torch.empty((B,), dtype=torch.float32, device=can.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B,):
        raise ValueError(f"mssd: out must be fp32 [{B}]")
    ins = [L.ptr(t) for t in (can, obj_transf, obj_idx, sym_R, sym_t, sym_count, pred_R, pred_t, pred_pts, center)]      # device tensors, or an error
    ws = _workspace(L.lib().ab_mssd_workspace(L.i(B), L.i(Kmax), L.i(V)), can.device)
    L.check(L.lib().ab_mssd(*ins[:6], L.i(n_obj), L.i(Kmax), *ins[6:], L.i(B), L.i(V), L.ptr(out), L.ptr(ws), L.stream()), "ab_mssd")
    return out


def _f32_of(op, what, t, numel):
    if t.dtype != torch.float32 or t.numel() != numel:
        raise ValueError(f"{op}: {what} must be fp32 with {numel} elements, got {t.dtype} {tuple(t.shape)}")
    return L.ptr(t)


def mspd(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, cam_intr, pred_R=None, pred_t=None, pred_pts=None, out=None):
    """ab_mspd (eager only): per-sample maximum symmetry-aware projection distance in pixels, min over the object's TRUE symmetry set of the
    max over the points of || proj(pred) - proj(sym(gt)) ||.  The arguments of `mssd` (same table, same sym_count semantics) plus cam_intr
    [B,3,3]; no centre.  A point at or behind the camera (Z <= 0) in either pose makes the sample +inf.  -> mspd [B] f32 (`out` when given)."""
    B, V = can.shape[0], can.shape[1]
    n_obj, Kmax = sym_R.shape[0], sym_R.shape[1]
    if obj_idx.dtype != torch.int64 or sym_count.dtype != torch.int32:
        raise ValueError(f"mspd: obj_idx must be int64 and sym_count int32, got {obj_idx.dtype} / {sym_count.dtype}")
    if (pred_pts is None) == (pred_R is None) or (pred_R is None) != (pred_t is None):
        raise ValueError("mspd: pass either pred_R and pred_t (rigid mode) or pred_pts (points mode)")
    for t, numel, what in ((can, B * V * 3, "can"), (obj_transf, B * 16, "obj_transf"), (obj_idx, B, "obj_idx"), (sym_R, n_obj * Kmax * 9, "sym_R"),
                           (sym_t, n_obj * Kmax * 3, "sym_t"), (sym_count, n_obj, "sym_count"), (pred_R, B * 9, "pred_R"), (pred_t, B * 3, "pred_t"),
                           (pred_pts, B * V * 3, "pred_pts"), (cam_intr, B * 9, "cam_intr")):
        if t is not None and (t.numel() != numel or (t.dtype != torch.float32 and what not in ("obj_idx", "sym_count"))):
            raise ValueError(f"mspd: {what} must hold {numel} elements (fp32 but for the indices), got {t.dtype} {tuple(t.shape)}")
    if out is None:
        out = torch.empty((B,), dtype=torch.float32, device=can.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B,):
        raise ValueError(f"mspd: out must be fp32 [{B}]")
    ins = [L.ptr(t) for t in (can, obj_transf, obj_idx, sym_R, sym_t, sym_count, pred_R, pred_t, pred_pts, cam_intr)]
    ws = _workspace(L.lib().ab_mspd_workspace(L.i(B), L.i(Kmax), L.i(V)), can.device)
    L.check(L.lib().ab_mspd(*ins[:6], L.i(n_obj), L.i(Kmax), *ins[6:], L.i(B), L.i(V), L.ptr(out), L.ptr(ws), L.stream()), "ab_mspd")
    return out


VSD_MAX_TAUS = 16                               # AB_VSD_MAX_TAUS
VSD_NEAR, VSD_RANGE = 0.01, 1 << 22             # AB_VSD_NEAR (metres), AB_VSD_RANGE (1/256 px)


def vsd(obj_verts, obj_faces, vert_off, face_off, max_obj_verts, rows, rot_est, tsl_est, rot_gt, tsl_gt, cam_intr, W, H, delta, taus, diameter,
        normalized_by_diameter=True, depth_test=None, occ_verts=None, occ_faces=None, want_depth=False):
    """ab_vsd (eager only): Visible Surface Discrepancy of a batch, the three depth images kept in LDS.  The packed object table of
    `interaction` (obj_verts [*,3] fp32, obj_faces int32 [*,3] local indices, vert_off / face_off int32 [n_obj+1]; max_obj_verts: the largest
    vertex count, a host number), rows int64 [B]; rot_est / rot_gt [B,3,3], tsl_est / tsl_gt [B,3], cam_intr [B,3,3] fp32; depth_test
    [B,H,W] fp32 or None (no measurement anywhere); the occluder occ_verts [B,Nv,3] (camera frame) with occ_faces int32 [Nf,3], or neither;
    delta and taus (up to 16 host numbers) and diameter fp32 [n_obj], all in the unit of the meshes.  -> dict: counts int32 [B,2+T]
    (union, complement, cost per tau), err [B,T] fp32 and, with want_depth, depth [B,3,H,W] (est, gt, test)."""
    B, n_obj = rows.shape[0], vert_off.numel() - 1
    for what, t, dt, numel in (("obj_faces", obj_faces, torch.int32, None), ("vert_off", vert_off, torch.int32, n_obj + 1),
                               ("face_off", face_off, torch.int32, n_obj + 1), ("rows", rows, torch.int64, B), ("obj_verts", obj_verts, torch.float32, None)):
        if t.dtype != dt or (t.numel() != numel if numel is not None else t.numel() < 3):
            raise ValueError(f"vsd: {what} must be {dt} with {numel if numel is not None else 'at least 3'} elements, got {t.dtype} {tuple(t.shape)}")
    if (occ_verts is None) != (occ_faces is None):
        raise ValueError("vsd: pass occ_verts and occ_faces together, or neither")
    Nv, Nf = (occ_verts.shape[1], occ_faces.shape[0]) if occ_verts is not None else (0, 0)
    if occ_faces is not None and (occ_faces.dtype != torch.int32 or occ_faces.numel() != Nf * 3):
        raise ValueError(f"vsd: occ_faces must be int32 [Nf,3], got {occ_faces.dtype} {tuple(occ_faces.shape)}")
    ins = [_f32_of("vsd", w, t, n) for w, t, n in (("rot_est", rot_est, B * 9), ("tsl_est", tsl_est, B * 3), ("rot_gt", rot_gt, B * 9), ("tsl_gt", tsl_gt, B * 3),
                                                   ("cam_intr", cam_intr, B * 9))]
    dtest = None if depth_test is None else _f32_of("vsd", "depth_test", depth_test, B * H * W)
    occ = None if occ_verts is None else _f32_of("vsd", "occ_verts", occ_verts, B * Nv * 3)
    diam = _f32_of("vsd", "diameter", diameter, n_obj)
    tau = torch.tensor([float(t) for t in taus], dtype=torch.float32)
    T, dev = tau.numel(), rows.device
    if not 1 <= T <= VSD_MAX_TAUS:
        raise ValueError(f"vsd: 1 to {VSD_MAX_TAUS} taus, got {T}")
    o = {"counts": torch.empty((B, 2 + T), dtype=torch.int32, device=dev), "err": torch.empty((B, T), dtype=torch.float32, device=dev)}
    if want_depth:
        o["depth"] = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    ws = _workspace(L.lib().ab_vsd_workspace(L.i(B), L.i(max_obj_verts), L.i(Nv), L.i(W), L.i(H), L.i(T)), dev)
    L.check(L.lib().ab_vsd(L.ptr(obj_verts), L.ptr(obj_faces), L.ptr(vert_off), L.ptr(face_off), L.i(n_obj), L.i(max_obj_verts), L.ptr(rows), *ins,
                           L.i(B), L.i(W), L.i(H), dtest, occ, L.ptr(occ_faces), L.i(Nv), L.i(Nf), L.f(delta), tau, L.i(T), diam,
                           L.i(1 if normalized_by_diameter else 0), o["counts"], o["err"], o.get("depth"), L.ptr(ws), L.stream()), "ab_vsd")
    return o


def chamfer_rigid(can, rot, tsl, targ, root, corners_vis, want_grad=True, want_dist=False):
    """ab_chamfer_rigid (eager only, never under graph capture): the two-way squared nearest-neighbour distance between keep (R can + t) and
    keep (targ + root), keep = any(corners_vis != 0) formed in the kernel.  can [B,N,3], rot [B,3,3] / [B,9], tsl [B,(1,)3], targ [B,M,3],
    root [B,3], corners_vis [B,8], all fp32.  -> dict: loss [1]; with want_grad g_rot [B,3,3] and g_tsl [B,3] (the gradient of loss);
    with want_dist dist_xy [B,N], dist_yx [B,M] and the int32 indices idx_xy, idx_yx."""
    B, N, M = can.shape[0], can.shape[1], targ.shape[1]
    ins = [_f32_of("chamfer_rigid", w, t, n) for w, t, n in (("can", can, B * N * 3), ("rot", rot, B * 9), ("tsl", tsl, B * 3), ("targ", targ, B * M * 3),
                                                            ("root", root, B * 3), ("corners_vis", corners_vis, B * 8))]
    dev = can.device
    o = {"loss": torch.empty((1,), dtype=torch.float32, device=dev)}
    if want_grad:
        o["g_rot"], o["g_tsl"] = torch.empty((B, 3, 3), dtype=torch.float32, device=dev), torch.empty((B, 3), dtype=torch.float32, device=dev)
    if want_dist:
        o["dist_xy"], o["dist_yx"] = torch.empty((B, N), dtype=torch.float32, device=dev), torch.empty((B, M), dtype=torch.float32, device=dev)
        o["idx_xy"], o["idx_yx"] = torch.empty((B, N), dtype=torch.int32, device=dev), torch.empty((B, M), dtype=torch.int32, device=dev)
    ws = _workspace(L.lib().ab_chamfer_rigid_workspace(L.i(B), L.i(N), L.i(M)), dev)
    L.check(L.lib().ab_chamfer_rigid(*ins, L.i(B), L.i(N), L.i(M), o["loss"], o.get("dist_xy"), o.get("dist_yx"), o.get("idx_xy"), o.get("idx_yx"),
                                     o.get("g_rot"), o.get("g_tsl"), L.ptr(ws), L.stream()), "ab_chamfer_rigid")
    return o


def procrustes_loss(pred, targ, root, want_grad=True, want_aligned=False):
    """ab_procrustes_loss (eager only, never under graph capture): the MSE between targ + root and pred aligned to it by the optimal
    similarity (rotation or reflection, scale, translation).  pred, targ [B,n,3], root [B,3], fp32, n >= 3.  -> dict: loss [1],
    sample_loss [B]; with want_grad g_pred [B,n,3] (the gradient of loss); with want_aligned aligned [B,n,3]."""
    B, n = pred.shape[0], pred.shape[1]
    ins = [_f32_of("procrustes_loss", w, t, k) for w, t, k in (("pred", pred, B * n * 3), ("targ", targ, B * n * 3), ("root", root, B * 3))]
    dev = pred.device
    o = {"loss": torch.empty((1,), dtype=torch.float32, device=dev), "sample_loss": torch.empty((B,), dtype=torch.float32, device=dev)}
    if want_grad:
        o["g_pred"] = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    if want_aligned:
        o["aligned"] = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    L.check(L.lib().ab_procrustes_loss(*ins, L.i(B), L.i(n), o["sample_loss"], o["loss"], o.get("aligned"), o.get("g_pred"), L.stream()),
            "ab_procrustes_loss")
    return o


MM_PAIRED, MM_PROCRUSTES, MM_NN = 1, 2, 4      # AB_MM_* flags of ab_mesh_metrics
MM_ROW = {"epe": 0, "ra_epe": 1, "pa_epe": 2, "scale": 3, "mean_pg": 4, "mean_gp": 5, "pa_mean_pg": 6, "pa_mean_gp": 7, "f": 8, "pa_f": 12}
MM_MAX_THRESHOLDS = 4


def mesh_metrics(pred, targ, root=None, center_idx=-1, thresholds=(), flags=MM_PAIRED | MM_PROCRUSTES | MM_NN, want_dist=False):
    """ab_mesh_metrics (eager only, never under graph capture): per-sample paired / Procrustes-aligned errors and the two-way
    nearest-neighbour distances, means (mean_gp is ADD-S) and F-score counts of pred [B,N,3] against targ [B,M,3] + root [B,3] (None:
    zero), all fp32.  thresholds: up to 4 distances in metres (host numbers).  flags: MM_PAIRED | MM_PROCRUSTES | MM_NN; the first two
    need N == M.  -> dict: rows [B,16] (columns MM_ROW; NaN where a group was not asked for), counts int32 [B,T,4] (pg, gp, pa_pg, pa_gp);
    want_dist: True for all of d_pg [B,N], d_gp [B,M], pa_d_pg, pa_d_gp, or the names wanted."""
    B, N, M = pred.shape[0], pred.shape[1], targ.shape[1]
    ins = [_f32_of("mesh_metrics", "pred", pred, B * N * 3), _f32_of("mesh_metrics", "targ", targ, B * M * 3),
           None if root is None else _f32_of("mesh_metrics", "root", root, B * 3)]
    thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)
    T, dev = thr.numel(), pred.device
    o = {"rows": torch.empty((B, 16), dtype=torch.float32, device=dev), "counts": torch.empty((B, T, 4), dtype=torch.int32, device=dev)}
    names = ("d_pg", "d_gp", "pa_d_pg", "pa_d_gp") if want_dist is True else tuple(want_dist or ())
    for k in names:
        o[k] = torch.empty((B, N if k.endswith("pg") else M), dtype=torch.float32, device=dev)
    ws = _workspace(L.lib().ab_mesh_metrics_workspace(L.i(B), L.i(N), L.i(M)), dev)
    L.check(L.lib().ab_mesh_metrics(*ins, L.i(B), L.i(N), L.i(M), L.i(center_idx), thr, L.i(T), L.i(flags), o["rows"], o["counts"], o.get("d_pg"),
                                    o.get("d_gp"), o.get("pa_d_pg"), o.get("pa_d_gp"), L.ptr(ws), L.stream()), "ab_mesh_metrics")
    return o


IA_VERTS, IA_VOLUME = 1, 2                     # AB_IA_* flags of ab_interaction
IA_ROW = {"pen_max": 0, "pen_mean": 1, "min_dist": 2, "inside_frac": 3, "contact": 4, "volume": 5}      # slots 6, 7 reserved (NaN)
IA_COUNTS = {"n_inside": 0, "n_lattice": 1, "n_both": 2, "capped": 3}


def interaction(hand_verts, hand_faces, hand_orient, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_row, rot, tsl,
                contact_thr=0.005, voxel=0.005, max_voxels=262144, flags=IA_VERTS | IA_VOLUME, want_sdf=False):
    """ab_interaction (eager only, never under graph capture): hand vertices [B,Nh,3] against the object rot[b] can + tsl[b] of the packed
    table (obj_verts [*,3] fp32, obj_faces int32 [*,3] local indices, vert_off / face_off int32 [n_obj+1], obj_orient fp32 [n_obj] of +-1,
    obj_row int64 [B]) and the lattice intersection volume with the hand mesh (hand_faces int32 [Fh,3], hand_orient +-1).  Distances in
    metres.  -> dict: rows [B,8] (columns IA_ROW; NaN where a group was not asked for), counts int32 [B,4] (IA_COUNTS); with want_sdf
    sdf [B,Nh] (-d inside, +d outside) and wind [B,Nh] (orientation x winding number)."""
    B, Nh, Fh, n_obj = hand_verts.shape[0], hand_verts.shape[1], hand_faces.shape[0], obj_orient.numel()
    for what, t, dt, numel in (("hand_faces", hand_faces, torch.int32, Fh * 3), ("obj_faces", obj_faces, torch.int32, None),
                               ("vert_off", vert_off, torch.int32, n_obj + 1), ("face_off", face_off, torch.int32, n_obj + 1),
                               ("obj_row", obj_row, torch.int64, B), ("obj_verts", obj_verts, torch.float32, None)):
        if t.dtype != dt or (t.numel() != numel if numel is not None else t.numel() < 3):
            raise ValueError(f"interaction: {what} must be {dt} with {numel if numel is not None else 'at least 3'} elements, got {t.dtype} {tuple(t.shape)}")
    ins = {"hand_verts": _f32_of("interaction", "hand_verts", hand_verts, B * Nh * 3), "obj_orient": _f32_of("interaction", "obj_orient", obj_orient, n_obj),
           "rot": _f32_of("interaction", "rot", rot, B * 9), "tsl": _f32_of("interaction", "tsl", tsl, B * 3)}
    dev = hand_verts.device
    o = {"rows": torch.empty((B, 8), dtype=torch.float32, device=dev), "counts": torch.empty((B, 4), dtype=torch.int32, device=dev)}
    if want_sdf:
        o["sdf"], o["wind"] = torch.empty((B, Nh), dtype=torch.float32, device=dev), torch.empty((B, Nh), dtype=torch.float32, device=dev)
    ws = _workspace(L.lib().ab_interaction_workspace(L.i(B), L.i(Nh), L.i(max_voxels)), dev)
    L.check(L.lib().ab_interaction(ins["hand_verts"], L.ptr(hand_faces), L.i(Nh), L.i(Fh), L.f(hand_orient), L.ptr(obj_verts), L.ptr(obj_faces),
                                   L.ptr(vert_off), L.ptr(face_off), ins["obj_orient"], L.i(n_obj), L.ptr(obj_row), ins["rot"], ins["tsl"], L.i(B),
                                   L.f(contact_thr), L.f(voxel), L.i(max_voxels), L.i(flags), o["rows"], o["counts"], o.get("sdf"), o.get("wind"),
                                   L.ptr(ws), L.stream()), "ab_interaction")
    return o


IAS_ROW = {"obj_pen_max": 0, "obj_pen_mean": 1, "obj_min_dist": 2, "obj_inside_frac": 3, "obj_contact": 4}      # slots 5..7 reserved (NaN)
IAS_COUNTS = {"n_obj_inside": 0, "n_obj_verts": 1}


def interaction_sym(hand_verts, hand_faces, hand_orient, obj_verts, vert_off, obj_row, rot, tsl, no_max, contact_thr=0.005, want_sdf=False):
    """ab_interaction_sym (eager only, never under graph capture): the reverse direction of `interaction`, the vertices of the object
    rot[b] can + tsl[b] of the packed table (obj_verts [*,3] fp32, vert_off int32 [n_obj+1], obj_row int64 [B]) against the hand mesh
    (hand_verts [B,Nh,3], hand_faces int32 [Fh,3], hand_orient +-1), scanned in the object's canonical frame.  no_max: the largest vertex
    count of the table's objects (ObjectMeshTable.no_max).  Distances in metres.  -> dict: rows [B,8] (columns IAS_ROW, the others NaN),
    counts int32 [B,2] (IAS_COUNTS); with want_sdf sdf_obj [B,no_max] (-d inside the hand, +d outside) and wind_obj [B,no_max]
    (orientation x winding number), NaN past the sample's object."""
    B, Nh, Fh, n_obj, no_max = hand_verts.shape[0], hand_verts.shape[1], hand_faces.shape[0], vert_off.numel() - 1, int(no_max)
    for what, t, dt, numel in (("hand_faces", hand_faces, torch.int32, Fh * 3), ("vert_off", vert_off, torch.int32, None),
                               ("obj_row", obj_row, torch.int64, B), ("obj_verts", obj_verts, torch.float32, None)):
        if t.dtype != dt or (t.numel() != numel if numel is not None else t.numel() < (3 if what == "obj_verts" else 2)):
            raise ValueError(f"interaction_sym: {what} must be {dt} with {numel if numel is not None else 'enough'} elements, got {t.dtype} {tuple(t.shape)}")
    ins = {"hand_verts": _f32_of("interaction_sym", "hand_verts", hand_verts, B * Nh * 3), "rot": _f32_of("interaction_sym", "rot", rot, B * 9),
           "tsl": _f32_of("interaction_sym", "tsl", tsl, B * 3)}
    dev = hand_verts.device
    o = {"rows": torch.empty((B, 8), dtype=torch.float32, device=dev), "counts": torch.empty((B, 2), dtype=torch.int32, device=dev)}
    if want_sdf:
        o["sdf_obj"], o["wind_obj"] = torch.empty((B, no_max), dtype=torch.float32, device=dev), torch.empty((B, no_max), dtype=torch.float32, device=dev)
    ws = _workspace(L.lib().ab_interaction_sym_workspace(L.i(B), L.i(Nh), L.i(no_max)), dev)
    L.check(L.lib().ab_interaction_sym(ins["hand_verts"], L.ptr(hand_faces), L.i(Nh), L.i(Fh), L.f(hand_orient), L.ptr(obj_verts), L.ptr(vert_off),
                                       L.i(n_obj), L.ptr(obj_row), ins["rot"], ins["tsl"], L.i(B), L.i(no_max), L.f(contact_thr), o["rows"], o["counts"],
                                       o.get("sdf_obj"), o.get("wind_obj"), L.ptr(ws), L.stream()), "ab_interaction_sym")
    return o


CL_SCAN_ALL = 1                               # AB_CL_SCAN_ALL: scan every vertex, not only the candidates (same bits; the A/B of the benchmark)
CL_MAX_ZONES = 16
CL_COUNTS = {"n_inside": 0, "n_candidates": 1}


def contact_loss(hand_verts, zone_id, n_zones, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_box, obj_row, rot, tsl, mask=None,
                 rho=0.02, alpha=0.01, lambda_r=0.5, lambda_a=0.5, flags=0, want_grad=True, want_sdf=False):
    """ab_contact_loss (eager only, never under graph capture): repulsion of the hand vertices [B,Nh,3] inside the object rot[b] can + tsl[b]
    of the packed table (the arguments of `interaction`, plus obj_box fp32 [n_obj,6]) and attraction of the zones zone_id int32 [Nh]
    (-1 = none, 0 .. n_zones-1; None when n_zones == 0) that do not touch it; mask fp32 [B] or None (0 = the sample contributes nothing).
    rho, alpha in metres.  -> dict: loss [1], rep [B], att [B], counts int32 [B,2] (CL_COUNTS); with want_grad g_hand [B,Nh,3], g_rot [B,3,3],
    g_tsl [B,3] (the gradient of loss; the rotation's nine entries free); with want_sdf sdf [B,Nh] (NaN: no candidate, -d inside, +d outside)."""
    B, Nh, n_obj = hand_verts.shape[0], hand_verts.shape[1], obj_orient.numel()
    if not 0 <= int(n_zones) <= CL_MAX_ZONES:
        raise ValueError(f"contact_loss: 0 <= n_zones <= {CL_MAX_ZONES}, got {n_zones}")
    if (zone_id is None and n_zones) or not (float(rho) > 0 and float(alpha) > 0):
        raise ValueError("contact_loss: zone_id is needed with n_zones > 0, and rho, alpha must be > 0")
    for what, t, dt, numel in (("zone_id", zone_id, torch.int32, Nh), ("obj_faces", obj_faces, torch.int32, None), ("vert_off", vert_off, torch.int32, n_obj + 1),
                               ("face_off", face_off, torch.int32, n_obj + 1), ("obj_row", obj_row, torch.int64, B), ("obj_verts", obj_verts, torch.float32, None)):
        if t is not None and (t.dtype != dt or (t.numel() != numel if numel is not None else t.numel() < 3)):
            raise ValueError(f"contact_loss: {what} must be {dt} with {numel if numel is not None else 'at least 3'} elements, got {t.dtype} {tuple(t.shape)}")
    ins = {"hand_verts": _f32_of("contact_loss", "hand_verts", hand_verts, B * Nh * 3), "obj_orient": _f32_of("contact_loss", "obj_orient", obj_orient, n_obj),
           "obj_box": _f32_of("contact_loss", "obj_box", obj_box, n_obj * 6), "rot": _f32_of("contact_loss", "rot", rot, B * 9),
           "tsl": _f32_of("contact_loss", "tsl", tsl, B * 3), "mask": None if mask is None else _f32_of("contact_loss", "mask", mask, B)}
    dev = hand_verts.device
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    o = {"loss": z(1), "rep": z(B), "att": z(B), "counts": torch.empty((B, 2), dtype=torch.int32, device=dev)}
    if want_grad:
        o["g_hand"], o["g_rot"], o["g_tsl"] = z(B, Nh, 3), z(B, 3, 3), z(B, 3)
    if want_sdf:
        o["sdf"] = z(B, Nh)
    ws = _workspace(L.lib().ab_contact_loss_workspace(L.i(B), L.i(Nh)), dev)
    L.check(L.lib().ab_contact_loss(ins["hand_verts"], L.ptr(zone_id), L.i(Nh), L.i(n_zones), L.ptr(obj_verts), L.ptr(obj_faces), L.ptr(vert_off),
                                    L.ptr(face_off), ins["obj_orient"], ins["obj_box"], L.i(n_obj), L.ptr(obj_row), ins["rot"], ins["tsl"], ins["mask"],
                                    L.i(B), L.f(rho), L.f(alpha), L.f(lambda_r), L.f(lambda_a), L.i(flags), o["loss"], o["rep"], o["att"], o["counts"],
                                    o.get("sdf"), o.get("g_hand"), o.get("g_rot"), o.get("g_tsl"), L.ptr(ws), L.stream()), "ab_contact_loss")
    return o


FIT_NP = 59             # parameters per hand of ab_mano_fit: so3 48 | beta 10 | bone 1


def mano_fit(quat, pred_joints, tables, n_iter=20, step0=1, state=None, want_mesh=True, want_loss=False, want_grad=False):
    """ab_mano_fit: B hands through n_iter Adam steps of the submission's MANO fit in one launch.  quat [B,64] raw IKNet output,
    pred_joints [B,21,3]; tables: v_template, shapedirs, posedirs, J_regressor, weights, J_template [16,3], J_shapedirs [16,3,10]
    (fitting.mano_fit_tables).  state None: start as the submit pass does (initialised inside the kernel); else (params, m, v), each
    [B,59], copied first.  -> dict params / m / v [B,59], verts [B,778,3] / joints [B,21,3] (want_mesh), loss [B,n_iter]
    (want_loss), grad [B,59] of the last step (want_grad)."""
    B, dev = quat.shape[0], quat.device
    z = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    if state is None:
        params, m, v = z(B, FIT_NP), z(B, FIT_NP), z(B, FIT_NP)
    else:
        params, m, v = (t.to(dev, torch.float32).clone().contiguous() for t in state)
    o = dict(params=params, m=m, v=v, verts=z(B, 778, 3) if want_mesh else None, joints=z(B, 21, 3) if want_mesh else None,
             loss=z(B, n_iter) if want_loss else None, grad=z(B, FIT_NP) if want_grad else None)
    L.check(L.lib().ab_mano_fit(L.ptr(quat), L.ptr(pred_joints), L.ptr(tables["v_template"]), L.ptr(tables["shapedirs"]),
                                L.ptr(tables["posedirs"]), L.ptr(tables["J_regressor"]), L.ptr(tables["weights"]),
                                L.ptr(tables["J_template"]), L.ptr(tables["J_shapedirs"]), L.i(B), L.i(n_iter), L.i(step0),
                                L.i(1 if state is None else 0), L.ptr(params), L.ptr(m), L.ptr(v), L.ptr(o["verts"]), L.ptr(o["joints"]),
                                L.ptr(o["loss"]), L.ptr(o["grad"]), L.stream()), "ab_mano_fit")
    return o


DRAW_REC_WORDS = 12     # int32 words per vertex record of ab_draw_meshes


def draw_meshes(hand_verts, tables, image, cam_intr, out, obj_id=None, obj_rot=None, obj_tsl=None, corners=None, debug=False):
    """ab_draw_meshes: panels 2 (hand over the frame, the sample's camera) and 3 (hand + object on white, orbit camera) of the contact
    sheet `out` uint8 [B,H,4W,3], in place; panels 1 and 4 are not touched.  hand_verts [B,778,3], image float [B,3,H,W] (frame - 0.5),
    cam_intr [B,3,3].  tables (draw.MeshDrawer.tables): hand_faces [nhf,3] / adj_off [779] / adj_face int32 and, with an object
    library, obj_verts / obj_normals / obj_faces / obj_vert_off / obj_face_off plus the ints n_obj, max_obj_verts, max_obj_faces.
    obj_id int32 [B] (>= 0 library object, -1 none, -2 the box over corners[b]), obj_rot [B,3,3], obj_tsl [B,3], corners [B,8,3].
    -> the orbit camera positions float [B,4] (xyz, pad), a view of the workspace; debug: -> (positions, vertex records int32
    [B, 778 + max(max_obj_verts, 8), 12], keys int64 [B,2,H,W]), all views of the workspace."""
    B, H, W = image.shape[0], image.shape[2], image.shape[3]
    dev = hand_verts.device
    if tuple(out.shape) != (B, H, 4 * W, 3) or out.dtype != torch.uint8:
        raise ValueError(f"draw_meshes: out must be uint8 [{B},{H},{4 * W},3], got {out.dtype} {tuple(out.shape)}")
    n_obj = int(tables.get("n_obj", 0))
    mov, mof = int(tables.get("max_obj_verts", 0)), int(tables.get("max_obj_faces", 0))
    if obj_id is None:
        obj_id = torch.full((B,), -1, dtype=torch.int32, device=dev)
    if obj_rot is None:
        obj_rot = torch.zeros((B, 3, 3), dtype=torch.float32, device=dev)
    if obj_tsl is None:
        obj_tsl = torch.zeros((B, 3), dtype=torch.float32, device=dev)
    ws = torch.empty((L.lib().ab_draw_workspace_bytes(L.i(B), L.i(W), L.i(H), L.i(mov)),), dtype=torch.uint8, device=dev)
    g = lambda k: L.ptr(tables[k]) if n_obj else None      # noqa: E731
    L.check(L.lib().ab_draw_meshes(L.ptr(hand_verts), L.ptr(tables["hand_faces"]), L.i(tables["hand_faces"].shape[0]), L.ptr(tables["adj_off"]),
                                   L.ptr(tables["adj_face"]), L.i(tables["adj_face"].numel()), g("obj_verts"), g("obj_normals"), g("obj_faces"),
                                   g("obj_vert_off"), g("obj_face_off"), L.i(n_obj), L.i(tables["obj_verts"].shape[0] if n_obj else 0),
                                   L.i(tables["obj_faces"].shape[0] if n_obj else 0), L.i(mov), L.i(mof), L.ptr(obj_id), L.ptr(obj_rot),
                                   L.ptr(obj_tsl), L.ptr(corners), L.ptr(cam_intr), L.ptr(image), L.i(B), L.i(W), L.i(H), L.ptr(out), L.ptr(ws),
                                   L.stream()), "ab_draw_meshes")
    VP = 778 + max(mov, 8)
    koff = L.lib().ab_draw_workspace_keys_offset(L.i(B), L.i(mov))
    cam = ws[koff - (B * 16 + 255) // 256 * 256:][:B * 16].view(torch.float32).view(B, 4)
    if not debug:
        return cam
    rec = ws[:B * VP * DRAW_REC_WORDS * 4].view(torch.int32).view(B, VP, DRAW_REC_WORDS)
    keys = ws[koff:koff + B * 2 * H * W * 8].view(torch.int64).view(B, 2, H, W)
    return cam, rec, keys
