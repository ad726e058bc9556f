"""float64 restatement of PWC-Net's 2-channel layers (csrc/xpt_flowtail.hip, hip/flowtail.py) as the explicit gather sums of
their definition -- no convolution call, no autograd:

  flow head    y[b,n,oh,ow]    = bias[n] + sum_{kh,kw,c} x[b,c,oh+kh-1,ow+kw-1] w[n,c,kh,kw]            (zeros outside the map)
               dx[b,c,ih,iw]   = sum_{n,kh,kw} g[b,n,ih-kh+1,iw-kw+1] w[n,c,kh,kw]
               dw[n,c,kh,kw]   = sum_{b,oh,ow} g[b,n,oh,ow] x[b,c,oh+kh-1,ow+kw-1],   db[n] = sum g[b,n,:,:]
  up-sampler   y[b,n,oy,ox]    = bias[n] + sum_{c,ky,kx : oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx} x[b,c,iy,ix] W[c,n,ky,kx]
               dx[b,c,iy,ix]   = sum_{n,ky,kx} g[b,n,2iy-1+ky,2ix-1+kx] W[c,n,ky,kx]                    (g outside the map: zero)
               dW[c,n,ky,kx]   = sum_{b,iy,ix} x[b,c,iy,ix] g[b,n,2iy-1+ky,2ix-1+kx],  db[n] = sum g[b,n,:,:]

Every function returns, next to each result, the sum of the MAGNITUDES of its terms per output element ("abs") and the largest
number of terms of one element ("terms"): an fp32 evaluation in any order stays within terms * 2^-23 * abs of the exact value
(the reassociation bound of DESIGN.md section 14).  Tensors are NCHW-indexed, as the operators take them."""
import torch
import torch.nn.functional as F


def _head_sums(x, w, b, g):
    B, C, H, W = x.shape
    xp, gp = F.pad(x, (1, 1, 1, 1)), F.pad(g, (1, 1, 1, 1))
    y = torch.zeros(B, 2, H, W, dtype=torch.float64)
    dx = torch.zeros(B, C, H, W, dtype=torch.float64)
    dw = torch.zeros(2, C, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xp[:, :, kh:kh + H, kw:kw + W]                       # x[b, c, oh + kh - 1, ow + kw - 1]
            gs = gp[:, :, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]       # g[b, n, ih - kh + 1, iw - kw + 1]
            y += torch.einsum("bchw,nc->bnhw", xs, w[:, :, kh, kw])
            dx += torch.einsum("bnhw,nc->bchw", gs, w[:, :, kh, kw])
            dw[:, :, kh, kw] = torch.einsum("bnhw,bchw->nc", g, xs)
    if b is not None:
        y += b.view(1, 2, 1, 1)
    return y, dx, dw, g.sum(dim=(0, 2, 3))


def _up_sums(x, w, b, g):
    B, C, H, W = x.shape
    gp = F.pad(g, (1, 1, 1, 1))                                       # index oy + 1 = 2 iy + ky
    yf = torch.zeros(B, 2, 2 * H + 2, 2 * W + 2, dtype=torch.float64)
    dx = torch.zeros(B, C, H, W, dtype=torch.float64)
    dw = torch.zeros(C, 2, 4, 4, dtype=torch.float64)
    for ky in range(4):
        for kx in range(4):
            gs = gp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]           # g[b, n, 2 iy - 1 + ky, 2 ix - 1 + kx]
            yf[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += torch.einsum("bchw,cn->bnhw", x, w[:, :, ky, kx])
            dx += torch.einsum("bnhw,cn->bchw", gs, w[:, :, ky, kx])
            dw[:, :, ky, kx] = torch.einsum("bchw,bnhw->cn", x, gs)
    y = yf[:, :, 1:2 * H + 1, 1:2 * W + 1].clone()
    if b is not None:
        y += b.view(1, 2, 1, 1)
    return y, dx, dw, g.sum(dim=(0, 2, 3))


def _with_magnitudes(fn, x, w, b, g, terms):
    x, w, g = x.detach().double().cpu(), w.detach().double().cpu(), g.detach().double().cpu()
    b = None if b is None else b.detach().double().cpu()
    val = fn(x, w, b, g)
    mag = fn(x.abs(), w.abs(), None if b is None else b.abs(), g.abs())
    names = ("y", "dx", "dw", "db")
    return {"x": x, "w": w, "b": b, "g": g, **dict(zip(names, val)), "abs": dict(zip(names, mag)), "terms": terms}


def flow_head(x, w, b, g):
    """x [B,C,H,W], w [2,C,3,3], b [2] or None, g [B,2,H,W] -> dict(y, dx, dw, db, abs={...}, terms={...}) in float64."""
    B, C, H, W = x.shape
    terms = {"y": 9 * C + (b is not None), "dx": 18, "dw": B * H * W, "db": B * H * W}
    return _with_magnitudes(_head_sums, x, w, b, g, terms)


def upconv4x4s2(x, w, b, g):
    """x [B,C,H,W], w [C,2,4,4], b [2] or None, g [B,2,2H,2W] -> dict(y, dx, dw, db, abs={...}, terms={...}) in float64."""
    B, C, H, W = x.shape
    terms = {"y": 4 * C + (b is not None), "dx": 32, "dw": B * H * W, "db": 4 * B * H * W}
    return _with_magnitudes(_up_sums, x, w, b, g, terms)
