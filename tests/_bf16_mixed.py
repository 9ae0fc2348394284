"""CPU emulation of what TSPO_SEL_BF16_MIXED computes (include/tspo_hip.h), shared by tests/test_bf16_mixed_abi.py (CPU: with the
rounding switched off it must equal the oracle's autograd) and tests/test_gpu_bf16_mixed.py (GPU: with the rounding on, the kernels
must equal it to fp32 summation order).

The five dense GEMMs of the forward and the five of the backward are written out with their operands passed through `r`
(round-to-nearest-even to bf16, or the identity); everything else - positional add, banded softmax and its backward, ReLU mask,
residual, cosine score and its backward, the bias gradients (column sums of the unrounded dY) - is fp32.  Autograd is used only
for the two fp32 pieces between the GEMMs (score -> dh2, attention -> dqkv), never through a cast."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tspo_oracle as O

TRAINED = [n for n in O.SELECTOR_KEYS if "ffn_o" not in n]


def rbf16(t):
    return t.to(torch.bfloat16).float()


def _ident(t):
    return t


def _banded_attention(qkv, T, D, H, w):
    """ctx [B,T,D] from qkv [B,T,3D]: softmax over the key set [max(0, t-w/2), min(T-1, t-w/2+w-1)] per head (O(T.w) memory;
    the same set as oracle.create_window_mask)."""
    B = qkv.shape[0]
    hd = D // H
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, T, H, hd) for i in range(3))
    j = torch.arange(T)[:, None] - w // 2 + torch.arange(w)[None, :]          # [T, w]
    valid = (j >= 0) & (j <= T - 1)
    jc = j.clamp(0, T - 1)
    kw, vw = k[:, jc], v[:, jc]                                                # [B, T, w, H, hd]
    s = torch.einsum("bthd,btwhd->bthw", q, kw) / hd ** 0.5
    s = s.masked_fill(~valid[None, :, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bthw,btwhd->bthd", p, vw).reshape(B, T, D)


def _scores(h2, txt, clip, tau):
    return (O.pair_cosine(h2, txt).mean(-1) + clip) / tau


def forward_backward(params, img, txt, clip, dscores, H, w, tau, rounding=True):
    """params {name: fp32 tensor} (oracle names), img [B,T,D], txt [B,M,D], clip [B,T], dscores [B,T] (all fp32 CPU tensors) ->
    (scores [B,T], {name: gradient summed over B and T}).  rounding=False: the exact fp32 arithmetic."""
    r = rbf16 if rounding else _ident
    B, T, D = img.shape
    p = {n: v.float() for n, v in params.items()}
    wqkv = torch.cat([p[f"temporal.Self_{c}.weight"] for c in "qkv"], 0)
    bqkv = torch.cat([p[f"temporal.Self_{c}.bias"] for c in "qkv"], 0)
    w1, b1, w2, b2 = p["mlp.0.weight"], p["mlp.0.bias"], p["mlp.2.weight"], p["mlp.2.bias"]
    with torch.no_grad():
        xpe = img + O.positional_encoding(T, D)
        qkv = r(xpe) @ r(wqkv).T + bqkv
        ctx = _banded_attention(qkv, T, D, H, w)
        h1 = torch.relu(r(ctx) @ r(w1).T + b1)
        h2 = r(h1) @ r(w2).T + b2 + img
    # score backward (fp32)
    h2l = h2.clone().requires_grad_(True)
    sc = _scores(h2l, txt, clip, tau)
    sc.backward(dscores)
    dh2 = h2l.grad
    X = lambda t: t.reshape(B * T, -1)   # noqa: E731
    with torch.no_grad():
        g = {}
        g["mlp.2.weight"] = r(X(dh2)).T @ r(X(h1))
        g["mlp.2.bias"] = X(dh2).sum(0)
        dh1 = (r(dh2) @ r(w2)) * (h1 > 0)
        g["mlp.0.weight"] = r(X(dh1)).T @ r(X(ctx))
        g["mlp.0.bias"] = X(dh1).sum(0)
        dctx = r(dh1) @ r(w1)
    # banded attention backward (fp32)
    qkvl = qkv.clone().requires_grad_(True)
    _banded_attention(qkvl, T, D, H, w).backward(dctx)
    dqkv = qkvl.grad
    with torch.no_grad():
        dw = r(X(dqkv)).T @ r(X(xpe))
        db = X(dqkv).sum(0)
        for i, c in enumerate("qkv"):
            g[f"temporal.Self_{c}.weight"] = dw[i * D:(i + 1) * D]
            g[f"temporal.Self_{c}.bias"] = db[i * D:(i + 1) * D]
    return sc.detach(), g


def oracle_autograd(params, img, txt, clip, dscores, H, w, tau):
    """The oracle's forward (oracle.selector_forward, dense window mask) per video, autograd gradients summed over the batch."""
    ps = {n: v.float().clone().requires_grad_(True) for n, v in params.items()}
    total = 0.0
    outs = []
    for b in range(img.shape[0]):
        s, _ = O.selector_forward(ps, img[b], txt[b], clip[b], w, tau, H)
        total = total + (s * dscores[b]).sum()
        outs.append(s.detach())
    total.backward()
    return torch.stack(outs), {n: (ps[n].grad if ps[n].grad is not None else torch.zeros_like(ps[n])) for n in TRAINED}


def rel_fro(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
