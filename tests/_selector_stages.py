"""The scoring head's workspace as named tensors, float64 restatements of every stage of its forward and backward, and the error
bounds the stage tests assert (tests/test_gpu_selector_stages.py).  The method of tests/_clip_stages.py applied to
csrc/selector.hip: every stage is compared with float64 applied to THAT STAGE'S OWN STORED INPUT, so an error confined to one
head, one band edge, one row tile or one padding row is not averaged away in a summed gradient, and no ReLU kink or rounding
boundary upstream can move a downstream reference.

The restatements are written from the mathematics (include/tspo_hip.h), not from the kernels; they run in torch.float64 on the
device their inputs live on.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  Every E below is a worst-case, order-independent bound of the evaluation the
kernel performs (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum of n terms in ANY order errs by at
most (n - 1) u sum |t_i| to first order; the few u of slack `c` in the operation counts cover the second-order terms and the
roundings of the epilogue).  Nothing is fitted to a measurement.

Arithmetic of the GEMM stages per precision (what the dispatch of csrc/selector.hip gives each stage; `arith()` below):

    stage                               fp32     bf16x3                              bf16_mixed
    q,k,v projection, mlp.0, mlp.2      fp32     bf16x3                              bf16
    mlp.2 / mlp.0 data gradients        fp32     bf16x3                              bf16
    weight gradients                    fp32     bf16x3 if D % 128 == 0 else fp32    bf16
    bias gradients (column sums)        fp32     fp32                                fp32 (of the UNROUNDED dY)
    everything between the GEMMs        fp32     fp32                                fp32

  fp32    products and sums in fp32: E = (K + c) u sum |x| |w|.
  bf16    the stored fp32 operands rounded to nearest-even bf16 (torch's conversion - the same values the kernel's converter gives),
          exact products (8 x 8 significand bits), float64 sum: the operands are identical to the kernel's, so there are no
          rounding-boundary flips; E = (K + c) u sum |r(x)| |r(w)| is the fp32 accumulation alone.
  bf16x3  the split emulated exactly: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32), ref = sum (hi hi + hi lo + lo hi)
          in float64; E = (3 K + c) u sum (|hi hi| + |hi lo| + |lo hi|), the accumulation bound over the 3 K terms.

Device functions.  ROCm's documentation of the accuracy of expf / sincosf is not on the build machine; the figures below are
ASSUMED (the HIP programming guide's math-function table gives 1 ulp for expf, sinf and cosf).  If a measured error exceeds a
bound because of them, that is a finding to explain, not a constant to raise."""
import math

import torch

from tspo_amd import ops

U = 2.0 ** -24
ULP = 2.0 * U                # one ulp of an fp32 value y is at most 2 u |y|
TINY = 2.0 ** -126           # smallest normal fp32: absolute floor where a softmax weight may be a denormal
EXPF_ULP = 1.0               # ASSUMED (see above)
SINCOSF_ULP = 1.0            # ASSUMED (see above)
C_SUM = 8                    # the slack `c` in every (n + c) u sum |terms|
LN1E4_F32 = -9.21034049987793   # the literal of posenc_add_kernel (-ln 1e4 rounded to fp32)

FORWARD = ("xpe", "qkv", "P", "ctx", "h1", "h2")
BACKWARD = ("dh2", "dh1", "dctx", "dqkv", "dS", "w1t", "w2t")


def f32(x):
    """A Python float rounded to fp32 (what a `float` argument of the C ABI or an `f` literal holds)."""
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- layout
def carve(B, T, D, H, w):
    """{name: (byte offset, shape)} + "__prefix__": the prefix of carve() in csrc/selector.hip - every buffer 256-byte aligned, in
    the order xpe | qkv | P | ctx | h1 | h2 | dh2 | dh1 | dctx | dqkv | dS | w1t | w2t.  Stops before the split-contraction planes
    (`part`), whose size depends on the split rule."""
    BT = B * T
    order = [("xpe", (BT, D)), ("qkv", (BT, 3 * D)), ("P", (BT, H, w)), ("ctx", (BT, D)), ("h1", (BT, D)), ("h2", (BT, D)),
             ("dh2", (BT, D)), ("dh1", (BT, D)), ("dctx", (BT, D)), ("dqkv", (BT, 3 * D)), ("dS", (BT, H, w)), ("w1t", (D, D)),
             ("w2t", (D, D))]
    out, off = {}, 0
    for name, shape in order:
        off = (off + 255) // 256 * 256
        out[name] = (off, shape)
        off += 4 * math.prod(shape)
    out["__prefix__"] = off
    return out


def views(ws, B, T, D, H, w):
    """Named fp32 views (no copies) of the byte tensor `ws` that ops.selector_forward returns."""
    lay = carve(B, T, D, H, w)
    assert lay["__prefix__"] <= ws.numel(), f"workspace of {ws.numel()} B is shorter than the mirrored prefix {lay['__prefix__']} B"
    out = {}
    for name, v in lay.items():
        if name != "__prefix__":
            off, shape = v
            out[name] = ws[off:off + 4 * math.prod(shape)].view(torch.float32).view(*shape)
    return out


# ---------------------------------------------------------------------------------------------------------------- report
class Report:
    """Collects `worst err / E` per stage; finish() prints every line and raises ONE AssertionError naming the stages that failed
    (a downstream stage reads stored inputs, so it does not fail because an upstream one did)."""

    def __init__(self, case):
        self.case, self.lines, self.failed = case, [], []

    def check(self, stage, got, ref, E):
        """|got - ref| <= E for EVERY element (E may be 0 where the value must be exact)."""
        got = got.double()
        assert got.shape == ref.shape and ref.shape == E.shape, (stage, got.shape, ref.shape, E.shape)
        if not bool(torch.isfinite(ref).all() & torch.isfinite(E).all()):
            return self._fail(stage, "the reference is not finite: a stored INPUT of this stage was never written")
        if not bool(torch.isfinite(got).all()):
            return self._fail(stage, f"{int((~torch.isfinite(got)).sum())} of {got.numel()} output elements are not finite "
                                     f"(never written, or computed from unwritten memory)")
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / E)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self.lines.append(f"[stage] {self.case}: {stage}: max err/E {worst:.3g}")
        if not worst <= 1.0:
            i = int(ratio.reshape(-1).argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
            self._fail(stage, f"max err/E {worst:.3g}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound, worst at "
                              f"{idx}: got {got.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} E {E.reshape(-1)[i].item():.3g}")
        return worst

    def exact(self, stage, ok, what):
        self.lines.append(f"[stage] {self.case}: {stage}: {'ok' if ok else 'FAILED'}")
        if not ok:
            self._fail(stage, what)

    def _fail(self, stage, what):
        self.failed.append(stage)
        self.lines.append(f"[stage] {self.case}: {stage}: FAILED: {what}")

    def finish(self):
        print("\n".join(self.lines))
        if self.failed:
            bad = [ln for ln in self.lines if "FAILED" in ln]
            raise AssertionError(f"{self.case}: stages that failed: {sorted(set(self.failed))}\n" + "\n".join(bad))


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.int32), b.contiguous().view(-1).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- GEMMs
def arith(precision, stage, D):
    """The arithmetic of a GEMM stage ("forward", "dgrad", "wgrad") under a precision: the table of the module docstring."""
    if precision == "fp32":
        return "fp32"
    if precision == "bf16_mixed":
        return "bf16"
    assert precision == "bf16x3", precision
    return "fp32" if (stage == "wgrad" and D % 128 != 0) else "bf16x3"


def rne_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def split_bf16(x):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)          # x - hi is exact in fp32
    return hi.double(), lo.double()


def gemm64(A, Bm, how):
    """sum_k A[m, k] Bm[n, k] in float64 under the arithmetic `how` -> (ref, sum |terms|, number of terms per output)."""
    K = A.shape[-1]
    if how == "bf16x3":
        ah, al = split_bf16(A)
        bh, bl = split_bf16(Bm)
        ref = ah @ bh.t() + ah @ bl.t() + al @ bh.t()
        mag = ah.abs() @ bh.abs().t() + ah.abs() @ bl.abs().t() + al.abs() @ bh.abs().t()
        return ref, mag, 3 * K
    a, b = (rne_bf16(A), rne_bf16(Bm)) if how == "bf16" else (A.double(), Bm.double())
    return a @ b.t(), a.abs() @ b.abs().t(), K


def linear64(X, W, bias, how, resid=None):
    """X W^T + bias (+ resid) and its bound E = (n + c) u (sum |x| |w| + |bias| + |resid|), n = K (3 K for bf16x3)."""
    ref, mag, n = gemm64(X, W, how)
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if resid is not None:
        ref, mag = ref + resid.double(), mag + resid.double().abs()
    return ref, (n + C_SUM) * U * mag


# ---------------------------------------------------------------------------------------------------------------- stages
def posenc64(img, lens):
    """x + pe(t / L_b), pe[t, 2i] = sin(a), pe[t, 2i + 1] = cos(a), a = (t / L_b) exp(2i c), c = fp32(-ln 1e4) / D in fp32 as the
    kernel holds it; padding rows 0.
    E = a (|2i c| + 2 EXPF_ULP + 3) u   the angle: rounding of the product 2i c (u relative, amplified by |2i c| <= 9.3 through the
                                        exponential), expf, the rounding of t / L and of the product; sin / cos are 1-Lipschitz
      + SINCOSF_ULP 2 u |pe|            sincosf
      + u |x + pe|                      the add."""
    B, T, D = img.shape
    dev = img.device
    c = (torch.tensor(LN1E4_F32, dtype=torch.float32, device=dev) / torch.tensor(float(D), dtype=torch.float32, device=dev)).double()
    arg = torch.arange(0, D, 2, device=dev, dtype=torch.float64) * c                       # [D / 2]
    t = torch.arange(T, device=dev, dtype=torch.float64)
    L = torch.tensor(lens, device=dev, dtype=torch.float64)
    ang = (t[None, :] / L[:, None])[..., None] * torch.exp(arg)                            # [B, T, D / 2]
    pe = torch.stack([torch.sin(ang), torch.cos(ang)], -1).reshape(B, T, D)
    valid = (t[None, :] < L[:, None])[..., None]
    ref = (img.double() + pe) * valid
    dang = (ang * (arg.abs() + 2 * EXPF_ULP + 3) * U).repeat_interleave(2, -1)
    E = (dang + SINCOSF_ULP * ULP * pe.abs() + U * ref.abs()) * valid
    return ref, E


def band_index(L, w, dev):
    """Per query t of a video of L frames: the distinct keys [max(0, t - w/2), min(L - 1, t - w/2 + w - 1)] as (key [L, w]
    clamped, valid [L, w], n [L])."""
    t = torch.arange(L, device=dev)
    lo = (t - w // 2).clamp(min=0)
    hi = (t - w // 2 + w - 1).clamp(max=L - 1)
    n = hi - lo + 1
    slot = torch.arange(w, device=dev)
    valid = slot[None, :] < n[:, None]
    return (lo[:, None] + slot[None, :]).clamp(max=L - 1), valid, n


def _heads(x, H):
    return x.double().view(x.shape[0], H, -1)


def band_softmax64(qkv, H, w):
    """One video's stored q | k | v [L, 3 D] -> (P [L, H, w], E).  P = softmax_j(q . k_j / sqrt(hd)) over the distinct keys, 0 in
    the slots past the clipped window.  With A = max_j sum_d |q_d k_jd| and s = 1 / sqrt(hd), every exponential carries a relative
    perturbation of at most
        eta = (hd + c + 2) u s A + EXPF_ULP 2 u :  the dot product and the (twice-rounded) scale ((hd + c) u s A), the rounding of
                                                   s_j - m (u |s_j - m| <= 2 u s A; the choice of m itself cancels), expf;
    P_j (1 + eta_j) / sum_i P_i (1 + eta_i) moves P_j by at most 2 eta P_j (1 % second order); the sum of n <= w exponentials and
    the division add (w + 4) u P_j.  TINY: a weight below the normal range."""
    L, D = qkv.shape[0], qkv.shape[1] // 3
    hd = D // H
    key, valid, _ = band_index(L, w, qkv.device)
    q, k = _heads(qkv[:, :D], H), _heads(qkv[:, D:2 * D], H)
    kg = k[key]                                                                           # [L, w, H, hd]
    sc = 1.0 / math.sqrt(hd)
    s = torch.einsum("thd,tjhd->thj", q, kg) * sc
    A = torch.einsum("thd,tjhd->thj", q.abs(), kg.abs()).masked_fill(~valid[:, None, :], 0).amax(-1, keepdim=True)
    P = torch.softmax(s.masked_fill(~valid[:, None, :], float("-inf")), -1)
    eta = (hd + C_SUM + 2) * U * sc * A + EXPF_ULP * ULP
    return P, P * (2.02 * eta + (w + 4) * U) + TINY * valid[:, None, :]


def band_context64(P, qkv, H, w):
    """ctx = sum_j P_j v_j with the STORED P; E = (w + c) u sum |P_j| |v_j|."""
    L, D = qkv.shape[0], qkv.shape[1] // 3
    key, valid, _ = band_index(L, w, qkv.device)
    vg = _heads(qkv[:, 2 * D:], H)[key]
    Pm = P.double().masked_fill(~valid[:, None, :], 0)
    ref = torch.einsum("thj,tjhd->thd", Pm, vg).reshape(L, D)
    return ref, (w + C_SUM) * U * torch.einsum("thj,tjhd->thd", Pm.abs(), vg.abs()).reshape(L, D)


def band_bwd_q64(qkv, P, dctx, dS, H, w):
    """dp_j = dctx . v_j, dS_j = P_j (dp_j - sum_i P_i dp_i) / sqrt(hd) from the stored P; dq = sum_j dS_j k_j from the STORED dS.
    With e_j = (hd + c) u sum_d |dctx_d v_jd| the error of dp_j and dd = sum_j P_j e_j + (w + c) u sum_j |P_j dp_j| that of the
    weighted sum:  E_dS = P_j s (e_j + dd + 6 u (|dp_j| + |dot|)) (the subtraction, two products, the twice-rounded scale);
    E_dq = (w + c) u sum_j |dS_j| |k_j|.  -> (dS ref, E_dS, dq ref, E_dq)."""
    L, D = qkv.shape[0], qkv.shape[1] // 3
    hd = D // H
    key, valid, _ = band_index(L, w, qkv.device)
    m = valid[:, None, :]
    kg, vg = _heads(qkv[:, D:2 * D], H)[key], _heads(qkv[:, 2 * D:], H)[key]
    dc = _heads(dctx, H)
    Pm = P.double().masked_fill(~m, 0)
    sc = 1.0 / math.sqrt(hd)
    dp = torch.einsum("thd,tjhd->thj", dc, vg).masked_fill(~m, 0)
    e = (hd + C_SUM) * U * torch.einsum("thd,tjhd->thj", dc.abs(), vg.abs())
    dot = (Pm * dp).sum(-1, keepdim=True)
    dd = (Pm * e).sum(-1, keepdim=True) + (w + C_SUM) * U * (Pm * dp).abs().sum(-1, keepdim=True)
    dS_ref = Pm * (dp - dot) * sc
    E_dS = Pm * sc * (e + dd + 6 * U * (dp.abs() + dot.abs())) + TINY * m
    dSm = dS.double().masked_fill(~m, 0)
    dq = torch.einsum("thj,tjhd->thd", dSm, kg).reshape(L, D)
    return dS_ref, E_dS, dq, (w + C_SUM) * U * torch.einsum("thj,tjhd->thd", dSm.abs(), kg.abs()).reshape(L, D)


def band_bwd_kv64(qkv, P, dS, dctx, H, w):
    """dk_j = sum_t dS[t, j - lo_t] q_t, dv_j = sum_t P[t, j - lo_t] dctx_t over the (at most w) queries t whose window holds key j,
    from the STORED dS and P; E = (w + c) u sum |coefficient| |row|.  -> (dk, E_dk, dv, E_dv), each [L, D]."""
    L, D = qkv.shape[0], qkv.shape[1] // 3
    key, valid, _ = band_index(L, w, qkv.device)
    sel = valid.reshape(-1)
    kf = key.reshape(-1)[sel]
    out = []
    for coef, rows in ((dS, _heads(qkv[:, :D], H)), (P, _heads(dctx, H))):
        c = coef.double().permute(0, 2, 1)[..., None]                                      # [L, w, H, 1]
        contrib = (c * rows[:, None]).reshape(L * w, H, -1)[sel]
        ref = torch.zeros_like(rows).index_add_(0, kf, contrib)
        mag = torch.zeros_like(rows).index_add_(0, kf, contrib.abs())
        out += [ref.reshape(L, D), (w + C_SUM) * U * mag.reshape(L, D)]
    return out


EPS_COS = f32(1e-6)


def _cos_parts(h2, txt):
    h, e = h2.double(), txt.double()
    de = torch.einsum("btd,bmd->btm", h, e)
    A = torch.einsum("btd,bmd->btm", h.abs(), e.abs())
    hn, en = h.norm(dim=-1), e.norm(dim=-1)
    den = hn[..., None] * en[:, None, :] + EPS_COS
    return h, e, de, A, hn, en, den


def score64(h2, txt, clip, tau, valid):
    """scores = (mean_m h . e_m / (|h| |e_m| + 1e-6) + clip) / tau from the stored h2 [B, T, D]; -inf on padding frames.
    R = (D + c) u bounds the relative error of the sums of squares and (times A_m = sum |h| |e_m|) the absolute error of the dot
    products; the norms are R / 2 + u each, the denominator R + 4 u, so a cosine errs by (2 R + 8 u) A_m / den_m; the mean over M,
    the clip add and the division by tau add (M + 4) u (mean |cos| + |clip|) and 2 u |score|."""
    D, M = h2.shape[-1], txt.shape[1]
    _, _, de, A, _, _, den = _cos_parts(h2, txt)
    tau = f32(tau)
    cl = clip.double() if clip is not None else torch.zeros_like(de[..., 0])
    cos = de / den
    s = (cos.mean(-1) + cl) / tau
    R = (D + C_SUM) * U
    E = (((2 * R + 8 * U) * A / den).mean(-1) + (M + 4) * U * (cos.abs().mean(-1) + cl.abs())) / abs(tau) + 2 * U * s.abs()
    ninf = torch.full_like(s, float("-inf"))
    return torch.where(valid, s, ninf), E * valid


def score_grad_unit64(h2, txt, tau):
    """d score_t / d h2_t by float64 AUTOGRAD of the score formula alone (each score depends on its own row only), and the bound of
    the kernel's evaluation ca e - cb h per unit of dL/dscore, g = 1 / (tau M), ca = g / den, cb = g (h . e) |e| / (den^2 |h|):
      ca: the denominator (R + 4 u), the division and the two roundings of g:                    (R + 8 u) |ca e|
      cb: the dot product (R A), |e| and |h| (R / 2 + u each), den^2 (2 R + 8 u), 4 operations:  g |e| / (den^2 |h|) |h_d| A (4 R + 16 u)
      the two products, the subtraction and the sum over m:                                      (M + 3) u sum_m (|ca e| + |cb h|)."""
    D, M = h2.shape[-1], txt.shape[1]
    tau = f32(tau)
    hg = h2.double().requires_grad_(True)
    e = txt.double()
    cos = torch.einsum("btd,bmd->btm", hg, e) / (hg.norm(dim=-1)[..., None] * e.norm(dim=-1)[:, None, :] + EPS_COS)
    (cos.mean(-1) / tau).sum().backward()
    unit = hg.grad
    h, e, de, A, hn, en, den = _cos_parts(h2, txt)
    g = 1.0 / abs(tau) / M
    R = (D + C_SUM) * U
    ca_e = g * e.abs()[:, None, :, :] / den[..., None]                                          # [B, T, M, D]
    cbase = g * (en[:, None, :] / (den * den * hn[..., None]))[..., None] * h.abs()[:, :, None, :]
    E = ((R + 8 * U) * ca_e + cbase * (A * (4 * R + 16 * U))[..., None] + (M + 3) * U * (ca_e + cbase * de.abs()[..., None])).sum(2)
    return unit, E


def advantage64(rewards, adv, eps):
    """A = (r - mean) / (std + eps), unbiased std over the G rollouts; loss_b = -mean_g A from the STORED advantages.
    e = (G + 2) u max |r| bounds r - mean; the standard deviation then errs by 1.5 e + (G + 3) u std, so
    E_adv = (e (1 + 1.5 |A|) + |A| (G + 3) u std) / (std + eps) + 2 u |A|;  E_loss = (G + 2) u mean |A|."""
    r = rewards.double()
    G = r.shape[1]
    eps = f32(eps)
    mean = r.mean(-1, keepdim=True)
    sd = torch.sqrt(((r - mean) ** 2).sum(-1, keepdim=True) / (G - 1))
    a = (r - mean) / (sd + eps)
    e = (G + 2) * U * r.abs().amax(-1, keepdim=True)
    E_adv = (e * (1 + 1.5 * a.abs()) + a.abs() * (G + 3) * U * sd) / (sd + eps) + 2 * U * a.abs()
    st = adv.double()
    return a, E_adv, -st.mean(-1), (G + 2) * U * st.abs().mean(-1)


def pg_dscores64(adv, logp, idx, scale):
    """The header's closed form dL/ds_t = -(1/G) sum_g A_g (1[t in S_g] / k - exp(logp_t)) scale from the STORED advantages.
    E = (G + c + 2 EXPF_ULP) u (1/G) sum_g |A_g| (1[t in S_g] / k + p_t) |scale|: expf, 1 / k, the subtraction, the G-term sum and the
    three final products."""
    B, G, k = idx.shape
    T = logp.shape[1]
    hit = torch.zeros((B, G, T), dtype=torch.float64, device=logp.device).scatter_(2, idx, 1.0)
    p = torch.exp(logp.double())[:, None, :]
    a = adv.double()[..., None]
    scale = f32(scale)
    ds = -(a * (hit / k - p)).sum(1) / G * scale
    return ds, (G + C_SUM + 2 * EXPF_ULP) * U * (a.abs() * (hit / k + p)).sum(1) / G * abs(scale)


def weight_grad64(dY, X, rows, how):
    """dY^T X over the valid stored rows (`rows`: bool [BT]) and the bias gradient, the column sums of the unrounded fp32 dY;
    E = (BT + c) u sum |dy| |x| (3 BT terms for bf16x3), valid for any split of the contraction; (BT + c) u sum |dy| for the bias."""
    BT = dY.shape[0]
    y, x = dY[rows], X[rows]
    ref, mag, _ = gemm64(y.t(), x.t(), how)
    n = (3 if how == "bf16x3" else 1) * BT
    yb = y.double()
    return ref, (n + C_SUM) * U * mag, yb.sum(0), (BT + C_SUM) * U * yb.abs().sum(0)


def grad_views(grad, D):
    """The six gradients of the flat bucket as (wqkv [3D, D], bqkv [3D], w1, b1, w2, b2)."""
    o = ops.flat_offsets(D)
    take = lambda name, n: grad[o[name][0]:o[name][0] + n]
    return {"wqkv": take("temporal.Self_q.weight", 3 * D * D).view(3 * D, D), "bqkv": take("temporal.Self_q.bias", 3 * D),
            "w1": take("mlp.0.weight", D * D).view(D, D), "b1": take("mlp.0.bias", D),
            "w2": take("mlp.2.weight", D * D).view(D, D), "b2": take("mlp.2.bias", D)}
