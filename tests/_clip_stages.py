"""The CLIP encoder's workspace as named tensors, float64 restatements of every encoder stage and the error bounds the stage
tests assert (tests/test_gpu_encoder_stages.py; the layout check alone also runs on the CPU, tests/test_host_logic.py).

The restatements are written from the mathematics (LayerNorm, x.sigmoid(1.702 x), softmax(q k^T / 8) v, the stride-p convolution
as a gather), not from the kernels; they run in torch.float64 on whatever device their inputs live on.

Bounds.  u = 2^-24 is the unit roundoff of fp32.  A stage stores bf16(f), f evaluated in fp32 from exact bf16 / fp32 inputs,
|f - ref64| <= E.  Then |got - ref64| <= 1/2 ulp_bf16(|ref64| + E) + E: the 1/2 ulp is that of f, and f may lie in the binade
above ref64's when ref64 is within E of a power of two (that is the only reason for the `+ E` inside the ulp).  E per stage is
written at each function below; all of them are worst-case, order-independent bounds (Higham, Accuracy and Stability of Numerical
Algorithms, section 3.1: a sum of n terms in any order errs by at most (n - 1) u sum |t_i| to first order; the few u of slack in
the operation counts `c` below cover the second-order terms)."""
import ctypes as C

import torch

U = 2.0 ** -24
GELU_K = 1.702


# ---------------------------------------------------------------------------------------------------------------- layout
def geometry(cfg, n_frames):
    gw = cfg["image"] // cfg["patch"]
    P = gw * gw
    S = P + 1
    return dict(gw=gw, P=P, S=S, M=n_frames * S, Kreal=3 * cfg["patch"] ** 2, Kp=(3 * cfg["patch"] ** 2 + 63) // 64 * 64)


def carve(cfg, n_frames):
    """{name: (byte offset, shape, dtype)} + "__total__": the workspace layout of clip_carve() in csrc/clip_vit.hip - every buffer
    256-byte aligned, in the order wqkv_f | w1_f | cq | dq | c1 | d1 | x | h | qkv | a | u | patches | pooled | stats | spart."""
    g = geometry(cfg, n_frames)
    Cc, mlp, M, Lf = cfg["hidden"], cfg["mlp"], g["M"], max(1, cfg["layers"])
    bf, f32 = torch.bfloat16, torch.float32
    order = [("wqkv_f", (Lf, 3 * Cc, Cc), bf), ("w1_f", (Lf, mlp, Cc), bf), ("cq", (Lf, 3 * Cc), f32), ("dq", (Lf, 3 * Cc), f32),
             ("c1", (Lf, mlp), f32), ("d1", (Lf, mlp), f32), ("x", (M, Cc), bf), ("h", (M, Cc), bf), ("qkv", (M, 3 * Cc), bf),
             ("a", (M, Cc), bf), ("u", (M, mlp), bf), ("patches", (n_frames * g["P"], g["Kp"]), bf), ("pooled", (n_frames, Cc), bf),
             ("stats", (M, 2), f32), ("spart", (M, Cc // 64, 2), f32)]
    out, off = {}, 0
    for name, shape, dt in order:
        nbytes = (2 if dt == bf else 4)
        for s in shape:
            nbytes *= s
        off = (off + 255) // 256 * 256
        out[name] = (off, shape, dt)
        off += nbytes
    out["__total__"] = (off + 255) // 256 * 256      # (the total is rounded up too: Carver::bytes())
    return out


def library_workspace_bytes(cfg, n_frames):
    """tspo_clip_workspace_bytes of the built library for this configuration (pure host code: no GPU needed)."""
    from tspo_amd import _lib
    c = _lib.ClipConfig(cfg["hidden"], cfg["layers"], cfg["heads"], cfg["mlp"], cfg["patch"], cfg["image"], cfg["proj"],
                        float(cfg.get("ln_eps", 1e-5)))
    return int(_lib.lib().tspo_clip_workspace_bytes(C.byref(c), n_frames))


def assert_layout_matches_library(cfg, n_frames):
    lay = carve(cfg, n_frames)
    want = library_workspace_bytes(cfg, n_frames)
    assert lay["__total__"] == want, f"workspace layout drifted: this mirror {lay['__total__']} B, the library {want} B ({cfg}, {n_frames} frames)"
    return lay


def views(W, n_frames):
    """Typed tensor views (no copies) into W.workspace(n_frames), by the names of carve().  Asking for the workspace makes the
    next encode fold its weights again (ops.ClipVitWeights.workspace), which is what the stage tests want."""
    lay = assert_layout_matches_library(W.cfg, n_frames)
    ws = W.workspace(n_frames)
    out = {}
    for name, v in lay.items():
        if name == "__total__":
            continue
        off, shape, dt = v
        numel = 1
        for s in shape:
            numel *= s
        out[name] = ws[off:off + numel * (2 if dt == torch.bfloat16 else 4)].view(dt).view(*shape)
    return out


# ------------------------------------------------------------------------------------------------- float64 restatements
def d64(t):
    return t.to(torch.float64)


def rne_bf16(t):
    """float64 -> nearest bf16 (ties to even) -> float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def layernorm64(x, gamma, beta, eps):
    x = d64(x)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * d64(gamma) + d64(beta)


def row_stats64(x, eps):
    """(rstd, -mean * rstd) per row: what the LayerNorm-folded epilogues read."""
    x = d64(x)
    mu = x.mean(-1)
    r = 1.0 / torch.sqrt(((x - mu[:, None]) ** 2).mean(-1) + eps)
    return r, -mu * r


def quick_gelu64(y):
    return y * torch.sigmoid(GELU_K * y)


def attention64(qkv, n_frames, S, heads, scale=0.125, rows=None, keys=None):
    """softmax(q k^T * scale) v per (frame, head) from the row-major [M, 3 * hidden] q | k | v image; head_dim 64.  Returns
    (out [n_frames, R, hidden], sum_j p_j |v_j| in the same shape, max_j sum_d |q_d k_jd| [n_frames, R, heads]); rows = query rows
    (default all S).  `keys` (a slice) restricts the key set - only for the hand-run self-check that the test can fail."""
    hid = heads * 64
    t = d64(qkv).view(n_frames, S, 3, heads, 64)
    q, k, v = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2), t[:, :, 2].transpose(1, 2)   # [F, H, S, 64]
    if rows is not None:
        q = q[:, :, rows]
    if keys is not None:
        k, v = k[:, :, keys], v[:, :, keys]
    s = q @ k.transpose(-1, -2)
    qk_abs = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)                                          # [F, H, R]
    p = torch.softmax(s * scale, dim=-1)
    out = (p @ v).transpose(1, 2).reshape(n_frames, -1, hid)
    pv_abs = (p @ v.abs()).transpose(1, 2).reshape(n_frames, -1, hid)
    return out, pv_abs, qk_abs.transpose(1, 2)


def read_head_major(img, M, hidden):
    """The head-major q/k/v image [3 * heads][M][64] (GE_BIAS_LN_HM) -> row-major [M][3 * hidden]: block b holds columns
    64 b .. 64 b + 63 of every row."""
    nb = 3 * hidden // 64
    return img.reshape(-1)[:nb * M * 64].view(nb, M, 64).transpose(0, 1).reshape(M, nb * 64)


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def patches_ref(pixels, cfg):
    """Patch extraction (+ CLIP normalisation of uint8 frames): [n, 3, H, W] -> bf16 [n * P, Kp], row n * P + py * gw + px, column
    c * p * p + ky * p + kx, zero beyond 3 p p.  uint8: ((x / 255 - mean_c) / std_c), each operation rounded to fp32 (IEEE division
    and subtraction: torch on the CPU reproduces it exactly), then one RNE to bf16; float pixels: one RNE to bf16."""
    px = pixels.cpu()
    n, p = px.shape[0], cfg["patch"]
    g = geometry(cfg, n)
    if px.dtype == torch.uint8:
        mean = torch.tensor(CLIP_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
        std = torch.tensor(CLIP_STD, dtype=torch.float32).view(1, 3, 1, 1)
        v = (px.to(torch.float32) / torch.tensor(255.0, dtype=torch.float32) - mean) / std
    else:
        v = px.to(torch.float32)
    v = v.to(torch.bfloat16).view(n, 3, g["gw"], p, g["gw"], p).permute(0, 2, 4, 1, 3, 5).reshape(n * g["P"], g["Kreal"])
    return torch.nn.functional.pad(v, (0, g["Kp"] - g["Kreal"]))


# ---------------------------------------------------------------------------------------------------------------- bounds
def half_ulp_bf16(x):
    """1/2 ulp of the bf16 binade of |x| (8 significand bits: ulp = 2^(e - 7) for 2^e <= |x| < 2^(e + 1)); normal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))      # |x| = m 2^e with 1/2 <= m < 1
    return torch.ldexp(torch.ones_like(x), e - 9)


def bound_bf16(ref, E):
    return half_ulp_bf16(ref.abs() + E) + E


def gemm_abs64(a, w):
    """sum_k |a_k w_k| per output element."""
    return d64(a).abs() @ d64(w).abs().t()


def stats_err(x, eps, extra=256):
    """Worst-case error of the fp32 row statistics of bf16 rows x [M, C], for both producers (row_stats_kernel: two passes over
    the row; GE_RESID_ST + stats_finalize{,16}: per-64-column (sum, sum of squares) on the matrix pipe, M2 = sum x^2 - sum x . mean,
    Chan merges).  Sums: |d mean| <= (C + c) u mean|x|; C var is a sum of C squares (or of C squares minus products bounded by
    them, sum |x| |m| <= sum x^2) -> |d (C var)| <= (C + c) u sum x^2 + 2 |d mean| sum |x - mu| + C dmean^2; c = 256 covers the
    per-slice one-pass form (64 + 128 + 1 roundings' worth), four merge levels of eight operations and the final division /
    rsqrt (1 ulp).  Returns (relative error of rstd, absolute error of -mean * rstd)."""
    x = d64(x)
    Cn = x.shape[-1]
    mu = x.mean(-1)
    dv = x - mu[:, None]
    var = (dv ** 2).mean(-1)
    r = 1.0 / torch.sqrt(var + eps)
    dmean = (Cn + extra) * U * x.abs().mean(-1)
    dvar = ((Cn + extra) * U * (x ** 2).sum(-1) + 2 * dmean * dv.abs().sum(-1) + Cn * dmean ** 2) / Cn
    rel_r = 0.5 * dvar / (var + eps) + 4 * U
    return rel_r, r * dmean + (mu * r).abs() * (rel_r + U)


def layernorm_err(x, gamma, beta, eps):
    """E of layernorm_kernel: out = (v - mean) rstd gamma + beta in fp32, two-pass statistics (stats_err with c = 8), five
    roundings in the output expression."""
    x = d64(x)
    rel_r, _ = stats_err(x, eps, extra=8)
    mu = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    dmean = (x.shape[-1] + 8) * U * x.abs().mean(-1, keepdim=True)
    g = d64(gamma).abs()
    xh = ((x - mu) * r).abs()
    return g * r * dmean + g * xh * (rel_r[:, None] + 5 * U) + U * d64(beta).abs()


def flips(ref64, E):
    """Where the kernel's bf16 store of a value within E of ref64 may differ from RNE_bf16(ref64), and by how much: one bf16 ulp
    where ref64 lies within E of a rounding boundary, else 0."""
    r0 = rne_bf16(ref64)
    may = (rne_bf16(ref64 + E) != r0) | (rne_bf16(ref64 - E) != r0)
    return may.to(torch.float64) * 2 * half_ulp_bf16(ref64.abs() + E)


def layernorm_sensitivity(y, delta, gamma, eps):
    """|LN(y + e) - LN(y)| for |e| <= delta elementwise, first order + 1 %: out_n = yh_n gamma_n + beta_n with yh = (y - mu) r,
    d out_n = r gamma_n (e_n - mean e) - gamma_n yh_n r mean_k(yh_k e_k)."""
    y = d64(y)
    mu = y.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(((y - mu) ** 2).mean(-1, keepdim=True) + eps)
    yh = ((y - mu) * r).abs()
    return 1.01 * r * d64(gamma).abs() * (delta + delta.mean(-1, keepdim=True) + yh * (yh * delta).mean(-1, keepdim=True))


def quick_gelu_err(y, Ey):
    """E of x / (1 + 2^(-k x)) in fp32 given |dy| <= Ey: |g'| <= 1.1 everywhere; t = -k x (1 rounding, which the exponential
    turns into |t| ln 2 u relative), v_exp_f32 and v_rcp_f32 1 ulp = 2 u each, the add and the final product u each."""
    t = (GELU_K * 1.4426950408889634 * y).abs()
    return 1.1 * Ey + (0.7 * t + 8) * U * quick_gelu64(y).abs()


def attention_err(out, pv_abs, qk_abs, S, heads, scale=0.125):
    """E of the attention kernels, per output element.  With pi = softmax: out = sum_j pt_j v_j / sum_j pt_j where the kernel's
    pt_j = bf16(p_j) = p_j (1 + e_j), |e_j| <= 2^-8 (P is rounded to bf16 for the P V product on the matrix pipe and the row sum
    is taken of the ROUNDED P; bf16 has 8 significand bits, so round-to-nearest errs by up to 2^-8 RELATIVE - half an ulp of
    2^-7 at the bottom of a binade.  The first statement of this bound had 2^-9 there, half the unit roundoff: with S = 5, where
    nothing averages, the kernel measured up to 1.17 x that form, as 2^-8 allows and 2^-9 does not).
    out - ref = (sum p_j e_j v_j - ref sum p_j e_j) / sum pt_j, so
        |out - ref| <= 2^-8 (1 + 2^-7) (sum_j pi_j |v_j| + |ref|).
    fp32 terms, as relative perturbations eta_j of p_j entering the same expression twice (numerator and denominator): the
    64-term dot product ((64 + 2) u scale sum_d |q_d k_jd|), the scaled subtraction of the maximum and the exponential's
    argument rounding (|t| ln 2 u with |t| <= 2 scale log2e max|s|, bounded through the same sum), v_exp_f32 1 ulp, up to three
    online-softmax rescalings; and the fp32 accumulation of S products and the final division ((S + 3) u).  The class-token
    kernel keeps P in fp32: the same bound holds a fortiori."""
    hid = heads * 64
    eta = (66 + 3) * U * scale * qk_abs + 12 * U                                   # [F, R, H]
    eta = eta[..., None].expand(*eta.shape, 64).reshape(out.shape[0], out.shape[1], hid)
    return (2.0 ** -8 * (1 + 2.0 ** -7) + 2 * eta + (S + 3) * U) * (pv_abs + out.abs())


# ---------------------------------------------------------------------------------------------------------------- report
def check(name, got, ref, bound, tile=None, lines=None, rounded=True):
    """Print `max |got - ref| / bound` and the share of elements that differ from RNE_bf16(ref) at all (rounded=False, fp32
    outputs: from ref itself); assert the ratio <= 1 for EVERY element.  On failure the coordinates of the worst elements are printed (row, column[, and tile coordinates])."""
    got, ref = d64(got), ref
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values in the kernel's output"
    ratio = (got - ref).abs() / bound
    worst = ratio.max().item()
    share = (got != (rne_bf16(ref) if rounded else ref)).double().mean().item()
    line = (f"[stage] {name}: max err/bound {worst:.3f}, differs from {'RNE_bf16(ref64)' if rounded else 'ref64 (fp32 output)'} in "
            f"{100 * share:.3f} % of {got.numel()} elements")
    print(line)
    if lines is not None:
        lines.append(line)
    if not worst <= 1.0:
        flat = ratio.reshape(-1, ratio.shape[-1])
        top = torch.topk(flat.reshape(-1), min(8, flat.numel())).indices.tolist()
        msg = [line + " - worst elements:"]
        for i in top:
            r, c = divmod(i, flat.shape[-1])
            msg.append(f"  row {r} col {c} (256-row tile {r // 256}, row in tile {r % 256}; 64-col slice {c // 64}): got "
                       f"{got.reshape(-1)[i].item():.9g} ref {ref.reshape(-1)[i].item():.9g} err/bound {flat.reshape(-1)[i].item():.3f}"
                       + (f" {tile(r, c)}" if tile else ""))
        bad_rows = (flat > 1).any(-1).nonzero().flatten()
        bad_cols = (flat > 1).any(0).nonzero().flatten()
        msg.append(f"  {int((flat > 1).sum())} elements over the bound, in {bad_rows.numel()} rows (first {bad_rows[:12].tolist()}) "
                   f"and {bad_cols.numel()} columns (first {bad_cols[:12].tolist()})")
        raise AssertionError("\n".join(msg))
    return worst, share


def check_two_roundings(name, got, ref_exact, ref_stored, bound, lines=None):
    """A stage that spans two bf16 roundings (an intermediate stored and read again).  ref_exact: float64 throughout; ref_stored:
    float64 with RNE_bf16 at the one intermediate storage point.  The derived one-rounding bound is asserted against ref_stored;
    and against ref_exact the kernel may not be worse than that arithmetic itself is: RMS <= 1.25 x and max <= 2 x the error of
    RNE_bf16(ref_stored) (the margins of _assert_within_reference_noise for means and extremes)."""
    w = check(name, got, ref_stored, bound, lines=lines)
    eg, er = (d64(got) - ref_exact), (rne_bf16(ref_stored) - ref_exact)
    rms_g, rms_r = eg.pow(2).mean().sqrt().item(), er.pow(2).mean().sqrt().item()
    max_g, max_r = eg.abs().max().item(), er.abs().max().item()
    line = (f"[stage] {name} vs float64 throughout: rms {rms_g:.3e} = x{rms_g / rms_r:.3f} of the two-rounding arithmetic's own, "
            f"max {max_g:.3e} = x{max_g / max_r:.3f}")
    print(line)
    if lines is not None:
        lines.append(line)
    assert rms_g <= 1.25 * rms_r and max_g <= 2.0 * max_r, line
    return w
