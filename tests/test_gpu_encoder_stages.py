"""Every stage of the CLIP encoder against float64 applied to that stage's own STORED input.

The encoder's kernels other than the plain GEMM epilogues run only inside tspo_clip_vit_forward*, and what leaves it is row 0 of
each frame after all the layers: an error confined to some patch-token rows, one key, one head or one 64-column slice reaches the
features diluted and under the legitimate bf16 noise of every layer.  Here one-block models with zeroed weights leave each stage's
input and output in the workspace (tests/_clip_stages.py reads it by name), so that every comparison spans ONE rounding to bf16 and
its bound is derived, not tuned: |got - ref64| <= 1/2 ulp_bf16 + E with E the worst-case error of the fp32 evaluation
(_clip_stages: the formula is next to each E).  Every element is checked; the float64 references run in torch.float64 on the GPU
(vendor library - independent of this project's kernels).

How a stage is isolated (layers = 1, synthetic weights of synth.clip_vision_state otherwise):
  run Z  layers = 0: x = x0 = pre-LN(patch embedding) and nothing else.
  run P  out-proj and fc2 weights and biases zero: x stays x0 bit for bit (asserted against run Z, and fold on == fold off);
         left behind: patches, x0, qkv, a and with fold the folded weights wqkv_f, cq, dq, w1_f, c1, d1.
  run Q  real out-proj, fc2 zero: x = x1; a, stats = LN2 (rstd, -mean rstd), spart, u, and without fold h = LN2(x1).
  run R  everything real: x = x2, u, pooled, the features.
  run T  layers = 2, block 1's out-proj and fc2 zero, fold on: qkv of block 1 comes from x2 and the statistics the fc2 epilogue
         (GE_RESID_ST, K = mlp, next_needs_stats) produced.

Kernels and the configuration that reaches each (names as in csrc/):
  patch_gather_u8_l14_kernel            L/14 uint8, 16-byte aligned pixels (l14_70_fold, l14_64_fold)
  patch_gather_kernel<uint8_t,224,14,640>  L/14 uint8 from a misaligned buffer (l14_70_nofold)
  patch_gather_kernel<uint8_t>          every other geometry (vitb16_112_fold, the small models)
  patch_gather_kernel<float|bf16_t|_Float16>  h512_130_fold (f32), vitb16_112_nofold (bf16), l14_70_heavy (f16)
  GE_PATCH row remap, cls_rows_kernel, layernorm_kernel in place (pre-LN)   "embed" of every configuration; persistent kernel
                                        at >= 64 L/14 frames, small kernel below
  ln_fold_kernel                        "fold" of every folding configuration (bitwise W', c and d within the fp32 sum bound)
  row_stats_kernel + GE_BIAS_LN_HM      "qkv" of l14_*_fold, h512_130_fold (N = 1536: np = 8)
  row_stats_kernel + GE_BIAS_LN (row-major, epilogue 5 of gemm_bf16_a9_kernel)   "qkv" of vitb16_112_fold (S = 197)
  layernorm_kernel + GE_BIAS            "qkv" of every non-folding configuration
  clip_attn257_kernel hm = 1 / hm = 0   "attention" of l14_*_fold, h512 / l14_70_nofold, s257_3 (3 frames)
  clip_attn_kernel<0>                   "attention" of vitb16_112_* (S = 197: 13 key tiles, 5 valid keys in the last, fed by the
                                        persistent GEMM) and of S = 2, 17, 65, 226 (one key; one tile + 1; the largest generic S)
  clip_attn_cls_kernel                  test_prune_last_layer_class_token_attention (hm = 1 at 70 frames, hm = 0 at 3)
  GE_RESID_ST / GE_RESID in place       "out-proj" (K = hidden) and "fc2" (K = mlp)
  stats_finalize16_kernel               "LN2 statistics" of l14_*_fold (hidden 1024)
  stats_finalize_kernel (generic Chan merge)   "LN2 statistics" of vitb16_112_fold (np = 12: unequal groups) and h512_130_fold
                                        (np = 8: half of the 16 sub-lanes idle)
  layernorm_kernel<2>, <4>, <8>         hidden 192 (a partly filled 512-column chunk), 1088 and 2048 (<4>), 4096 (<8>): pre-LN,
                                        LN1, LN2 and the strided post-LN of those models
  GE_GELU_LN / GE_GELU                  "fc1"
  strided post-LN, GE_F32 small kernel  "pooled", "features"
  GE_F32 of the persistent kernel (epilogue 3 of gemm_bf16_a9_kernel)   test_gemm_f32_output_on_the_persistent_kernel
  small-problem kernel forced (act = 1 << 8) on a shape the automatic choice gives to the persistent kernel
                                        test_gemm_small_kernel_forced
  ClipVitWeights.library_folds vs what the library does   test_library_folds_matches_the_library_at_the_boundary
"""
import numpy as np
import pytest
import torch

import _clip_stages as cs
from tspo_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"

L14 = dict(synth.CLIP_L14, layers=1)
VITB16 = dict(hidden=768, layers=1, heads=12, mlp=3072, patch=16, image=224, proj=512)
H512 = dict(hidden=512, layers=1, heads=8, mlp=2048, patch=14, image=224, proj=512)
P_ = "vision_model."
L0 = P_ + "encoder.layers.0."


def _small(hidden, image, mlp=128):
    return dict(hidden=hidden, layers=1, heads=hidden // 64, mlp=mlp, patch=14, image=image, proj=64)


def _state(cfg, heavy):
    return synth.clip_vision_state_heavy_tailed(cfg) if heavy else synth.clip_vision_state(**cfg)


def _zeroed(state, layer, names):
    s = dict(state)
    for nm in names:
        for k in ("weight", "bias"):
            key = f"{P_}encoder.layers.{layer}.{nm}.{k}"
            s[key] = np.zeros_like(s[key])
    return s


def _pixels(kind, n, image, seed):
    u8 = torch.from_numpy(synth.uniform_u8((n, 3, image, image), seed))
    if kind == "u8":
        return u8.to(DEV)
    if kind == "u8_misaligned":   # data pointer 1 (mod 16): the 16-byte staged loads of the L/14 uint8 kernel do not apply
        buf = torch.empty(u8.numel() + 1, dtype=torch.uint8, device=DEV)
        px = buf[1:].view(u8.shape)
        px.copy_(u8)
        assert px.data_ptr() % 16 != 0 and px.is_contiguous()
        return px
    mean = torch.tensor(cs.CLIP_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(cs.CLIP_STD).view(1, 3, 1, 1)
    v = (u8.float() / 255 - mean) / std
    return v.to({"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[kind]).to(DEV)


def _run(cfg, state, px, fold, prune=False):
    """One encode; returns (weights object - keeps the workspace alive -, features, named views of the workspace)."""
    W = ops.ClipVitWeights({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, cfg, DEV)
    feat = ops.clip_vit_forward(W, px, fold_layernorm=fold, prune_last_layer=prune)
    torch.cuda.synchronize()
    return W, feat, cs.views(W, px.shape[0])


def _weights(state, cfg, layer=0):
    """The operands as ops.ClipVitWeights packs them (bf16 [out, in] matrices, fp32 vectors, q | k | v fused, class embedding
    added to position row 0 in fp32, patch weight flattened and zero-padded to Kp), on the GPU."""
    T = lambda k: torch.from_numpy(np.asarray(state[k])).float()
    b16 = lambda t: t.to(torch.bfloat16).to(DEV)
    g = cs.geometry(cfg, 1)
    q = f"{P_}encoder.layers.{layer}."
    pos = T(P_ + "embeddings.position_embedding.weight").clone()
    pos[0] += T(P_ + "embeddings.class_embedding")
    w = dict(patch_w=b16(torch.nn.functional.pad(T(P_ + "embeddings.patch_embedding.weight").reshape(cfg["hidden"], g["Kreal"]),
                                                 (0, g["Kp"] - g["Kreal"]))),
             pos=pos.to(DEV), pre_g=T(P_ + "pre_layrnorm.weight").to(DEV), pre_b=T(P_ + "pre_layrnorm.bias").to(DEV),
             post_g=T(P_ + "post_layernorm.weight").to(DEV), post_b=T(P_ + "post_layernorm.bias").to(DEV),
             proj=b16(T("visual_projection.weight")))
    if cfg["layers"] > layer:
        w.update(wqkv=b16(torch.cat([T(q + f"self_attn.{n}_proj.weight") for n in "qkv"], 0)),
                 bqkv=torch.cat([T(q + f"self_attn.{n}_proj.bias") for n in "qkv"], 0).to(DEV),
                 wo=b16(T(q + "self_attn.out_proj.weight")), bo=T(q + "self_attn.out_proj.bias").to(DEV),
                 w1=b16(T(q + "mlp.fc1.weight")), b1=T(q + "mlp.fc1.bias").to(DEV),
                 w2=b16(T(q + "mlp.fc2.weight")), b2=T(q + "mlp.fc2.bias").to(DEV),
                 ln1_g=T(q + "layer_norm1.weight").to(DEV), ln1_b=T(q + "layer_norm1.bias").to(DEV),
                 ln2_g=T(q + "layer_norm2.weight").to(DEV), ln2_b=T(q + "layer_norm2.bias").to(DEV))
    return w


def _folded_gemm(x, wf, c, d, eps):
    """(ref64, E) of y = rstd acc + (-mean rstd) c[n] + d[n] (GE_*_LN) from the STORED folded operands and the float64 row
    statistics of the stored rows x.  E = (K + 6) u (rstd sum_k |x_k w'_k| + |mean rstd c[n]| + |d[n]|): the order-independent
    sum bound over everything that is added, the terms that cancel when rows are far from zero mean included; + the kernel's
    fp32 statistics (_clip_stages.stats_err) through |acc| rstd and |c[n]|."""
    r, nmr = cs.row_stats64(x, eps)
    rel_r, d_nmr = cs.stats_err(x, eps)
    acc = cs.d64(x) @ cs.d64(wf).t()
    c, d = cs.d64(c), cs.d64(d)
    ref = r[:, None] * acc + nmr[:, None] * c + d
    E = (x.shape[1] + 6) * cs.U * (r[:, None] * cs.gemm_abs64(x, wf) + (nmr[:, None] * c).abs() + d.abs())
    E = E + acc.abs() * (r * rel_r)[:, None] + c.abs() * d_nmr[:, None]
    return ref, E


def _plain_gemm(a, w, bias, resid=None):
    """(ref64, E) of a w^T + bias (+ residual): E = (K + 3) u (sum_k |a_k w_k| + |bias| + |residual|)."""
    ref = cs.d64(a) @ cs.d64(w).t() + cs.d64(bias)
    mag = cs.gemm_abs64(a, w) + cs.d64(bias).abs()
    if resid is not None:
        ref = ref + cs.d64(resid)
        mag = mag + cs.d64(resid).abs()
    return ref, (a.shape[1] + 3) * cs.U * mag


def _check_qkv_folded(tag, v, x, layer, cfg, n, hm, lines):
    M, Cn = x.shape
    got = cs.read_head_major(v["qkv"], M, Cn) if hm else v["qkv"]
    ref, E = _folded_gemm(x, v["wqkv_f"][layer], v["cq"][layer], v["dq"][layer], 1e-5)
    cs.check(f"{tag} qkv ({'GE_BIAS_LN_HM' if hm else 'GE_BIAS_LN'}, block {layer})", got, ref, cs.bound_bf16(ref, E), lines=lines)
    return got


def _stages(tag, cfg, n, fold, pix, heavy=False, run_t=True, must_fold=False):
    lines = []
    g = cs.geometry(cfg, n)
    S, M, Cn, heads, eps = g["S"], g["M"], cfg["hidden"], cfg["heads"], 1e-5
    state = _state(cfg, heavy)
    px = _pixels(pix, n, cfg["image"], 100 + n)
    WP, _, vP = _run(cfg, _zeroed(state, 0, ("self_attn.out_proj", "mlp.fc2")), px, fold)
    assert WP.library_folds(n) or not must_fold, f"{tag}: this size was chosen so that the library folds"
    folds = fold and WP.library_folds(n)
    hm = folds and S == 257
    w = _weights(state, cfg)

    # ---- gather: bitwise
    want = cs.patches_ref(px, cfg)
    same = torch.equal(vP["patches"].cpu().view(torch.int16), want.view(torch.int16))
    nbad = 0 if same else int((vP["patches"].cpu().view(torch.int16) != want.view(torch.int16)).sum())
    print(f"[stage] {tag} gather ({pix}): bitwise, {nbad} of {want.numel()} elements differ")
    assert same, f"{tag}: patches differ from the fp32 normalisation + RNE in {nbad} elements"

    # ---- embed: patches -> GE_PATCH (+ position rows, remapped past each frame's class row) -> stored bf16 -> pre-LN in place.
    # Two roundings: E_g = (Kp + 2) u (sum |a w| + |pos|) decides where the stored GEMM output may be the other neighbour
    # (_clip_stages.flips); that one-ulp difference goes through the LayerNorm's derivative (layernorm_sensitivity).
    x0 = vP["x"]
    pat = vP["patches"]
    y = (cs.d64(pat) @ cs.d64(w["patch_w"]).t()).view(n, g["P"], Cn) + cs.d64(w["pos"][1:])
    Eg = (g["Kp"] + 2) * cs.U * (cs.gemm_abs64(pat, w["patch_w"]).view(n, g["P"], Cn) + cs.d64(w["pos"][1:]).abs())
    cls = cs.rne_bf16(cs.d64(w["pos"][0])).expand(n, 1, Cn)          # cls_rows_kernel stores bf16(pos[0]): exact
    y = torch.cat([cls, y], 1).reshape(M, Cn)
    Eg = torch.cat([torch.zeros_like(cls), Eg], 1).reshape(M, Cn)
    y_r = cs.rne_bf16(y)
    ref_exact, ref_stored = cs.layernorm64(y, w["pre_g"], w["pre_b"], eps), cs.layernorm64(y_r, w["pre_g"], w["pre_b"], eps)
    E = cs.layernorm_err(y_r, w["pre_g"], w["pre_b"], eps) + cs.layernorm_sensitivity(y_r, cs.flips(y, Eg), w["pre_g"], eps)
    cs.check_two_roundings(f"{tag} embed (GE_PATCH + class rows + pre-LN)", x0, ref_exact, ref_stored, cs.bound_bf16(ref_stored, E), lines)
    del y, y_r, Eg, ref_exact, ref_stored, E
    # x0 is what a model without blocks leaves, and the zeroed block kept it bit for bit; fold on == fold off
    _, _, vZ = _run(dict(cfg, layers=0), state, px, fold)
    assert torch.equal(vZ["x"], x0), f"{tag}: the block with zero out-proj / fc2 changed the residual stream"
    if folds:
        _, _, vP2 = _run(cfg, _zeroed(state, 0, ("self_attn.out_proj", "mlp.fc2")), px, False)
        assert torch.equal(vP2["x"], x0), f"{tag}: x0 differs between fold on and fold off"
        del vP2
    del vZ

    # ---- fold: W' = RNE_bf16(fp32(w gamma)) bitwise; c = sum of the ROUNDED W' and d = b + sum w beta within (K + 8) u sum |.|
    if folds:
        for nm, wk, bk, gk, bek, cn, dn in (("wqkv_f", "wqkv", "bqkv", "ln1_g", "ln1_b", "cq", "dq"), ("w1_f", "w1", "b1", "ln2_g", "ln2_b", "c1", "d1")):
            wf = (w[wk].cpu().float() * w[gk].cpu()).to(torch.bfloat16)
            assert torch.equal(vP[nm][0].cpu().view(torch.int16), wf.view(torch.int16)), f"{tag}: {nm} is not RNE_bf16(fp32(w gamma))"
            cref = cs.d64(vP[nm][0]).sum(-1)
            cs.check(f"{tag} fold {cn}", vP[cn][0], cref, (Cn + 8) * cs.U * cs.d64(vP[nm][0]).abs().sum(-1), lines=lines, rounded=False)
            dref = cs.d64(w[bk]) + cs.d64(w[wk]) @ cs.d64(w[bek])
            cs.check(f"{tag} fold {dn}", vP[dn][0], dref, (Cn + 8) * cs.U * (cs.d64(w[bk]).abs() + cs.d64(w[wk]).abs() @ cs.d64(w[bek]).abs()),
                     lines=lines, rounded=False)
        print(f"[stage] {tag} fold: wqkv_f and w1_f bitwise")

    # ---- q/k/v
    if folds:
        qkv = _check_qkv_folded(tag, vP, x0, 0, cfg, n, hm, lines)
    else:   # layernorm_kernel (h not kept: LN2 overwrites it) + GE_BIAS: two roundings, the flips of h go through |W|
        h = cs.layernorm64(x0, w["ln1_g"], w["ln1_b"], eps)
        h_r = cs.rne_bf16(h)
        ref_exact = h @ cs.d64(w["wqkv"]).t() + cs.d64(w["bqkv"])
        ref_stored, E = _plain_gemm(h_r, w["wqkv"], w["bqkv"])
        E = E + cs.flips(h, cs.layernorm_err(x0, w["ln1_g"], w["ln1_b"], eps)) @ cs.d64(w["wqkv"]).abs().t()
        qkv = vP["qkv"]
        cs.check_two_roundings(f"{tag} qkv (layernorm + GE_BIAS)", qkv, ref_exact, ref_stored, cs.bound_bf16(ref_stored, E), lines)
        del h, h_r, ref_exact, ref_stored, E

    # ---- attention from the stored q | k | v
    out, pv_abs, qk_abs = cs.attention64(qkv, n, S, heads)
    E = cs.attention_err(out, pv_abs, qk_abs, S, heads)
    kern = f"clip_attn257_kernel hm={int(hm)}" if S == 257 else "clip_attn_kernel<0>"
    cs.check(f"{tag} attention ({kern}, S={S})", vP["a"].view(n, S, Cn), out, cs.bound_bf16(out, E), lines=lines,
             tile=lambda r, c: f"(frame {r // S} token {r % S} head {c // 64})")
    del out, pv_abs, qk_abs, E, qkv

    # ---- out-proj in place: x1 = a wo^T + bo + x0
    WQ, _, vQ = _run(cfg, _zeroed(state, 0, ("mlp.fc2",)), px, fold)
    assert torch.equal(vQ["a"], vP["a"])
    x1 = vQ["x"]
    ref, E = _plain_gemm(vQ["a"], w["wo"], w["bo"], x0)
    cs.check(f"{tag} out-proj ({'GE_RESID_ST' if folds else 'GE_RESID'}, K={Cn})", x1, ref, cs.bound_bf16(ref, E), lines=lines)
    del ref, E

    # ---- LN2: statistics (folded) or rows (unfolded), then fc1
    if folds:
        r, nmr = cs.row_stats64(x1, eps)
        rel_r, d_nmr = cs.stats_err(x1, eps)
        fin = "stats_finalize16_kernel" if Cn == 1024 else f"stats_finalize_kernel np={Cn // 64}"
        cs.check(f"{tag} LN2 rstd (GE_RESID_ST + {fin})", vQ["stats"][:, 0], r, r * rel_r, lines=lines, rounded=False)
        cs.check(f"{tag} LN2 -mean.rstd", vQ["stats"][:, 1], nmr, d_nmr, lines=lines, rounded=False)
        y, Ey = _folded_gemm(x1, vQ["w1_f"][0], vQ["c1"][0], vQ["d1"][0], eps)
    else:
        ref = cs.layernorm64(x1, w["ln2_g"], w["ln2_b"], eps)
        cs.check(f"{tag} LN2 (layernorm_kernel, C={Cn})", vQ["h"], ref, cs.bound_bf16(ref, cs.layernorm_err(x1, w["ln2_g"], w["ln2_b"], eps)), lines=lines)
        y, Ey = _plain_gemm(vQ["h"], w["w1"], w["b1"])
    ref, E = cs.quick_gelu64(y), cs.quick_gelu_err(y, Ey)
    cs.check(f"{tag} fc1 ({'GE_GELU_LN' if folds else 'GE_GELU'})", vQ["u"], ref, cs.bound_bf16(ref, E), lines=lines)
    del y, Ey, ref, E

    # ---- fc2 in place: x2 = u w2^T + b2 + x1; pool + project
    WR, feat, vR = _run(cfg, state, px, fold)
    assert torch.equal(vR["u"], vQ["u"])
    x2 = vR["x"]
    ref, E = _plain_gemm(vR["u"], w["w2"], w["b2"], x1)
    cs.check(f"{tag} fc2 (GE_RESID, K={cfg['mlp']})", x2, ref, cs.bound_bf16(ref, E), lines=lines)
    del ref, E
    rows0 = x2.view(n, S, Cn)[:, 0]
    ref = cs.layernorm64(rows0, w["post_g"], w["post_b"], eps)
    cs.check(f"{tag} pooled (strided post-LN)", vR["pooled"], ref, cs.bound_bf16(ref, cs.layernorm_err(rows0, w["post_g"], w["post_b"], eps)), lines=lines)
    ref = cs.d64(vR["pooled"]) @ cs.d64(w["proj"]).t()
    cs.check(f"{tag} features (GE_F32)", feat, ref, (Cn + 1) * cs.U * cs.gemm_abs64(vR["pooled"], w["proj"]), lines=lines, rounded=False)
    del vP, vQ, vR, WP, WQ, WR

    # ---- run T: the statistics of the fc2 epilogue (GE_RESID_ST, K = mlp) through block 1's folded q/k/v
    if folds and run_t:
        cfg2 = dict(cfg, layers=2)
        st2 = _zeroed(_state(cfg2, heavy), 1, ("self_attn.out_proj", "mlp.fc2"))
        WT, _, vT = _run(cfg2, st2, px, True)
        _check_qkv_folded(f"{tag} run T: fc2 statistics ->", vT, vT["x"], 1, cfg2, n, hm, lines)
        r, nmr = cs.row_stats64(vT["x"], eps)
        rel_r, d_nmr = cs.stats_err(vT["x"], eps)
        cs.check(f"{tag} run T: rstd of x2", vT["stats"][:, 0], r, r * rel_r, lines=lines, rounded=False)
        cs.check(f"{tag} run T: -mean.rstd of x2", vT["stats"][:, 1], nmr, d_nmr, lines=lines, rounded=False)
    torch.cuda.empty_cache()
    return lines


BIG = [("l14_70_fold", L14, 70, True, "u8", False), ("l14_70_nofold", L14, 70, False, "u8_misaligned", False),
       ("l14_64_fold", L14, 64, True, "u8", False), ("l14_70_heavy", L14, 70, True, "f16", True),
       ("vitb16_112_fold", VITB16, 112, True, "u8", False), ("vitb16_112_nofold", VITB16, 112, False, "bf16", False),
       ("h512_130_fold", H512, 130, True, "f32", False)]


@pytest.mark.parametrize("tag,cfg,n,fold,pix,heavy", BIG, ids=[b[0] for b in BIG])
def test_encoder_stages_production_sizes(tag, cfg, n, fold, pix, heavy):
    """Every row of the stage table (module docstring) at the sizes where the persistent GEMM, the folded epilogues and the
    statistics kernels run.  CLIP-L/14 at 70 frames: M = 17 990 = 70 whole 256-row tiles + a ragged one (the 64x64 remainder
    sub-tiles), fold on (GE_BIAS_LN_HM, clip_attn257_kernel hm = 1, GE_RESID_ST, stats_finalize16_kernel, GE_GELU_LN) and off
    (layernorm_kernel<2>, GE_BIAS, clip_attn257_kernel hm = 0, GE_RESID, GE_GELU on the persistent kernel); 64 frames = the fold
    boundary; heavy-tailed weights (rows far from zero mean, gains 0.1 - 10: y = rstd acc + (-mean rstd) c[n] + d[n] cancels).
    CLIP ViT-B/16 at 112 frames (M = 22 064, S = 197): GE_BIAS_LN row-major, clip_attn_kernel<0> with 13 key tiles and 5 valid
    keys in the last, stats_finalize_kernel with np = 12, patch K = 768.  hidden 512 at 130 frames: head-major with N = 1536,
    stats_finalize_kernel with np = 8.  All three fold as the issue expects - asserted, so a change of the fold rule cannot
    turn these cases into repeats of the unfolded ones."""
    _stages(tag, cfg, n, fold, pix, heavy, must_fold=True)


SMALL = [("s2", _small(128, 14), 3), ("s17", _small(128, 56), 3), ("s65", _small(128, 112), 3), ("s226", _small(128, 210), 3),
         ("s257_3", _small(128, 224), 3), ("c192", _small(192, 28, 64), 2), ("c1088", _small(1088, 28, 128), 2),
         ("c2048", _small(2048, 28, 256), 2), ("c4096", _small(4096, 28, 64), 2)]


@pytest.mark.parametrize("tag,cfg,n", SMALL, ids=[s[0] for s in SMALL])
def test_encoder_stages_small_models(tag, cfg, n):
    """The kernels whose edges are in S and C, on models small enough to cost nothing (none folds; every GEMM is the
    small-problem kernel).  clip_attn_kernel<0> at S = 2 (one patch: one key besides the class token), 17 (one key tile + 1),
    65 (four tiles + 1: the two-tiles-at-a-time pass AND the single-tile pass) and 226 (image = 15 patches: the largest S the
    generic kernel sees); clip_attn257_kernel with hm = 0 on 3 frames (grid not a multiple of 8: the identity item map);
    layernorm_kernel at hidden = 192 (<2>, a partly filled 512-column chunk), 1088 (<4>, partly filled third chunk), 2048 (<4>
    full) and 4096 (<8>): pre-LN in place, LN1, LN2 and the strided post-LN."""
    _stages(tag, cfg, n, False, "u8")


@pytest.mark.parametrize("n", [70, 3])
def test_prune_last_layer_class_token_attention(n):
    """clip_attn_cls_kernel (prune_last_layer=True): the compact [n_frames, hidden] rows of `a` against float64 attention of
    query row 0 from the stored q | k | v - head-major at 70 frames (the folded q/k/v GEMM wrote it, hm = 1), row-major at 3
    (hm = 0).  Bound: _clip_stages.attention_err (this kernel keeps P in fp32, so the bf16-P term is slack here)."""
    cfg = L14
    px = _pixels("u8", n, 224, 7 + n)
    W, feat, v = _run(cfg, _state(cfg, False), px, True, prune=True)
    hm = W.library_folds(n)
    assert hm == (n == 70)
    M, Cn = n * 257, cfg["hidden"]
    qkv = cs.read_head_major(v["qkv"], M, Cn) if hm else v["qkv"]
    out, pv_abs, qk_abs = cs.attention64(qkv, n, 257, cfg["heads"], rows=[0])
    E = cs.attention_err(out, pv_abs, qk_abs, 257, cfg["heads"])
    got = v["a"].reshape(-1)[:n * Cn].view(n, 1, Cn)
    cs.check(f"prune_{n} attention (clip_attn_cls_kernel hm={int(hm)})", got, out, cs.bound_bf16(out, E),
             tile=lambda r, c: f"(frame {r} head {c // 64})")
    assert torch.isfinite(feat).all()


@pytest.mark.parametrize("cfg,n", [(L14, 63), (L14, 64), (VITB16, 110), (VITB16, 111)], ids=["l14_63", "l14_64", "vitb16_110", "vitb16_111"])
def test_library_folds_matches_the_library_at_the_boundary(cfg, n):
    """ADVICE r6, first item: ClipVitWeights.library_folds() mirrors the library's fold decision in Python; if the two drift the
    fold cache trusts weights nobody wrote.  At the boundary (CLIP-L/14: 63 frames do not fold, 64 do; ViT-B/16: 110 / 111) the
    front of the workspace (wqkv_f) and the statistics partials (spart) are filled with a sentinel, one encode runs, and the
    library has written them exactly when library_folds(n) says it folds."""
    W = ops.ClipVitWeights({k: torch.from_numpy(np.asarray(v)) for k, v in _state(cfg, False).items()}, cfg, DEV)
    says = W.library_folds(n)
    assert says == (n in (64, 111))
    v = cs.views(W, n)
    for nm in ("wqkv_f", "spart"):
        v[nm].view(-1).view(torch.uint8).fill_(0xA5)
    feat = ops.clip_vit_forward(W, _pixels("u8", n, cfg["image"], 3))
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all()
    for nm in ("wqkv_f", "spart"):
        b = v[nm].view(-1).view(torch.uint8)
        untouched = int((b == 0xA5).sum())
        if says:   # every element written (a float / bf16 whose bytes are all 0xA5 would be -2.9e-16 / the same: not a value here)
            assert untouched < 0.02 * b.numel(), f"{nm}: library_folds says the library folds, {untouched} of {b.numel()} bytes untouched"
        else:
            assert untouched == b.numel(), f"{nm}: library_folds says no fold, but {b.numel() - untouched} bytes were written"


EDGE = [(70001, 264, 128), (20011, 1000, 192), (9000, 3000, 320), (66000, 256, 640), (5000, 4096, 128)]


def _rand_bf16(shape, seed, std=1.0):
    return torch.from_numpy(synth.normal(shape, seed, std)).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("M,N,K", EDGE, ids=[f"{m}x{n}x{k}" for m, n, k in EDGE])
def test_gemm_f32_output_on_the_persistent_kernel(M, N, K):
    """GE_F32 of gemm_bf16_a9_kernel (epilogue 3): tspo_gemm_bf16(..., TSPO_F32) on the shapes of
    test_gemm_dma_kernel_edge_shapes (ragged M and N, 2 / 3 / 5 K-steps, one column tile, the widest N), kernel choice 0
    (automatic = persistent for these), 77 and 83: EVERY element against float64 within E = (K + 1) u sum_k |a_k w_k| (no
    rounding to bf16: E alone), and 77 == 83 == 0 bitwise."""
    A, W = _rand_bf16((M, K), 21 + N), _rand_bf16((N, K), 22 + K, 0.05)
    ref = cs.d64(A) @ cs.d64(W).t()
    E = (K + 1) * cs.U * cs.gemm_abs64(A, W)
    outs = {}
    for var in (0, 77, 83):
        outs[var] = ops.gemm_bf16(A, W, out_f32=True, act=var << 8)
        cs.check(f"gemm f32 {M}x{N}x{K} variant {var}", outs[var], ref, E, rounded=False)
    assert torch.equal(outs[77], outs[0]) and torch.equal(outs[83], outs[0])


@pytest.mark.parametrize("M,N,K", [(771, 3072, 1024), (9000, 3000, 320)], ids=["771x3072x1024", "9000x3000x320_big"])
def test_gemm_small_kernel_forced(M, N, K):
    """Kernel choice 1 (act = 1 << 8): the 128x128 small-problem kernel, on a shape it gets anyway and on one the automatic
    choice gives to the persistent kernel (asserted: choice 0 == 77 bitwise there) - bias, quick-gelu, residual and fp32
    outputs against float64, every element, 1/2 ulp_bf16 + E with E = (K + 3) u (sum |a w| + |bias| + |residual|)."""
    A, W = _rand_bf16((M, K), 31), _rand_bf16((N, K), 32, 0.05)
    bias = torch.from_numpy(synth.normal((N,), 33, 0.1)).to(DEV)
    R = _rand_bf16((M, N), 34)
    y, Ey = _plain_gemm(A, W, bias)
    cs.check(f"gemm v1 {M}x{N}x{K} bias", ops.gemm_bf16(A, W, bias=bias, act=1 << 8), y, cs.bound_bf16(y, Ey))
    g, Eg = cs.quick_gelu64(y), cs.quick_gelu_err(y, Ey)
    cs.check(f"gemm v1 {M}x{N}x{K} gelu", ops.gemm_bf16(A, W, bias=bias, act=1 | (1 << 8)), g, cs.bound_bf16(g, Eg))
    yr, Er = _plain_gemm(A, W, bias, R)
    cs.check(f"gemm v1 {M}x{N}x{K} resid", ops.gemm_bf16(A, W, bias=bias, residual=R, act=1 << 8), yr, cs.bound_bf16(yr, Er))
    ref = cs.d64(A) @ cs.d64(W).t()
    cs.check(f"gemm v1 {M}x{N}x{K} f32", ops.gemm_bf16(A, W, out_f32=True, act=1 << 8), ref, (K + 1) * cs.U * cs.gemm_abs64(A, W), rounded=False)
    if M * N >= 256 ** 3:
        assert torch.equal(ops.gemm_bf16(A, W, bias=bias), ops.gemm_bf16(A, W, bias=bias, act=77 << 8))
