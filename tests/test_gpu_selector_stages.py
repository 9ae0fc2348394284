"""Every stage of the scoring head (csrc/selector.hip) against float64 applied to that stage's own stored input, at every kernel
form the dispatch can select.  References, bounds and the precision table: tests/_selector_stages.py.  Run with -s for the worst
`err / E` per stage.

Form-to-shape map.  x = (N / 96) * ceil(BT / 64) with C integer division decides the forward / data-gradient tile
(launch_gemm_nt_p); N = D for the D x D layers (mlp.0, mlp.2 and the two data gradients), N = 3 D for q,k,v.  S = split_for(BT, D)
planes of chunk = roundup4(ceil(BT / S)) rows split the weight-gradient contraction.  "fused" = the backward that shares a launch
between a data gradient and a weight gradient: not bf16x3, D % 128 == 0 and D % 96 == 0.

  small_fused         B 2, T 350, D 768, H 8, w 12    BT 700, 11 row tiles: D x D x = 8 * 11 = 88 < 256: 32x32 tiles; q,k,v
                      x = 24 * 11 = 264 in (256, 512): 32x96 tiles.  Fused; 8 * 11 = 88 < 128 64x96 tiles: the small fused launch whose
                      weight-gradient tiles are FINAL 64x64 ones (144 of them; 5 * 144 <= 2048 also with norm_partials).
  one_per_cu_ragged   B 2, T 1000, D 768              BT 2000, 32 row tiles: D x D x = 256: the exact-fit 64x96 form (two slabs per
                      barrier) whose last row tile holds 2000 - 31 * 64 = 16 rows; q,k,v x = 768 > 512: 2-deep ring.  Large fused
                      backward (256 >= 128), S = 7 planes of 288 rows, the last with 272.
  three_deep_ragged   B 1, T 4050, D 768              64 row tiles: D x D x = 512 (neither <= 256 nor > 512): the 3-deep 64x96 form,
                      last tile 18 rows.  S = 7 planes of 580 rows, the last with 570.  T % 16 = 2: a 2-row band block.
  tile64              B 2, T 805, D 1024, w 17, M 2   BT 1610, 26 row tiles, N % 96 = 64: D x D x = 10 * 26 = 260 >= 256: the 64x64
                      tile (gemm_f32_nt_lds_kernel<EPI, 2, 4, 3, P>) for all four epilogues - ReLU (mlp.0), residual (mlp.2), mask
                      (mlp.2 data gradient), plain (mlp.0 data gradient); q,k,v (N = 3072) takes the 2-deep 64x96 form.  D % 96 != 0: unfused backward,
                      128x128 LDS weight gradient with S = 4 planes of 404 rows (last 398), colsum3 bias gradients.  Head width 128
                      at the widest window (17) of the MFMA band kernels.
  direct_wgrad        B 3, T 100, D 192, H 8          D % 128 != 0: the direct-load weight gradient (exact fp32 under bf16x3), S = 2
                      planes of 152 / 148 rows.  Head width 24: the generic band kernels, one channel per lane.
  wide_window_33/64   B 2, T 70 / B 1, T 40, D 256, H 2, w 33 / 64   window > 32: the SECOND key lane (s1 / e1 / p1, hl + 32) of the
                      generic band kernels, T > w and T < w, head width 128 = 4 channels per lane.
  d1536               B 2, T 150, D 1536, H 12        D > 1024: the second trip of row_dots in the score kernels.  Fused, 16 * 5 = 80
                      < 128: the small fused launch - FINAL 64x64 tiles (576 of them) without norm_partials; with norm_partials
                      5 * 576 > 2048, so the non-final branch (128x128 tile body inside the small launch) and reduce_segments capped at
                      2048 blocks.  The smallest D that reaches that branch: fused needs D % 384 == 0, 5 (D / 64)^2 > 2048 D >= 1344.
  tiny_T5 / tiny_T1   B 1, T 5, D 128, M 3 / B 1, T 1, D 64   T below one 16-row block, a single frame, three text rows.

Variants: every shape x {fp32, bf16x3, bf16_mixed} x {no lengths, lengths}; the policy form, norm_partials and accumulate on the
shapes named at each test.  Lengths: one video full, the others with L % 16 in {0, 1, other}, one L < w where B allows."""
import functools
import math

import pytest
import torch

import _selector_stages as S
from tspo_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU = 0.025

#        name                 B, T,    D,    H,  w,  M
CASES = {"small_fused":       (2, 350, 768, 8, 12, 1),
         "one_per_cu_ragged": (2, 1000, 768, 8, 12, 1),
         "three_deep_ragged": (1, 4050, 768, 8, 12, 1),
         "tile64":            (2, 805, 1024, 8, 17, 2),
         "direct_wgrad":      (3, 100, 192, 8, 12, 1),
         "wide_window_33":    (2, 70, 256, 2, 33, 1),
         "wide_window_64":    (1, 40, 256, 2, 64, 1),
         "d1536":             (2, 150, 1536, 12, 12, 1),
         "tiny_T5":           (1, 5, 128, 8, 12, 3),
         "tiny_T1":           (1, 1, 64, 8, 12, 1)}
# one video full, the others L % 16 in {0, 1, other} across the shapes, L < w where B > 1 allows; B = 1: a single L < T (T = 1: L = 1)
LENGTHS = {"small_fused": (350, 177), "one_per_cu_ragged": (1000, 640), "three_deep_ragged": (2049,), "tile64": (805, 11),
           "direct_wgrad": (100, 33, 7), "wide_window_33": (70, 17), "wide_window_64": (25,), "d1536": (150, 96), "tiny_T5": (3,),
           "tiny_T1": (1,)}
PRECISIONS = ("fp32", "bf16x3", "bf16_mixed")
POLICY_SHAPES = ("small_fused", "one_per_cu_ragged", "d1536")


@functools.lru_cache(maxsize=None)
def _inputs(name, padded):
    """Built once per (shape, padded) and never written.  padded: the padding rows of img / clip / dscores hold finite junk."""
    B, T, D, H, w, M = CASES[name]
    g = torch.Generator(device=DEV).manual_seed(4000 + sorted(CASES).index(name))
    rn = lambda shape, std=1.0: torch.randn(*shape, generator=g, device=DEV) * std
    x = {"flat": rn((ops.flat_offsets(D)["__total__"][0],), 0.5 / math.sqrt(D)), "img": rn((B, T, D)), "txt": rn((B, M, D)),
         "clip": rn((B, T), 0.1), "ds": rn((B, T), 0.01)}
    if padded:
        for b, L in enumerate(LENGTHS[name]):
            x["img"][b, L:] = rn((T - L, D), 1e3)
            x["clip"][b, L:] = rn((T - L,), 1e3)
            x["ds"][b, L:] = rn((T - L,), 1e3)
    torch.cuda.synchronize()
    return x


def _lens(name, padded):
    B, T = CASES[name][:2]
    return LENGTHS[name] if padded else (T,) * B


def _valid_rows(name, padded):
    B, T = CASES[name][:2]
    L = torch.tensor(_lens(name, padded), device=DEV)
    return torch.arange(T, device=DEV)[None, :] < L[:, None]                               # [B, T]


def _forward(name, precision, padded):
    B, T, D, H, w, M = CASES[name]
    x = _inputs(name, padded)
    ws = ops.selector_workspace(B, T, D, H, M, w, DEV)
    ws.fill_(0xFF)                                      # NaN as fp32: a wrong layout, or a slot a stage should have written, shows
    kw = {"lengths": list(LENGTHS[name])} if padded else {}
    scores, attn, ws = ops.selector_forward(x["flat"], x["img"], x["txt"], x["clip"], H, w, TAU, want_attn=True, ws=ws,
                                            precision=precision, **kw)
    return x, ws, S.views(ws, B, T, D, H, w), scores, attn, kw


def _per_video(name, padded):
    B, T = CASES[name][:2]
    return [(b * T, L) for b, L in enumerate(_lens(name, padded))]


def _cat(parts):
    return [torch.cat(p) for p in zip(*parts)]


def _check_forward(rep, name, precision, padded, x, v, scores, attn):
    B, T, D, H, w, M = CASES[name]
    W = S.grad_views(x["flat"], D)                       # (the parameter bucket has the layout of the gradient bucket)
    how = S.arith(precision, "forward", D)
    valid = _valid_rows(name, padded)
    rows = valid.reshape(-1)
    ref, E = S.posenc64(x["img"], _lens(name, padded))
    rep.check("position add", v["xpe"].view(B, T, D), ref, E)
    rep.check("q,k,v projection", v["qkv"], *S.linear64(v["xpe"], W["wqkv"], W["bqkv"], how))
    soft, ctxs, tail_ok = [], [], True
    for r0, L in _per_video(name, padded):
        qkv, P = v["qkv"][r0:r0 + L], v["P"][r0:r0 + L]
        _, inwin, _ = S.band_index(L, w, DEV)
        tail_ok &= bool((P.masked_select(~inwin[:, None, :].expand_as(P)) == 0).all())
        soft.append((P,) + S.band_softmax64(qkv, H, w))
        ctxs.append((v["ctx"][r0:r0 + L],) + S.band_context64(P, qkv, H, w))
    rep.check("band softmax", *_cat(soft))
    rep.exact("band softmax: slots past the clipped window are exactly 0", tail_ok, "a slot past the clipped window is not 0")
    rep.check("band context", *_cat(ctxs))
    ref, E = S.linear64(v["ctx"], W["w1"], W["b1"], how)
    rep.check("mlp.0", v["h1"], torch.relu(ref), E)     # relu is 1-Lipschitz: where |pre-activation| <= E both 0 and the value pass
    rep.check("mlp.2", v["h2"], *S.linear64(v["h1"], W["w2"], W["b2"], how, resid=x["img"].view(B * T, D)))
    ref, E = S.score64(v["h2"].view(B, T, D), x["txt"], x["clip"], TAU, valid)
    rep.check("score", scores[valid], ref[valid], E[valid])
    rep.exact("score: temporal_attn is h2 bitwise", S.bits_equal(attn.view(B * T, D), v["h2"]), "temporal_attn differs from the stored h2")
    if padded:
        rep.exact("padding: scores are -inf", bool((scores[~valid] == float("-inf")).all()), "a padding score is not -inf")
        for n_ in ("xpe", "ctx"):
            rep.exact(f"padding: rows of {n_} are exactly 0", bool((v[n_][~rows] == 0).all()), f"a padding row of {n_} is not 0")


def _check_backward(rep, name, precision, padded, x, v, grad, ds, E_ds):
    """ds / E_ds [B, T]: dL/dscores in float64 and the bound of the kernel's own evaluation of it (0 where it is an input)."""
    B, T, D, H, w, M = CASES[name]
    valid = _valid_rows(name, padded)
    rows = valid.reshape(-1)
    unit, E_unit = S.score_grad_unit64(v["h2"].view(B, T, D), x["txt"], TAU)
    vm = valid[..., None]
    ref = torch.where(vm, ds[..., None] * unit, torch.zeros_like(unit))
    E = torch.where(vm, ds.abs()[..., None] * E_unit + E_ds[..., None] * unit.abs(), torch.zeros_like(unit))
    rep.check("score gradient", v["dh2"].view(B, T, D), ref, E)
    W = S.grad_views(x["flat"], D)
    rep.exact("weight transposes", S.bits_equal(v["w1t"], W["w1"].t().contiguous()) and S.bits_equal(v["w2t"], W["w2"].t().contiguous()),
              "w1t / w2t are not bitwise the transposes")
    how = S.arith(precision, "dgrad", D)
    ref, mag, n = S.gemm64(v["dh2"], v["w2t"], how)
    mask = (v["h1"] > 0).double()                       # the stored mask: no kink ambiguity
    rep.check("mlp.2 data gradient", v["dh1"], ref * mask, (n + S.C_SUM) * S.U * mag * mask)
    ref, mag, n = S.gemm64(v["dh1"], v["w1t"], how)
    rep.check("mlp.0 data gradient", v["dctx"], ref, (n + S.C_SUM) * S.U * mag)
    bq, bkv, tail_ok = [], [], True
    for r0, L in _per_video(name, padded):
        sl = slice(r0, r0 + L)
        qkv, P, dS, dctx, dqkv = v["qkv"][sl], v["P"][sl], v["dS"][sl], v["dctx"][sl], v["dqkv"][sl]
        _, inwin, _ = S.band_index(L, w, DEV)
        tail_ok &= bool((dS.masked_select(~inwin[:, None, :].expand_as(dS)) == 0).all())
        dS_ref, E_dS, dq, E_dq = S.band_bwd_q64(qkv, P, dctx, dS, H, w)
        bq.append((dS, dS_ref, E_dS, dqkv[:, :D], dq, E_dq))
        dk, E_dk, dv, E_dv = S.band_bwd_kv64(qkv, P, dS, dctx, H, w)
        bkv.append((dqkv[:, D:2 * D], dk, E_dk, dqkv[:, 2 * D:], dv, E_dv))
    c = _cat(bq)
    rep.check("band backward, queries: dS", *c[:3])
    rep.exact("band backward, queries: dS past the clipped window is exactly 0", tail_ok, "a dS slot past the clipped window is not 0")
    rep.check("band backward, queries: dq", *c[3:])
    c = _cat(bkv)
    rep.check("band backward, keys: dk", *c[:3])
    rep.check("band backward, keys: dv", *c[3:])
    G = S.grad_views(grad, D)
    how = S.arith(precision, "wgrad", D)
    for wn, bn, dY, X in (("w2", "b2", v["dh2"], v["h1"]), ("w1", "b1", v["dh1"], v["ctx"]), ("wqkv", "bqkv", v["dqkv"], v["xpe"])):
        ref, E, bref, Eb = S.weight_grad64(dY, X, rows, how)
        rep.check(f"weight gradients: {wn}", G[wn], ref, E)
        rep.check(f"weight gradients: {bn}", G[bn], bref, Eb)
    if padded:
        for n_ in ("dh2", "dh1", "dctx", "dqkv"):
            rep.exact(f"padding: rows of {n_} are exactly 0", bool((v[n_][~rows] == 0).all()), f"a padding row of {n_} is not 0")


def _bucket(x):
    return torch.full_like(x["flat"], float("nan"))     # every trainable element must be WRITTEN by an overwriting backward


# ------------------------------------------------------------------------------------------------------- 1. every stage, every form
@pytest.mark.parametrize("padded", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_against_float64(name, precision, padded):
    B, T, D, H, w, M = CASES[name]
    rep = S.Report(f"{name} {precision} {'lengths' if padded else 'full'}")
    x, ws, v, scores, attn, kw = _forward(name, precision, padded)
    _check_forward(rep, name, precision, padded, x, v, scores, attn)
    grad = _bucket(x)
    ops.selector_backward(x["flat"], grad, x["img"], x["txt"], x["ds"], H, w, TAU, ws, precision=precision, **kw)
    ds = x["ds"].double()
    _check_backward(rep, name, precision, padded, x, v, grad, ds, torch.zeros_like(ds))
    rep.finish()


# ----------------------------------------------------------------------------------------------- 2. policy form and norm_partials
def _policy(name, precision, G, k, norm, accumulate=False, state=None):
    """forward -> rollouts -> policy_backward on a NaN-filled bucket (or, accumulate, on the bucket of `state`)."""
    B, T, D, H, w, M = CASES[name]
    if state is None:
        x, ws, v, scores, _, _ = _forward(name, precision, False)
        g = torch.Generator(device=DEV).manual_seed(77)
        ro = ops.gumbel_topk(scores, k, G, seed=5, offset=2)
        rew = (torch.rand(B, G, generator=g, device=DEV) > 0.5).float() + torch.rand(B, G, generator=g, device=DEV)
        state = dict(x=x, ws=ws, v=v, ro=ro, rew=rew, grad=_bucket(x), part=torch.full((2048,), float("nan"), device=DEV))
    x, ro = state["x"], state["ro"]
    out = ops.policy_backward(x["flat"], state["grad"], x["img"], x["txt"], state["rew"], ro["logp"], ro["idx"], H, w, TAU, state["ws"],
                              scale=1.0 / B, precision=precision, norm_partials=state["part"] if norm else None, accumulate=accumulate)
    state.update(adv=out[0], loss=out[1], npart=out[2] if norm else None)
    return state


POLICY = [((4, 8), False, "fp32"), ((3, 100), False, "fp32"), ((4, 8), True, "fp32"), ((3, 100), True, "bf16_mixed"),
          ((4, 8), True, "bf16x3")]


@pytest.mark.parametrize("Gk,norm,precision", POLICY, ids=[f"G{g}k{k}-{'norm_partials' if n else 'plain'}-{p}" for (g, k), n, p in POLICY])
@pytest.mark.parametrize("name", POLICY_SHAPES)
def test_policy_form_and_norm_partials(name, Gk, norm, precision):
    """policy_backward derives dL/dscores itself: G * k = 32 <= 256 takes the ballot membership test, 300 the binary search.  With
    norm_partials, d1536 takes the non-final small fused launch (fp32, bf16_mixed) and reduce_segments capped at 2048 blocks."""
    B, T, D, H, w, M = CASES[name]
    G, k = Gk
    st = _policy(name, precision, G, k, norm)
    rep = S.Report(f"{name} {precision} policy G{G} k{k}{' norm_partials' if norm else ''}")
    a, E_a, loss, E_l = S.advantage64(st["rew"], st["adv"], 1e-4)
    rep.check("score gradient, policy form: adv", st["adv"], a, E_a)
    rep.check("score gradient, policy form: loss", st["loss"], loss, E_l)
    ds, E_ds = S.pg_dscores64(st["adv"], st["ro"]["logp"], st["ro"]["idx"], 1.0 / B)
    _check_backward(rep, name, precision, False, st["x"], st["v"], st["grad"], ds, E_ds)
    if norm:
        n = ops.trainable_numel(D)
        assert 1 <= st["npart"] <= 2048
        ref_norm = float(torch.linalg.vector_norm(st["grad"][:n].double()))
        got = float(st["part"][:st["npart"]].double().sum().sqrt())
        rep.lines.append(f"[stage] {rep.case}: gradient norm partials: {st['npart']} partials, |norm - ref| / ref "
                         f"{abs(got - ref_norm) / ref_norm:.3g} (bound 2e-6)")
        rep.exact("gradient norm partials", abs(got - ref_norm) <= 2e-6 * ref_norm,      # the bound of tests/test_gpu_dp.py
                  f"norm from the partials {got!r}, from the bucket {ref_norm!r}")
    rep.finish()


# ------------------------------------------------------------------------------------------------------------------ 3. accumulate
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,route", [("one_per_cu_ragged", "selector_backward"), ("d1536", "selector_backward"),
                                        ("d1536", "norm_partials")])
def test_second_accumulating_call_doubles_the_gradient_bitwise(name, route, precision):
    """The same backward twice, the second with accumulate=True: g + g = 2 g exactly (one rounding, of an exact sum).  d1536 through
    selector_backward writes final 64x64 tiles, with norm_partials it goes through reduce_segments."""
    B, T, D, H, w, M = CASES[name]
    n = ops.trainable_numel(D)
    if route == "norm_partials":
        st = _policy(name, precision, 4, 8, True)
        first = st["grad"][:n].clone()
        st = _policy(name, precision, 4, 8, True, accumulate=True, state=st)
        grad = st["grad"]
    else:
        x, ws, v, _, _, _ = _forward(name, precision, False)
        grad = _bucket(x)
        ops.selector_backward(x["flat"], grad, x["img"], x["txt"], x["ds"], H, w, TAU, ws, precision=precision)
        first = grad[:n].clone()
        ops.selector_backward(x["flat"], grad, x["img"], x["txt"], x["ds"], H, w, TAU, ws, precision=precision, accumulate=True)
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    assert S.bits_equal(grad[:n], 2 * first), f"{int((grad[:n] != 2 * first).sum())} of {n} elements differ from twice the first call"
