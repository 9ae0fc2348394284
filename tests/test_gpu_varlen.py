"""GPU tests of the policy step over videos of DIFFERENT lengths in one padded batch (the `_len` entries of include/tspo_hip.h,
`lengths=` of ops / PolicyTrainer / MultiModal_Align.forward_batched, `train._pad_stack`).

The expected values are the project's own un-padded entries run per video on its `[:L_b]` slice - the paths the oracle and golden
tests already pin - plus the oracle's autograd per video.  Lengths (83, 17, 48, 33, 64) padded to T = 83: partial and whole 16-row
blocks of padding, one video just past a block (17, 33), one exact multiple of 64.  Shapes, one per internally different path:
  D = 384, H = 4   head width 96 on the MFMA band kernels, fused backward, whole-contraction 64x64 weight gradients
  D = 128, H = 2   head width 64 on the MFMA band kernels, unfused backward, column-sum kernel + split reduction
  D = 192, H = 8   head width 24: the scalar band kernels
Tolerances are the ones the existing tests use for the same comparison and are named where they are used."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _contract as K
from _policy_full import check_every_element
from oracle import tspo_oracle as O
from tspo_amd import _lib, ops
from tspo_amd.pipeline import PolicyTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, G, KSEL, TAU = 12, 4, 8, 0.025
LENS = (83, 17, 48, 33, 64)
B, T = len(LENS), max(LENS)
SEED, OFFSET = 2024, 5
SHAPES = [(384, 4, 1), (128, 2, 3), (192, 8, 1)]
IDS = [f"D{d}-H{h}-M{m}" for d, h, m in SHAPES]
TRAINED = [n for n in O.SELECTOR_KEYS if "ffn_o" not in n]


def _zero_padding(x, lens=LENS):
    for b, L in enumerate(lens):
        x[b, L:] = 0
    return x


# Seeds of the inputs, per D.  The oracle comparison differentiates through a ReLU: where a pre-activation of mlp.0 lies within fp32
# rounding of zero, the GPU and the CPU oracle may take different sides of the kink and a whole row of the mlp.0 weight gradient
# differs by that frame's term - nothing to do with padding (the un-padded calls differ the same way).  The inputs are therefore
# drawn on the CPU, from the first seed >= 300 for which the oracle's smallest |pre-activation| over the 245 valid frames is at
# least 5e-6 (fp32 rounding of these sums is ~1e-7); test_gradients_against_the_oracle_autograd_per_video asserts that margin.
SEEDS = {384: 304, 128: 300, 192: 300}
MIN_PREACT = 5e-6


@functools.lru_cache(maxsize=None)
def _host_inputs(D, M, Gn=G, seed=None):
    g = torch.Generator().manual_seed(SEEDS[D] if seed is None else seed)
    rn = lambda shape, std=1.0: torch.randn(*shape, generator=g) * std
    flat = rn((ops.flat_offsets(D)["__total__"][0],), 0.5 / np.sqrt(D))
    img, txt, clip = _zero_padding(rn((B, T, D))), rn((B, M, D)), _zero_padding(rn((B, T), 0.1))
    rew = (torch.rand(B, Gn, generator=g) > 0.5).float() + torch.rand(B, Gn, generator=g)
    noise = -torch.log(-torch.log(torch.rand(B, Gn, T, generator=g).clamp(1e-6, 1 - 1e-6)))
    for b, L in enumerate(LENS):
        noise[b, :, L:] = 0
    return flat, img, txt, clip, rew, noise


@functools.lru_cache(maxsize=None)
def _inputs(D, M, Gn=G):
    """Built once per shape and never written: flat, img [B,T,D] and clip [B,T] with zero padding, txt, rewards, Gumbel noise."""
    out = tuple(t.to(DEV) for t in _host_inputs(D, M, Gn))
    torch.cuda.synchronize()
    return out


def _oracle_step(D, H, M, idx, scale, seed=None):
    """The oracle per video on [:L_b] (CPU autograd) for the given rollouts: (scores per video, adv per video, {name: gradient of
    scale x the summed loss}, the smallest |pre-activation| of mlp.0)."""
    flat, img, txt, clip, rew, _ = _host_inputs(D, M, G, seed)
    ps = {n: v.clone().requires_grad_(True) for n, v in K.state_from_flat(flat, D).items()}
    pre, relu = [], F.relu
    F.relu = lambda x: (pre.append(float(x.detach().abs().min())), relu(x))[1]
    try:
        confs, advs, total = [], [], 0.0
        for b, L in enumerate(LENS):
            conf, _ = O.selector_forward(ps, img[b, :L], txt[b], clip[b, :L], W, TAU, H)
            adv = O.grpo_advantage(rew[b], G)
            confs.append(conf.detach())
            advs.append(adv)
            if idx is not None:
                logp = F.softmax(conf, dim=0).log()
                total = total + O.pg_loss([logp[i] for i in idx[b]], adv) * scale
    finally:
        F.relu = relu
    if idx is None:
        return confs, advs, None, min(pre)
    total.backward()
    return confs, advs, {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in ps.items()}, min(pre)


def _poisoned_ws(D, H, M, nb=B, t=T):
    ws = ops.selector_workspace(nb, t, D, H, M, W, DEV)
    ws.fill_(0xFF)                                      # NaN as fp32: whatever the call reads without writing it first shows
    return ws


def _padded(D, H, M, precision="fp32", img=None, clip=None, lengths=LENS, Gn=G, noise=None, path="policy_backward", backward=True):
    """One padded call chain: forward -> rollouts -> backward into a zeroed bucket."""
    flat, img0, txt, clip0, rew, _ = _inputs(D, M, Gn)
    img, clip = img0 if img is None else img, clip0 if clip is None else clip
    kw = {} if lengths is None else {"lengths": list(lengths)}
    scores, _, ws = ops.selector_forward(flat, img, txt, clip, H, W, TAU, want_attn=False, ws=_poisoned_ws(D, H, M), precision=precision,
                                         **kw)
    ro = ops.gumbel_topk(scores, KSEL, Gn, noise=noise, seed=SEED, offset=OFFSET, prompts_per_offset=1, want_probs=True,
                         want_noise=True, **kw)
    out = {"scores": scores, "idx": ro["idx"], "logp": ro["logp"], "probs": ro["probs"], "noise": ro["noise"]}
    if not backward:
        return out
    grad = torch.zeros_like(flat)
    if path == "two_call":                              # what PolicyTrainer.backward issues for G > 64
        adv, dlog, loss = ops.grpo_pg_grad(rew, ro["logp"], ro["idx"], scale=1.0 / B, **kw)
        ops.selector_backward(flat, grad, img, txt, dlog, H, W, TAU, ws, precision=precision, **kw)
        out["dlogits"] = dlog
    elif path == "norm_partials":
        part = torch.full((2048,), float("nan"), device=DEV)
        adv, loss, npart = ops.policy_backward(flat, grad, img, txt, rew, ro["logp"], ro["idx"], H, W, TAU, ws, scale=1.0 / B,
                                               precision=precision, norm_partials=part, **kw)
        out["sumsq"] = part[:npart].double().sum()
    else:
        adv, loss = ops.policy_backward(flat, grad, img, txt, rew, ro["logp"], ro["idx"], H, W, TAU, ws, scale=1.0 / B,
                                        precision=precision, **kw)
    out.update(adv=adv, loss=loss, grad=grad)
    return out


@functools.lru_cache(maxsize=None)
def _per_video(D, H, M, precision="fp32", Gn=G, injected=False, path="policy_backward", lens=LENS):
    """The same step as B = 1 un-padded calls on the [:L_b] slices, chained with accumulate=True and the same scale; prompt b draws
    from Philox offset OFFSET + b (what prompts_per_offset = 1 means).  Computed once per configuration, never written."""
    flat, img, txt, clip, rew, noise = _inputs(D, M, Gn)
    grad = torch.zeros_like(flat)
    per = []
    for b, L in enumerate(lens):
        im, tx, cl = img[b:b + 1, :L].contiguous(), txt[b:b + 1], clip[b:b + 1, :L].contiguous()
        scores, _, ws = ops.selector_forward(flat, im, tx, cl, H, W, TAU, want_attn=False, precision=precision)
        ro = ops.gumbel_topk(scores, KSEL, Gn, noise=noise[b:b + 1, :, :L].contiguous() if injected else None, seed=SEED,
                             offset=OFFSET + b, want_probs=True, want_noise=True)
        if path == "two_call":
            adv, dlog, loss = ops.grpo_pg_grad(rew[b:b + 1], ro["logp"], ro["idx"], scale=1.0 / B)
            ops.selector_backward(flat, grad, im, tx, dlog, H, W, TAU, ws, precision=precision, accumulate=b > 0)
        else:
            adv, loss = ops.policy_backward(flat, grad, im, tx, rew[b:b + 1], ro["logp"], ro["idx"], H, W, TAU, ws, scale=1.0 / B,
                                            precision=precision, accumulate=b > 0)
        per.append({"scores": scores[0], "idx": ro["idx"][0], "logp": ro["logp"][0], "probs": ro["probs"][0], "noise": ro["noise"][0],
                    "adv": adv[0], "loss": loss[0]})
    torch.cuda.synchronize()
    return per, grad


def _tensors(grad, D):
    offs = ops.flat_offsets(D)
    return {n: grad[offs[n][0]:offs[n][0] + int(np.prod(offs[n][1]))] for n in TRAINED}


def _assert_grads_close(got, ref, D, what):
    """The criterion of tests/test_gpu_dp.py:123 for the same kind of difference (one sum over the same terms in another order),
    applied as it is there: every element of the gradient bucket within rtol 1e-4, atol 1e-6 x max|ref| of the bucket.  Also
    printed per tensor (run with -s): the difference against the tensor's own maximum.  Measured on an earlier draw of these inputs:
    7e-8 ... 1.1e-6 on every tensor of every case except mlp.2.bias at G = 80, D = 384 (2.3e-6, on one of its 384 elements, whose
    value is 6e-4 of the tensor's maximum: a column sum over 245 rows that nearly cancels), and 3e-9 ... 8e-9 of the bucket's
    maximum on the key-bias gradient, which is mathematically zero (a common key offset cancels in the softmax) and holds rounding
    noise on both sides - so a per-tensor atol would not be meaningful for it."""
    g, r = _tensors(got, D), _tensors(ref, D)
    whole = float(ref.abs().max())
    for n in TRAINED:
        err = float((g[n] - r[n]).abs().max())
        print(f"{what}: {n}: max|diff| {err:.3e} = {err / max(float(r[n].abs().max()), 1e-30):.2e} of the tensor's max|ref|, "
              f"{err / whole:.2e} of the bucket's")
        np.testing.assert_allclose(g[n].cpu().numpy(), r[n].cpu().numpy(), rtol=1e-4, atol=1e-6 * whole, err_msg=f"{what}: {n}")


def _assert_forward_and_rollouts(out, per, lens, what):
    for b, L in enumerate(lens):
        for key in ("scores", "logp"):
            assert K.bits_equal(out[key][b, :L], per[b][key]), f"{what}: {key}[{b}, :{L}] differs from the un-padded call"
            assert bool((out[key][b, L:] == float("-inf")).all()), f"{what}: {key} padding of video {b} is not -inf"
        assert torch.equal(out["idx"][b], per[b]["idx"]), f"{what}: idx[{b}]"
        assert int(out["idx"][b].max()) < L and int(out["idx"][b].min()) >= 0
        for key in ("probs", "noise"):
            assert K.bits_equal(out[key][b, :, :L], per[b][key]), f"{what}: {key}[{b}]"
            assert bool((out[key][b, :, L:] == 0).all()), f"{what}: {key} padding of video {b} is not 0"


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_forward_scores_and_logp_are_bitwise_the_unpadded_calls(D, H, M, precision):
    """Rows of the forward GEMMs do not depend on the row count (tests/test_gpu_dp.py asserts the same for the stacked window)."""
    fwd = "bf16_mixed" if precision == "bf16" else precision       # the same forward arithmetic, and _per_video can run its backward
    out = _padded(D, H, M, precision=fwd, backward=False)
    per, _ = _per_video(D, H, M, precision=fwd)
    _assert_forward_and_rollouts(out, per, LENS, f"{IDS[SHAPES.index((D, H, M))]} {precision}")
    if precision == "bf16":                                         # the inference flag itself, forward only
        flat, img, txt, clip, _, _ = _inputs(D, M)
        s16, _, _ = ops.selector_forward(flat, img, txt, clip, H, W, TAU, want_attn=False, precision="bf16", lengths=list(LENS))
        assert K.bits_equal(s16, out["scores"])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_forward_of_videos_shorter_than_the_window(D, H, M, precision):
    lens = (83, 1, 5, 17)
    g = K.gen_(77 + D)
    flat = _inputs(D, M)[0]
    img, txt, clip = K.randn((4, T, D), g), K.randn((4, M, D), g), K.randn((4, T), g, 0.1)
    scores, attn, _ = ops.selector_forward(flat, img, txt, clip, H, W, TAU, ws=_poisoned_ws(D, H, M, 4), precision=precision,
                                           lengths=list(lens))
    for b, L in enumerate(lens):
        want, wattn, _ = ops.selector_forward(flat, img[b:b + 1, :L].contiguous(), txt[b:b + 1], clip[b:b + 1, :L].contiguous(), H, W,
                                              TAU, precision=precision)
        assert K.bits_equal(scores[b, :L], want[0]), (b, L)
        assert K.bits_equal(attn[b, :L], wattn[0]), (b, L)
        assert bool((scores[b, L:] == float("-inf")).all())


# ------------------------------------------------------------------------------------------------------------------ 2. sampler
@pytest.mark.parametrize("injected", [False, True], ids=["philox", "injected"])
def test_rollouts_are_bitwise_the_single_prompt_calls(injected):
    D, H, M = SHAPES[1]
    noise = _inputs(D, M)[5] if injected else None
    out = _padded(D, H, M, noise=noise, backward=False)
    per, _ = _per_video(D, H, M, injected=injected)
    _assert_forward_and_rollouts(out, per, LENS, "injected noise" if injected else "in-kernel Philox")
    if injected:                                        # padding noise is not read: junk there changes nothing
        junk = noise.clone()
        for b, L in enumerate(LENS):
            junk[b, :, L:] = float("nan")
        again = _padded(D, H, M, noise=junk, backward=False)
        assert torch.equal(again["idx"], out["idx"]) and K.bits_equal(again["probs"], out["probs"])


def test_rollouts_of_a_long_row():
    """T = 16500 > 16384: the padded call takes the global-key kernel for both rows; the 9000-frame row alone takes the LDS one."""
    Tl, lens, k, Gn = 16500, (16500, 9000), 8, 2
    scores = K.randn((2, Tl), K.gen_(5), 3.0)
    out = ops.gumbel_topk(scores, k, Gn, seed=SEED, offset=OFFSET, prompts_per_offset=1, want_probs=True, lengths=list(lens))
    for b, L in enumerate(lens):
        one = ops.gumbel_topk(scores[b:b + 1, :L].contiguous(), k, Gn, seed=SEED, offset=OFFSET + b, want_probs=True)
        assert torch.equal(out["idx"][b], one["idx"][0]) and int(out["idx"][b].max()) < L
        assert K.bits_equal(out["logp"][b, :L], one["logp"][0]) and bool((out["logp"][b, L:] == float("-inf")).all())
        assert K.bits_equal(out["probs"][b, :, :L], one["probs"][0]) and bool((out["probs"][b, :, L:] == 0).all())


def test_sampler_rejects_k_above_min_length_and_a_bad_min_length():
    l, st = _lib.lib(), ops._stream()
    scores = K.randn((2, 40), K.gen_(6))
    idx = torch.zeros((2, 2, 8), dtype=torch.int64, device=DEV)
    lens = torch.tensor([40, 20], dtype=torch.int32, device=DEV)
    call = lambda k, ml: l.tspo_gumbel_topk_len(ops._ptr(scores), None, 1, 0, 2, 2, 40, k, 1.0, ops._ptr(idx), None, None, None, st, 0,
                                                ops._ptr(lens), ml)
    assert call(8, 7) == -1 and b"min_length" in l.tspo_last_error()
    for ml in (0, 41):
        assert call(8, ml) == -1 and b"min_length" in l.tspo_last_error()
    assert call(8, 8) == 0                               # a device value below min_length is clamped up to it: k frames are there
    torch.cuda.synchronize()
    assert int(idx.max()) < 40 and int(idx[1].max()) < 20
    with pytest.raises(RuntimeError, match="out of range"):
        ops.gumbel_topk(scores, 21, 2, lengths=[40, 20])
    with pytest.raises(ValueError, match="min_length"):
        ops.gumbel_topk(scores, 8, 2, lengths=lens)      # device lengths: the caller must vouch for a minimum


# ---------------------------------------------------------------------------------------------------------------- 3. gradients
@pytest.mark.parametrize("precision,path", [("fp32", "policy_backward"), ("bf16_mixed", "policy_backward"), ("fp32", "norm_partials"),
                                            ("fp32", "two_call")], ids=["fp32", "bf16_mixed", "norm_partials", "G80-two-call"])
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_gradients_equal_the_per_video_calls(D, H, M, precision, path):
    Gn = 80 if path == "two_call" else G                 # G > 64: grpo_pg_grad + selector_backward
    out = _padded(D, H, M, precision=precision, Gn=Gn, path=path)
    per, gref = _per_video(D, H, M, precision=precision, Gn=Gn, path="two_call" if path == "two_call" else "policy_backward")
    what = f"{IDS[SHAPES.index((D, H, M))]} {precision} {path}"
    for b, L in enumerate(LENS):
        assert torch.equal(out["idx"][b], per[b]["idx"]), what
        assert K.bits_equal(out["adv"][b], per[b]["adv"]) and K.bits_equal(out["loss"][b], per[b]["loss"]), what
        if path == "two_call":
            assert bool((out["dlogits"][b, L:] == 0).all()), "dL/dscores of padding frames must be exactly 0"
    assert bool(torch.isfinite(out["grad"]).all())
    _assert_grads_close(out["grad"], gref, D, what)
    if path == "norm_partials":                          # tests/test_gpu_dp.py:259: the norm from the partials, 2e-6 relative
        n = ops.trainable_numel(D)
        ref_norm = float(torch.linalg.vector_norm(out["grad"][:n].double()))
        assert abs(float(out["sumsq"].sqrt()) - ref_norm) <= 2e-6 * ref_norm


# --------------------------------------------------------------------------------------------------------------------- 4. oracle
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_gradients_against_the_oracle_autograd_per_video(D, H, M):
    """The oracle per video on [:L_b] with the rollouts the padded call drew; every element of every gradient at the tolerances of
    tests/_policy_full.check_every_element; the scores at the tolerance of the oracle comparisons (rtol 2e-5, atol 2e-5 / tau)."""
    out = _padded(D, H, M)
    confs, advs, ref, min_pre = _oracle_step(D, H, M, out["idx"].cpu(), 1.0 / B)
    assert min_pre >= MIN_PREACT, f"ill-conditioned inputs: a ReLU pre-activation of {min_pre:.2e} (see SEEDS)"
    for b, L in enumerate(LENS):
        np.testing.assert_allclose(out["scores"][b, :L].cpu().numpy(), confs[b].numpy(), rtol=2e-5, atol=2e-5 / TAU)
        np.testing.assert_allclose(out["adv"][b].cpu().numpy(), advs[b].numpy(), rtol=1e-5, atol=1e-6)
    offs = ops.flat_offsets(D)
    got = {n: out["grad"][offs[n][0]:offs[n][0] + int(np.prod(offs[n][1]))].cpu().numpy() for n in O.SELECTOR_KEYS}
    worst = check_every_element(got, ref, IDS[SHAPES.index((D, H, M))])
    print({n: f"{v:.2e}" for n, v in worst.items()})


# ------------------------------------------------------------------------------------------------------- 5. padding is inert
@pytest.mark.parametrize("precision", ["fp32", "bf16_mixed"])
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_padding_rows_do_not_matter_and_are_written_by_the_call(D, H, M, precision):
    """Zero padding against finite junk (randn x 1e3) in img / clip, both on a NaN-filled workspace (_padded poisons it): bitwise the
    same valid scores, rollouts, advantages, loss and all six gradient tensors, every one finite."""
    _, img, _, clip, _, _ = _inputs(D, M)
    g = K.gen_(9)
    jimg, jclip = img.clone(), clip.clone()
    for b, L in enumerate(LENS):
        jimg[b, L:] = K.randn((T - L, D), g, 1e3)
        jclip[b, L:] = K.randn((T - L,), g, 1e3)
    a, j = _padded(D, H, M, precision=precision), _padded(D, H, M, precision=precision, img=jimg, clip=jclip)
    for key in ("scores", "idx", "logp", "adv", "loss", "grad"):
        assert K.bits_equal(a[key], j[key]), f"{key} depends on the padding rows of img / clip"
    assert bool(torch.isfinite(a["grad"]).all()) and bool(torch.isfinite(a["adv"]).all()) and bool(torch.isfinite(a["loss"]).all())
    assert float(a["grad"].abs().max()) > 0


# ----------------------------------------------------------------------------------------------- 6. lengths == T is lengths=None
@pytest.mark.parametrize("precision,path", [("fp32", "policy_backward"), ("bf16_mixed", "policy_backward"), ("fp32", "two_call")])
@pytest.mark.parametrize("D,H,M", SHAPES, ids=IDS)
def test_full_lengths_are_bitwise_the_calls_without_lengths(D, H, M, precision, path):
    img, clip = K.randn((B, T, D), K.gen_(12)), K.randn((B, T), K.gen_(13), 0.1)
    a = _padded(D, H, M, precision=precision, img=img, clip=clip, lengths=None, path=path)
    f = _padded(D, H, M, precision=precision, img=img, clip=clip, lengths=(T,) * B, path=path)
    for key in ("scores", "idx", "logp", "probs", "noise", "adv", "loss", "grad"):
        assert K.bits_equal(a[key], f[key]), key


# ------------------------------------------------------------------------------------------------------------------ 7. trainer
WIN = (83, 17, 48, 33)


def _window(step, D):
    g = K.gen_(500 + step)
    out = []
    for L in WIN:
        f, t = K.randn((1, L, D), g), K.randn((1, 1, D), g)
        out.append((f, t, ops.clip_scores(t, f), (K.rand((1, G), g) > 0.5).float() + K.rand((1, G), g)))
    return out


def _pad_to(x, Tn):
    out = x.new_zeros((x.shape[0], Tn) + tuple(x.shape[2:]))
    out[:, :x.shape[1]] = x
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16_mixed"])
def test_trainer_padded_window_equals_the_sequential_micro_steps(precision):
    """Four B = 1 micro-steps of different T as ONE padded rollout / backward (`micro_steps=4, lengths=...`): the indices of the
    sequential path bit for bit (every prompt draws from the offset its own rollout() would have used), and the parameters after
    clip + AdamW within rtol 1e-5, atol 5e-7 (tests/test_gpu_dp.py:198); two optimizer steps."""
    D, H, M = SHAPES[1]
    flat0 = _inputs(D, M)[0]
    mk = lambda: PolicyTrainer(flat0.clone(), dim=D, heads=H, window_size=W, max_grad_norm=1e-3, grad_accum_steps=4, seed=77,
                               gemm_precision=precision)
    seq, pad = mk(), mk()
    for step in range(2):
        win = _window(step, D)
        outs = []
        for f, t, c, r in win:
            sc, idx, lp, ctx = seq.rollout(f, t, c, G, KSEL, TAU)
            st = seq.backward(ctx, f, t, lp, idx, r)
            outs.append((sc, idx, lp, st["advantages"], st["loss"]))
        f, c = torch.cat([_pad_to(w[0], T) for w in win]), torch.cat([_pad_to(w[2], T) for w in win])
        t, r = torch.cat([w[1] for w in win]), torch.cat([w[3] for w in win])
        sc, idx, lp, ctx = pad.rollout(f, t, c, G, KSEL, TAU, micro_steps=4, lengths=list(WIN))
        assert ctx.micro_steps == 4 and ctx.min_length == 17 and pad._rollouts == seq._rollouts
        st = pad.backward(ctx, f, t, lp, idx, r)
        assert pad.at_boundary() and seq.at_boundary()
        for b, L in enumerate(WIN):
            assert torch.equal(idx[b], outs[b][1][0]), f"step {step}: indices of prompt {b}"
            assert K.bits_equal(sc[b, :L], outs[b][0][0]) and K.bits_equal(lp[b, :L], outs[b][2][0])
            assert K.bits_equal(st["advantages"][b], outs[b][3][0]) and K.bits_equal(st["loss"][b], outs[b][4][0])
        n = seq.n_train
        _assert_grads_close(pad.grad, seq.grad, D, f"trainer step {step}")
        seq.optimizer_step()
        pad.optimizer_step()
        np.testing.assert_allclose(pad.flat[:n].cpu().numpy(), seq.flat[:n].cpu().numpy(), rtol=1e-5, atol=5e-7)
        pad.flat.copy_(seq.flat); pad.m.copy_(seq.m); pad.v.copy_(seq.v)      # (as test_gpu_dp.py: the next window checks bits again)
    with pytest.raises(RuntimeError, match="out of range"):
        pad.rollout(f, t, c, G, 18, TAU, micro_steps=4, lengths=list(WIN))    # k > the shortest video


class _Fixed:
    """A data set of prepared micro-batches, in order."""

    def __init__(self, batches):
        self.b = batches

    def batches(self, rank, world, bs, skip=0):
        assert bs == 1
        i = int(skip)
        while True:
            yield self.b[i % len(self.b)]
            i += 1


# The parameter tolerance (rtol 1e-5, atol 5e-7, tests/test_gpu_dp.py:198) was set there with a clip far below the raw gradient
# norm (MAX_NORM = 1e-3), and the driver runs below are in that regime too.  It matters: the first AdamW steps move a parameter by
# lr g / (|g| + 1e-8), so where |g| is at or below 1e-8 a rounding difference d of the gradient moves the parameter by up to
# lr d / 1e-8 = 5e4 d: d must stay below 1e-11 for atol 5e-7.  The padded and the sequential bucket differ by d ~ 1e-9 before the
# clip (1e-6 of the largest element, above); raw norms here are 0.03 - 0.05, so clipping at 1e-4 scales d to ~3e-12.  Measured on
# the D = 128 window: 0.17 of the tolerance with the clip at 1e-3 after one and after two steps, 1.25 / 2.8 x the tolerance on 3 / 24
# of 82 560 elements without a clip - a property of the optimizer at near-zero gradient entries, not of the padded path.
CLIP = 1e-4


def _train_pair(tt, data, tmp_path, flat0, **kw):
    res = {}
    for pad in (False, True):
        seen = []

        def reward(idx, batch, seen=seen):
            seen.append((idx.clone(), batch.lengths, batch.feats.shape[0]))
            return tt.mask_reward_model(idx, batch)

        cfg = tt.TrainConfig(output_dir=str(tmp_path / f"pad{int(pad)}"), pad_variable_length=pad, save_steps=100, **kw)
        m = tt.train(cfg, data, reward_model=reward, flat=flat0.clone(), resume=False)
        res[pad] = (m["flat"], seen)
    return res


def test_train_pads_a_window_of_different_lengths(tmp_path):
    """`train(pad_variable_length=True)` on feature batches of different length: one reward call per window with B = 4 and the
    lengths, the indices of the default (sequential) run bit for bit in the first window, the parameters after two optimizer steps
    within rtol 1e-5, atol 5e-7.  Off by default: the default run makes one call per micro-batch."""
    from tspo_amd import train as tt
    D, H, M = SHAPES[1]
    flat0 = _inputs(D, M)[0]
    g = K.gen_(41)
    bs = []
    for i in range(8):
        f, t = K.randn((1, WIN[i % 4], D), g), K.randn((1, 1, D), g)
        bs.append(tt.Batch(f, t, ops.clip_scores(t, f), K.rand((1, WIN[i % 4]), g) > 0.6, "specific", [{"item": i}]))
    res = _train_pair(tt, _Fixed(bs), tmp_path, flat0, max_steps=2, num_generations=G, training_sample_len=KSEL,
                      gradient_accumulation_steps=4, dim=D, heads=H, seed=3, max_grad_norm=CLIP)
    (fs, ss), (fp, sp) = res[False], res[True]
    assert [s[2] for s in ss] == [1] * 8 and all(s[1] is None for s in ss)
    assert [s[2] for s in sp] == [4, 4] and sp[0][1] == list(WIN)
    assert torch.equal(sp[0][0], torch.cat([s[0] for s in ss[:4]]))
    n = ops.trainable_numel(D)
    np.testing.assert_allclose(fp[:n].cpu().numpy(), fs[:n].cpu().numpy(), rtol=1e-5, atol=5e-7)
    assert not torch.equal(fp, flat0)


def test_train_from_frames_padded(tmp_path):
    """From frames: three small in-memory videos, `FrameDataset(pad_batches=True).batches(bs=2)` yields ONE padded micro-batch of two
    haystacks of different length whose `selected_frames` is the per-prompt result; and a window of two prepared frame batches
    through `train(pad_variable_length=True)` equals the default run."""
    from test_gpu_api import _StubProcessor
    from test_gpu_select_frames import ITEMS, _tiny_model, _videos
    from tspo_amd import preprocess as P, train as tt
    model = _tiny_model(6).to(DEV)
    vids = _videos()
    items = [dict(it, type="specific") for it in ITEMS]
    load = lambda path, *a: (vids[path.rsplit("/", 1)[-1]], None, None, None)
    mk = lambda **kw: tt.FrameDataset(items, model, _StubProcessor(), load_video=load, seed=4, device=DEV, **kw)
    with pytest.raises(ValueError, match="one prompt per micro-batch"):
        next(mk().batches(0, 1, 2))
    both = next(mk(pad_batches=True).batches(0, 1, 2))
    one = [mk().prepare(0), mk().prepare(1)]
    Ls = [b.feats.shape[1] for b in one]
    assert both.lengths == Ls and Ls[0] != Ls[1] and both.feats.shape == (2, max(Ls), 768) and len(both.frames) == 2
    for b, L in enumerate(Ls):
        assert torch.equal(both.feats[b, :L], one[b].feats[0]) and not bool(both.feats[b, L:].any()) and not bool(both.mask[b, L:].any())
    tr = PolicyTrainer(model.selector.flatten_parameters().clone(), dim=768, heads=8, window_size=W)
    scores, idx, logp, ctx = tr.rollout(both.feats, both.txt, both.clip, G, KSEL, TAU, lengths=both.lengths)
    spec = P.PreprocessSpec(size=(40, 56), out_dtype=torch.float16)
    got = both.selected_frames(idx, spec)
    for b, L in enumerate(Ls):
        assert int(idx[b].max()) < L
        assert torch.equal(got[b:b + 1], one[b].selected_frames(idx[b:b + 1], spec))
    # the driver: the two prepared batches as a window of two micro-steps, padded against sequential
    flat0 = model.selector.flatten_parameters().clone()
    res = _train_pair(tt, _Fixed(one), tmp_path, flat0, max_steps=1, num_generations=G, training_sample_len=KSEL,
                      gradient_accumulation_steps=2, dim=768, heads=8, seed=3, max_grad_norm=CLIP)
    (fs, ss), (fp, sp) = res[False], res[True]
    assert len(ss) == 2 and len(sp) == 1 and sp[0][1] == Ls
    assert torch.equal(sp[0][0], torch.cat([s[0] for s in ss]))
    n = ops.trainable_numel(768)
    np.testing.assert_allclose(fp[:n].cpu().numpy(), fs[:n].cpu().numpy(), rtol=1e-5, atol=5e-7)


def test_forward_batched_with_lengths():
    """MultiModal_Align.forward_batched(lengths=...): the no-grad path and the autograd bridge (its backward gets the lengths)."""
    from tspo_amd.temporal_agent import MultiModal_Align
    D, H, M = SHAPES[1]
    flat, img, txt, clip, _, _ = _inputs(D, M)
    mod = MultiModal_Align(dim=D, num_heads=H).to(DEV)
    mod.load_state_dict({k: v.to(DEV) for k, v in K.state_from_flat(flat, D).items()})
    with torch.no_grad():
        s0, _ = mod.forward_batched(img, txt, clip, W, TAU, lengths=list(LENS))
    want, _, _ = ops.selector_forward(flat, img, txt, clip, H, W, TAU, lengths=list(LENS))
    assert K.bits_equal(s0, want)
    ds = _zero_padding(K.randn((B, T), K.gen_(3)))
    s1, _ = mod.forward_batched(img, txt, clip, W, TAU, lengths=list(LENS))
    assert K.bits_equal(s1.detach(), want)
    torch.nan_to_num(s1, neginf=0.0).mul(ds).sum().backward()
    total = None
    for b, L in enumerate(LENS):                         # per video, without lengths
        mod2 = MultiModal_Align(dim=D, num_heads=H).to(DEV)
        mod2.load_state_dict(mod.state_dict())
        s, _ = mod2.forward_batched(img[b:b + 1, :L].contiguous(), txt[b:b + 1], clip[b:b + 1, :L].contiguous(), W, TAU)
        (s * ds[b:b + 1, :L]).sum().backward()
        gs = {n: p.grad for n, p in mod2.named_parameters() if p.grad is not None}
        total = gs if total is None else {n: total[n] + gs[n] for n in gs}
    whole = max(float(v.abs().max()) for v in total.values())
    for n, p in mod.named_parameters():
        if n in total:
            rmax = whole if n == "temporal.Self_k.bias" else float(total[n].abs().max())
            np.testing.assert_allclose(p.grad.cpu().numpy(), total[n].cpu().numpy(), rtol=1e-4, atol=1e-6 * rmax, err_msg=n)


# -------------------------------------------------------------------------------------------------------------------- 8. graph
def test_graph_replays_with_the_lengths_buffer_changed_in_place():
    """forward -> rollouts -> policy_backward captured with a device lengths buffer and min_length = 17; each replay, after the
    buffer was rewritten in place (values >= min_length) and everything else poisoned, equals its eager twin bit for bit."""
    D, H, M = SHAPES[0]
    flat, _, txt, _, rew, _ = _inputs(D, M)
    img, clip = K.randn((B, T, D), K.gen_(21)), K.randn((B, T), K.gen_(22), 0.1)
    sets = {0: LENS, 1: (40, 83, 17, 64, 20), 2: (83, 83, 17, 18, 49)}
    lens = torch.tensor(sets[0], dtype=torch.int32, device=DEV)
    ws = ops.selector_workspace(B, T, D, H, M, W, DEV)
    grad = torch.zeros_like(flat)

    def run(ln, w, gr):
        scores, _, _ = ops.selector_forward(flat, img, txt, clip, H, W, TAU, want_attn=False, ws=w, lengths=ln, min_length=17)
        ro = ops.gumbel_topk(scores, KSEL, G, seed=SEED, offset=OFFSET, prompts_per_offset=1, lengths=ln, min_length=17)
        adv, loss = ops.policy_backward(flat, gr, img, txt, rew, ro["logp"], ro["idx"], H, W, TAU, w, scale=1.0 / B, lengths=ln,
                                        min_length=17)
        # (the trainable part of the bucket: the call never touches ffn_o behind it)
        return {"scores": scores, "idx": ro["idx"], "logp": ro["logp"], "adv": adv, "loss": loss, "grad": gr[:ops.trainable_numel(D)]}

    want = {}
    for s, v in sets.items():
        out = run(torch.tensor(v, dtype=torch.int32, device=DEV), _poisoned_ws(D, H, M), torch.zeros_like(flat))
        torch.cuda.synchronize()
        want[s] = {k_: t.clone() for k_, t in out.items()}
    S = torch.cuda.Stream()                              # warm-up on the capture stream, as tests/test_gpu_contract.py does
    S.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(S):
        run(lens, ws, grad)
    torch.cuda.current_stream().wait_stream(S)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        out = run(lens, ws, grad)
    for s in (1, 2, 0):
        for t in [ws] + list(out.values()):
            K.poison_tensor(t)
        lens.copy_(torch.tensor(sets[s], dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        K.assert_same(out, want[s], f"replay with lengths {sets[s]}")
    del graph
