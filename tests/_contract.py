"""The table of cases of tests/test_gpu_contract.py and what goes with it: inputs by seed, static buffers, safe poison, the eager
default-stream twin and each case's independent reference.

A case is a closure over pre-built static buffers that returns a dict of named output tensors.  `Inst` owns one set of buffers:
  bufs     the LIVE inputs (and the state a call updates in place: flat, m, v, an accumulating gradient bucket, the residual a GEMM
           overwrites).  `load(seed)` copies the real values in on the current stream - that copy is part of the ordered work;
  scratch  workspaces and caller-supplied output buffers.
`poison()` fills all of them with wrong data that cannot fault: NaN for floating point, and for everything a kernel uses as an
address, an index or pixel data the case's OWN inputs of another seed (valid by construction: ascending index lists, in-range
frame indices, bytes).  The oob word gets 7.  Nothing a test does here can make a kernel read or write out of bounds.

Everything that would synchronise (host -> device uploads of index tensors and tap tables, workspace sizing, first-use allocations)
happens in `build`, never in `run`."""
import numpy as np
import torch

import _bf16_mixed as BM
import _clip_stages as cs
from oracle import tspo_oracle as O
from tspo_amd import ops, preprocess as P, synth

DEV = "cuda"
NAN = float("nan")
POISON_SEED = 99


def gen_(seed):
    return torch.Generator(device=DEV).manual_seed(7919 * (seed + 1))


def randn(shape, g, std=1.0):
    return torch.randn(*shape, generator=g, device=DEV) * std


def rand(shape, g):
    return torch.rand(*shape, generator=g, device=DEV)


def randu8(shape, g):
    return torch.randint(0, 256, shape, generator=g, device=DEV, dtype=torch.uint8)


def gumbel_noise(shape, g):
    u = rand(shape, g).clamp(1e-6, 1 - 1e-6)
    return -torch.log(-torch.log(u))


class Case:
    def __init__(self, name, gen, build, check):
        self.name, self.gen, self.build, self.check = name, gen, build, check
        self._real = {}

    def real(self, seed):
        """The real inputs of a seed, on the device, built once and never written."""
        if seed not in self._real:
            self._real[seed] = {k: v.contiguous() for k, v in self.gen(seed).items()}
            torch.cuda.synchronize()
        return self._real[seed]


def poison_tensor(t, src=None):
    if t.is_floating_point():
        t.fill_(NAN)
    elif src is not None:
        t.copy_(src)
    elif t.dtype == torch.uint8:
        t.fill_(0xFF)          # a workspace seen as bytes: 0xFFFF / 0xFFFFFFFF are NaN as bf16 / fp32
    else:
        t.zero_()              # an index OUTPUT: zeros are in range


class Inst:
    """One set of static buffers of a case and the closure over them."""

    def __init__(self, case):
        self.case = case
        r0 = case.real(0)
        self.bufs = {k: torch.empty_like(v) for k, v in r0.items()}
        self._poison_src = {k: v for k, v in case.real(POISON_SEED).items() if not v.is_floating_point()}
        for k, b in self.bufs.items():
            b.copy_(r0[k])
        built = case.build(self.bufs)
        self.run, self.scratch = built[0], built[1]
        self.reset = built[2] if len(built) > 2 else (lambda: None)
        torch.cuda.synchronize()

    def load(self, seed):
        r = self.case.real(seed)
        for k, b in self.bufs.items():
            b.copy_(r[k])

    def poison(self):
        for k, b in self.bufs.items():
            poison_tensor(b, self._poison_src.get(k))
        for s in self.scratch:
            poison_tensor(s)
        self.reset()


def bits_equal(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        if not bits_equal(got[k], want[k]):
            g, w = got[k].double().flatten(), want[k].double().flatten()
            bad = ~((g == w) | (g.isnan() & w.isnan()))
            d = (g - w)[bad]
            raise AssertionError(f"{what}: output {k!r} differs from the eager default-stream twin in {int(bad.sum())} of {g.numel()} "
                                 f"elements ({int(g.isnan().sum())} NaN); first at {bad.nonzero()[:4].flatten().tolist()}: got "
                                 f"{g[bad][:4].tolist()} want {w[bad][:4].tolist()}, max |difference| {d.abs().max().item():.3e}")


_EAGER_INST, _EAGER = {}, {}


def eager(case, seed, fresh=False):
    """The case run eagerly on the default stream with the inputs of `seed`: computed once, cloned, shared.  fresh=True runs it
    again (for a reference that reads what the run left in a workspace)."""
    key = (case.name, seed)
    if fresh or key not in _EAGER:
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        if case.name not in _EAGER_INST:
            _EAGER_INST[case.name] = Inst(case)
        inst = _EAGER_INST[case.name]
        inst.poison()
        inst.load(seed)
        out = inst.run()
        torch.cuda.synchronize()
        _EAGER[key] = {k: v.clone() for k, v in out.items()}
    return _EAGER[key]


# ----------------------------------------------------------------------------------------------------------------- references
def _np(t):
    return t.detach().cpu().numpy()


def check_logp(got, ref):
    """tests/test_gpu_ops.py:_check_logp (exact in the normal range; only 'very negative' where the probability is a denormal)."""
    normal = ref > -87.0
    np.testing.assert_allclose(got[normal], ref[normal], rtol=1e-5, atol=2e-5)
    assert np.all(got[~normal] < -86.0)


def state_from_flat(flat, D):
    f = flat.detach().cpu()
    return {n: f[off:off + int(np.prod(shape))].view(*shape).clone() for n, (off, shape) in ops.flat_offsets(D).items()
            if not n.startswith("__")}


def bucket(grad, D):
    g = grad.detach().cpu()
    offs = ops.flat_offsets(D)
    return {n: g[offs[n][0]:offs[n][0] + int(np.prod(offs[n][1]))].numpy() for n in BM.TRAINED}


def oracle_selector(flat, img, txt, clip, ds, H, w, tau):
    """oracle.selector_forward per video + autograd of sum(scores * ds): (scores [B,T], h [B,T,D], {name: gradient})."""
    D = img.shape[-1]
    st = state_from_flat(flat, D)
    ps = {n: v.clone().requires_grad_(n in BM.TRAINED) for n, v in st.items()}
    img, txt, clip, ds = img.cpu(), txt.cpu(), clip.cpu(), ds.cpu()
    ss, hs, total = [], [], 0.0
    for b in range(img.shape[0]):
        s, h = O.selector_forward(ps, img[b], txt[b], clip[b], w, tau, H)
        total = total + (s * ds[b]).sum()
        ss.append(s.detach())
        hs.append(h[0].detach())
    total.backward()
    return torch.stack(ss), torch.stack(hs), {n: ps[n].grad.numpy().flatten() for n in BM.TRAINED}


def check_grads_vs_oracle(got, ref):
    """tests/test_gpu_ops.py:test_selector_fwd_bwd_vs_oracle_autograd: rtol 5e-4, atol 5e-5 of the tensor's maximum; the key bias
    gradient (mathematically zero) within 1e-4 of the query bias gradient's maximum."""
    qb = np.abs(ref["temporal.Self_q.bias"]).max()
    for pn in BM.TRAINED:
        if pn == "temporal.Self_k.bias":
            assert np.abs(got[pn]).max() <= 1e-4 * max(qb, 1e-12), pn
        else:
            np.testing.assert_allclose(got[pn], ref[pn], rtol=5e-4, atol=5e-5 * max(np.abs(ref[pn]).max(), 1e-12), err_msg=pn)


# --------------------------------------------------------------------------------------------------------------------- samplers
def _sampler_case(fn, B, T, k):
    def gen(seed):
        s = randn((B, T), gen_(seed))
        s[:, ::7] = torch.round(s[:, ::7] * 10) / 10          # plenty of exact ties
        return {"scores": s}

    def build(b):
        return (lambda: {"idx": getattr(ops, fn)(b["scores"], k)}), []

    def check(r, o):
        for i in range(B):                                    # integer outputs: exact (test_topk_ties_and_batch)
            assert o["idx"][i].cpu().tolist() == getattr(O, fn)(r["scores"][i].cpu(), k).tolist(), (fn, i)
    return Case(f"{fn}-B{B}-T{T}-k{k}", gen, build, check)


def _gumbel_case(tag, B, G, T, k, injected, ppo=0):
    seed_, off_ = 11, 3

    def gen(seed):
        g = gen_(seed)
        d = {"logits": randn((B, T), g, 3.0)}
        if injected:
            d["noise"] = gumbel_noise((B, G, T), g)
        return d

    def build(b):
        if injected:
            return (lambda: {k_: v for k_, v in ops.gumbel_topk(b["logits"], k, G, noise=b["noise"], want_probs=True).items()
                             if v is not None}), []
        return (lambda: {k_: v for k_, v in ops.gumbel_topk(b["logits"], k, G, seed=seed_, offset=off_, want_noise=True,
                                                           prompts_per_offset=ppo).items() if v is not None}), []

    def check(r, o):
        logits = r["logits"].cpu()
        if injected:      # test_gumbel_topk_long_rows_beyond_lds / test_gumbel_topk_injected_noise
            noise = r["noise"].cpu()
        else:             # test_gumbel_topk_philox_and_batch: same Philox bits, libm-level log differences
            noise = o["noise"].cpu()
            if ppo:       # prompt b draws what prompt b % p of a call with offset + b / p would (include/tspo_hip.h)
                ref = np.concatenate([O.gumbel_noise_philox(ppo, G, T, seed_, off_ + j) for j in range(B // ppo)], 0)
            else:
                ref = O.gumbel_noise_philox(B, G, T, seed_, off_)
            np.testing.assert_allclose(noise.numpy(), ref, rtol=2e-5, atol=2e-5)
        for b in range(B):
            for g in range(G):
                idx, probs, lp = O.gumbel_topk(logits[b], noise[b, g], k)
                assert o["idx"][b, g].cpu().tolist() == idx.tolist(), (b, g)
                if injected:
                    np.testing.assert_allclose(_np(o["probs"][b, g]), probs.numpy(), rtol=0, atol=2e-6)
            check_logp(_np(o["logp"][b]), lp.numpy())
    return Case(f"gumbel_topk-{tag}", gen, build, check)


def _policy_ops_case(fn):
    B, G, T, k, scale = 3, 8, 700, 16, 0.25

    def gen(seed):
        g = gen_(seed)
        ro = ops.gumbel_topk(randn((B, T), g), k, G, seed=5 + seed)     # set-up: ascending index lists and a normalised logp
        return {"rewards": rand((B, G), g), "logp": ro["logp"], "idx": ro["idx"], "adv": randn((B, G), g)}

    def build(b):
        if fn == "grpo_advantage":
            return (lambda: {"adv": ops.grpo_advantage(b["rewards"])}), []
        if fn == "pg_grad_logits":
            return (lambda: dict(zip(("dlogits", "loss"), ops.pg_grad_logits(b["logp"], b["idx"], b["adv"], scale=scale)))), []
        return (lambda: dict(zip(("adv", "dlogits", "loss"), ops.grpo_pg_grad(b["rewards"], b["logp"], b["idx"], scale=scale)))), []

    def check(r, o):      # tolerances of test_advantage_and_pg_grad
        adv = O.grpo_advantage(r["rewards"].cpu().flatten(), G).view(B, G)
        if "adv" in o:
            np.testing.assert_allclose(_np(o["adv"]), adv.numpy(), rtol=1e-5, atol=1e-6)
        if "dlogits" in o:
            a = r["adv"].cpu() if fn == "pg_grad_logits" else o["adv"].cpu()
            for b in range(B):      # softmax(logp) == exp(logp): the oracle's closed form takes logp as its logits
                l_ref, g_ref = O.pg_grad_logits(r["logp"][b].cpu(), r["idx"][b].cpu(), a[b])
                ref = scale * g_ref.numpy()
                np.testing.assert_allclose(_np(o["dlogits"][b]), ref, rtol=1e-4, atol=1e-6 * np.abs(ref).max())
                assert abs(o["loss"][b].item() - float(l_ref)) < 1e-5
    return Case(fn, gen, build, check)


# --------------------------------------------------------------------------------------------------------------------- selector
SEL_SHAPES = {"T96-D128": (2, 96, 128, 8, 2, 12), "T300-D768": (1, 300, 768, 8, 1, 12)}
SEL_TAU = 0.05


def _sel_gen(shape):
    B, T, D, H, M, w = shape

    def gen(seed):
        g = gen_(seed)
        tot = ops.flat_offsets(D)["__total__"][0]
        flat = randn((tot,), g, 0.5 / np.sqrt(D))
        return {"flat": flat, "img": randn((B, T, D), g), "txt": randn((B, M, D), g), "clip": randn((B, T), g, 0.1),
                "ds": randn((B, T), g, 0.01)}
    return gen


def _selector_case(sname, precision, backward=True, accumulate=False):
    shape = SEL_SHAPES[sname]
    B, T, D, H, M, w = shape
    n = ops.trainable_numel(D)
    base_gen = _sel_gen(shape)

    def gen(seed):
        d = base_gen(seed)
        if accumulate:
            d["grad"] = randn((d["flat"].numel(),), gen_(seed + 500), 0.01)
        return d

    def build(b):
        ws = ops.selector_workspace(B, T, D, H, M, w, DEV)
        fg = b["grad"] if accumulate else torch.zeros_like(b["flat"])

        def run():
            s, h, _ = ops.selector_forward(b["flat"], b["img"], b["txt"], b["clip"], H, w, SEL_TAU, want_attn=True, ws=ws,
                                           precision=precision)
            out = {"scores": s, "attn": h}
            if backward:
                ops.selector_backward(b["flat"], fg, b["img"], b["txt"], b["ds"], H, w, SEL_TAU, ws, precision=precision,
                                      accumulate=accumulate)
                out["grad"] = fg[:n]
            return out
        return run, [ws] + ([] if accumulate else [fg])

    name = f"selector-{sname}-{precision}" + ("" if backward else "-fwd") + ("-accumulate" if accumulate else "")

    def check(r, o):
        if precision == "fp32":      # test_selector_fwd_bwd_vs_oracle_autograd
            s_ref, h_ref, g_ref = oracle_selector(r["flat"], r["img"], r["txt"], r["clip"], r["ds"], H, w, SEL_TAU)
            np.testing.assert_allclose(_np(o["scores"]), s_ref.numpy(), rtol=5e-5, atol=5e-5 / SEL_TAU)
            np.testing.assert_allclose(_np(o["attn"]), h_ref.numpy(), rtol=2e-4, atol=5e-5)
            if accumulate:
                # test_selector_small_micro_batch_forms_and_accumulate: what the bucket held + the gradient of the overwriting
                # call (the case selector-<shape>-fp32, itself held to the oracle), within 5e-6 of the maximum
                want = r["grad"][:n] + eager(CASES[f"selector-{sname}-fp32"], 0)["grad"]
                assert (o["grad"] - want).abs().max().item() <= 5e-6 * want.abs().max().item()
            else:
                check_grads_vs_oracle(bucket(o["grad"], D), g_ref)
            return
        e32 = eager(CASES[f"selector-{sname}-fp32"], 0)      # same inputs: the generator depends on the shape only
        if precision == "bf16x3":    # test_selector_bf16x3_split_precision_vs_exact: against the exact path (itself a case above)
            assert ((o["scores"] - e32["scores"]).abs().max() / e32["scores"].abs().max()).item() < 2e-4
            assert ((o["attn"] - e32["attn"]).abs().max() / e32["attn"].abs().max()).item() < 5e-5
            g0, g1 = bucket(e32["grad"], D), bucket(o["grad"], D)
            for pn in BM.TRAINED:
                if pn != "temporal.Self_k.bias":
                    assert np.abs(g0[pn] - g1[pn]).max() / np.abs(g0[pn]).max() < 2e-4, pn
            return
        # bf16 operands: the CPU emulation of the contract with the rounding on
        params = state_from_flat(r["flat"], D)
        s_em, g_em = BM.forward_backward(params, r["img"].cpu(), r["txt"].cpu(), r["clip"].cpu(), r["ds"].cpu(), H, w, SEL_TAU,
                                         rounding=True)
        # test_selector_bf16_operand_inference_precision (1): all but 1 % of the scores to fp32 summation order, none beyond 4e-4 / tau
        d = np.abs(_np(o["scores"]) - s_em.numpy())
        tight = 5e-5 * np.abs(s_em.numpy()) + 5e-5 / SEL_TAU
        assert (d > tight).mean() <= 0.01 and d.max() <= 4e-4 / SEL_TAU, ((d > tight).sum(), d.max())
        if precision == "bf16_mixed":   # test_bf16_mixed_exact_arithmetic
            assert bits_equal(o["scores"], eager(CASES[f"selector-{sname}-bf16-fwd"], 0)["scores"])
            got, ref32 = bucket(o["grad"], D), bucket(e32["grad"], D)
            qb = np.abs(g_em["temporal.Self_q.bias"].numpy()).max()
            for pn in BM.TRAINED:
                em = g_em[pn].numpy().flatten()
                if pn == "temporal.Self_k.bias":
                    assert np.abs(got[pn]).max() <= 1e-3 * qb, pn
                    continue
                rf, rf32 = BM.rel_fro(got[pn], em), BM.rel_fro(ref32[pn], em)
                assert rf <= 6e-3 and rf * 10 < rf32, (pn, rf, rf32)
                assert np.abs(got[pn] - em).max() / np.abs(em).max() <= 3e-2, pn
    return Case(name, gen, build, check)


PB_SHAPE = (2, 300, 128, 8, 1, 12)


def _policy_backward_case(G, k, with_adamw=False):
    B, T, D, H, M, w = PB_SHAPE
    n = ops.trainable_numel(D)
    scale, lr = 0.5, 5e-4
    base_gen = _sel_gen(PB_SHAPE)

    def gen(seed):
        d = base_gen(seed)
        del d["ds"]
        g = gen_(seed + 300)
        d["rewards"] = rand((B, G), g)
        if with_adamw:
            d["m"] = randn((d["flat"].numel(),), g, 1e-3)
            d["v"] = rand((d["flat"].numel(),), g) * 1e-6
        return d

    def build(b):
        ws = ops.selector_workspace(B, T, D, H, M, w, DEV)
        fg = torch.zeros_like(b["flat"])
        part = torch.zeros(2048, dtype=torch.float32, device=DEV)
        out2, nws = torch.zeros(2, device=DEV), torch.zeros(2048, dtype=torch.uint8, device=DEV)

        def run():
            s, _, _ = ops.selector_forward(b["flat"], b["img"], b["txt"], b["clip"], H, w, SEL_TAU, want_attn=False, ws=ws)
            ro = ops.gumbel_topk(s, k, G, seed=7, offset=1)
            out = {"scores": s, "idx": ro["idx"], "logp": ro["logp"]}
            if with_adamw:
                adv, loss, npart = ops.policy_backward(b["flat"], fg, b["img"], b["txt"], b["rewards"], ro["logp"], ro["idx"], H, w,
                                                       SEL_TAU, ws, scale=scale, norm_partials=part)
                out["grad"] = fg[:n].clone()
                ops.adamw_clip_step(b["flat"], fg, b["m"], b["v"], n, lr, 3, weight_decay=0.01, out=out2, ws=nws,
                                    norm_partials=part, n_partials=npart)
                out.update(flat=b["flat"][:n], m=b["m"][:n], v=b["v"][:n], norm=out2)
            else:
                adv, loss = ops.policy_backward(b["flat"], fg, b["img"], b["txt"], b["rewards"], ro["logp"], ro["idx"], H, w,
                                                SEL_TAU, ws, scale=scale)
                out["grad"] = fg[:n]
            out.update(adv=adv, loss=loss)
            return out
        return run, [ws, fg, part, out2, nws]

    def check(r, o):
        # the rollouts are a sampler's (its own cases); the policy gradient from the oracle's closed form through the oracle's
        # autograd, at the tolerance of test_stress_config_T4096_G16 (the same chain) = test_selector_fwd_bwd_vs_oracle_autograd
        adv = O.grpo_advantage(r["rewards"].cpu().flatten(), G).view(B, G)
        np.testing.assert_allclose(_np(o["adv"]), adv.numpy(), rtol=1e-5, atol=1e-6)
        ds = []
        for b in range(B):
            l_ref, g_ref = O.pg_grad_logits(o["logp"][b].cpu(), o["idx"][b].cpu(), o["adv"][b].cpu())
            assert abs(o["loss"][b].item() - float(l_ref)) < 1e-5
            ds.append(scale * g_ref)
        # (d-scores are formed from the logp / idx / adv the code under test returned: the rollouts and the advantage have their
        # own cases above, and the forward's scores are held to the oracle here as in the selector cases)
        s_ref, _, g_ref = oracle_selector(r["flat"], r["img"], r["txt"], r["clip"], torch.stack(ds), H, w, SEL_TAU)
        np.testing.assert_allclose(_np(o["scores"]), s_ref.numpy(), rtol=5e-5, atol=5e-5 / SEL_TAU)
        check_grads_vs_oracle(bucket(o["grad"], D), g_ref)
        if with_adamw:            # test_adamw_matches_oracle_on_identical_inputs
            g = o["grad"].cpu()
            tn = float(np.linalg.norm(g.numpy().astype(np.float64)))
            assert abs(o["norm"][0].item() - tn) < 1e-5 * tn
            assert abs(o["norm"][1].item() - O.clip_grad_scale(tn, 1.0)) < 1e-6
            po, mo, vo = O.adamw_step(r["flat"][:n].cpu().clone(), g, r["m"][:n].cpu().clone(), r["v"][:n].cpu().clone(), 3, lr,
                                      wd=0.01, grad_scale=o["norm"][1].item())
            np.testing.assert_allclose(_np(o["flat"]), po.numpy(), rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(_np(o["m"]), mo.numpy(), rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(_np(o["v"]), vo.numpy(), rtol=1e-5, atol=1e-12)
    return Case(f"policy_backward-G{G}-k{k}" + ("-norm_partials-adamw_clip_step" if with_adamw else ""), gen, build, check)


def _adamw_case(n, fused):
    lr, step = 5e-4, 2

    def gen(seed):
        g = gen_(seed)
        return {"p": randn((n,), g, 0.05), "g": randn((n,), g, 3e-3), "m": randn((n,), g, 1e-3), "v": rand((n,), g) * 1e-6}

    def build(b):
        out2, ws = torch.zeros(2, device=DEV), torch.zeros(2048, dtype=torch.uint8, device=DEV)

        def run():
            if fused:
                ops.adamw_clip_step(b["p"], b["g"], b["m"], b["v"], n, lr, step, weight_decay=0.01, pre_scale=0.5, max_norm=1.0,
                                    out=out2, ws=ws)
            else:
                ops.grad_norm_scale(b["g"], n, 0.5, 1.0, out=out2, ws=ws)
                ops.adamw_step(b["p"], b["g"], b["m"], b["v"], n, lr, step, weight_decay=0.01, d_grad_scale=out2)
            return {"p": b["p"], "m": b["m"], "v": b["v"], "norm": out2}
        return run, [out2, ws]

    def check(r, o):              # test_adamw_matches_oracle_on_identical_inputs
        tn = float(np.linalg.norm(_np(r["g"]).astype(np.float64)))
        assert abs(o["norm"][0].item() - tn) < 1e-5 * tn
        assert abs(o["norm"][1].item() - O.clip_grad_scale(tn, 1.0) * 0.5) < 1e-6
        po, mo, vo = O.adamw_step(r["p"].cpu().clone(), r["g"].cpu(), r["m"].cpu().clone(), r["v"].cpu().clone(), step, lr, wd=0.01,
                                  grad_scale=o["norm"][1].item())
        np.testing.assert_allclose(_np(o["p"]), po.numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(_np(o["m"]), mo.numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(_np(o["v"]), vo.numpy(), rtol=1e-5, atol=1e-12)
    return Case(("adamw_clip_step" if fused else "grad_norm_scale+adamw_step") + f"-n{n}", gen, build, check)


def _clip_scores_case():
    B, T, D = 2, 300, 768

    def gen(seed):
        g = gen_(seed)
        return {"txt": randn((B, 1, D), g), "feat": randn((B, T, D), g)}

    def check(r, o):              # test_clip_scores
        for b in range(B):
            np.testing.assert_allclose(_np(o["clip"][b]), O.clip_cosine_scores(r["txt"][b].cpu(), r["feat"][b].cpu()).numpy(),
                                       rtol=1e-5, atol=1e-6)
    return Case("clip_scores", gen, lambda b: ((lambda: {"clip": ops.clip_scores(b["txt"], b["feat"])}), []), check)


# ---------------------------------------------------------------------------------------------------------------------- encoder
L14 = dict(synth.CLIP_L14, layers=1)          # the configuration of tests/test_gpu_encoder_stages.py
_CLIP = {}


def clip_state():
    if "state" not in _CLIP:
        _CLIP["state"] = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.clip_vision_state(**L14).items()}
    return _CLIP["state"]


def new_clip_weights(max_frames=128):
    W = ops.ClipVitWeights(clip_state(), L14, DEV)
    W._workspace(max_frames)                   # sized once, at set-up: no call under test allocates or moves it
    return W


def shared_clip_weights():
    """One weights object (and workspace) for the encoder cases of Parts A and B: they run one after the other."""
    if "W" not in _CLIP:
        _CLIP["W"] = new_clip_weights()
    return _CLIP["W"]


def _encoder_case(tag, n, twice=False, chunk=None, **kw):
    def gen(seed):
        return {"pixels": randu8((n, 3, 224, 224), gen_(seed))}

    def build(b):
        W = shared_clip_weights()

        def run():
            if chunk:
                return {"feat": ops.clip_vit_forward_chunked(W, b["pixels"], chunk, **kw)}
            out = {"feat": ops.clip_vit_forward(W, b["pixels"], **kw)}
            if twice:                          # the fold of the first call is still in the workspace: TSPO_CLIP_FOLD_CACHED
                out["feat_cached"] = ops.clip_vit_forward(W, b["pixels"], **kw)
            return out
        # poisoning the workspace destroys the folded weights at its front, so the next call must fold again
        return run, [W._ws], W.invalidate_fold_cache

    def check(r, o):
        # "features (GE_F32)" of tests/test_gpu_encoder_stages.py:_stages: the features against float64 of the pooled rows the
        # call left in the workspace times the projection, within (C + 1) u sum |pooled . proj| - every element.  This holds the
        # twin to a reference from pooling on ONLY: nothing upstream of the pooled rows is compared here, for any of the encoder
        # cases.  That the stages before it are right rests entirely on tests/test_gpu_encoder_stages.py (every stage against
        # float64 from its stored input, at these configurations).
        # Needs the workspace as THIS eager run left it (chunked: as its last chunk left it).
        W = shared_clip_weights()
        last = ops.clip_chunk_plan(W, n, chunk)[-1] if chunk else n
        pooled = cs.views(W, last)["pooled"]
        proj = clip_state()["visual_projection.weight"].float().to(torch.bfloat16).to(DEV)
        feat = o["feat_cached"] if twice else o["feat"][n - last:]
        cs.check(f"{tag} features", feat, cs.d64(pooled) @ cs.d64(proj).t(), (L14["hidden"] + 1) * cs.U * cs.gemm_abs64(pooled, proj),
                 rounded=False)
        assert torch.isfinite(o["feat"]).all()
        if twice:
            assert bits_equal(o["feat"], o["feat_cached"])
    return Case(f"clip_vit_forward-{tag}", gen, build, check)


# ---------------------------------------------------------------------------------------------------------------- preprocessing
def pil_u8(frame_hwc, spec):
    """tests/test_gpu_select_frames.py:pil_u8 - one frame through Pillow the way the processors do it."""
    from PIL import Image
    H, W = frame_hwc.shape[:2]
    new_h, new_w, top, left, oh, ow = P.spec_resize_geometry(H, W, spec)
    img = np.array(Image.fromarray(frame_hwc).resize((new_w, new_h), resample=Image.BICUBIC))
    return np.ascontiguousarray(img[top:top + oh, left:left + ow].transpose(2, 0, 1))


SPEC_BYTES = dict(size=(98, 222), mean=(0.5, 0.4, 0.3), std=(0.5, 0.25, 0.2))     # test_select_plain_scalar_form_and_rectangular_output


def _matrix_pass(flag, fn):
    """USE_MATRIX_PASS switched around one call, as tests/test_preprocess.py does with monkeypatch."""
    def run():
        old = P.USE_MATRIX_PASS
        P.USE_MATRIX_PASS = flag
        try:
            return fn()
        finally:
            P.USE_MATRIX_PASS = old
    return run


def _preprocess_case(tag, hw, spec, matrix=True):
    def gen(seed):
        return {"frames": randu8((3, hw[0], hw[1], 3), gen_(seed))}

    def build(b):
        run = _matrix_pass(matrix, lambda: {"out": P.select_frames(b["frames"], None, spec, what="preprocess_frames")})
        run()                                  # the throw-away call that uploads the tap tables of this geometry
        return run, []

    def check(r, o):                           # Pillow, bit for bit (test_gpu_preprocess_bit_exact / ..._plain_scalar_fallback)
        fr = _np(r["frames"])
        np.testing.assert_array_equal(_np(o["out"]), np.stack([pil_u8(f, spec) for f in fr]))
    return Case(f"preprocess_frames-{tag}", gen, build, check)


def _select_case(tag, dtype, oob=False):
    Pn, hw = 4, (240, 320)
    spec = P.PreprocessSpec.clip_default(out_dtype=dtype)

    def gen(seed):
        g = gen_(seed)
        ix = torch.randint(0, Pn, (6,), generator=g, device=DEV).sort(descending=True).values     # repeats, descending
        ix[1] = ix[0]
        d = {"pool": randu8((Pn, hw[0], hw[1], 3), g), "index": ix}
        if oob:
            d["index"][2] = Pn + 5
            d["flag"] = torch.full((1,), 7 if seed == POISON_SEED else 0, dtype=torch.int32, device=DEV)
        return d

    def build(b):
        def run():
            out = {"out": P.select_frames(b["pool"], b["index"], spec, oob_flag=b.get("flag"))}
            if oob:
                out["flag"] = b["flag"]
            return out
        run()
        return run, []

    def check(r, o):
        from test_gpu_select_frames import _assert_float_bound
        ix = _np(r["index"]).clip(0, Pn - 1)           # documented: clamped to the nearest valid frame
        u8 = np.stack([pil_u8(f, spec) for f in _np(r["pool"])])[ix]
        if oob:                                        # test_select_out_of_range_index_is_clamped_and_flagged
            assert int(o["flag"].item()) == 1
        if dtype == torch.uint8:
            np.testing.assert_array_equal(_np(o["out"]), u8)
        elif dtype == torch.float32:                   # test_select_float_outputs_within_derived_bound
            _assert_float_bound(o["out"], torch.from_numpy(u8), spec)
        else:                                          # one further rounding to nearest even: bitwise
            assert torch.equal(o["out"], eager(CASES["select_frames-float32"], 0)["out"].to(dtype))
    return Case(f"select_frames-{tag}", gen, build, check)


# ------------------------------------------------------------------------------------------------------------------------- GEMM
GEMM_SHAPE = (70001, 264, 128)    # the smallest of EDGE (tests/test_gpu_encoder_stages.py); kernels 1, 77 and 83 all accept it


def _gemm_case(kernel, in_place):
    M, N, K = GEMM_SHAPE

    def gen(seed):
        g = gen_(seed)
        d = {"A": randn((M, K), g).to(torch.bfloat16), "W": randn((N, K), g, 0.05).to(torch.bfloat16), "bias": randn((N,), g, 0.1)}
        if in_place:
            d["R"] = randn((M, N), g).to(torch.bfloat16)
        return d

    def build(b):
        if in_place:
            return (lambda: {"C": ops.gemm_bf16(b["A"], b["W"], bias=b["bias"], residual=b["R"], act=kernel << 8, out=b["R"])}), []
        c = torch.zeros((M, N), dtype=torch.bfloat16, device=DEV)
        return (lambda: {"C": ops.gemm_bf16(b["A"], b["W"], bias=b["bias"], act=kernel << 8, out=c)}), [c]

    def check(r, o):              # test_gemm_small_kernel_forced: float64 of the same operands, 1/2 ulp_bf16 + (K + 3) u sum |.|
        from test_gpu_encoder_stages import _plain_gemm
        ref, E = _plain_gemm(r["A"], r["W"], r["bias"], r["R"] if in_place else None)
        cs.check(f"gemm kernel {kernel}" + (" in place" if in_place else ""), o["C"], ref, cs.bound_bf16(ref, E))
    return Case(f"gemm_bf16-k{kernel}" + ("-residual-in-place" if in_place else ""), gen, build, check)


def _all_cases():
    c = [_sampler_case("topk_sorted", 3, 777, 33), _sampler_case("topk_sorted", 2, 16385, 64),
         _sampler_case("binmax", 3, 777, 33), _sampler_case("binmax", 2, 16385, 64),
         _gumbel_case("injected-T777-k33", 2, 3, 777, 33, True), _gumbel_case("philox-T777-k33", 2, 3, 777, 33, False),
         _gumbel_case("long-T16385-k48", 2, 3, 16385, 48, True), _gumbel_case("prompts_per_offset1", 2, 3, 777, 33, False, ppo=1),
         _policy_ops_case("grpo_advantage"), _policy_ops_case("pg_grad_logits"), _policy_ops_case("grpo_pg_grad")]
    for s in SEL_SHAPES:
        c += [_selector_case(s, "fp32"), _selector_case(s, "bf16x3"), _selector_case(s, "bf16", backward=False),
              _selector_case(s, "bf16_mixed")]
    c += [_selector_case("T96-D128", "fp32", accumulate=True),
          _policy_backward_case(8, 16), _policy_backward_case(3, 100), _policy_backward_case(8, 16, with_adamw=True)]
    for n in (100003, 1003):
        c += [_adamw_case(n, False), _adamw_case(n, True)]
    c += [_clip_scores_case(),
          _encoder_case("n3", 3), _encoder_case("n70-fold-twice", 70, twice=True),
          _encoder_case("n70-nofold", 70, fold_layernorm=False), _encoder_case("n70-prune_last", 70, prune_last_layer=True),
          _encoder_case("chunked-n192-c128", 192, chunk=128),
          _preprocess_case("240x320-matrix", (240, 320), P.PreprocessSpec.clip_default(224, torch.uint8), True),
          _preprocess_case("240x320-lds", (240, 320), P.PreprocessSpec.clip_default(224, torch.uint8), False),
          _preprocess_case("97x131-bytes", (97, 131), P.PreprocessSpec(out_dtype=torch.uint8, **SPEC_BYTES)),
          _select_case("uint8", torch.uint8), _select_case("float32", torch.float32), _select_case("bfloat16", torch.bfloat16),
          _select_case("float16", torch.float16), _select_case("oob_flag", torch.uint8, oob=True)]
    for kernel in (1, 77, 83):
        c += [_gemm_case(kernel, False), _gemm_case(kernel, True)]
    return {x.name: x for x in c}


CASES = _all_cases()
