"""TSPO_SEL_BF16_MIXED on the GPU: the reference's bf16 training precision (`--bf16 --torch_dtype bfloat16`, train_deepspeed.sh:33-34)
as a forward + backward mode of the scoring head - bf16 GEMM operands (rounded in registers), fp32 accumulation, fp32 everywhere
else (include/tspo_hip.h).

1. Exact arithmetic: the kernels compute the contract (tests/_bf16_mixed.py with the rounding on) in every tile form the exact path
   selects - D = 64 (unfused fallback), BT = 300 / 512 (64x64 whole-contraction tiles), 1024 (split 3), 2048 (split 7), 4096.
2. Bounded by the reference's own bf16 noise (tests/golden/bf16_train_noise.json) at the sizes bench.py times.
3. The DP path (coalesced 1 x 2 window and two sequential micro-steps with TSPO_SEL_ACCUMULATE).
4. Race screen; 5. the autograd bridge; 6. the training driver with checkpoint / resume."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bf16_mixed as BM
import _policy_full as P
from inputs import SELECTOR_CASES, selector_inputs
from oracle import tspo_oracle as O
from tspo_amd import ops, synth
from tspo_amd.pipeline import PolicyTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def G_(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _flat(state, D):
    offs = ops.flat_offsets(D)
    flat = torch.zeros(offs["__total__"][0], dtype=torch.float32)
    for name, (off, shape) in offs.items():
        if not name.startswith("__"):
            flat[off:off + int(np.prod(shape))] = torch.from_numpy(np.asarray(state[name])).flatten()
    return flat.to(DEV)


def _bucket(grad, D):
    offs = ops.flat_offsets(D)
    g = grad.detach().cpu().numpy()
    return {pn: g[offs[pn][0]:offs[pn][0] + int(np.prod(offs[pn][1]))].reshape(offs[pn][1]).copy() for pn in O.SELECTOR_KEYS}


def _noise_fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bf16_train_noise.json")))["cases"]


def _synth_case(B, T, D=768, seed=0):
    M = 1
    img = synth.normal((B, T, D), 5100 + seed)
    txt = synth.normal((B, M, D), 5101 + seed)
    clip = synth.normal((B, T), 5102 + seed, 0.1)
    ds = synth.normal((B, T), 5103 + seed, 0.01)
    state = synth.selector_state(D, seed=23 + seed, std=0.5 / np.sqrt(D), bias_std=0.05)
    return img, txt, clip, ds, state


def _selector_cases():
    out = []
    for c in SELECTOR_CASES:
        if c[0] in ("s32", "s300", "s1024"):
            name, T, D, H, w, tau, M, ks = c
            out.append((name, 1, T, D, H, w, tau))
    for B, T in ((1, 512), (2, 512), (4, 512), (1, 4096)):
        out.append((f"bt{B * T}", B, T, 768, 8, 12, 0.025))
    return out


@pytest.mark.parametrize("case", _selector_cases(), ids=lambda c: c[0])
def test_bf16_mixed_exact_arithmetic(case):
    """The kernels' gradients equal the CPU emulation of the contract with the rounding ON, to fp32 summation order plus rounding-boundary
    flips.  (An operand that differs by one fp32 ulp between the GPU and the CPU - dh1, dqkv, a ReLU output - can fall on the other
    side of a bf16 rounding boundary and move ONE term of a later sum by 2^-9 relative; the rule and wording of
    test_selector_bf16_operand_inference_precision.  At D = 768 the attention backward's dS = p (dp - dot) amplifies such
    differences (measured: dh2 agrees to ~1e-6, dh1 / dctx / dqkv to 2e-4 ... 4e-3 depending on the inputs) - the exact path's own
    parity with the oracle needs rtol 5e-4 there - so the criterion is relative: every gradient tensor of the kernel must sit at
    least 10x closer to the bf16 contract than the exact fp32 path does (measured 14x ... 100x), within 6e-3 of it in Frobenius norm
    and 3e-2 of its maximum element-wise.)  Forward scores are bitwise those of precision="bf16", and the gradients really differ from the exact path's."""
    name, B, T, D, H, w, tau = case
    if name.startswith("s"):
        img, txt, clip, state = selector_inputs(name, T, D, 1)
        img, txt, clip = img[None], txt[None], clip[None]
        ds = synth.normal((1, T), 991, 0.05)
    else:
        img, txt, clip, ds, state = _synth_case(B, T, D)
    flat = _flat(state, D)
    s_mix, _, ws = ops.selector_forward(flat, G_(img), G_(txt), G_(clip), H, w, tau, want_attn=False, precision="bf16_mixed")
    s_b16, _, _ = ops.selector_forward(flat, G_(img), G_(txt), G_(clip), H, w, tau, want_attn=False, precision="bf16")
    assert torch.equal(s_mix, s_b16), "bf16_mixed forward must be the bf16 forward, bit for bit"
    g = torch.zeros_like(flat)
    ops.selector_backward(flat, g, G_(img), G_(txt), G_(ds), H, w, tau, ws, precision="bf16_mixed")
    s32, _, ws32 = ops.selector_forward(flat, G_(img), G_(txt), G_(clip), H, w, tau, want_attn=False)
    g32 = torch.zeros_like(flat)
    ops.selector_backward(flat, g32, G_(img), G_(txt), G_(ds), H, w, tau, ws32)
    torch.cuda.synchronize()
    assert not torch.equal(g, g32), "bf16_mixed must change the gradients"
    params = {n: torch.from_numpy(np.asarray(v)) for n, v in state.items()}
    s_em, g_em = BM.forward_backward(params, torch.from_numpy(img), torch.from_numpy(txt), torch.from_numpy(clip),
                                     torch.from_numpy(ds), H, w, tau, rounding=True)
    got, ref32 = _bucket(g, D), _bucket(g32, D)
    qb = np.abs(g_em["temporal.Self_q.bias"].numpy()).max()
    stats = []
    for pn in BM.TRAINED:
        em = g_em[pn].numpy()
        if pn == "temporal.Self_k.bias":    # mathematically zero: both sides hold rounding noise
            assert np.abs(got[pn]).max() <= 1e-3 * qb, pn
            continue
        d = np.abs(got[pn] - em)
        emax = np.abs(em).max()
        rf = BM.rel_fro(got[pn], em)
        rf32 = BM.rel_fro(ref32[pn], em)      # the exact path against the same emulation: how much the rounding itself moves
        stats.append((pn, rf, rf32, d.max() / emax, (d > 2e-3 * np.abs(em) + 2e-4 * emax).mean()))
    print(f"\n[bf16_mixed exact arithmetic {name}: B={B} T={T} D={D}] rel. Frobenius vs emulation (exact path), max err / max, "
          "fraction beyond 2e-3|g| + 2e-4 max: " +
          ", ".join(f"{pn.replace('temporal.', '')} {rf:.1e} ({rf32:.1e}) {mx:.1e} {fr:.3f}" for pn, rf, rf32, mx, fr in stats))
    for pn, rf, rf32, mx, fr in stats:
        assert rf <= 6e-3 and rf * 10 < rf32, (pn, rf, rf32)
        assert mx <= 3e-2, (pn, mx)


def _rollout_and_backward(tr, name, g, prompts, micro_steps=1):
    """rollout() under the fixture's noise, backward() with the fixture's fp32 indices (the reference's rollouts): -> changed sets."""
    _, B, T, D, H, w, tau, k, G = P.CASES[name]
    img, txt, clip, state, rew = P.train_full_inputs(name, B, T, D, G)
    sl = list(prompts)
    f, t, c = G_(img[sl]), G_(txt[sl]), G_(clip[sl])
    scores, idx, logp, ctx = tr.rollout(f, t, c, G, k, tau, noise=G_(g[f"{name}.noise"][sl]), micro_steps=micro_steps)
    ref_idx = g[f"{name}.idx"][sl]
    got = idx.cpu().numpy()
    changed = sum(set(got[i, j].tolist()) != set(ref_idx[i, j].tolist()) for i in range(len(sl)) for j in range(G))
    tr.backward(ctx, f, t, logp, G_(ref_idx.astype(np.int64)), G_(rew[sl]))
    return changed


def _bounded_by_reference_noise(name, bucket, mean, what):
    fx = _noise_fixture()[name]
    lines = []
    for pn in BM.TRAINED:
        if pn == "temporal.Self_k.bias":
            continue
        ref = mean[pn].numpy().reshape(bucket[pn].shape)
        rf, rm = BM.rel_fro(bucket[pn], ref), BM.rel_max(bucket[pn], ref)
        qf, qm = rf / fx["rel_fro"][pn], rm / fx["rel_max"][pn]
        lines.append(f"{pn.replace('temporal.', '')} fro x{qf:.2f} max x{qm:.2f}")
        assert qf <= 1.25 and qm <= 2.0, (what, pn, rf, fx["rel_fro"][pn], rm, fx["rel_max"][pn])
    print(f"\n[{what}] bf16_mixed error / the reference's own bf16 error: " + ", ".join(lines))


@pytest.mark.parametrize("name", ["c2", "c4"], ids=["configs2_B4_T512_G8_k16", "configs4_B1_T4096_G16_k16"])
def test_bf16_mixed_policy_step_within_reference_bf16_noise(golden, name):
    _, B, T, D, H, w, tau, k, G = P.CASES[name]
    g = golden["train_full"]
    img, txt, clip, state, rew = P.train_full_inputs(name, B, T, D, G)
    tr = PolicyTrainer(_flat(state, D), dim=D, heads=H, window_size=w, lr=5e-4, max_grad_norm=1.0, gemm_precision="bf16_mixed")
    changed = _rollout_and_backward(tr, name, g, range(B))
    fx = _noise_fixture()[name]
    print(f"\n[{name}] index sets changed by the bf16_mixed rollouts: {changed} of {B * G} (reference bf16: {fx['changed_index_sets']})")
    assert changed <= max(2 * fx["changed_index_sets"], 2)
    torch.cuda.synchronize()
    bucket = _bucket(tr.grad, D)
    mean, _ = P.oracle_mean_grads(name, g, range(B))
    _bounded_by_reference_noise(name, bucket, mean, f"{name} B={B} T={T}")
    # the clip norm from the backward's fused partials == a separate pass over the bucket
    assert tr._norm_np > 0, "single rank, whole window in one backward: the fused-norm path must be taken"
    sep = float(tr.grad[:tr.n_train].double().norm())
    ost = tr.optimizer_step()
    assert abs(float(ost["grad_norm_scale"][0]) - sep) <= 1e-4 * sep, (float(ost["grad_norm_scale"][0]), sep)


def test_bf16_mixed_dp_window_coalesced_and_sequential(golden):
    """The reference's 1 x 2 accumulation window as ONE coalesced micro_steps=2 step (BT = 1024 forms) and as two sequential steps
    (BT = 512 whole-contraction tiles, TSPO_SEL_ACCUMULATE on the second): the two agree to rounding, both bounded like test 2."""
    name = "c2"
    _, B, T, D, H, w, tau, k, G = P.CASES[name]
    g = golden["train_full"]
    img, txt, clip, state, rew = P.train_full_inputs(name, B, T, D, G)
    pair = (0, 1)
    coa = PolicyTrainer(_flat(state, D), dim=D, heads=H, window_size=w, lr=5e-4, grad_accum_steps=2, gemm_precision="bf16_mixed")
    _rollout_and_backward(coa, name, g, pair, micro_steps=2)
    seq = PolicyTrainer(_flat(state, D), dim=D, heads=H, window_size=w, lr=5e-4, grad_accum_steps=2, gemm_precision="bf16_mixed")
    for j in pair:
        _rollout_and_backward(seq, name, g, (j,))
    torch.cuda.synchronize()
    bc, bs = _bucket(coa.grad, D), _bucket(seq.grad, D)
    for pn in BM.TRAINED:
        if pn != "temporal.Self_k.bias":
            assert BM.rel_fro(bs[pn], bc[pn]) <= 5e-4, (pn, BM.rel_fro(bs[pn], bc[pn]))
    mean, _ = P.oracle_mean_grads(name, g, pair)
    _bounded_by_reference_noise(name, bc, mean, "1x2 window coalesced")
    _bounded_by_reference_noise(name, bs, mean, "1x2 window sequential")
    for trn in (coa, seq):
        ost = trn.optimizer_step()
        assert np.isfinite(float(ost["grad_norm_scale"][0]))


@pytest.mark.parametrize("B,T", [(4, 512), (1, 4096)])
def test_bf16_mixed_bitwise_repeatable(B, T):
    """Race screen: two identical bf16_mixed forward + backward calls give bit-identical scores and gradients."""
    D, H, w, tau = 768, 8, 12, 0.025
    img, txt, clip, ds, state = _synth_case(B, T, D, seed=7)
    flat = _flat(state, D)
    outs = []
    for _ in range(2):
        s, _, ws = ops.selector_forward(flat, G_(img), G_(txt), G_(clip), H, w, tau, want_attn=False, precision="bf16_mixed")
        gr = torch.zeros_like(flat)
        ops.selector_backward(flat, gr, G_(img), G_(txt), G_(ds), H, w, tau, ws, precision="bf16_mixed")
        outs.append((s.clone(), gr.clone()))
    assert torch.isfinite(outs[0][1]).all() and outs[0][1].abs().max() > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_bf16_mixed_autograd_bridge(golden):
    """MultiModal_Align.training_gemm_precision = "bf16_mixed": loss.backward() through the module (the reference's loss of
    tspo_trainer.py:594-607 on the scores) leaves the gradient ops.policy_backward(precision="bf16_mixed") computes."""
    from tspo_amd.temporal_agent import MultiModal_Align
    name = "c2"
    _, B, T, D, H, w, tau, k, G = P.CASES[name]
    g = golden["train_full"]
    img, txt, clip, state, rew = P.train_full_inputs(name, B, T, D, G)
    m = MultiModal_Align(dim=D, num_heads=H)
    m.load_state_dict({kk: torch.from_numpy(np.asarray(v)) for kk, v in state.items()})
    m.to(DEV)
    flat = m.flatten_parameters()
    m.training_gemm_precision = "bf16_mixed"
    b = 0
    idx = G_(np.sort(g[f"{name}.idx"][b], axis=-1).astype(np.int64))
    r = G_(rew[b])
    scores, _ = m.forward_batched(G_(img[b:b + 1]), G_(txt[b:b + 1]), G_(clip[b:b + 1]), w, tau)
    lp = torch.log_softmax(scores[0], dim=0)
    adv = (r - r.mean()) / (r.std() + 1e-4)
    loss = 0.0
    for j in range(G):
        sel = lp[idx[j]]
        loss = loss + (-(torch.exp(sel - sel.detach()).mean() * adv[j]))
    (loss / G).backward()
    offs = ops.flat_offsets(D)
    got = {pn: p.grad.detach().flatten().clone() for pn, p in m._trainable_named()}
    ws = ops.selector_workspace(1, T, D, H, 1, w, DEV)
    s2, _, ws = ops.selector_forward(flat.detach(), G_(img[b:b + 1]), G_(txt[b:b + 1]), G_(clip[b:b + 1]), H, w, tau, want_attn=False,
                                     ws=ws, precision="bf16_mixed")
    assert torch.equal(s2, scores.detach())
    ref = torch.zeros_like(flat)
    logp = torch.log_softmax(s2, dim=-1)
    ops.policy_backward(flat.detach(), ref, G_(img[b:b + 1]), G_(txt[b:b + 1]), r[None], logp, idx[None], H, w, tau, ws,
                        precision="bf16_mixed")
    # the same step in the exact mode: how far the precision itself moves the gradient
    s32, _, ws32 = ops.selector_forward(flat.detach(), G_(img[b:b + 1]), G_(txt[b:b + 1]), G_(clip[b:b + 1]), H, w, tau, want_attn=False)
    ref32 = torch.zeros_like(flat)
    ops.policy_backward(flat.detach(), ref32, G_(img[b:b + 1]), G_(txt[b:b + 1]), r[None], torch.log_softmax(s32, dim=-1), idx[None], H,
                        w, tau, ws32)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(BM.TRAINED)
    g_a = torch.cat([got[pn] for pn in BM.TRAINED])
    g_k = torch.cat([ref[offs[pn][0]:offs[pn][0] + got[pn].numel()] for pn in BM.TRAINED])
    g_32 = torch.cat([ref32[offs[pn][0]:offs[pn][0] + got[pn].numel()] for pn in BM.TRAINED])
    rel = float((g_a - g_k).norm() / g_k.norm())
    rel32 = float((g_a - g_32).norm() / g_32.norm())
    print(f"\n[autograd bridge, bf16_mixed] |autograd - policy_backward| / |policy_backward| = {rel:.2e} (vs the exact mode: {rel32:.2e})")
    # (dL/dscores formed by torch instead of inside the kernel differs by fp32 rounding; bf16 rounding-boundary flips carry that on)
    assert rel <= 1e-3 and rel * 10 < rel32, (rel, rel32)


def test_bf16_mixed_training_driver_with_resume(tmp_path):
    """`python -m tspo_amd.train --gemm-precision bf16_mixed` on synthetic features, as fresh child processes: finite losses, and a
    second run resumes from the checkpoint the first one left."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = str(tmp_path / "run")
    common = [sys.executable, "-m", "tspo_amd.train", "--gemm-precision", "bf16_mixed", "--frames", "256", "--num-generations", "4",
              "--training-sample-len", "8", "--save-steps", "1", "--output-dir", out]

    def run(steps):
        r = subprocess.run(common + ["--max-steps", str(steps)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return [json.loads(ln) for ln in r.stdout.splitlines() if ln.strip().startswith("{") and ln.strip().endswith("}")]

    first = run(2)
    assert [l["step"] for l in first] == [1, 2]
    assert all(np.isfinite(l["loss"]) and np.isfinite(l["grad_norm"]) for l in first)
    second = run(3)
    assert [l["step"] for l in second] == [3], "the second run must resume after checkpoint 2"
    assert np.isfinite(second[0]["loss"]) and np.isfinite(second[0]["grad_norm"])
