#!/usr/bin/env python
"""Policy-step micro-benchmark (configs[2]: B=4, T=512, G=8, k=16) for profiling.
    python tools/bench_policy.py [steps] [fp32|bf16x3] [dp|dpc|pad]
`dp` = the reference's training configuration (train_deepspeed.sh:30-31): B = 1 per micro-step, 2 micro-steps per optimizer step,
the bucket all-reduce issued on a live one-rank nccl (= RCCL) group - bench.py's `rollouts_dp_path.sequential`; `dpc` = the same
window as ONE stacked rollout / backward (coalesced micro-steps, production since round 5: `rollouts_dp_path`).
`pad` = a window of four haystacks of DIFFERENT length (650, 700, 750, 800 frames: T = 50 x (r + 12), tspo_trainer.py:469-481), which
cannot stack: (seq) four sequential B = 1 micro-steps, the only way to run it without lengths; (a) the same four micro-steps as ONE
batch padded to 800 frames (`rollout(lengths=..., micro_steps=4)`); (b) one micro-step of bs = 4 padded.  The three are timed
alternately, three rounds on the same box, on the live one-rank group like `dp`; one JSON line with every round, the medians, the
spread of the sequential rounds (the margin a difference has to clear) and the padding waste 1 - sum L / (B T)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from tspo_amd import ops
from tspo_amd.pipeline import PolicyTrainer
dev = "cuda"
B, T, G, k, tau = 4, 512, 8, 16, 0.025
gen = torch.Generator(device=dev).manual_seed(99)
feats = torch.randn(B, T, 768, generator=gen, device=dev)
txt = torch.randn(B, 1, 768, generator=gen, device=dev)
clip = ops.clip_scores(txt, feats)
rew = (torch.rand(B, G, generator=gen, device=dev) > 0.5).float() + torch.rand(B, G, generator=gen, device=dev)
flat = bench.flat_from_state(bench.random_selector_state(768, dev), 768, dev)
prec = sys.argv[2] if len(sys.argv) > 2 else "fp32"
DP = len(sys.argv) > 3 and sys.argv[3] in ("dp", "dpc")
COALESCE = len(sys.argv) > 3 and sys.argv[3] == "dpc"
if len(sys.argv) > 3 and sys.argv[3] == "pad":
    import json
    pg = bench.one_rank_group("nccl", torch.device("cuda", 0))
    LENS = (650, 700, 750, 800)
    n, Tp = int(sys.argv[1]) if len(sys.argv) > 1 else 50, max(LENS)
    fl = [torch.randn(1, L, 768, generator=gen, device=dev) for L in LENS]
    tl = [torch.randn(1, 1, 768, generator=gen, device=dev) for _ in LENS]
    cl = [ops.clip_scores(t, f) for t, f in zip(tl, fl)]
    rl = [(torch.rand(1, G, generator=gen, device=dev) > 0.5).float() + torch.rand(1, G, generator=gen, device=dev) for _ in LENS]
    fp, cp = torch.zeros(4, Tp, 768, device=dev), torch.zeros(4, Tp, device=dev)
    for b, L in enumerate(LENS):
        fp[b, :L], cp[b, :L] = fl[b][0], cl[b][0]
    tp, rp = torch.cat(tl), torch.cat(rl)
    lens_d = torch.tensor(LENS, dtype=torch.int32, device=dev)      # uploaded once, as a data loader would with the batch
    trainers = {"seq": PolicyTrainer(flat.clone(), gemm_precision=prec, grad_accum_steps=4),
                "a": PolicyTrainer(flat.clone(), gemm_precision=prec, grad_accum_steps=4),
                "b": PolicyTrainer(flat.clone(), gemm_precision=prec, grad_accum_steps=1)}

    def seq():
        for i in range(4):
            trainers["seq"].step(fl[i], tl[i], cl[i], lambda idx, i=i: rl[i], G, k, tau)
    runs = {"seq": seq,
            "a": lambda: trainers["a"].step(fp, tp, cp, lambda idx: rp, G, k, tau, micro_steps=4, lengths=lens_d, min_length=min(LENS)),
            "b": lambda: trainers["b"].step(fp, tp, cp, lambda idx: rp, G, k, tau, lengths=lens_d, min_length=min(LENS))}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    rates = {name: [] for name in runs}
    for _ in range(3):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            rates[name].append(4 * G / ((time.perf_counter() - t0) / n))
    med = {name: sorted(r)[1] for name, r in rates.items()}
    print(json.dumps({"mode": "pad", "precision": prec, "lengths": LENS, "T_padded": Tp, "G": G, "k": k, "steps_per_round": n,
                      "rollouts_per_s": {name: [round(v) for v in r] for name, r in rates.items()},
                      "median": {name: round(v) for name, v in med.items()},
                      "seq_spread": round((max(rates["seq"]) - min(rates["seq"])) / med["seq"], 4),
                      "speedup_vs_seq": {name: round(med[name] / med["seq"], 3) for name in ("a", "b")},
                      "padding_waste": round(1 - sum(LENS) / (4 * Tp), 4)}))
    sys.exit(0)
if DP:
    pg = bench.one_rank_group("nccl", torch.device("cuda", 0))
    B, accum = 1, 2
    fl = [torch.randn(1, T, 768, generator=gen, device=dev) for _ in range(accum)]
    tl = [torch.randn(1, 1, 768, generator=gen, device=dev) for _ in range(accum)]
    cl = [ops.clip_scores(t, f) for t, f in zip(tl, fl)]
    rl = [(torch.rand(1, G, generator=gen, device=dev) > 0.5).float() + torch.rand(1, G, generator=gen, device=dev) for _ in range(accum)]
    tr = PolicyTrainer(flat, gemm_precision=prec, grad_accum_steps=accum)

    f2, t2, c2, r2 = torch.cat(fl), torch.cat(tl), torch.cat(cl), torch.cat(rl)

    def one():
        if COALESCE:
            tr.step(f2, t2, c2, lambda idx: r2, G, k, tau, micro_steps=accum)
            return
        for i in range(accum):
            tr.step(fl[i], tl[i], cl[i], lambda idx, i=i: rl[i], G, k, tau)
    for _ in range(5):
        one()
    torch.cuda.synchronize()
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(f"dp-path optimizer step ({prec}): {dt * 1e6:.1f} us -> {accum * G / dt:.0f} rollouts/s")
    sys.exit(0)
tr = PolicyTrainer(flat, gemm_precision=prec)
for _ in range(5):
    tr.step(feats, txt, clip, lambda i: rew, G, k, tau)
torch.cuda.synchronize()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
t0 = time.perf_counter()
for _ in range(n):
    tr.step(feats, txt, clip, lambda i: rew, G, k, tau)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
print(f"policy step ({prec}): {dt * 1e3:.3f} ms -> {B * G / dt:.0f} rollouts/s")
