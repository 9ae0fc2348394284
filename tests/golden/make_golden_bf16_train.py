"""Generate tests/golden/bf16_train_noise.json: how far the REFERENCE's own bf16 training step sits from its fp32 one.

Run in the authoring container only (needs the reference checkout, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bf16_train.py

For each case of TRAIN_FULL_CASES (c2: B=4, T=512, G=8, k=16; c4: B=1, T=4096, G=16, k=16), with the inputs, rewards and Gumbel
noise of train_full.npz, the re-evaluation loop and loss of tspo_trainer.py:540-609 (the streamed form of
make_golden.trainer_step_streamed: one rollout's term back-propagated at a time) run twice with the indices forced to
train_full.npz's fp32 indices: once on the imported MultiModal_Align in fp32, once on a copy `.to(torch.bfloat16)` fed bf16
inputs - what DeepSpeed bf16 with fp32 master weights computes (train_deepspeed.sh:33-34, scripts/zero3.json:10).  Both start from
the same fp32 parameters.  Stored per trained tensor, as the mean over prompts:
  rel_fro  ||g_bf16 - g_fp32||_F / ||g_fp32||_F
  rel_max  max|g_bf16 - g_fp32| / max|g_fp32|
and the number of (prompt, rollout) index sets the bf16 module's own Gumbel-top-k changes under the fixture's noise (same seeds as
make_golden.py train_full).  Nothing of the reference's source is copied; only these numbers are committed.

CPU time (8 host threads): c2 4 s, c4 35 s (the dense T x T attention of T = 4096 dominates) - about that of
`make_golden.py train_full`.
"""
import copy
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG   # noqa: E402  (puts the repository and the reference on sys.path; imports the reference's modules)

import numpy as np   # noqa: E402
import torch   # noqa: E402

from inputs import TRAIN_FULL_CASES, train_full_inputs   # noqa: E402


def reeval_grads(m, img, txt, clip, w, tau, k, G, idx, adv):
    """tspo_trainer.py:540-609 for one prompt with the rollouts' indices given: {param: fp32 gradient}."""
    m.zero_grad()
    for g in range(G):
        conf, _ = m(img, txt, clip, w, tau)
        _, _, logp_ts = MG.gumbel_softmax(conf.unsqueeze(1), sample_len=k)
        sel = logp_ts[torch.from_numpy(idx[g])]
        term = -(torch.exp(sel - sel.detach()).mean() * adv[g]) / G
        term.backward()
    return {pn: (p.grad.float().clone() if p.grad is not None else torch.zeros(p.shape)) for pn, p in m.named_parameters()}


def main():
    fx = np.load(os.path.join(HERE, "train_full.npz"))
    res = {"what": "reference bf16 (module .to(bfloat16), bf16 inputs) vs fp32 training gradients, indices forced to train_full.npz",
           "cases": {}}
    for name, B, T, D, H, w, tau, k, G in TRAIN_FULL_CASES:
        t0 = time.time()
        img, txt, clip, state, rew = train_full_inputs(name, B, T, D, G)
        m32 = MG.ref_selector(D, H, state)
        m16 = copy.deepcopy(m32).to(torch.bfloat16)
        per = {}
        changed = 0
        for b in range(B):
            idx = fx[f"{name}.idx"][b]
            r = torch.from_numpy(rew[b])
            mean_g = r.view(-1, G).mean(dim=1).repeat_interleave(G, dim=0)
            std_g = r.view(-1, G).std(dim=1).repeat_interleave(G, dim=0)
            adv = (r - mean_g) / (std_g + 1e-4)
            x, e, c = torch.from_numpy(img[b]), torch.from_numpy(txt[b]), torch.from_numpy(clip[b])
            g32 = reeval_grads(m32, x, e, c, w, tau, k, G, idx, adv)
            bf = torch.bfloat16
            g16 = reeval_grads(m16, x.to(bf), e.to(bf), c.to(bf), w, tau, k, G, idx, adv.to(bf))
            for pn in g32:
                if "ffn_o" in pn:
                    continue
                d = (g16[pn] - g32[pn]).double()
                ref = g32[pn].double()
                per.setdefault(pn, []).append((float(d.norm() / max(ref.norm(), 1e-30)), float(d.abs().max() / max(ref.abs().max(), 1e-30))))
            with torch.no_grad():    # the bf16 module's own rollouts under the fixture's noise (seeds of make_golden.gen_train_full)
                conf16, _ = m16(x.to(bf), e.to(bf), c.to(bf), w, tau)
                for g in range(G):
                    torch.manual_seed(6000 + 100 * b + T + g)
                    i16, _, _ = MG.gumbel_softmax(conf16.unsqueeze(1), sample_len=k)
                    changed += int(set(i16.tolist()) != set(idx[g].tolist()))
            print(f"  {name}: prompt {b + 1}/{B} ({time.time() - t0:.0f}s)", flush=True)
        res["cases"][name] = {
            "rel_fro": {pn: float(np.mean([v[0] for v in vs])) for pn, vs in per.items()},
            "rel_max": {pn: float(np.mean([v[1] for v in vs])) for pn, vs in per.items()},
            "changed_index_sets": changed, "index_sets": B * G, "cpu_seconds": round(time.time() - t0, 1)}
        print(f"  {name}: {json.dumps(res['cases'][name])}", flush=True)
    with open(os.path.join(HERE, "bf16_train_noise.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
