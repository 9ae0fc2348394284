"""A training step that starts from frames, timed phase by phase (one JSON line):

    python tools/bench_train_frames.py [--T 800 512] [--height 720 --width 1280] [--G 8 --k 16] [--iters 5 --rounds 3]

Per haystack length T (800 = 4 true clips + 12 distractor clips of 50 frames; 512 = BASELINE configs[2]): upload of the uint8 pool
[128 video frames || 600 distractor frames], CLIP front end through the index plan (tspo_preprocess_select, uint8 224 x 224), CLIP-L/14
encode + clip score, policy step (G rollouts of k frames, reward = mask overlap, backward, AdamW), and the reward model's input:
the G x k selected frames -> bf16 384 x 384, mean = std = 0.5 (Batch.selected_frames).  prompts/s and the policy share refer to the
sum of the phases.  The last phase is compared with two other ways to the same tensor:
  * "parent_composition": what the library offered before tspo_preprocess_select - gather pool[plan[idx]] with torch, the uint8
    resampling entry on the gathered copy (384-tables), then torch rescale / normalise / cast;
  * "reference_cpu": the reference's way (tspo_trainer.py:516,524): fancy-index on the host, PIL resize + rescale + normalise per
    frame (transformers.image_transforms, as siglip_encoder.py:56-61), to the GPU, to bf16.  Host threads as the process has them.
Timing: hipEvents around `iters` back-to-back calls, one untimed warm-up call per variant, variants ALTERNATED for `rounds` >= 3
rounds; every variant reports the median of its rounds and their min / max (the run-to-run spread)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("upload", "front_end", "encode", "policy_step", "selected_frames")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--T", type=int, nargs="+", default=[800, 512], help="haystack lengths (frames the policy scores)")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--video-frames", type=int, default=128)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the compared variants (>= 3)")
    ap.add_argument("--no-reference-cpu", action="store_true", help="skip the reference's CPU path (seconds per call)")
    ap.add_argument("--dry-run", action="store_true", help="print the JSON skeleton without touching a GPU")
    a = ap.parse_args(argv)
    if a.rounds < 3:
        ap.error("--rounds must be >= 3")
    if a.iters < 1 or min(a.T) < a.k or a.video_frames < 50:
        ap.error("need iters >= 1, T >= k, video-frames >= 50")
    return a


def skeleton(a):
    return {"metric": "train_step_from_frames", "unit": "prompts/s", "G": a.G, "k": a.k, "frame": [a.height, a.width],
            "pool_frames": a.video_frames + 12 * 50, "iters": a.iters, "rounds": a.rounds, "timing": "hipEvents, warm-up discarded",
            "by_T": {str(T): {"prompts_per_s": None, "ms": {p: None for p in PHASES}, "policy_share": None,
                              "selected_frames_ms": {v: None for v in ("new_entry", "parent_composition", "reference_cpu")}}
                     for T in a.T}}


def summarise(ms_rounds):
    return {"median": round(statistics.median(ms_rounds), 4), "min": round(min(ms_rounds), 4), "max": round(max(ms_rounds), 4)}


def main(argv=None):
    a = parse(argv)
    out = skeleton(a)
    if a.dry_run:
        print(json.dumps(out))
        return 0
    import numpy as np
    import torch
    import bench as B
    from tspo_amd import haystack, ops, preprocess as P, rewards
    from tspo_amd.pipeline import PolicyTrainer
    from tspo_amd.train import Batch

    dev = torch.device("cuda", 0)
    H, W, L, G, k = a.height, a.width, a.video_frames, a.G, a.k

    def gpu_ms(fn, iters):
        """ms per call: events around `iters` back-to-back calls."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    def alternate(variants, iters_of=None):
        """{name: fn} -> {name: [ms per round]}: one warm-up call each, then `rounds` rounds in which the variants take turns."""
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        res = {n: [] for n in variants}
        for _ in range(a.rounds):
            for n, fn in variants.items():
                res[n].append(gpu_ms(fn, (iters_of or {}).get(n, a.iters)))
        return res

    clipw = ops.ClipVitWeights(B.random_clip_state(B.CLIP_L14, dev), B.CLIP_L14, dev)
    flat = B.flat_from_state(B.random_selector_state(768, dev), 768, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    pool_host = torch.randint(0, 256, (L + 12 * 50, H, W, 3), generator=g, device=dev, dtype=torch.uint8).cpu().pin_memory()
    txt = torch.randn(1, 1, 768, generator=g, device=dev)
    clip_u8 = P.PreprocessSpec.clip_default(out_dtype=torch.uint8)
    llm = P.PreprocessSpec(size=(384, 384), mean=(0.5,) * 3, std=(0.5,) * 3, out_dtype=torch.bfloat16)
    llm_u8 = llm.with_dtype(torch.uint8)
    mean_d = torch.tensor(llm.mean, device=dev).view(1, 3, 1, 1)
    std_d = torch.tensor(llm.std, device=dev).view(1, 3, 1, 1)

    for T in a.T:
        plan, mask = haystack.build_specific_plan(L, 12, repeat_times=4, rng=np.random.RandomState(T), py_random=None)
        plan, mask = plan[:T].to(dev), mask[:T].to(dev)[None]
        pool = pool_host.to(dev, non_blocking=True)
        state = {}

        def upload():
            state["pool"] = pool_host.to(dev, non_blocking=True)

        def front_end():
            state["px"] = P.select_frames(pool, plan, clip_u8)

        front_end()

        def encode():
            state["feats"] = ops.clip_vit_forward(clipw, state["px"])[None]
            state["clip"] = ops.clip_scores(txt, state["feats"])

        encode()
        trainer = PolicyTrainer(flat.clone())
        reward = lambda idx: rewards.selection_mask_reward_gpu(idx, mask)

        def policy_step():
            state["idx"] = trainer.step(state["feats"], txt, state["clip"], reward, G, k, 0.025)["idx"]

        policy_step()
        batch = Batch(state["feats"], txt, state["clip"], mask, frames=[(pool, plan)])
        idx = state["idx"]

        def new_entry():
            state["sel"] = batch.selected_frames(idx, llm)

        def parent_composition():
            u8 = P.select_frames(pool[plan[idx[0]].reshape(-1)], None, llm_u8)
            state["sel_parent"] = ((u8.float() * llm.rescale - mean_d) / std_d).to(torch.bfloat16).view(1, G, k, 3, 384, 384)

        ph = alternate({"upload": upload, "front_end": front_end, "encode": encode, "policy_step": policy_step})
        cmp_ = alternate({"new_entry": new_entry, "parent_composition": parent_composition})
        agree = float((state["sel"].float() - state["sel_parent"].float()).abs().max())
        r = out["by_T"][str(T)]
        r["ms"] = {n: summarise(v) for n, v in ph.items()}
        r["ms"]["selected_frames"] = summarise(cmp_["new_entry"])
        total = sum(r["ms"][p]["median"] for p in PHASES)
        r["prompts_per_s"] = round(1e3 / total, 3)
        r["policy_share"] = round(r["ms"]["policy_step"]["median"] / total, 5)
        r["selected_frames_ms"] = {n: summarise(v) for n, v in cmp_.items()}
        r["selected_frames_ms"]["max_abs_diff_new_vs_parent"] = agree
        if not a.no_reference_cpu:
            from functools import partial, reduce
            from transformers.image_transforms import normalize, rescale, resize
            from transformers.image_utils import ChannelDimension, PILImageResampling
            df = ChannelDimension.FIRST
            chain = [partial(resize, size=llm.size, resample=PILImageResampling.BICUBIC, data_format=df),
                     partial(rescale, scale=llm.rescale, data_format=df), partial(normalize, mean=llm.mean, std=llm.std, data_format=df)]
            hay_host = pool_host.numpy()
            plan_host = plan.cpu().numpy()

            def reference_cpu():
                outs = []
                for gi in range(G):                                             # G times per prompt, as tspo_trainer.py:508-524
                    sel = hay_host[plan_host[idx[0, gi].cpu().numpy()]]
                    px = np.stack(reduce(lambda x, f: [*map(f, x)], chain, list(sel)))
                    outs.append(torch.from_numpy(px).to(dev).to(torch.bfloat16))
                torch.cuda.synchronize()
                return outs

            reference_cpu()
            wall = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                reference_cpu()
                wall.append((time.perf_counter() - t0) * 1e3)
            r["selected_frames_ms"]["reference_cpu"] = dict(summarise(wall), timing="wall clock, 1 call per round",
                                                            host_threads=torch.get_num_threads())
        del pool, batch, state
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
