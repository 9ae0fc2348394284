#!/usr/bin/env python
"""Several questions about one video: the per-question path against the shared one (T = 1024 frames, random-init CLIP-L/14).
    python tools/bench_questions.py [pixel_iters] [feature_iters]
The reference's harness asks one question per call (mp_tools/vlmeval/vlm/gen_id_tspo.py:59-92) and a benchmark asks Q of them
about a video (VideoMME 3, LVBench ~15).  For Q in {1, 3, 15}:
  pixels    Q sequential FrameScorer.__call__ (encode + clip scores + selector + top-k each: what Q extract_feature_from_pixels +
            temporal_sampling calls launch, the only way before) against ONE FrameScorer.questions (encode once, Q score rows);
  features  from cached features: Q sequential score + top-k calls against one score_questions + one batched top-k.
The two arms of every (mode, Q) are timed alternately, three rounds on the same box; one JSON line with every round in ms per
video, the medians, the speed-up of the medians and the spread of the sequential rounds (the margin a difference has to clear:
at Q = 1 the shared path must not be slower than the single one by more than that)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from tspo_amd import ops
from tspo_amd.pipeline import FrameScorer

dev = "cuda"
T, D, K, QS = 1024, 768, 64, (1, 3, 15)
n_px = int(sys.argv[1]) if len(sys.argv) > 1 else 2
n_ft = int(sys.argv[2]) if len(sys.argv) > 2 else 200
c = bench.CLIP_L14
scorer = FrameScorer(ops.ClipVitWeights(bench.random_clip_state(c, dev), c, dev),
                     bench.flat_from_state(bench.random_selector_state(D, dev), D, dev))
gen = torch.Generator(device=dev).manual_seed(99)
px = torch.randint(0, 256, (T, 3, 224, 224), generator=gen, device=dev, dtype=torch.uint8)
txt = torch.randn(max(QS), 1, D, generator=gen, device=dev)
feats = scorer.encode(px)


def pixels_seq(Q):
    for q in range(Q):
        scorer(px[None], txt[q][None], K)


def pixels_shared(Q):
    scorer.questions(px, txt[:Q], K)


def features_seq(Q):
    for q in range(Q):
        s, _ = scorer.score(feats[None], txt[q][None])
        ops.topk_sorted(s, K)


def features_shared(Q):
    s, _ = scorer.score_questions(feats, txt[:Q])
    ops.topk_sorted(s, K)


out = {"T": T, "k": K, "rounds": 3, "iters": {"pixels": n_px, "features": n_ft}}
for mode, seq, shared, n in (("pixels", pixels_seq, pixels_shared, n_px), ("features", features_seq, features_shared, n_ft)):
    for Q in QS:
        for fn in (seq, shared):      # warm-up: code objects, workspaces, the encoder's folded weights
            fn(Q)
        torch.cuda.synchronize()
        ms = {"seq": [], "shared": []}
        for _ in range(3):
            for name, fn in (("seq", seq), ("shared", shared)):
                t0 = time.perf_counter()
                for _ in range(n):
                    fn(Q)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / n * 1e3)
        med = {name: sorted(v)[1] for name, v in ms.items()}
        out[f"{mode}.Q{Q}"] = {"ms_per_video": {name: [round(v, 4) for v in vs] for name, vs in ms.items()},
                               "median_ms": {name: round(v, 4) for name, v in med.items()},
                               "speedup": round(med["seq"] / med["shared"], 3),
                               "seq_spread": round((max(ms["seq"]) - min(ms["seq"])) / med["seq"], 4),
                               "shared_minus_seq_over_seq": round((med["shared"] - med["seq"]) / med["seq"], 4)}
print(json.dumps(out))
