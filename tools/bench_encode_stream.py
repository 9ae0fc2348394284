#!/usr/bin/env python
"""Host frames -> CLIP features, wall clock: today's one-call path against the streamed, chunked path (DESIGN "Long videos").
1024 synthetic 1280x720 uint8 frames in PAGEABLE numpy (2.8 GB, what a video decoder hands over), CLIP-L/14 with random weights.
  (a) encode_chunk_frames=None: the statements of extract_clip_features_impl - one synchronous copy of the whole video to the
      device, preprocess_frames, ONE clip_vit_forward;
  (b) (c) (d) preprocess.encode_frames_streamed at chunk 256 / 512 / 1024: pinned staging, copies on a side stream under the
      previous chunk's compute, workspace of one chunk.
The variants alternate `rounds` times (default 3) after one untimed pass each; frames/s of every run and the best per variant
are printed, and the peak torch.cuda.max_memory_allocated of each variant from a pass of its own with the encoder workspace and
the staging buffers dropped first (weights and the caching allocator's baseline excluded).
Condition (ISSUE "Encode long videos in bounded memory"): best of (b)-(d) not slower than (a) of the same run by more than the
+-3 % box-to-box noise VERDICT.md records.
    python tools/bench_encode_stream.py [frames] [rounds]"""
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from tspo_amd import ops
from tspo_amd.preprocess import encode_frames_streamed, preprocess_frames

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
H, W = 720, 1280
DEV = torch.device("cuda", 0)
c = bench.CLIP_L14
clipw = ops.ClipVitWeights(bench.random_clip_state(c, DEV), c, DEV)
block = np.random.default_rng(5).integers(0, 256, (32, H, W, 3), dtype=np.uint8)
frames = np.concatenate([block] * ((T + 31) // 32))[:T]          # pageable; the content does not matter to the clock
del block


def one_call():
    px = preprocess_frames(torch.from_numpy(frames).to(DEV))
    return ops.clip_vit_forward(clipw, px)


VARIANTS = [("a one call (encode_chunk_frames=None)", one_call)] + \
           [(f"{tag} streamed, chunk {n}", (lambda n=n: encode_frames_streamed(clipw, frames, n))) for tag, n in
            (("b", 256), ("c", 512), ("d", 1024))]


def run(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


peak, ref = {}, None
for name, fn in VARIANTS:                                         # memory pass: nothing cached from another variant
    clipw._ws, clipw._fold_key = None, None
    if hasattr(clipw, "_streamed"):
        del clipw._streamed
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _, out = run(fn)
    peak[name] = torch.cuda.max_memory_allocated() - base
    if ref is None:
        ref = out.clone()
    print(f"{name:40s} peak device memory {peak[name] / 2 ** 30:6.2f} GiB   bitwise == one call: {bool(torch.equal(out, ref))}", flush=True)
    del out
for name, fn in VARIANTS:                                         # untimed pass: workspace, pinned staging, fold, tables
    run(fn)
fps = {name: [] for name, _ in VARIANTS}
for r in range(ROUNDS):
    for name, fn in VARIANTS:
        dt, _ = run(fn)
        fps[name].append(T / dt)
        print(f"round {r + 1}  {name:40s} {dt * 1e3:9.1f} ms  {T / dt:8.1f} frames/s", flush=True)
best = {name: max(v) for name, v in fps.items()}
a = best[VARIANTS[0][0]]
s = max(v for name, v in best.items() if name != VARIANTS[0][0])
print(f"best one call {a:.1f} frames/s; best streamed {s:.1f} frames/s = {s / a:.3f} x   (condition: >= 0.97 x)")
print(json.dumps({"frames": T, "hw": [H, W], "rounds": ROUNDS, "frames_per_s": fps, "best_frames_per_s": best,
                  "peak_bytes": peak, "streamed_over_one_call": s / a}))
