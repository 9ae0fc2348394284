#!/usr/bin/env python
"""bench.py - frames scored/s (+ rollouts/s) of the TSPO temporal-sampling hot path on MI355X.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python bench.py --gpus 1 --steps 5 --warmup 2 --full   # + every non-headline measurement (see below)
    python bench.py --gpus 8                      # no launcher: spawns its own 8 ranks (one per GPU, RCCL)
    python bench.py --gpus 8 --frames 4096 --shard-frames --rollout-cfg 1,4096,16,16 --full   # configs[4]: ONE 4096-frame video over 8 GPUs (strong scaling)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): TSPO-0.4B frame selection, T=1024 synthetic frames per video,
top-k=32: pixels [B,T,3,224,224] resident in HBM -> CLIP-L/14 encode (bf16 MFMA) -> cosine clip score ->
temporal scoring head (fp32, window 12, tau 0.025) -> greedy top-k.  One "step" = one such pass over one
batch of B videos per GPU.  value = B*T*N*K / max-over-ranks wall time (weak scaling: videos are
independent, no data-path collective).  Weights are random-init tensors of the CLIP-L/14 + selector shapes
(no network for checkpoints).

A plain run does only what `value` needs: set up, warm up, time the steps, write --dump-outputs, print the line.
Everything else runs with --full alone (the --no-* options skip parts of it): the policy side of one TSPO training
step (configs[2]: B=4, T=512, G=8, k=16; reward LLM excluded, rewards synthetic) -> "rollouts_per_s", the DP-path
and bf16x3 rollout figures, the pruned-last-block and 720p variants, the score / select split, the N > 1 sharded
4096-frame point, the RCCL probe, the GEMM roofline with the clock / power sampled during the timed steps, and the
CPU baseline.  Fields a plain run did not measure are null, and "full" says which kind of run printed the line.
"""
import argparse
import json
import os
import sys
import time
import threading

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CLIP_L14 = dict(hidden=1024, layers=24, heads=16, mlp=4096, patch=14, image=224, proj=768)
PEAK_BF16_TFLOPS = 2500.0     # dense MFMA bf16, MI355X_MICROARCH.md (2.5 PF dense; 5 PF figure is 2:1 sparse)


def gemm_flops_per_frame(c):
    S = (c["image"] // c["patch"]) ** 2 + 1
    P = S - 1
    C, mlp = c["hidden"], c["mlp"]
    patch = 2 * P * (3 * c["patch"] ** 2) * C
    layer = 2 * S * C * 3 * C + 2 * S * C * C + 2 * 2 * S * C * mlp
    return patch + c["layers"] * layer + 2 * C * c["proj"]


def alg_bytes_per_launch(c, n_frames):
    """Algorithmic HBM bytes of the encoder GEMMs averaged over the launches of one encode: each operand read
    once, each output written once (bf16 activations, bf16 weights)."""
    S = (c["image"] // c["patch"]) ** 2 + 1
    M, C, mlp = S * n_frames, c["hidden"], c["mlp"]
    qkv = 2 * (M * C + 3 * C * C + M * 3 * C)
    out = 2 * (M * C + C * C + 2 * M * C)            # + residual read
    fc1 = 2 * (M * C + mlp * C + M * mlp)
    fc2 = 2 * (M * mlp + mlp * C + 2 * M * C)
    kp = (3 * c["patch"] ** 2 + 63) // 64 * 64
    patch = 2 * ((M - n_frames) * kp + C * kp + (M - n_frames) * C)
    proj = 2 * (n_frames * C + c["proj"] * C) + 4 * n_frames * c["proj"]
    return (c["layers"] * (qkv + out + fc1 + fc2) + patch + proj) / (4 * c["layers"] + 2)


def attn_flops_per_frame(c):
    S = (c["image"] // c["patch"]) ** 2 + 1
    return c["layers"] * 2 * 2 * S * S * c["hidden"]


def random_clip_state(c, device, seed=11, dtype=torch.float32):
    """Random-init CLIP-L/14 vision tower (HF key names), generated on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)

    def rn(*shape, std=0.02, mean=0.0):
        return torch.randn(*shape, generator=g, device=device, dtype=dtype) * std + mean

    C, mlp, p = c["hidden"], c["mlp"], "vision_model."
    S = (c["image"] // c["patch"]) ** 2 + 1
    st = {p + "embeddings.class_embedding": rn(C), p + "embeddings.patch_embedding.weight": rn(C, 3, c["patch"], c["patch"]),
          p + "embeddings.position_embedding.weight": rn(S, C), p + "pre_layrnorm.weight": rn(C, std=0.05, mean=1.0),
          p + "pre_layrnorm.bias": rn(C), p + "post_layernorm.weight": rn(C, std=0.05, mean=1.0),
          p + "post_layernorm.bias": rn(C), "visual_projection.weight": rn(c["proj"], C)}
    for l in range(c["layers"]):
        q = f"{p}encoder.layers.{l}."
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            st[q + f"self_attn.{nm}.weight"] = rn(C, C)
            st[q + f"self_attn.{nm}.bias"] = rn(C)
        for nm in ("layer_norm1", "layer_norm2"):
            st[q + nm + ".weight"] = rn(C, std=0.05, mean=1.0)
            st[q + nm + ".bias"] = rn(C)
        st[q + "mlp.fc1.weight"], st[q + "mlp.fc1.bias"] = rn(mlp, C), rn(mlp)
        st[q + "mlp.fc2.weight"], st[q + "mlp.fc2.bias"] = rn(C, mlp), rn(C)
    return st


def random_selector_state(D, device, seed=7):
    g = torch.Generator(device=device).manual_seed(seed)
    names = ["temporal.Self_q", "temporal.Self_k", "temporal.Self_v", "temporal.ffn_o", "mlp.0", "mlp.2"]
    st = {}
    for n in names:   # HF _init_weights: N(0, 0.02) weights, zero bias (tspo_trainer.py:201)
        st[n + ".weight"] = torch.randn(D, D, generator=g, device=device) * 0.02
        st[n + ".bias"] = torch.zeros(D, device=device)
    return st


def flat_from_state(st, D, device):
    from tspo_amd import ops
    offs = ops.flat_offsets(D)
    flat = torch.zeros(offs["__total__"][0], dtype=torch.float32, device=device)
    for name, (off, shape) in offs.items():
        if not name.startswith("__"):
            flat[off:off + st[name].numel()] = st[name].flatten().to(device)
    return flat


def cpu_baseline(T, k):
    """The oracle (CPU restatement of the reference path, oracle/tspo_oracle.py) on the host cores, bounded sample:
    CLIP-L on n frames (frames are independent -> per-frame cost), selector + top-k at the full T."""
    from oracle import tspo_oracle as O
    c = CLIP_L14
    w = random_clip_state(c, "cpu")
    sel = random_selector_state(768, "cpu")
    g = torch.Generator().manual_seed(1234)
    if torch.get_num_threads() > 32:
        torch.set_num_threads(32)   # measured on the 128-thread EPYC host: 16/32/64/128 threads -> 3.6/3.9/2.9/1.7 frames/s
    cores = torch.get_num_threads()

    def enc(n):
        px = torch.randn(n, 3, c["image"], c["image"], generator=g)
        t0 = time.perf_counter()
        with torch.no_grad():
            O.clip_vit_forward(w, px, num_heads=c["heads"], patch=c["patch"])
        return time.perf_counter() - t0

    enc(4)                                     # warm-up (thread pool, allocator)
    n = 64                                     # encode timed at N = 64 frames, scaled linearly
    tn = enc(n)
    feats = torch.randn(T, 768, generator=g)
    txt = torch.randn(1, 768, generator=g)
    with torch.no_grad():
        clip = O.clip_cosine_scores(txt, feats)
        O.selector_forward(sel, feats, txt, clip, 12, 0.025)
        t0 = time.perf_counter()
        s, _ = O.selector_forward(sel, feats, txt, clip, 12, 0.025)
        O.topk_sorted(s, k)
        tsel = time.perf_counter() - t0
    per_frame = tn / n + tsel / T
    model = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": round(1.0 / per_frame, 3), "unit": "frames/s", "cores": cores, "kind": "port",
            "cpu_model": model, "host_logical_cpus": os.cpu_count(),
            "sample": f"oracle (torch-CPU fp32): CLIP-L/14 on {n} frames in {tn:.2f}s + selector/top-k at T={T} in "
                      f"{tsel * 1e3:.1f}ms, {cores} threads"}


PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X dense fp32 matrix peak (MI355X_MICROARCH.md)


LAST_RUNTIME_COPIES = {}     # memcpy / memset device records per call of the last count_kernel_launches (runtime work, not library kernels)


def count_kernel_launches(fn, reps: int = 3):
    """Kernel launches of one call of `fn`, counted LIVE by the profiler's device-activity records (roctracer) over
    `reps` calls; returns (launches per call, {kernel name: launches per call}) or (None, reason) if tracing is
    unavailable in this process."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        names, runtime = {}, {}
        for ev in prof.events():
            if not (str(getattr(ev, "device_type", "")).endswith("CUDA") and ev.name):
                continue
            if ev.name.lower().startswith(("memcpy", "memset")):     # the runtime's own copies / fills (not kernels of the library):
                key = ev.name.split("(")[0].strip()                  # named and counted beside the kernels, not hidden
                runtime[key] = runtime.get(key, 0) + 1
                continue
            short = ev.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0].split("::")[-1]
            names[short] = names.get(short, 0) + 1
        total = sum(names.values())
        if total == 0 or total % reps:
            return None, f"profiler saw {total} device kernels over {reps} calls"
        LAST_RUNTIME_COPIES.clear()
        LAST_RUNTIME_COPIES.update({k: v / reps for k, v in sorted(runtime.items())})
        return total // reps, {k: v / reps for k, v in sorted(names.items())}
    except Exception as e:      # tracing unavailable (e.g. under rocprofv3): report why, never a made-up constant
        return None, f"{type(e).__name__}: {e}"


def policy_step_roofline(B: int, T: int, D: int, step_s: float, launches=None, per_kernel=None) -> dict:
    """What bounds one policy step (selector forward + G rollouts + backward + clip + AdamW): its fp32 MFMA GEMMs.
    Forward: q|k|v [BT,D]x[D,3D] + two [BT,D]x[D,D]; backward: two data gradients [BT,D]x[D,D] and the three weight
    gradients (D*D, D*D, 3*D*D outputs over BT rows).  Everything else (banded attention, scores, Gumbel top-k, advantage,
    AdamW over 2.95 M parameters) is < 2 % of the FLOPs but ~28 % of the time: 17 dependent launches of a few us each."""
    bt = B * T
    fwd = 2.0 * bt * D * (3 * D + D + D)
    bwd = 2.0 * bt * D * (D + D) + 2.0 * bt * D * (D + D + 3 * D)
    ach = (fwd + bwd) / step_s / 1e12
    return {"bound": "mfma", "unit": "TFLOP/s", "dtype": "f32", "gemm_flop_per_step": fwd + bwd,
            "achieved": round(ach, 1), "peak": PEAK_FP32_MFMA_TFLOPS, "frac": round(ach / PEAK_FP32_MFMA_TFLOPS, 4),
            "launches_per_step": launches, "launches_source": "counted live (torch.profiler device records)" if launches else per_kernel,
            "launches_by_kernel": per_kernel if launches else None, "us_per_step": round(step_s * 1e6, 1),
            "note": "achieved = GEMM FLOPs / WHOLE step time (the non-GEMM launches are inside the denominator)"}


class GpuSampler:
    """sclk / package power of the GPU a rank runs on, sampled from a background thread DURING a timed region (the chip is
    power-limited under this workload: the clock it sustains, not the 2.4 GHz the nominal peak assumes, decides what a box
    delivers - VERDICT r3 weak #8).  Source: the amdgpu hwmon files of the device with this rank's PCI address
    (freq1_input = sclk in Hz, power1_average / power1_input in microwatts); amdsmi as the fallback.  Never fatal."""

    def __init__(self, dev, period_s: float = 0.02):
        import threading
        self.period, self.samples, self._stop, self._thr = period_s, [], threading.Event(), None
        self.source, self._read = None, None
        try:
            pr = torch.cuda.get_device_properties(dev)
            bdf = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            self.pci = bdf
            import glob
            for card in sorted(glob.glob("/sys/class/drm/card*/device")):
                if os.path.basename(os.path.realpath(card)).lower() != bdf:
                    continue
                for hw in glob.glob(os.path.join(card, "hwmon", "hwmon*")):
                    f_clk = os.path.join(hw, "freq1_input")
                    f_pw = next((q for q in (os.path.join(hw, "power1_average"), os.path.join(hw, "power1_input")) if os.path.exists(q)), None)
                    if os.path.exists(f_clk):
                        def rd(f_clk=f_clk, f_pw=f_pw):
                            clk = int(open(f_clk).read()) / 1e6
                            pw = int(open(f_pw).read()) / 1e6 if f_pw else None
                            return clk, pw
                        rd()
                        self._read, self.source = rd, f"sysfs {hw}"
                        break
        except Exception as e:
            self.source = f"sysfs unavailable ({type(e).__name__}: {e})"[:160]
        if self._read is None:
            try:
                import amdsmi
                amdsmi.amdsmi_init()
                hs = amdsmi.amdsmi_get_processor_handles()
                h = hs[dev.index if dev.index is not None and dev.index < len(hs) else 0]

                def rd():
                    ck = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX)
                    pw = amdsmi.amdsmi_get_power_info(h)
                    p = pw.get("current_socket_power", pw.get("average_socket_power"))
                    return float(ck.get("clk", ck.get("cur_clk"))), (float(p) if isinstance(p, (int, float)) else None)
                rd()
                self._read, self.source = rd, "amdsmi"
            except Exception as e:
                self.source = (self.source or "") + f"; amdsmi unavailable ({type(e).__name__})"

    def __enter__(self):
        import threading
        if self._read is not None:
            def loop():
                while not self._stop.is_set():
                    try:
                        self.samples.append(self._read())
                    except Exception:
                        pass
                    self._stop.wait(self.period)
            self._thr = threading.Thread(target=loop, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._thr is not None:
            self._thr.join(timeout=2)

    def summary(self) -> dict:
        out = {"source": self.source, "samples": len(self.samples), "pci": getattr(self, "pci", None)}
        if self.samples:
            ck = sorted(c for c, _ in self.samples)
            pw = sorted(p for _, p in self.samples if p is not None)
            out.update(sclk_mhz=round(sum(ck) / len(ck), 1), sclk_mhz_min=round(ck[0], 1), sclk_mhz_max=round(ck[-1], 1))
            if pw:
                out.update(power_w=round(sum(pw) / len(pw), 1), power_w_max=round(pw[-1], 1))
        return out


def rccl_debug_summary(path: str) -> dict:
    """What RCCL logged about its topology choice (NCCL_DEBUG=INFO into `path`, set by main() before the first communicator):
    channel / ring / tree counts and the algorithms / protocols it enabled - the first thing to read when an N > 1 run misbehaves."""
    import glob
    import re
    txt = ""
    for f in glob.glob(path.replace("%h", "*").replace("%p", "*")):
        try:
            txt += open(f, errors="replace").read()
        except OSError:
            pass
    if not txt:
        return {"log": "no RCCL debug output captured"}
    pick = [ln.split("NCCL INFO", 1)[-1].strip() for ln in txt.splitlines()
            if re.search(r"Ring|Tree|Channel|Connected all|algorithm|Algo|protocol|nChannels|comm 0x|xGMI|XGMI|P2P|SHM", ln)]
    return {"rings": len(re.findall(r"Connected all rings", txt)), "trees": len(re.findall(r"Connected all trees", txt)),
            "channel_lines": sum("Channel" in ln for ln in pick), "lines": pick[:24], "total_lines": len(txt.splitlines())}


def comm_probe(backend: str, world: int, dev, n_bucket: int) -> dict:
    """{"backend", "world", "allreduce_us", ...}: the gradient-bucket all-reduce (11.8 MB fp32, tspo_amd.dist.
    allreduce_bucket_, the one collective of a data-parallel TSPO step) timed on this job's process group, which device /
    PCI address every rank sits on, and - for N > 1 - the same all-reduce on communicators created with NCCL_ALGO=Ring and
    NCCL_ALGO=Tree (xGMI is point-to-point, so which one wins is a per-node fact).  The caller owns the group
    (a one-rank "nccl" group at N = 1, so librccl / the device binding are exercised on every run).  Never fatal."""
    import torch.distributed as dist
    from tspo_amd import dist as tdist
    info = {"backend": backend, "library": "rccl" if backend == "nccl" else backend, "world": world,
            "bucket_bytes": 4 * n_bucket, "allreduce_us": None}

    def time_allreduce(group, reps=20):
        return _time_allreduce(backend, dev, n_bucket, group, reps)

    try:
        info["world"] = dist.get_world_size()
        pr = torch.cuda.get_device_properties(dev)
        mine = {"rank": dist.get_rank(), "device": str(dev), "name": pr.name,
                "pci": f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0",
                "local_rank_env": os.environ.get("LOCAL_RANK"), "hsa_ipc_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}
        ranks = [None] * info["world"]
        dist.all_gather_object(ranks, mine)
        info["ranks"] = ranks
        info["distinct_devices"] = len({r["pci"] for r in ranks})
        bucket = torch.ones(n_bucket + 8, dtype=torch.float32, device=dev)
        for _ in range(4):          # 1 -> world^4 stays exact in fp32 for any world size
            tdist.allreduce_bucket_(bucket, n_bucket)
        torch.cuda.synchronize()
        ok = bool((bucket[:n_bucket] == float(info["world"]) ** 4).all()) and bool((bucket[n_bucket:] == 1.0).all())
        us = time_allreduce(None)
        info.update(allreduce_us=round(us, 1), sum_correct=ok, algbw_GBps=round(4 * n_bucket / (us * 1e-6) / 1e9, 2))
        if backend == "nccl":
            try:
                info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                pass
            # (Ring vs Tree needs extra communicators: comm_algo_probe, run LAST and under a watchdog - never before a timed region)
            if os.environ.get("NCCL_DEBUG_FILE"):
                info["rccl_debug"] = rccl_debug_summary(os.environ["NCCL_DEBUG_FILE"])
    except Exception as e:
        info["error"] = f"{type(e).__name__}: {e}"[:300]
    return info


def _time_allreduce(backend: str, dev, n_bucket: int, group, reps: int = 20) -> float:
    """us per all-reduce of the gradient bucket on `group` (max over ranks)."""
    import torch.distributed as dist
    from tspo_amd import dist as tdist
    bucket = torch.zeros(n_bucket + 8, dtype=torch.float32, device=dev)
    for _ in range(3):
        tdist.allreduce_bucket_(bucket, n_bucket, group)
    torch.cuda.synchronize()
    if dist.get_world_size(group) > 1:
        dist.barrier(group)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        tdist.allreduce_bucket_(bucket, n_bucket, group)
    torch.cuda.synchronize()
    t = torch.tensor([(time.perf_counter() - t0) / reps * 1e6], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    if dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return t.item()


def comm_algo_probe(dev, n_bucket: int) -> dict:
    """N > 1, RCCL: the bucket all-reduce on communicators created with NCCL_ALGO=Ring and =Tree (the variable is read when a
    communicator is created).  Creates extra communicators, so the caller runs it AFTER every timed region and under a watchdog."""
    import torch.distributed as dist
    by_algo, keep = {}, os.environ.get("NCCL_ALGO")
    for algo in ("Ring", "Tree"):
        try:
            os.environ["NCCL_ALGO"] = algo
            grp = dist.new_group(backend="nccl")
            by_algo[algo] = round(_time_allreduce("nccl", dev, n_bucket, grp), 1)
        except Exception as e:
            by_algo[algo] = f"{type(e).__name__}: {e}"[:120]
    if keep is None:
        os.environ.pop("NCCL_ALGO", None)
    else:
        os.environ["NCCL_ALGO"] = keep
    return by_algo


def one_rank_group(backend: str, dev):
    """A live world-size-1 process group (own TCPStore: under torch.distributed.run env:// would go to the agent's store)."""
    import datetime
    import torch.distributed as dist
    from tspo_amd import dist as tdist
    store = dist.TCPStore("127.0.0.1", tdist.free_port(), 1, is_master=True, timeout=datetime.timedelta(seconds=60))
    kw = {"device_id": dev} if backend == "nccl" else {}
    dist.init_process_group(backend, store=store, rank=0, world_size=1, timeout=datetime.timedelta(seconds=120), **kw)


def dp_path_rollouts(flat, dev, world: int, rank: int, cfg, steps: int, timed) -> dict:
    """rollouts/s on the path the REFERENCE'S training configuration takes (train_deepspeed.sh:30-31: per_device_train_batch_size
    1, gradient_accumulation_steps 2, data-parallel ranks): one prompt per micro-step, two micro-steps per optimizer step, the
    second micro-batch added into the bucket, ONE all-reduce of the bucket really issued on the live process group every
    optimizer step, then clip + AdamW.  Needs an initialised process group (the caller's)."""
    from tspo_amd import ops
    from tspo_amd.pipeline import PolicyTrainer
    _, Tt, G, kt = cfg
    tau, accum = 0.025, 2
    gen = torch.Generator(device=dev).manual_seed(199 + rank)
    feats = [torch.randn(1, Tt, 768, generator=gen, device=dev) for _ in range(accum)]
    ttxt = [torch.randn(1, 1, 768, generator=gen, device=dev) for _ in range(accum)]
    clip = [ops.clip_scores(t, f) for t, f in zip(ttxt, feats)]
    rew = [(torch.rand(1, G, generator=gen, device=dev) > 0.5).float() + torch.rand(1, G, generator=gen, device=dev) for _ in range(accum)]
    seen = {}
    # (a) coalesced (production since round 5, what tspo_amd.train does when the micro-batches stack): the two prompts of the
    #     optimizer step as ONE stacked rollout / backward - same Philox draws per prompt, same weights (no update between the
    #     reference's micro-steps, tspo_trainer.py:500-552)
    f2, t2, c2, r2 = torch.cat(feats), torch.cat(ttxt), torch.cat(clip), torch.cat(rew)
    trainer = PolicyTrainer(flat.clone(), grad_accum_steps=accum)

    def opt_step():
        st = trainer.step(f2, t2, c2, lambda idx: r2, G, kt, tau, micro_steps=accum)
        seen["world"] = st["world"]

    # (b) sequential (round 4): one rollout / backward per micro-step, the second accumulated into the bucket
    trainer_seq = PolicyTrainer(flat.clone(), grad_accum_steps=accum)

    def opt_step_seq():
        for i in range(accum):
            trainer_seq.step(feats[i], ttxt[i], clip[i], lambda idx, i=i: rew[i], G, kt, tau)

    n = max(steps, 200)
    sec = timed(opt_step, n, 3)
    sec_seq = timed(opt_step_seq, n, 3)
    n_launch, by_kernel = (None, "counted on rank 0 of a single-rank job only") if (rank or world > 1) else count_kernel_launches(opt_step)
    copies = dict(LAST_RUNTIME_COPIES) if n_launch else None
    n_seq = None if (rank or world > 1) else count_kernel_launches(opt_step_seq)[0]
    return {"rollouts_per_s": round(accum * G * world * n / sec, 1), "us_per_optimizer_step": round(sec / n * 1e6, 1),
            "config": {"prompts_per_micro_step": 1, "grad_accum_steps": accum, "T": Tt, "G": G, "k": kt, "ranks": world},
            "variant": "coalesced micro-steps: the window's prompts as one stacked rollout / backward (indices bitwise those of the sequential path)",
            "allreduce": f"issued every optimizer step on the live {seen.get('world')}-rank process group (11.8 MB fp32 bucket)",
            "launches_per_optimizer_step": n_launch, "launches_by_kernel": by_kernel if n_launch else None,
            "runtime_copies_per_optimizer_step": copies,
            "launches_note": None if n_launch else by_kernel,
            "roofline": policy_step_roofline(accum, Tt, 768, sec / n, n_launch, by_kernel if n_launch else None),
            "sequential": {"rollouts_per_s": round(accum * G * world * n / sec_seq, 1), "us_per_optimizer_step": round(sec_seq / n * 1e6, 1),
                           "launches_per_optimizer_step": n_seq},
            "note": "the reference's configuration (train_deepspeed.sh:30-31); `rollouts_per_s` above is the fused single-rank variant"}


def workload_name(T: int, B: int, k: int, world: int, shard: bool) -> str:
    """config.workload, derived from what is actually run (never a constant: VERDICT r5 weak #7)."""
    what = "TSPO-0.4B frame selection (CLIP-L/14 encode + scoring head + top-k)"
    if shard:
        return (f"configs[4] long-form option: ONE T={T}-frame video per step, frames sharded over {world} rank(s) for the encode, "
                f"all-gather of the features, replicated scoring head + top-{k} (SURVEY 8e)")
    if T == 1024 and B == 1 and k == 32:
        return f"configs[1]: {what}, T=1024, top-k 32" + ("" if world == 1 else f", one video per GPU on {world} GPUs")
    if T == 4096:
        return f"configs[4] per-GPU share (long-form stress, frame scoring side): {what}, T=4096, top-k {k}, {B} video(s) per GPU"
    return f"custom: {what}, T={T}, top-k {k}, {B} video(s) per GPU"


def committed_traffic(n_frames: int, ln_fold: bool):
    """(HBM-side bytes per GEMM launch, source, per-form rows) from a committed rocprofv3 --pmc summary (FETCH_SIZE / WRITE_SIZE
    passes cannot run inside this process) - but ONLY from a file that tools/pmc_traffic.py bound to the library this process
    loaded (sha256 of the .so, or of the sources it is built from): a stale round's bytes are never quoted for new kernels.
    Otherwise (None, why, None)."""
    import glob
    if not ln_fold:
        return None, "no committed traffic pass for --no-ln-fold with this library", None
    try:
        from tspo_amd.build import lib_identity
        me = lib_identity()
    except Exception as e:
        return None, f"library identity unavailable ({type(e).__name__}: {e})", None
    seen = []
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_gemm_hbm_traffic_T{n_frames}.json")), reverse=True):
        try:
            tj = json.load(open(path))
        except Exception:
            continue
        lib = tj.get("library") or {}
        how = ("library sha256" if lib.get("lib_sha256") and lib.get("lib_sha256") == me["lib_sha256"] else
               "source sha256" if lib.get("src_sha256") and lib.get("src_sha256") == me["src_sha256"] else None)
        seen.append(os.path.basename(path))
        if how:
            rel = "profiles/" + os.path.basename(path)
            return tj["hbm_bytes_per_launch_avg"], f"{rel} (rocprofv3 --pmc passes of this command; bound to the loaded library by {how})", tj.get("forms")
    return None, (f"no profiles/*_gemm_hbm_traffic_T{n_frames}.json is bound to the loaded library (lib {str(me['lib_sha256'])[:12]}, "
                  f"src {me['src_sha256'][:12]}); {len(seen)} older file(s) ignored - run tools/prof_round.sh on this build"), None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path: str, tensors: dict, limit: int = DUMP_LIMIT_BYTES) -> dict:
    """Write each tensor as path/<name>.npy (floating point as float32, integers as float64: exact below 2**53), at most `limit`
    bytes in all.  An array over its share of the budget keeps a fixed, seeded sample of its rows (last axis intact), and
    <name>_rows.npy lists the kept row numbers.  Returns {file name: shape written}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrs = {}
    for name, t in tensors.items():
        t = t.detach().cpu()
        arrs[name] = (t.float() if t.is_floating_point() else t.double()).numpy()
    written, left = {}, limit - 4096 * len(arrs)      # (headroom for the .npy headers)
    for i, name in enumerate(sorted(arrs, key=lambda n: arrs[n].nbytes)):       # the small ones first, whole
        a = arrs[name]
        share = left // (len(arrs) - i)
        if a.nbytes > share:
            rows = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 1)
            keep = np.sort(np.random.default_rng(0).choice(len(rows), size=max(1, share // (rows[0].nbytes + 8)), replace=False))
            a = rows[keep]
            np.save(os.path.join(path, f"{name}_rows.npy"), keep.astype(np.float64))
            written[f"{name}_rows.npy"] = list(keep.shape)
            left -= keep.size * 8
        np.save(os.path.join(path, f"{name}.npy"), a)
        written[f"{name}.npy"] = list(a.shape)
        left -= a.nbytes
    return written


FULL_ONLY = ("no_cpu_baseline", "no_rollouts", "no_profile", "no_pruned", "no_720p", "no_long_form", "no_comm_probe")


def parse_args(argv=None):
    """The command line; without --full every non-headline measurement is switched off (each FULL_ONLY option set)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1024, help="T, frames per video")
    ap.add_argument("--videos", type=int, default=1, help="B, videos per GPU per step")
    ap.add_argument("--topk", type=int, default=32)
    ap.add_argument("--pixels", default="u8", choices=["u8", "bf16", "f16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-rollouts", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for dry runs)")
    ap.add_argument("--same-device", action="store_true", help="dry-run aid: every rank uses cuda:0")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads for the CPU baseline (0 = torch default)")
    ap.add_argument("--rollout-cfg", default="4,512,8,16", help="B,T,G,k of the policy step (configs[2]: 4,512,8,16; configs[4] stress: 1,4096,16,16)")
    ap.add_argument("--no-pruned", action="store_true", help="skip the extra (non-headline) run with the pruned last block")
    ap.add_argument("--no-ln-fold", action="store_true", help="A/B: stand-alone LayerNorm passes instead of folding them into the GEMMs")
    ap.add_argument("--no-720p", action="store_true", help="skip the extra (non-headline) run that starts from 720p uint8 frames")
    ap.add_argument("--shard-frames", action="store_true",
                    help="configs[4] long-form option (SURVEY 8e): ONE --frames video per step, its frames sharded over the N ranks for the "
                         "encode (FrameScorer.encode(shard_frames=True)), one all-gather of the features, replicated selector + top-k; "
                         "value = frames of that one video / s (STRONG scaling)")
    ap.add_argument("--no-long-form", action="store_true", help="N > 1: skip the extra (non-headline) sharded 4096-frame video measurement")
    ap.add_argument("--no-comm-probe", action="store_true", help="skip the RCCL probe (init + timed all-reduce of the gradient bucket)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what rank 0's last timed step returned (top-k indices, scores, features) as "
                         "DIR/<name>.npy, float32 / float64, at most 64 MB in all; the inputs are seeded, so two builds compare output for output")
    ap.add_argument("--full", action="store_true",
                    help="also run every non-headline measurement (rollouts, variants, score / select split, comm probe, roofline, "
                         "CPU baseline); without it the --no-* options have nothing to skip")
    a = ap.parse_args(argv)
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:
        for opt in FULL_ONLY:
            setattr(a, opt, True)
    return a


def main():
    a = parse_args()

    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X (no CPU path in the product); use gpurun")
    if not a.no_comm_probe and "NCCL_DEBUG" not in os.environ:
        # RCCL's own account of the topology it chose, into a file (read back by comm_probe): must be set before the first communicator
        import tempfile
        os.environ["NCCL_DEBUG"] = "INFO"
        os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,GRAPH,TUNING"
        # (a directory of this launch's own - every rank of a torchrun job gets its own - removed again once the summary is taken;
        #  RCCL writes its INIT / GRAPH / TUNING lines at communicator creation, not during the timed collectives)
        os.environ["TSPO_RCCL_LOG_DIR"] = tempfile.mkdtemp(prefix="tspo_rccl_")
        os.environ["NCCL_DEBUG_FILE"] = os.path.join(os.environ["TSPO_RCCL_LOG_DIR"], "rccl_%h_%p.log")
    from tspo_amd import dist as tdist
    if a.gpus > 1 and not tdist.launched_by_torchrun():
        # bare `python bench.py --gpus N`: become the launcher - one rank per GPU, like torch.distributed.run would
        if not a.same_device and torch.cuda.device_count() < a.gpus:
            sys.exit(f"--gpus {a.gpus} but only {torch.cuda.device_count()} GPU(s) visible (use --same-device --backend gloo for a dry run)")
        sys.exit(tdist.self_spawn(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        # the launcher's WORLD_SIZE is what actually runs; say so instead of dying (the JSON line reports n_gpus = world)
        print(f"bench.py: --gpus {a.gpus} but the launcher set WORLD_SIZE={world}; running {world} rank(s)", file=sys.stderr)
    if a.same_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1:
        tdist.init_from_env(a.backend, device=dev)              # "nccl" = RCCL over xGMI

    from tspo_amd import ops
    from tspo_amd.pipeline import FrameScorer, PolicyTrainer

    # ---- comm probe: how many ranks the collective library sees and what THE all-reduce of the step costs.  N > 1: on the
    #      job's group, now; N = 1: on a one-rank group created AFTER the fused single-rank rollout figure (an initialised
    #      process group switches PolicyTrainer to the data-parallel path), together with the DP-path rollout figure ----------
    comm = None
    if not a.no_comm_probe and world > 1:
        comm = comm_probe(a.backend, world, dev, ops.trainable_numel(768))

    c = CLIP_L14
    B, T, k = a.videos, a.frames, a.topk
    clipw = ops.ClipVitWeights(random_clip_state(c, dev), c, dev)
    flat = flat_from_state(random_selector_state(768, dev), 768, dev)
    scorer = FrameScorer(clipw, flat, fold_layernorm=not a.no_ln_fold)
    shard = bool(a.shard_frames)
    if shard and B != 1:
        sys.exit("--shard-frames scores ONE video per step (B = 1): its frames are what is sharded")
    # (sharded: every rank holds the same video and encodes its own contiguous slice of frames)
    g = torch.Generator(device=dev).manual_seed(1234 + (0 if shard else rank))
    if a.pixels == "u8":
        pixels = torch.randint(0, 256, (B, T, 3, c["image"], c["image"]), generator=g, device=dev, dtype=torch.uint8)
    else:
        dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.pixels]
        pixels = torch.randn(B, T, 3, c["image"], c["image"], generator=g, device=dev).to(dt)
    txt = torch.randn(B, 1, 768, generator=torch.Generator(device=dev).manual_seed(4321), device=dev)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, warmup, per_step=None, after_warmup=None, per_rank=None):
        """`steps` calls of fn between two barriers; per_step (a list) additionally receives every step's duration from HIP
        events recorded on the launch stream inside the same region (no extra synchronisation).  after_warmup() runs behind the
        first barrier (the clock / power sampler starts there: warm-up and barrier time stay out of its averages);
        per_rank (a list) receives EVERY rank's own wall time of the region, so a slow rank shows in the first N > 1 record."""
        for _ in range(warmup):
            fn()
        barrier()
        if after_warmup is not None:
            after_warmup()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if per_step is not None else None
        t0 = time.perf_counter()
        for i in range(steps):
            if evs:
                evs[i].record()
            fn()
        if evs:
            evs[steps].record()
        barrier()
        dt_ = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        if evs:
            per_step.extend(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
        if per_rank is not None:
            if world > 1:      # (an all-reduce of a one-hot-placed vector: works on every backend, also gloo with device tensors)
                allt = torch.zeros(world, device=dev, dtype=torch.float64)
                allt[rank] = dt_[0]
                dist.all_reduce(allt, op=dist.ReduceOp.SUM)
                per_rank.extend(float(x) for x in allt.tolist())
            else:
                per_rank.append(float(dt_.item()))
        if world > 1:
            dist.all_reduce(dt_, op=dist.ReduceOp.MAX)
        return dt_.item()

    # ---- frames scored / s ---------------------------------------------------
    out = {}

    def score_step():
        if shard:      # frames of the one video over the ranks -> all-gather [T/N, 768] shards -> replicated selector + top-k
            feats = scorer.encode(pixels, shard_frames=True)
            sc, _ = scorer.score(feats, txt)
            out["idx"], out["scores"], out["feats"] = ops.topk_sorted(sc, k), sc, feats
        else:
            out["idx"], out["scores"], out["feats"] = scorer(pixels, txt, k)

    step_ms, rank_sec = [], []
    sampler = GpuSampler(dev) if a.full else None      # (read by the roofline only)
    try:
        sec = timed(score_step, a.steps, a.warmup, per_step=step_ms, per_rank=rank_sec,
                    after_warmup=sampler.__enter__ if sampler is not None else None)
    finally:
        if sampler is not None:
            sampler.__exit__(None, None, None)
    gpu_state = sampler.summary() if sampler is not None else None
    frames = B * T * (1 if shard else world) * a.steps      # sharded: the ranks share ONE video (strong scaling)
    fps = frames / sec
    assert out["idx"].shape == (B, min(T, k)) and bool((out["idx"][:, 1:] > out["idx"][:, :-1]).all())
    dumped = None
    if a.dump_outputs and rank == 0:      # the last timed step's results, before the variants below reuse `out`
        dumped = {"dir": a.dump_outputs, "rank": 0,
                  "arrays": dump_outputs(a.dump_outputs, {"topk_idx": out["idx"], "scores": out["scores"], "features": out["feats"]})}

    # ---- opt-in variant (NOT the headline): last transformer block evaluated for the class-token row only --------
    # (its other 256 token rows have no consumer; identical features, 3.5 % fewer executed FLOPs; reported separately
    # because `value` must execute the full model like the reference does)
    pruned_fps = None
    if not a.no_pruned and not shard:
        scorer.prune_last_layer = True
        psec = timed(score_step, a.steps, 1)
        scorer.prune_last_layer = False
        pruned_fps = frames / psec
        assert bool((out["idx"][:, 1:] > out["idx"][:, :-1]).all())
        score_step()   # restore the full-model outputs used by the checks below

    # ---- non-headline: the real front end of the path (temporal_agent.py:156-164): 1280x720 uint8 frames in HBM ->
    # Pillow-exact antialiased bicubic resize + centre crop on the GPU (tspo_preprocess_frames) -> the same scoring path ----
    from_720p = None
    if not a.no_720p and not shard:
        from tspo_amd import preprocess as PP
        raw = torch.randint(0, 256, (T, 720, 1280, 3), generator=g, device=dev, dtype=torch.uint8)     # one video's frames

        def raw_step():
            px = PP.preprocess_frames(raw)
            out["idx720"], _, _ = scorer(px[None], txt[:1], k)

        rsec_ = timed(raw_step, a.steps, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        PP.preprocess_frames(raw)
        e0.record()
        for _ in range(5):
            PP.preprocess_frames(raw)
        e1.record()
        torch.cuda.synchronize()
        pre_ms = e0.elapsed_time(e1) / 5
        from_720p = {"frames_scored_per_s": round(T * world * a.steps / rsec_, 2), "preprocess_ms": round(pre_ms, 3),
                     "preprocess_input_TBps": round(raw.numel() / (pre_ms * 1e-3) / 1e12, 3),
                     "note": "1280x720 uint8 THWC frames resident in HBM -> on-device CLIPImageProcessor-exact resize + crop -> "
                             "same scoring path (one video per GPU); not used for `value` (SURVEY 8d defines it on 224x224 pixels)"}
        assert bool((out["idx720"][:, 1:] > out["idx720"][:, :-1]).all())
        del raw

    # ---- N > 1, non-headline: configs[4]'s long-form option measured in the SAME launch (the driver's scaling run only passes
    #      --gpus / --steps / --warmup): ONE 4096-frame video per step, frames sharded over the N ranks for the encode, one all-gather,
    #      replicated scoring head + top-k -> a STRONG-scaling frames/s point per N; `--shard-frames` makes it the headline ----
    long_form = None
    if world > 1 and not shard and not a.no_long_form:
        try:
            TL = 4096
            gl = torch.Generator(device=dev).manual_seed(40960)          # the same video on every rank
            pxl = torch.randint(0, 256, (1, TL, 3, c["image"], c["image"]), generator=gl, device=dev, dtype=torch.uint8)

            def long_step():
                f = scorer.encode(pxl, shard_frames=True)
                sc, _ = scorer.score(f, txt[:1])
                out["idx_long"] = ops.topk_sorted(sc, k)

            nl = max(2, a.steps // 2)
            lsec = timed(long_step, nl, 1)
            long_form = {"frames_scored_per_s": round(TL * nl / lsec, 2), "ms_per_video": round(lsec / nl * 1e3, 3), "frames_per_video": TL,
                         "frames_per_gpu": -(-TL // world), "steps": nl, "scaling": "strong",
                         "workload": workload_name(TL, 1, k, world, True)}
            del pxl
        except Exception as e:
            long_form = {"error": f"{type(e).__name__}: {e}"[:300]}

    # ---- split: score + select only (features resident), SURVEY 8(d) ----------
    split = None
    if a.full:
        feats_res = scorer.encode(pixels, shard_frames=shard)

        def select_step():
            sc, _ = scorer.score(feats_res, txt)
            out["idx2"] = ops.topk_sorted(sc, k)

        sel_sec = timed(select_step, max(a.steps, 200), 3) / max(a.steps, 200)
        assert torch.equal(out["idx2"], out["idx"])
        # the same stage at the reference's own inference precision (gen_id_tspo.py:55 loads the scoring head in bf16): bf16 GEMM
        # operands, fp32 accumulation (TSPO_SEL_BF16) - opt-in, NOT used for `value`; how many of the fp32 path's k indices it keeps
        scorer.selector_precision = "bf16"
        sel16_sec = timed(select_step, max(a.steps, 200), 3) / max(a.steps, 200)
        keep16 = sum(len(set(x) & set(y)) for x, y in zip(out["idx2"].tolist(), out["idx"].tolist())) / max(1, out["idx"].numel())
        scorer.selector_precision = "fp32"
        split = {"encode": round(sec / a.steps * 1e3 - sel_sec * 1e3, 3), "score_select": round(sel_sec * 1e3, 3),
                 "score_select_bf16_operands": round(sel16_sec * 1e3, 3), "bf16_keeps_fraction_of_fp32_topk": round(keep16, 4),
                 "note": "score_select = clip cosine + scoring head + top-k on resident features, exact fp32 (used for `value`); "
                         "_bf16_operands = the same with FrameScorer(selector_precision='bf16'), the reference's inference precision"}

    # ---- rollouts / s (policy side of one TSPO step, configs[2]) --------------
    rollouts = rollouts_x3 = dp_path = None
    if not a.no_rollouts:
        Bt, Tt, G, kt = (int(v) for v in a.rollout_cfg.split(","))
        tau = 0.025
        gen = torch.Generator(device=dev).manual_seed(99 + rank)
        feats = torch.randn(Bt, Tt, 768, generator=gen, device=dev)
        ttxt = torch.randn(Bt, 1, 768, generator=gen, device=dev)
        clip = ops.clip_scores(ttxt, feats)
        rew = (torch.rand(Bt, G, generator=gen, device=dev) > 0.5).float() + torch.rand(Bt, G, generator=gen, device=dev)
        trainer = PolicyTrainer(flat.clone())
        rsec = timed(lambda: trainer.step(feats, ttxt, clip, lambda idx: rew, G, kt, tau), max(a.steps, 200), 3)
        rollouts = Bt * G * world * max(a.steps, 200) / rsec
        n_launch, by_kernel = (None, "counted on rank 0 only") if (rank or world > 1) else count_kernel_launches(
            lambda: trainer.step(feats, ttxt, clip, lambda idx: rew, G, kt, tau))
        # opt-in split-precision selector GEMMs (NOT the headline number): see DESIGN.md, TSPO_SEL_BF16X3
        trainer_x3 = PolicyTrainer(flat.clone(), gemm_precision="bf16x3")
        xsec = timed(lambda: trainer_x3.step(feats, ttxt, clip, lambda idx: rew, G, kt, tau), max(a.steps, 200), 3)
        rollouts_x3 = Bt * G * world * max(a.steps, 200) / xsec

    # ---- N = 1: the one-rank RCCL group lives from here: comm probe + the rollout figure of the reference's own configuration ----
    own_group = False
    try:
        if world == 1 and not a.no_comm_probe:
            one_rank_group(a.backend, dev)
            own_group = True
            comm = comm_probe(a.backend, world, dev, ops.trainable_numel(768))
        if not a.no_rollouts and dist.is_initialized():
            dp_path = dp_path_rollouts(flat, dev, world, rank, (Bt, Tt, G, kt), a.steps, timed)
    except Exception as e:
        dp_path = {"error": f"{type(e).__name__}: {e}"[:300]}
    finally:
        if own_group and dist.is_initialized():
            dist.destroy_process_group()

    # ---- roofline of the dominant kernel (bf16 MFMA GEMM), live HIP-event timing --------------------------
    roof = None
    if rank == 0 and not a.no_profile:
        px = pixels.reshape(B * T, *pixels.shape[2:])
        if shard and world > 1:      # rank 0's own slice of the video: what its GEMM launches actually process
            mine = tdist.shard_rows(B * T, world, 0)
            px = px[mine.start:mine.stop]
        n_prof = px.shape[0]
        ops.clip_vit_profile(clipw, px, fold_layernorm=not a.no_ln_fold)
        pr = ops.clip_vit_profile(clipw, px, fold_layernorm=not a.no_ln_fold)
        gflop = gemm_flops_per_frame(c) * n_prof
        ach = gflop / (pr["gemm_ms"] * 1e-3) / 1e12
        # HBM-side bytes per GEMM launch cannot be read from inside the process: they come from the committed rocprofv3
        # --pmc passes (FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 x2 read correction) of THIS command
        # (tools/prof_round.sh -> tools/pmc_traffic.py); the file name says which round's kernels they were taken on.
        traffic, tsrc, forms = committed_traffic(n_prof, not a.no_ln_fold)
        roof = {"bound": "mfma", "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "traffic_source": tsrc,
                "traffic_by_form": forms, "frames_per_launch": n_prof,
                "alg_bytes_per_launch_avg": alg_bytes_per_launch(c, n_prof), "kernel": "gemm_bf16_a9_kernel",
                "launches_per_step": pr["gemm_launches"],
                "avg_launch_ms": round(pr["gemm_ms"] / pr["gemm_launches"], 4),
                "alg_flop_per_launch_avg": gflop / pr["gemm_launches"],
                "breakdown_ms": {kk: round(v, 3) for kk, v in pr.items() if kk.endswith("_ms")},
                "attn_achieved_tflops": round(attn_flops_per_frame(c) * n_prof / (pr["attn_ms"] * 1e-3) / 1e12, 1)}
        # the clock / power the chip sustained during the TIMED steps above (sampled live): the nominal peak assumes 2.4 GHz
        roof.update(sclk_mhz=gpu_state.get("sclk_mhz"), power_w=gpu_state.get("power_w"), gpu_state=gpu_state)
        if gpu_state.get("sclk_mhz"):
            peak_at_clock = PEAK_BF16_TFLOPS * gpu_state["sclk_mhz"] / 2400.0
            roof.update(peak_at_sustained_clock=round(peak_at_clock, 1), frac_at_sustained_clock=round(ach / peak_at_clock, 4))

    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        if a.cpu_threads > 0:
            torch.set_num_threads(a.cpu_threads)
        cpu = cpu_baseline(T, k)

    if rank == 0:
        line = {
            "metric": "frames_scored_per_s", "value": round(fps, 2), "unit": "frames/s", "n_gpus": world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(sec / a.steps * 1e3, 3),
            "ms_per_step_min": round(min(step_ms), 3), "ms_per_step_median": round(sorted(step_ms)[len(step_ms) // 2], 3),
            "ms_per_step_max": round(max(step_ms), 3),
            "ms_per_step_by_rank": [round(x / a.steps * 1e3, 3) for x in rank_sec],     # each rank's own clock over the timed region
            "higher_is_better": True, "scaling": "strong" if shard else "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "full": a.full,
            "config": {"workload": workload_name(T, B, k, world, shard),
                       "frames_per_video": T, "videos_per_gpu_per_step": None if shard else B, "videos_per_step_total": 1 if shard else B * world,
                       "frames_per_gpu_per_step": -(-T // world) if shard else B * T, "topk": k, "window": 12, "tau": 0.025,
                       "pixels": a.pixels, "weights": "random-init CLIP-L/14 + selector",
                       "parallelism": (f"frames of one video sharded over {world} rank(s) + all-gather" if shard else f"dp{world}"),
                       "layernorm": "stand-alone" if a.no_ln_fold else "folded into GEMMs"},
            "rollouts_per_s": None if rollouts is None else round(rollouts, 1),
            "rollouts_variant": None if rollouts is None else (
                "fused single-rank step: grad_accum 1, no process group, gradient-norm partials out of the backward (15 launches)"
                if world == 1 else f"data-parallel step on {world} ranks: grad_accum 1, one bucket all-reduce per step"),
            "rollouts_dp_path": dp_path,
            "optional_rollouts_per_s_bf16x3": None if rollouts_x3 is None else {
                "rollouts_per_s": round(rollouts_x3, 1),
                "note": "opt-in PolicyTrainer(gemm_precision='bf16x3'): selector GEMMs as hi/lo bf16 splits on the bf16 MFMA "
                        "(~1e-5 relative error vs exact fp32); not used for `rollouts_per_s`"},
            "rollouts_config": None if rollouts is None else {
                "workload": ("policy step (reward LLM excluded): " + (
                    ("configs[2] (B=4/GPU, T=512, G=8, k=16, 1 GPU)" if world == 1 else
                     f"configs[3] (B=4/GPU, T=512, G=8, k=16 on {world} GPUs: global batch {Bt * world} prompts, ONE {'RCCL' if a.backend == 'nccl' else a.backend} all-reduce of the "
                     f"11.8 MB bucket per optimizer step)") if (Bt, Tt, G, kt) == (4, 512, 8, 16) else
                    (f"configs[4] policy side (B={Bt}/GPU, T=4096, G=16, k=16 on {world} GPU(s))" if (Tt, G, kt) == (4096, 16, 16) else "custom"))),
                "B": Bt, "T": Tt, "G": G, "k": kt, "global_batch_prompts": Bt * world, "ranks": world},
            "rollouts_roofline": None if rollouts is None else policy_step_roofline(Bt, Tt, 768, Bt * G * world / rollouts, n_launch, by_kernel),
            "encode_tflops": round((gemm_flops_per_frame(c) + attn_flops_per_frame(c)) * fps / 1e12, 1),
            "optional_pruned_last_block": None if pruned_fps is None else {
                "frames_scored_per_s": round(pruned_fps, 2),
                "note": "opt-in ops.clip_vit_forward(prune_last_layer=True): last block for the class-token row only "
                        "(same features); not used for `value`"},
            "frames_scored_per_s_from_720p_u8": from_720p,
            "configs4_long_form_sharded": long_form,
            "split_ms": split,
            "roofline": roof, "cpu_baseline": cpu, "comm": comm, "dumped_outputs": dumped,
            "launcher": "torch.distributed.run" if (world > 1 and not os.environ.get("TSPO_SELF_SPAWNED")) else
                        ("self-spawn" if world > 1 else "single process"),
        }
    else:
        line = None
    # ---- N > 1 on RCCL: Ring vs Tree all-reduce on extra communicators.  LAST, and under a watchdog: if creating them hangs on this
    #      node, rank 0 still prints the measured line (every number above is already final) and all ranks leave ----
    printed = threading.Event()

    def emit():
        if rank == 0 and not printed.is_set():
            printed.set()
            try:      # librccl announces itself through C stdio ("Librccl path : ..."), which would otherwise be flushed at exit,
                import ctypes                      # AFTER the line: push it out now so the JSON line is the last line of stdout
                ctypes.CDLL(None).fflush(None)
            except Exception:
                pass
            print(json.dumps(line), flush=True)

    if world > 1 and comm is not None and "error" not in comm and a.backend == "nccl" and not a.no_comm_probe:
        def bail():
            if rank == 0 and line is not None and isinstance(line.get("comm"), dict):
                line["comm"]["allreduce_us_by_algo"] = "skipped: the extra communicators did not come up within 120 s"
            emit()
            os._exit(0)
        dist.barrier()            # (rank 0 profiled a little longer: start the clock together)
        dog = threading.Timer(120.0, bail)
        dog.daemon = True
        dog.start()
        by_algo = comm_algo_probe(dev, ops.trainable_numel(768))
        dog.cancel()
        if rank == 0:
            line["comm"]["allreduce_us_by_algo"] = by_algo
    emit()
    if world > 1:
        dist.barrier()   # rank 0 is still profiling / printing while the others are done: leave together
        dist.destroy_process_group()
    if os.environ.get("TSPO_RCCL_LOG_DIR"):      # this process's RCCL debug files (summarised into `comm` above)
        import shutil
        shutil.rmtree(os.environ["TSPO_RCCL_LOG_DIR"], ignore_errors=True)
    if world > 1:
        # every number is printed and the process group is destroyed: leave WITHOUT running the interpreter's / the collective
        # libraries' static destructors - with several ranks (and, in dry runs, several ranks on ONE device) their order against the
        # HIP runtime's own teardown is not defined, and a crash there would turn a finished measurement into a failed launch
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
