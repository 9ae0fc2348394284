"""GPU tests of the indexed, normalising preprocessing (tspo_preprocess_select / preprocess.select_frames) and of the training
step driven from frames (train.FrameDataset, Batch.selected_frames).

Float outputs - the bounds are derived, not measured.  eps = 2^-24 (half an ulp of fp32, relative).  With u the Pillow-exact byte
(0..255), r = rescale, m = mean[c], s = std[c] and a = r / s, b = -m / s:

  kernel      out = fma(u, fl(a), fl(b)): the two constants are rounded once each (|fl(a) - a| <= eps |a|, |fl(b) - b| <= eps |b|),
              the product u * fl(a) is exact inside the fma, which rounds once:
                  |out - (u a + b)| <= eps (u |a| + |b|) + eps |u a + b|  =: E(u, c)          (+ second-order terms)
  HF / SigLIP chain in float32 (transformers.image_transforms.rescale: float64 product rounded to float32; normalize: float32
              (x - fl(m)) / fl(s), two roundings): x = u r (1 + d1), fl(m) = m (1 + d2), fl(s) = s (1 + d3), the subtraction and
              the division round once each (d4, d5), all |d| <= eps:
                  |ref - (u r - m) / s| <= eps ((u r + |m|) + 3 |u r - m|) / |s|  =: E_ref(u, c)  (+ second-order terms)
Second-order terms (eps^2) and the 2^-53 roundings of the float64 evaluations are covered by a factor (1 + 2^-20) on both."""
import json
import os

import numpy as np
import pytest
import torch

from tspo_amd import haystack, ops, preprocess as P, synth
from tspo_amd.pipeline import PolicyTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
S384 = dict(size=(384, 384), mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))


def _spec(kind, dtype):
    return P.PreprocessSpec.clip_default(out_dtype=dtype) if kind == "clip" else P.PreprocessSpec(out_dtype=dtype, **S384)


def pil_u8(frame_hwc: np.ndarray, spec) -> np.ndarray:
    """One uint8 frame [H,W,3] through PIL the way the processors do it: resize, then the centre window -> [3,h,w]."""
    from PIL import Image
    H, W = frame_hwc.shape[:2]
    new_h, new_w, top, left, oh, ow = P.spec_resize_geometry(H, W, spec)
    img = np.array(Image.fromarray(frame_hwc).resize((new_w, new_h), resample=Image.BICUBIC))
    return np.ascontiguousarray(img[top:top + oh, left:left + ow].transpose(2, 0, 1))


def _index_cases(Pn):
    g = np.random.RandomState(Pn)
    return {"repeats": [1, 1, 0, Pn - 1, 1], "descending": list(range(Pn - 1, -1, -1)), "one": [Pn // 2],
            "more_than_pool": g.randint(0, Pn, size=2 * Pn + 3).tolist()}


@pytest.mark.parametrize("path", ["matrix", "lds"])
@pytest.mark.parametrize("kind", ["clip", "384"])
@pytest.mark.parametrize("hw", [(720, 1280), (240, 320), (333, 517)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_select_u8_bit_exact(hw, kind, path, monkeypatch):
    monkeypatch.setattr(P, "USE_MATRIX_PASS", path == "matrix")
    H, W = hw
    Pn = 4
    frames = synth.uniform_u8((Pn, H, W, 3), 11 + H + W)
    spec = _spec(kind, torch.uint8)
    ref = np.stack([pil_u8(f, spec) for f in frames])
    pools = {"THWC": torch.from_numpy(frames).to(DEV),
             "TCHW": torch.from_numpy(np.ascontiguousarray(frames.transpose(0, 3, 1, 2))).to(DEV)}
    for lname, pool in pools.items():
        for cname, ix in _index_cases(Pn).items():
            got = P.select_frames(pool, torch.tensor(ix, device=DEV), spec)
            assert got.dtype == torch.uint8 and got.shape == (len(ix), 3) + spec.out_hw
            np.testing.assert_array_equal(got.cpu().numpy(), ref[ix], err_msg=f"{lname} {cname}")
        whole = P.select_frames(pool, None, spec)
        np.testing.assert_array_equal(whole.cpu().numpy(), ref, err_msg=lname)
        if kind == "clip":
            assert torch.equal(whole, P.preprocess_frames(pool))
    # an index of any shape comes back in that shape
    ix = torch.tensor([[[0, 1], [3, 3]], [[2, 0], [1, 2]]], device=DEV)
    got = P.select_frames(pools["THWC"], ix, spec)
    assert got.shape == (2, 2, 2, 3) + spec.out_hw
    np.testing.assert_array_equal(got.cpu().numpy(), ref[ix.cpu().numpy()])


def test_select_plain_scalar_form_and_rectangular_output():
    """out_w % 4 != 0 takes the byte-granular kernels; out_h != out_w; every output type through their epilogue."""
    frames = synth.uniform_u8((3, 97, 131, 3), 5)
    pool = torch.from_numpy(frames).to(DEV)
    ix = torch.tensor([2, 0, 2, 1], device=DEV)
    su8 = P.PreprocessSpec(size=(98, 222), out_dtype=torch.uint8, mean=(0.5, 0.4, 0.3), std=(0.5, 0.25, 0.2))
    ref = np.stack([pil_u8(f, su8) for f in frames])[ix.cpu().numpy()]
    u = P.select_frames(pool, ix, su8)
    np.testing.assert_array_equal(u.cpu().numpy(), ref)
    f32 = P.select_frames(pool, ix, su8.with_dtype(torch.float32))
    _assert_float_bound(f32, u, su8)
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(P.select_frames(pool, ix, su8.with_dtype(dt)), f32.to(dt))


def test_select_out_of_range_index_is_clamped_and_flagged():
    """Documented behaviour: a value outside [0, P) reads the nearest valid frame and raises the caller's flag word."""
    frames = synth.uniform_u8((3, 64, 80, 3), 8)
    pool = torch.from_numpy(frames).to(DEV)
    spec = P.PreprocessSpec(size=(32, 48), out_dtype=torch.uint8)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = P.select_frames(pool, torch.tensor([0, 2, 1], device=DEV), spec, oob_flag=flag)
    assert int(flag.item()) == 0
    got = P.select_frames(pool, torch.tensor([-3, 1, 3 + 5, 2 ** 40], device=DEV), spec, oob_flag=flag)
    assert int(flag.item()) == 1
    assert torch.equal(got, ok[[0, 2, 1, 1]])


def _bounds(spec):
    """E and E_ref of the module docstring as float64 tables [256, 3] and the exact value (u r - m) / s in float64."""
    u = np.arange(256, dtype=np.float64)[:, None]
    r, m, s = float(spec.rescale), np.array(spec.mean, np.float64)[None], np.array(spec.std, np.float64)[None]
    a, b = r / s, -m / s
    exact = (u * r - m) / s
    E = EPS * (u * np.abs(a) + np.abs(b) + np.abs(u * a + b)) * SLACK
    E_ref = EPS * ((u * r + np.abs(m)) + 3 * np.abs(u * r - m)) / np.abs(s) * SLACK
    return exact, E, E_ref


def _lookup(table, u8):
    """table [256,3] at every element of u8 [..., 3, h, w] (channel axis -3)."""
    u = u8.cpu().numpy().astype(np.int64)
    c = np.arange(3).reshape((1,) * (u.ndim - 3) + (3, 1, 1))
    return table[u, np.broadcast_to(c, u.shape)]


def _assert_float_bound(f32, u8, spec):
    exact, E, _ = _bounds(spec)
    assert f32.dtype == torch.float32 and f32.shape == u8.shape
    err = np.abs(f32.cpu().numpy().astype(np.float64) - _lookup(exact, u8))
    bound = _lookup(E, u8)
    print(f"fp32 vs float64: max err {err.max():.3e}, max err/E {np.max(err / bound):.3f}")
    assert np.all(err <= bound)                     # every element


@pytest.mark.parametrize("kind", ["clip", "384"])
@pytest.mark.parametrize("hw", [(720, 1280), (240, 320)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_select_float_outputs_within_derived_bound(hw, kind):
    from PIL import Image
    H, W = hw
    frames = synth.uniform_u8((3, H, W, 3), 21 + H).copy()
    frames[0, : H // 2] = 0                          # the ends of the byte range occur
    frames[0, H // 2:] = 255
    pool = torch.from_numpy(frames).to(DEV)
    ix = torch.tensor([2, 0, 1, 0], device=DEV)
    spec = _spec(kind, torch.float32)
    u8 = P.select_frames(pool, ix, spec.with_dtype(torch.uint8))
    np.testing.assert_array_equal(u8.cpu().numpy(), np.stack([pil_u8(frames[i], spec) for i in ix.tolist()]))
    f32 = P.select_frames(pool, ix, spec)
    _assert_float_bound(f32, u8, spec)
    for dt in (torch.bfloat16, torch.float16):
        out = P.select_frames(pool, ix, spec.with_dtype(dt))
        assert out.dtype == dt and torch.equal(out, f32.to(dt))           # bitwise: one further rounding to nearest even
    # against the installed processor itself, on the CPU in float32
    sel = [frames[i] for i in ix.tolist()]
    if kind == "clip":
        from transformers import CLIPImageProcessor
        ip = CLIPImageProcessor()
        assert P.PreprocessSpec.from_image_processor(ip) == spec
        ref = ip(images=[Image.fromarray(f) for f in sel], return_tensors="pt")["pixel_values"].numpy()
    else:
        from functools import partial, reduce
        from transformers.image_transforms import normalize, rescale, resize
        from transformers.image_utils import ChannelDimension, PILImageResampling
        df = ChannelDimension.FIRST                  # the chain of siglip_encoder.py:56-61 (frames are RGB arrays already)
        chain = [partial(resize, size=spec.size, resample=PILImageResampling.BICUBIC, data_format=df),
                 partial(rescale, scale=spec.rescale, data_format=df),
                 partial(normalize, mean=spec.mean, std=spec.std, data_format=df)]
        ref = np.stack(reduce(lambda x, f: [*map(f, x)], chain, sel))
    assert ref.dtype == np.float32 and ref.shape == tuple(f32.shape)
    _, E, E_ref = _bounds(spec)
    err = np.abs(f32.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
    bound = _lookup(E + E_ref, u8)
    print(f"fp32 vs installed processor: max err {err.max():.3e}, max err/(E+E_ref) {np.max(err / bound):.3f}")
    assert np.all(err <= bound)                     # every element


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver

def _tiny_model(seed=0):
    from test_gpu_flow import _tiny_model as tm
    return tm(seed)


def _videos():
    """Three small in-memory videos: two longer than a true clip (different sizes do not matter: one geometry per video), one
    shorter (the "whole video" branch: clips of 30 frames)."""
    return {"a.npy": synth.uniform_u8((64, 48, 64, 3), 1), "b.npy": synth.uniform_u8((30, 48, 64, 3), 2),
            "c.npy": synth.uniform_u8((70, 60, 40, 3), 3)}


ITEMS = [{"video": "a.npy", "original_question": "<image>\nWhere is the cat?\nA. left\nB. right", "type": "specific"},
         {"video": "b.npy", "original_question": "<image>\nWhat happens?\n(A) x\n(B) y", "type": "specific"},
         {"video": "c.npy", "original_question": "<image>\nWhat is the video about?\nA. x\nB. y", "type": "general"}]


def _dataset(model, seed=4, items=None):
    from test_gpu_api import _StubProcessor
    from tspo_amd import train as tt
    vids = _videos()
    reads = []

    def load_video(path, max_frames_num, fps, force_sample):
        assert (max_frames_num, fps, force_sample) == (128, 1, False)          # tspo_trainer.py:456-457
        reads.append(os.path.basename(path))
        return vids[os.path.basename(path)], None, None, None

    ds = tt.FrameDataset(items or ITEMS, model, _StubProcessor(), load_video=load_video, seed=seed, device=DEV, record=True)
    ds.reads = reads
    return ds


def test_batch_selected_frames_composition_without_host_copy():
    """`Batch.selected_frames(idx, spec)` with idx from a real rollout == select_frames on the materialised haystack pool[plan],
    bitwise.  No device-to-host copy of idx and no synchronisation: asserted with torch.cuda.set_sync_debug_mode("error") around
    the call (the tap tables of the geometry are uploaded by a first call outside the guarded region - a one-off per geometry)."""
    model = _tiny_model(5).to(DEV)
    ds = _dataset(model)
    batch = ds.prepare(0)
    pool, plan = batch.frames[0]
    T = plan.numel()
    assert batch.feats.shape == (1, T, 768) and T % 50 == 0 and 650 <= T <= 800
    G, k = 4, 8
    tr = PolicyTrainer(model.selector.flatten_parameters(), dim=768, heads=8, window_size=12)
    scores, idx, logp, ctx = tr.rollout(batch.feats, batch.txt, batch.clip, G, k, 0.025)
    assert idx.shape == (1, G, k) and idx.is_cuda
    spec = P.PreprocessSpec(out_dtype=torch.bfloat16, **S384)
    P.select_frames(pool, plan[:2], spec)                                       # uploads the tables of this geometry
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = batch.selected_frames(idx, spec)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    hay = pool[plan]                                                            # the materialised haystack
    want = P.select_frames(hay, idx[0], spec)
    assert got.shape == (1, G, k, 3, 384, 384) and got.dtype == torch.bfloat16
    assert torch.equal(got[0], want)
    with pytest.raises(ValueError):
        from tspo_amd.train import Batch
        Batch(batch.feats, batch.txt, batch.clip, batch.mask).selected_frames(idx, spec)


def test_training_step_from_frames(tmp_path):
    from tspo_amd import train as tt
    from tspo_amd.temporal_agent import _image_features
    model = _tiny_model(6).to(DEV)
    kw = dict(num_generations=4, training_sample_len=8, gradient_accumulation_steps=2, save_steps=100, dim=768, heads=8, seed=3)
    spec = P.PreprocessSpec(size=(40, 56), out_dtype=torch.uint8)
    seen = []

    def reward(idx, batch):
        """Checks what a video-LLM plug-in would see, then the default mask rewards."""
        got = batch.selected_frames(idx, spec)
        for b, (pool, plan) in enumerate(batch.frames):
            src = plan.cpu()[idx[b].cpu()]                                      # [G,k] pool frame numbers
            pool_c = pool.cpu().numpy()
            want = np.stack([[pil_u8(pool_c[int(j)], spec) for j in row] for row in src])
            np.testing.assert_array_equal(got[b].cpu().numpy(), want)           # (a)
            L = batch.meta[b]["n_video_frames"]
            assert torch.equal(batch.mask[b][idx[b]].cpu(), src < L)            # (b) relevant <=> from the question's video
            direct = _image_features(model, P.preprocess_frames(pool[plan]))
            assert torch.equal(batch.feats[b], direct)                          # (c)
            seen.append((batch.meta[b]["item"], batch.item_type, idx.shape[-1], int(plan.numel()), bool(batch.mask[b].all())))
        return tt.mask_reward_model(idx, batch)

    flat0 = model.selector.flatten_parameters().clone()
    ds = _dataset(model)
    cfg = tt.TrainConfig(output_dir=str(tmp_path / "a"), max_steps=3, **kw)
    ma = tt.train(cfg, ds, reward_model=reward, flat=flat0.clone(), resume=False)
    assert [s[0] for s in seen] == [0, 1, 2, 3, 4, 5] and ds.reads == ["a.npy", "b.npy", "c.npy"] * 2
    for item, typ, k, T, all_true in seen:
        if item % 3 == 2:
            assert typ == "general" and k == 4 and T == 70 and all_true         # k // 2, the video as it is, all-true mask
        else:
            glen = 50 if item % 3 == 0 else 30
            assert typ == "specific" and k == 8 and T % glen == 0 and 13 <= T // glen <= 16 and not all_true
    assert len({s[3] for s in seen[:2]}) == 2                                   # the first window holds two different T

    # two micro-steps of different T run sequentially == two accumulation steps by hand, bitwise
    ds1 = _dataset(model)
    cfg1 = tt.TrainConfig(output_dir=str(tmp_path / "one"), max_steps=1, **kw)
    m1 = tt.train(cfg1, ds1, flat=flat0.clone(), resume=False)
    from tspo_amd.pipeline import annealed_tau, linear_decay_lr
    from tspo_amd import rewards
    tr = PolicyTrainer(flat0.clone(), dim=768, heads=8, window_size=12, lr=cfg1.learning_rate, max_grad_norm=cfg1.max_grad_norm,
                       seed=cfg1.seed, grad_accum_steps=2, lr_schedule=linear_decay_lr(cfg1.learning_rate, 1),
                       gemm_precision=cfg1.gemm_precision)
    dsh = _dataset(model)
    for gi in (0, 1):
        b = dsh.prepare(gi)
        k = rewards.training_sample_len(8, b.item_type)
        scores, idx, logp, ctx = tr.rollout(b.feats, b.txt, b.clip, 4, k, annealed_tau(cfg1.score_tau, 0, 1), micro_steps=1)
        rpf = tt.mask_reward_model(idx, b)
        rew = rewards.combine_rewards(rpf.reshape(4, 2), b.item_type).reshape(1, 4)
        tr.backward(ctx, b.feats, b.txt, logp, idx, rew)
    tr.optimizer_step()
    assert torch.equal(tr.flat, m1["flat"]) and not torch.equal(tr.flat, flat0)

    # stop + resume: the haystack plans and the final weights of the straight run
    dsb = _dataset(model)
    cfgb = tt.TrainConfig(output_dir=str(tmp_path / "b"), max_steps=3, **dict(kw, save_steps=1))
    tt.train(cfgb, dsb, flat=flat0.clone(), resume=False, stop_after=2)
    n_before = len(dsb.history)
    mb = tt.train(cfgb, dsb, flat=flat0.clone(), resume=True)
    assert n_before == 4 and [h[0] for h in dsb.history] == [0, 1, 2, 3, 4, 5]  # nothing re-read for the skipped items
    for (ga, pa, ka), (gb, pb, kb) in zip(ds.history, dsb.history):
        assert ga == gb and torch.equal(pa, pb) and torch.equal(ka, kb)
    assert torch.equal(mb["flat"], ma["flat"])
    lines = [json.loads(l) for l in open(os.path.join(cfg.output_dir, "metrics.jsonl"))]
    assert [l["step"] for l in lines] == [1, 2, 3]


def test_frame_dataset_ranks_see_disjoint_items():
    model = _tiny_model(7).to(DEV)
    ds = _dataset(model)
    it0, it1 = ds.batches(0, 2, 1), ds.batches(1, 2, 1, skip=1)
    a, b = next(it0), next(it1)
    assert a.meta[0]["item"] == 0 and b.meta[0]["item"] == 3 and ds.reads == ["a.npy", "a.npy"]
    # item 3 is item 0's video again under another seed: another haystack
    p0, p1 = ds.history[0][1], ds.history[1][1]
    assert a.meta[0]["video"] == b.meta[0]["video"] and not (p0.shape == p1.shape and torch.equal(p0, p1))


def test_stacked_window_carries_frames():
    """Two micro-batches of equal T ("general" items keep their video: same length, same k) stack into ONE batch
    (train._stackable / _stack): `frames` travels along, and `selected_frames` on the stacked batch is the per-batch result."""
    from tspo_amd import train as tt
    model = _tiny_model(8).to(DEV)
    items = [dict(ITEMS[2]), dict(ITEMS[2], original_question="<image>\nWho speaks first?\n(A) x\n(B) y")]
    ds = _dataset(model, items=items)
    window = [ds.prepare(0), ds.prepare(1)]
    assert tt._stackable(window)
    st = tt._stack(window)
    assert st.feats.shape == (2, 70, 768) and len(st.frames) == 2 and st.frames[1][0] is window[1].frames[0][0]
    assert [m["item"] for m in st.meta] == [0, 1]
    tr = PolicyTrainer(model.selector.flatten_parameters(), dim=768, heads=8, window_size=12, grad_accum_steps=2)
    scores, idx, logp, ctx = tr.rollout(st.feats, st.txt, st.clip, 4, 4, 0.025, micro_steps=2)
    spec = P.PreprocessSpec(size=(40, 56), out_dtype=torch.float16)
    got = st.selected_frames(idx, spec)
    assert got.shape == (2, 4, 4, 3, 40, 56)
    for b in range(2):
        assert torch.equal(got[b:b + 1], window[b].selected_frames(idx[b:b + 1], spec))
    # a window in which only one batch has frames still stacks; selected_frames then refuses
    bare = tt.Batch(window[1].feats, window[1].txt, window[1].clip, window[1].mask, "general")
    mixed = tt._stack([window[0], bare])
    assert mixed.frames[0] is not None and mixed.frames[1] is None
    with pytest.raises(ValueError):
        mixed.selected_frames(idx, spec)
    # and the driver takes the stacked path for such a window: one reward call with B = 2
    calls = []

    def reward(idx, batch):
        calls.append((tuple(idx.shape), len(batch.frames)))
        assert batch.selected_frames(idx, spec).shape[:3] == idx.shape
        return tt.mask_reward_model(idx, batch)

    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cfg = tt.TrainConfig(output_dir=d, max_steps=1, num_generations=4, training_sample_len=8, gradient_accumulation_steps=2,
                             save_steps=100, dim=768, heads=8, seed=3)
        tt.train(cfg, _dataset(model, items=items), reward_model=reward, flat=model.selector.flatten_parameters().clone(), resume=False)
    assert calls == [((2, 4, 4), 2)]


def _write_frame_dir(root):
    """<root>/items.json (+ pre-tokenised problem text: no tokenizer files offline), .npy videos, <root>/model (tiny TSPOModel)."""
    os.makedirs(root, exist_ok=True)
    for name, arr in _videos().items():
        np.save(os.path.join(root, name), arr)
    ids = [49406, 320, 1125, 539, 320, 2368, 49407]
    items = [dict(it, input_ids=ids[:-1] + [1000 + i, ids[-1]]) for i, it in enumerate(ITEMS)]
    json.dump(items, open(os.path.join(root, "items.json"), "w"))
    _tiny_model(9).save_pretrained(os.path.join(root, "model"))
    return items


def _run_cli(args, timeout=600):
    import subprocess
    import sys
    from test_gpu_multi import ROOT, _clean_env, _json_lines, _ok
    r = subprocess.run([sys.executable, "-m", "tspo_amd.train"] + args, env=_clean_env(), cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    _ok(r, "train_cli_frame_dir")
    return _json_lines(r.stdout)


def test_train_cli_frame_dir_one_rank_and_two_ranks(tmp_path):
    """`python -m tspo_amd.train --frame-dir <tmp>` for 2 optimizer steps: as one rank, and as two ranks on the one GPU (the
    driver's own launcher, gloo, a fresh child process per rank): replicas bit-identical, disjoint items per rank."""
    root = str(tmp_path / "frames")
    _write_frame_dir(root)
    common = ["--frame-dir", root, "--num-generations", "4", "--training-sample-len", "8", "--max-steps", "2", "--save-steps", "1",
              "--seed", "5"]
    one = str(tmp_path / "one")
    lines = _run_cli(common + ["--output-dir", one])
    assert [l["step"] for l in lines] == [1, 2] and all(np.isfinite(l["loss"]) and np.isfinite(l["grad_norm"]) for l in lines)
    rec = json.load(open(os.path.join(one, "frames.rank0.json")))
    assert [i for i, _ in rec["items"]] == [0, 1, 2, 3] and rec["items"][2][1] == 70          # item 2 is the "general" video
    assert os.path.exists(os.path.join(one, "checkpoint-2", "model.safetensors"))
    two = str(tmp_path / "two")
    lines = _run_cli(common + ["--output-dir", two, "--gpus", "2", "--backend", "gloo"])
    assert [l["step"] for l in lines] == [1, 2]                                               # rank 0 alone prints
    r0, r1 = (json.load(open(os.path.join(two, f"frames.rank{r}.json"))) for r in (0, 1))
    assert [i for i, _ in r0["items"]] == [0, 2, 4, 6] and [i for i, _ in r1["items"]] == [1, 3, 5, 7]    # disjoint
    assert r0["flat_sha256"] == r1["flat_sha256"] and r0["flat_sha256"] != rec["flat_sha256"]  # replicas bit-identical
    from tspo_amd import io as tio
    ck = tio.load_selector_safetensors(os.path.join(two, "checkpoint-2", "model.safetensors"))
    ck1 = tio.load_selector_safetensors(os.path.join(two, "checkpoint-1", "model.safetensors"))
    assert any(not torch.equal(ck[k], ck1[k]) for k in ck)                                     # the run moved the parameters
