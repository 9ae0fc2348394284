"""The chunked / streamed encode on the GPU: tspo_clip_vit_forward_chunked against direct per-chunk calls and against the one-call
encode (bitwise), sampled frames against the CPU oracle, the workspace bound, the streamed host-frames front end against the
device-resident path (bitwise), and the `encode_chunk_frames` knob of TSPOModel / FrameScorer / FrameIdGenerator.

CLIP-L/14 geometry with 2 layers (the fold threshold, the GEMM kernels and their tile phases are those of the full model; the
depth only repeats them).  T = 200 at chunk 128 plans [128, 72]: two folding chunks, the second not a multiple of 64 frames.
T = 256 at chunk 128 plans [128, 128]: whole 64-frame blocks, the case that equals the one-call encode bit for bit."""
import pytest
import torch

import bench
from oracle import tspo_oracle as O
from tspo_amd import _lib, ops, synth
from tspo_amd.pipeline import FrameScorer
from tspo_amd.preprocess import PreprocessSpec, encode_frames_streamed, select_frames

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(bench.CLIP_L14, layers=2)
U8_SPEC = PreprocessSpec.clip_default(224, torch.uint8)


@pytest.fixture(scope="module")
def state():
    return bench.random_clip_state(CFG, DEV)


@pytest.fixture(scope="module")
def px():
    gen = torch.Generator(device=DEV).manual_seed(4321)
    return torch.randint(0, 256, (256, 3, 224, 224), generator=gen, device=DEV, dtype=torch.uint8)


@pytest.fixture(scope="module")
def chunked200(state, px):
    """features of px[:200] at chunk 128, computed once on a fresh ClipVitWeights (shared, never written to)."""
    w = ops.ClipVitWeights(state, CFG, DEV)
    return w, ops.clip_vit_forward_chunked(w, px[:200], 128).clone()


@pytest.fixture(scope="module")
def host_frames():
    return synth.uniform_u8((200, 90, 160, 3), 99)


def test_chunked_equals_direct_calls_on_the_plan_slices_bitwise(state, px, chunked200):
    w, got = chunked200
    plan = ops.clip_chunk_plan(w, 200, 128)
    assert plan == [128, 72] and all(w.library_folds(n) for n in plan)
    direct_w = ops.ClipVitWeights(state, CFG, DEV)
    direct = torch.cat([ops.clip_vit_forward(direct_w, px[lo:lo + n]).clone() for lo, n in ((0, 128), (128, 72))])
    assert got.shape == (200, 768) and got.dtype == torch.float32
    assert torch.equal(got, direct)
    assert w._fold_key is not None                                  # the second run takes the cached-fold path (no fold launches)
    again = ops.clip_vit_forward_chunked(w, px[:200], 128)
    assert torch.equal(again, got)
    out = torch.full((200, 768), float("nan"), device=DEV)
    assert ops.clip_vit_forward_chunked(w, px[:200], 128, out=out) is out and torch.equal(out, got)
    assert torch.equal(ops.clip_vit_forward_chunked(w, px[:200], 256), ops.clip_vit_forward(direct_w, px[:200]))   # one chunk = one call


def test_chunks_of_whole_64_frame_blocks_equal_one_call_bitwise(state, px):
    w = ops.ClipVitWeights(state, CFG, DEV)
    assert ops.clip_chunk_plan(w, 256, 128) == [128, 128]
    got = ops.clip_vit_forward_chunked(w, px, 128).clone()
    one = ops.clip_vit_forward(ops.ClipVitWeights(state, CFG, DEV), px)
    assert torch.equal(got, one)


def test_sampled_frames_against_the_oracle(state, px, chunked200):
    """First and last frame of each chunk of [128, 72] and one inside each; tolerance of test_long_video_encode_T4096."""
    _, got = chunked200
    sub = torch.tensor([0, 64, 127, 128, 150, 199], device=DEV)
    wq = {k: (v.float().cpu().to(torch.bfloat16).float() if v.ndim >= 2 and "position_embedding" not in k else v.float().cpu())
          for k, v in state.items()}
    with torch.no_grad():
        ref = O.clip_vit_forward(wq, O.clip_normalize_pixels(px[sub].cpu()), num_heads=CFG["heads"], patch=CFG["patch"])
    g = got[sub].cpu()
    err = (g - ref).abs().max().item() / ref.abs().max().item()
    cos = torch.nn.functional.cosine_similarity(g, ref, dim=-1).min().item()
    print(f"\n[chunked encode] sampled frames vs oracle: max|err|/max|ref| {err:.4f}, min cos {cos:.6f}")
    assert err < 3e-2 and cos > 0.999


def test_workspace_is_sized_by_the_largest_chunk(state, px):
    w = ops.ClipVitWeights(state, CFG, DEV)
    ops.clip_vit_forward_chunked(w, px[:200], 128)
    cfg = ops._clip_cfg_struct(CFG)
    import ctypes as C
    n128 = _lib.lib().tspo_clip_workspace_bytes(C.byref(cfg), 128)
    assert w._ws.numel() == n128
    assert n128 < _lib.lib().tspo_clip_workspace_bytes(C.byref(cfg), 200)


def test_streamed_host_frames_equal_the_resident_path_bitwise(state, host_frames):
    w = ops.ClipVitWeights(state, CFG, DEV)
    dev_frames = torch.from_numpy(host_frames).to(DEV)
    ref = ops.clip_vit_forward_chunked(ops.ClipVitWeights(state, CFG, DEV), select_frames(dev_frames, None, U8_SPEC), 128).clone()
    got = encode_frames_streamed(w, host_frames, 128)                                  # pageable numpy [T,H,W,3]
    assert got.shape == (200, 768) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got, ref)
    assert torch.equal(encode_frames_streamed(w, host_frames, 128), ref)               # buffers, events and the fold are reused
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                      # under a non-default current stream
        got_s = encode_frames_streamed(w, host_frames, 128)
    side.synchronize()
    assert torch.equal(got_s, ref)
    torch.cuda.current_stream().wait_stream(side)
    chw = torch.from_numpy(host_frames).permute(0, 3, 1, 2).contiguous()               # a CPU torch tensor, [T,3,H,W]
    ref_chw = ops.clip_vit_forward_chunked(ops.ClipVitWeights(state, CFG, DEV), select_frames(chw.to(DEV), None, U8_SPEC), 128)
    got_chw = encode_frames_streamed(w, chw, 128)
    assert torch.equal(got_chw, ref_chw) and torch.equal(got_chw, ref)
    assert torch.equal(encode_frames_streamed(w, torch.from_numpy(host_frames), 128), ref)     # a CPU torch tensor, [T,H,W,3]
    assert torch.equal(encode_frames_streamed(w, dev_frames, 128), ref)                # frames already on the device: same loop
    out = torch.empty((200, 768), device=DEV)
    assert encode_frames_streamed(w, host_frames, 128, out=out) is out and torch.equal(out, ref)
    assert isinstance(w._streamed.stream, torch.cuda.Stream)                           # ONE side stream, kept with the weights
    with pytest.raises(ValueError, match="below the 64 frames"):
        encode_frames_streamed(w, host_frames, 32)


class _StubProcessor:
    """CLIPProcessor stand-in (tokenizer files are not available offline): text -> fixed token ids, images -> the real
    CLIPImageProcessor; `image_processor` enables the on-device preprocessing path, as with CLIPProcessor."""

    def __init__(self):
        from transformers import CLIPImageProcessor
        self.ip = CLIPImageProcessor()
        self.image_processor = self.ip

    def __call__(self, text=None, images=None, return_tensors="pt", **kw):
        from transformers import BatchEncoding, BatchFeature
        if text is not None:
            ids = torch.tensor([[49406, 320, 1125, 539, 320, 2368, 49407]])
            return BatchEncoding({"input_ids": ids, "attention_mask": torch.ones_like(ids)})
        return BatchFeature(self.ip(images=images, return_tensors="pt"))


def _tspo_model(vision):
    from transformers import CLIPConfig
    from tspo_amd.temporal_agent import TSPOModel
    cfg = CLIPConfig(text_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      vocab_size=49408, max_position_embeddings=77, projection_dim=768),
                     vision_config=dict(vision, projection_dim=768), projection_dim=768)
    torch.manual_seed(0)
    model = TSPOModel(cfg).float().eval()
    for p in model.vision_model.parameters():          # default init is tiny; make the tower non-trivial
        if p.ndim >= 2:
            torch.nn.init.normal_(p, std=0.02)
    model.selector.load_state_dict({k: torch.from_numpy(v) for k, v in synth.selector_state(768, seed=2, std=0.02).items()})
    return model.to(DEV)


def test_tspo_model_knob_on_preprocessed_pixels():
    """A tower of synth.CLIP_TINY's size class (2 layers, 28 x 28 images, 5 tokens; hidden 192 = 3 heads of the head_dim 64 the
    kernels need, mlp 64 - the `c192` geometry of tests/test_gpu_encoder_stages.py).  Like CLIP_TINY it never folds, so any
    chunk size is accepted: encode_chunk_frames = None is the call of today, an int is the chunked op - [64, 64, 22] frames for
    T = 150 at 64."""
    from tspo_amd import temporal_agent as TA
    model = _tspo_model(dict(hidden_size=192, intermediate_size=64, num_hidden_layers=2, num_attention_heads=3, image_size=28,
                             patch_size=14))
    u8 = torch.from_numpy(synth.uniform_u8((150, 3, 28, 28), 5)).to(DEV)
    txt = torch.from_numpy(synth.normal((1, 768), 6)).to(DEV)
    assert model.encode_chunk_frames is None
    f0, t0, c0 = model.extract_feature_from_pixels(u8, txt)
    w = TA._packed_clip(model)
    assert torch.equal(f0, ops.clip_vit_forward(w, u8)) and t0 is txt
    assert torch.equal(c0, ops.clip_scores(txt[:1].unsqueeze(0), f0.unsqueeze(0))[0])
    model.encode_chunk_frames = 64
    assert ops.clip_chunk_plan(w, 150, 64) == [64, 64, 22]
    f1, t1, c1 = model.extract_feature_from_pixels(u8, txt)
    assert f1.shape == (150, 768) and f1.dtype == torch.float32 and c1.shape == (150,) and c1.dtype == torch.float32 and t1 is txt
    assert torch.equal(f1, ops.clip_vit_forward_chunked(w, u8, 64))
    assert torch.equal(c1, ops.clip_scores(txt[:1].unsqueeze(0), f1.unsqueeze(0))[0])      # scored once, over all T features


def test_frame_scorer_knob_equals_the_chunked_op_composed_by_hand(state, px):
    flat = bench.flat_from_state(bench.random_selector_state(768, DEV), 768, DEV)
    txt = torch.randn(1, 1, 768, generator=torch.Generator(device=DEV).manual_seed(8), device=DEV)
    scorer = FrameScorer(ops.ClipVitWeights(state, CFG, DEV), flat, encode_chunk_frames=128)
    idx, scores, feats = scorer(px[None, :200], txt, 8)
    by_hand = ops.clip_vit_forward_chunked(ops.ClipVitWeights(state, CFG, DEV), px[:200], 128)
    assert torch.equal(feats[0], by_hand)
    plain = FrameScorer(ops.ClipVitWeights(state, CFG, DEV), flat)
    assert plain.encode_chunk_frames is None
    s_hand, _ = plain.score(by_hand[None], txt)
    assert torch.equal(scores, s_hand) and torch.equal(idx, ops.topk_sorted(s_hand, 8))
    assert torch.equal(scorer.encode(px[:200]), by_hand)
    assert torch.equal(plain.encode(px[:200]), ops.clip_vit_forward(ops.ClipVitWeights(state, CFG, DEV), px[:200]))    # default: one call


def test_frame_id_generator_knob_writes_the_same_cache(tmp_path):
    """T = 256 host frames at chunk 128 (whole 64-frame blocks) through the reference-shaped harness entry: the streamed,
    chunked extract_feature caches bit for bit the `image` of the one-call path, and selects the same frames."""
    from tspo_amd.io import FrameIdGenerator, load_feature_cache, feature_cache_path
    model = _tspo_model(dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16, image_size=224,
                             patch_size=14))
    frames = synth.uniform_u8((256, 90, 160, 3), 31)
    sampled = list(range(0, 512, 2))
    reader_calls = []

    def reader(path, max_frames_num, fps, force_sample):
        reader_calls.append(max_frames_num)
        return frames, None, None, sampled
    msg = [{"value": "video.mp4"}, {"value": "<image>\nQuestion: what is shown?\nOptions:\nA. x\nB. y"}]
    proc = _StubProcessor()
    plain = FrameIdGenerator(model, proc, str(tmp_path / "plain"), sample_num=16, load_video=reader)
    knob = FrameIdGenerator(model, proc, str(tmp_path / "knob"), sample_num=16, load_video=reader, encode_chunk_frames=128)
    ids_plain = plain.generate_inner(msg, index=3, dataset="MLVU")
    ids_knob = knob.generate_inner(msg, index=3, dataset="MLVU")
    assert model.encode_chunk_frames is None and reader_calls == [50000, 50000]          # the knob is set for the call only
    a = load_feature_cache(feature_cache_path(str(tmp_path / "plain"), "MLVU", 3))
    b = load_feature_cache(feature_cache_path(str(tmp_path / "knob"), "MLVU", 3))
    assert a[0].shape == (256, 768) and torch.equal(a[0], b[0])                            # "image"
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert ids_plain == ids_knob and len(ids_knob) == 16
    assert knob.generate_inner(msg, index=3, dataset="MLVU") == ids_knob and knob.cache_hits == 1
