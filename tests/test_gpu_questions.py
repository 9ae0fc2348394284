"""Several questions about one video (the `_questions` entries and everything above them): every output is BIT FOR BIT what the
per-question path gives - the reference here is the existing entries (tspo_selector_forward_ex / tspo_clip_scores with B = 1, one
call per question), compared with torch.equal.  Shapes are the smallest that reach every row form of the two kernels: fewer rows
than a workgroup holds (T < 4), a partial last workgroup, T < window, lanes without data (D = 64), the three-chunk row (D = 768),
the second trip of the row loop (D = 1280), one / a few / more than one chunk of questions (Q = 1, 2, 3, 17)."""
import ctypes as C

import numpy as np
import pytest
import torch

from inputs import SELECTOR_CASES, selector_inputs
from tspo_amd import io as tio, ops, synth
from tspo_amd.pipeline import FrameScorer
from tspo_amd.temporal_agent import MultiModal_Align, TSPOModel

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU = 0.05


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(104729 * (seed + 1))


def _inputs(T, D, Q, M, seed=0):
    g = _gen(seed)
    r = lambda shape, std=1.0: torch.randn(*shape, generator=g, device=DEV) * std      # noqa: E731
    flat = r((ops.flat_offsets(D)["__total__"][0],), 0.5 / np.sqrt(D))
    return flat, r((T, D)), r((Q, M, D)), r((Q, T), 0.1)


def _per_question(flat, img, txt, clip, H, w, tau, precision):
    """The reference: one existing B = 1 forward per question."""
    rows, attn = [], None
    for q in range(txt.shape[0]):
        s, h, _ = ops.selector_forward(flat, img[None], txt[q][None], None if clip is None else clip[q][None], H, w, tau,
                                       precision=precision)
        rows.append(s[0])
        attn = h[0] if attn is None else attn
        assert torch.equal(h[0], attn), "temporal_attn does not depend on the question"
    return torch.stack(rows), attn


#        name                       T    D     H   Q   M  window  clip   precision     attn
CASES = [("T1-D64-Q1",              1,   64,   1,  1,  1, 12,     True,  "fp32",       True),
         ("T3-D768-Q2-M3-noclip",   3,   768,  8,  2,  3, 12,     False, "bf16x3",     True),
         ("T5-D1280-Q3-w1-noattn",  5,   1280, 10, 3,  1, 1,      True,  "bf16",       False),
         ("T13-D768-Q17-M3",        13,  768,  8,  17, 3, 12,     True,  "bf16_mixed", True),
         ("T257-D1280-Q17-M3",      257, 1280, 10, 17, 3, 12,     True,  "fp32",       True),
         ("T257-D64-Q3-noclip",     257, 64,   1,  3,  1, 12,     False, "fp32",       False),
         ("T257-D768-Q3",           257, 768,  8,  3,  1, 12,     True,  "fp32",       True)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scores_are_the_bits_of_the_per_question_entry(case):
    _, T, D, H, Q, M, w, with_clip, precision, want_attn = case
    flat, img, txt, clip = _inputs(T, D, Q, M)
    clip = clip if with_clip else None
    want, want_attn_t = _per_question(flat, img, txt, clip, H, w, TAU, precision)
    got, attn = ops.selector_forward_questions(flat, img, txt, clip, H, w, TAU, precision=precision, want_attn=want_attn)
    assert got.shape == (Q, T) and torch.isfinite(got).all()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} scores differ, max {(got - want).abs().max().item():.3e}"
    if want_attn:
        assert attn.shape == (T, D) and torch.equal(attn, want_attn_t)
    else:
        assert attn is None


#             T    D     Q   M
CLIP_CASES = [(1,   64,   1,  1), (3, 768, 2, 3), (5, 1280, 3, 1), (13, 768, 17, 3), (257, 1280, 17, 1), (257, 100, 5, 1),
              (257, 768, 3, 1)]


@pytest.mark.parametrize("T,D,Q,M", CLIP_CASES)
def test_clip_scores_are_the_bits_of_the_per_question_entry(T, D, Q, M):
    g = _gen(T + D + Q)
    txt, feat = torch.randn(Q, M, D, generator=g, device=DEV), torch.randn(T, D, generator=g, device=DEV)
    want = torch.stack([ops.clip_scores(txt[q][None], feat[None])[0] for q in range(Q)])
    got = ops.clip_scores_questions(txt, feat)
    assert got.shape == (Q, T) and torch.equal(got, want), (got - want).abs().max().item()


def test_golden_case_first_among_three_questions(golden):
    """A reference-generated case of tests/golden/selector.npz with its text as question 0 of 3: row 0 meets the golden scores at
    the tolerance tests/test_gpu_ops.py::test_selector_forward_golden uses for the case."""
    name, T, D, H, w, tau, M, _ = next(c for c in SELECTOR_CASES if c[0] == "s40m3")
    img, txt, clip, state = selector_inputs(name, T, D, M)
    offs = ops.flat_offsets(D)
    flat = torch.zeros(offs["__total__"][0])
    for pn, (off, shape) in offs.items():
        if not pn.startswith("__"):
            flat[off:off + int(np.prod(shape))] = torch.from_numpy(np.asarray(state[pn])).flatten()
    g = _gen(5)
    txts = torch.cat([torch.from_numpy(txt)[None].to(DEV), torch.randn(2, M, D, generator=g, device=DEV)])
    clips = torch.cat([torch.from_numpy(clip)[None].to(DEV), torch.randn(2, T, generator=g, device=DEV) * 0.1])
    s, _ = ops.selector_forward_questions(flat.to(DEV), torch.from_numpy(img).to(DEV), txts, clips, H, w, tau)
    np.testing.assert_allclose(s[0].cpu().numpy(), golden["selector"][f"{name}.scores"], rtol=2e-5, atol=2e-5 / tau)


def test_questions_are_independent():
    T, D, H, Q, M, w = 13, 768, 8, 5, 3, 12
    flat, img, txt, clip = _inputs(T, D, Q, M, seed=3)
    s, _ = ops.selector_forward_questions(flat, img, txt, clip, H, w, TAU)
    c = ops.clip_scores_questions(txt, img)
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    sp, _ = ops.selector_forward_questions(flat, img, txt[perm], clip[perm], H, w, TAU)
    assert torch.equal(sp, s[perm]) and torch.equal(ops.clip_scores_questions(txt[perm], img), c[perm])
    bad = txt.clone()
    bad[1] = float("nan")
    sn, _ = ops.selector_forward_questions(flat, img, bad, clip, H, w, TAU)
    cn = ops.clip_scores_questions(bad, img)
    keep = [0, 2, 3, 4]
    assert torch.equal(sn[keep], s[keep]) and sn[1].isnan().all()
    assert torch.equal(cn[keep], c[keep]) and cn[1].isnan().all()


@pytest.mark.parametrize("T,D,H,Q,M", [(5, 64, 1, 3, 1), (257, 768, 8, 17, 3)])
def test_nothing_is_written_behind_the_outputs_or_the_workspace(T, D, H, Q, M):
    """Canaries behind scores[Q*T], behind clip[Q*T] and behind a workspace of exactly the B = 1 size stay intact."""
    from tspo_amd import _lib
    w, pad = 12, 4096
    flat, img, txt, clip = _inputs(T, D, Q, M, seed=4)
    need = _lib.lib().tspo_selector_workspace_bytes(1, T, D, H, M, w)
    assert need == _lib.lib().tspo_selector_workspace_bytes(1, T, D, H, 1, w), "the workspace does not depend on the texts"
    ws = torch.full((need + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    scores = torch.full((Q * T + pad,), -7.25, device=DEV)
    attn = torch.full((T * D + pad,), -7.25, device=DEV)
    cout = torch.full((Q * T + pad,), -7.25, device=DEV)
    sw = ops._sel_structs(flat, D, _lib.SelectorWeights)
    p = ops._ptr
    _lib.check(_lib.lib().tspo_selector_forward_questions(C.byref(sw), p(img), p(txt), p(clip), Q, T, D, H, M, w, TAU, p(scores),
                                                          p(attn), p(ws), need, ops._stream(), 0), "forward_questions")
    _lib.check(_lib.lib().tspo_clip_scores_questions(p(txt), p(img), Q, T, D, M, p(cout), ops._stream()), "clip_scores_questions")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()) and bool((scores[Q * T:] == -7.25).all()) and bool((attn[T * D:] == -7.25).all())
    assert bool((cout[Q * T:] == -7.25).all())
    want, want_attn = ops.selector_forward_questions(flat, img, txt, clip, H, w, TAU)
    assert torch.equal(scores[:Q * T].view(Q, T), want) and torch.equal(attn[:T * D].view(T, D), want_attn)
    assert torch.equal(cout[:Q * T].view(Q, T), ops.clip_scores_questions(txt, img))


def test_side_stream_and_graph_replay_give_the_default_stream_bits():
    T, D, H, Q, M, w = 257, 768, 8, 3, 1, 12
    seeds = (0, 1, 2)
    real = {s: _inputs(T, D, Q, M, seed=10 + s) for s in seeds}
    bufs = [t.clone() for t in real[0]]
    ws = ops.selector_workspace(1, T, D, H, M, w, DEV)

    def run():
        flat, img, txt, clip = bufs
        s, h = ops.selector_forward_questions(flat, img, txt, clip, H, w, TAU, ws=ws)
        return s, h, ops.clip_scores_questions(txt, img)

    def load(seed):
        for b, t in zip(bufs, real[seed]):
            b.copy_(t)

    want = {}
    for s in seeds:
        load(s)
        want[s] = [t.clone() for t in run()]
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        ws.fill_(0xFF)
        load(1)
        got = run()
    S.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want[1])), "side stream"
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        out = run()
    for s in seeds:
        ws.fill_(0xFF)
        for t in out:
            t.fill_(float("nan"))
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, want[s])), f"graph replay on the inputs of seed {s}"
    del graph


def test_module_forward_questions_equals_a_loop_of_forward():
    D, T, Q, M = 64, 40, 3, 2
    m = MultiModal_Align(dim=D, num_heads=8).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.selector_state(D, seed=4, std=0.1, bias_std=0.05).items()})
    g = _gen(7)
    img, txt = torch.randn(T, D, generator=g, device=DEV), torch.randn(Q, M, D, generator=g, device=DEV)
    clip = torch.randn(Q, T, generator=g, device=DEV) * 0.1
    with pytest.raises(RuntimeError, match="inference only"):
        m.forward_questions(img, txt, clip, window_size=12)            # grad mode on, trainable parameters: training
    for precision in ("fp32", "bf16"):
        m.inference_gemm_precision = precision
        with torch.no_grad():
            s, h = m.forward_questions(img, txt, clip, window_size=12)
            for q in range(Q):
                s1, h1 = m(img, txt[q], clip[q], window_size=12)
                assert torch.equal(s[q], s1) and torch.equal(h, h1) and h.shape == (1, T, D)
    with torch.no_grad():
        bf16 = m.forward_questions(img, txt, clip, window_size=12)[0]          # (the loop left the module at "bf16")
        m.inference_gemm_precision = "fp32"
        assert not torch.equal(bf16, m.forward_questions(img, txt, clip, window_size=12)[0]), "inference_gemm_precision is honoured"
        with pytest.raises(TypeError):
            m.forward_questions(img, txt, None, window_size=12)


# ------------------------------------------------------------------------------------------------------------------ the model
class _Processor:
    """CLIPProcessor stand-in (no tokenizer files offline): text -> 7 token ids that depend on the text, images -> the real
    CLIPImageProcessor (as tests/test_gpu_api.py:_StubProcessor, whose ids are the same for every text)."""

    def __init__(self):
        from transformers import CLIPImageProcessor
        self.image_processor = CLIPImageProcessor()

    def __call__(self, text=None, images=None, return_tensors="pt", **kw):
        from transformers import BatchEncoding, BatchFeature
        if text is not None:
            h = sum((i + 1) * ord(c) for i, c in enumerate(text))
            ids = torch.tensor([[49406] + [1 + (h * (j + 3)) % 40000 for j in range(5)] + [49407]])
            return BatchEncoding({"input_ids": ids, "attention_mask": torch.ones_like(ids)})
        return BatchFeature(self.image_processor(images=images, return_tensors="pt"))


def _tiny_model(dtype):
    from transformers import CLIPConfig
    cfg = CLIPConfig(text_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      vocab_size=49408, max_position_embeddings=77, projection_dim=768),
                     vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                        image_size=224, patch_size=14, projection_dim=768), projection_dim=768)
    torch.manual_seed(0)
    model = TSPOModel(cfg).float().eval()
    for p in list(model.vision_model.parameters()) + list(model.text_model.parameters()):
        if p.ndim >= 2:
            torch.nn.init.normal_(p, std=0.05)
    model.selector.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.selector_state(768, seed=2, std=0.02).items()})
    return model.to(dtype).to(DEV)


PROBLEMS = ["what happens first?", "who enters the room?", "is it raining outside?"]


@pytest.fixture(scope="module")
def model_f32():
    return _tiny_model(torch.float32)


def test_model_questions_equal_a_loop_of_the_single_path(model_f32):
    model, proc = model_f32, _Processor()
    frames = synth.uniform_u8((72, 240, 320, 3), 77)
    with torch.no_grad():
        _model_questions_checks(model, proc, frames)


def _model_questions_checks(model, proc, frames):
    feats, texts, clips = model.extract_feature_questions(proc, frames, PROBLEMS)
    assert feats.shape == (72, 768) and texts.shape == (3, 1, 768) and clips.shape == (3, 72)
    single = [model.extract_feature(proc, frames, p) for p in PROBLEMS]
    assert not torch.equal(single[0][1], single[1][1]), "the stand-in processor tells the questions apart"
    for q, (f1, t1, c1) in enumerate(single):
        assert torch.equal(f1, feats) and torch.equal(t1, texts[q]) and torch.equal(c1, clips[q])
    for method in ("topk", "bin-max", "aks"):
        ids, pred = model.temporal_sampling_questions(feats, texts, clips, method, 12, 8)
        assert ids.shape == (3, 8) and pred.shape == (3, 72)
        for q, (f1, t1, c1) in enumerate(single):
            i1, p1 = model.temporal_sampling(f1, t1, c1, method, 12, 8)
            assert torch.equal(ids[q], i1) and torch.equal(pred[q], p1.detach()), (method, q)
    with pytest.raises(ValueError):
        model.extract_feature_questions(proc, frames, [])


def test_frame_scorer_questions(model_f32):
    from tspo_amd.temporal_agent import _packed_clip
    D, Q = 768, 3
    flat = _inputs(8, D, 1, 1)[0]
    scorer = FrameScorer(_packed_clip(model_f32), flat)
    g = _gen(21)
    px = torch.randint(0, 256, (70, 3, 224, 224), generator=g, device=DEV, dtype=torch.uint8)
    txt = torch.randn(Q, 1, D, generator=g, device=DEV)
    for method in ("topk", "bin-max"):
        idx, scores, feats = scorer.questions(px, txt, 6, method)
        assert idx.shape == (Q, 6) and scores.shape == (Q, 70) and feats.shape == (70, D)
        for q in range(Q):
            i1, s1, f1 = scorer(px[None], txt[q][None], 6, method)
            assert torch.equal(i1[0], idx[q]) and torch.equal(s1[0], scores[q]) and torch.equal(f1[0], feats)


@pytest.mark.parametrize("dataset", ["MLVU", "VideoMME"])
def test_generate_video_equals_a_generate_inner_loop(tmp_path, dataset):
    """The harness flow (gen_id_tspo.py:59-92, bf16 as it loads the model): one generate_video on one root against a generate_inner
    loop on another - identical ids, every cache file tensor for tensor equal, 1 decode against Q, then all cache hits."""
    model, proc = _tiny_model(torch.bfloat16), _Processor()
    T = 150
    frames = synth.uniform_u8((T, 224, 224, 3), 17)
    sampled = torch.arange(0, 30 * T, 30)
    calls = []

    def load_video(path, max_frames_num, fps, force_sample):
        calls.append(path)
        return frames, None, None, sampled
    items = [(7 + q, f"<image>\nQuestion: {p}\nOptions:\nA. a\nB. b") for q, p in enumerate(PROBLEMS)]
    one = tio.FrameIdGenerator(model, proc, str(tmp_path / "video"), sample_num=64, load_video=load_video)
    out = one.generate_video("long.mp4", items, dataset)
    assert calls == ["long.mp4"] and (one.cache_misses, one.cache_hits, one.videos_encoded) == (3, 0, 1)
    loop = tio.FrameIdGenerator(model, proc, str(tmp_path / "inner"), sample_num=64, load_video=load_video)
    for index, question in items:
        ids = loop.generate_inner([{"value": "long.mp4"}, {"value": question}], index=index, dataset=dataset)
        assert ids == out[index] and len(ids) == 64 and ids == sorted(ids)
        a, b = (torch.load(tio.feature_cache_path(str(tmp_path / r), dataset, index)) for r in ("video", "inner"))
        assert sorted(a) == sorted(b) == ["clip_scores", "image", "sampled_idx", "text"]
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (index, k)
    assert len(calls) == 1 + len(items) and loop.videos_encoded == 3
    for index, question in items:
        assert one.generate_inner([{"value": "long.mp4"}, {"value": question}], index=index, dataset=dataset) == out[index]
    assert one.cache_hits == 3 and len(calls) == 1 + len(items), "generate_inner after generate_video: all cache hits"
