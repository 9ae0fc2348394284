"""Several questions per video, the parts that need no GPU: the two `_questions` entries exist in header, binding and library and
validate before any device work; the new translation unit runs without scratch or spills; FrameIdGenerator.generate_video decodes
and encodes a video once for all its uncached questions and leaves the per-index cache files generate_inner would have written."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tspo_clip_scores_questions", "tspo_selector_forward_questions")
EINVAL, EWORKSPACE = -1, -2


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tspo_amd import _lib
    return _lib, _lib.lib()


def test_symbols_in_header_binding_and_library():
    _l, l = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tspo_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared in tspo_hip.h"
        assert name in _l.SIGNATURES and hasattr(l, name)
    assert l.tspo_version() == 4, "the capability is found by symbol lookup: the ABI version does not move"
    assert l.tspo_selector_supported_flags(3) == EINVAL, "tspo_selector_supported_flags keeps its three entries"
    assert l.tspo_selector_supported_flags(0) == 1 | 4 | 8


def test_validation_without_a_device():
    _l, l = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    w = _l.SelectorWeights()
    for f, _ in w._fields_:
        setattr(w, f, p.value)
    T, D, H, M, win = 13, 64, 1, 1, 12
    need = l.tspo_selector_workspace_bytes(1, T, D, H, M, win)
    assert need > 0

    def fwd(Q=3, img=p, txt=p, scores=p, ws=p, tau=0.025, nbytes=need, flags=0, wp=ctypes.byref(w)):
        return l.tspo_selector_forward_questions(wp, img, txt, None, Q, T, D, H, M, win, tau, scores, None, ws, nbytes, None, flags)

    def err():
        return l.tspo_last_error()

    assert fwd(Q=0) == EINVAL and b"Q=0" in err()
    for kw in (dict(img=None), dict(txt=None), dict(scores=None), dict(ws=None), dict(wp=None)):
        assert fwd(**kw) == EINVAL and b"selector_forward_questions: null pointer" in err(), kw
    assert fwd(flags=64) == EINVAL and b"unknown flags" in err()
    assert fwd(flags=2) == EINVAL and b"unknown flags" in err()            # TSPO_SEL_ACCUMULATE is a backward flag
    assert fwd(flags=4 | 1) == EINVAL and b"exclusive" in err()             # TSPO_SEL_BF16 | TSPO_SEL_BF16X3
    assert fwd(tau=0.0) == EINVAL and b"score_tau" in err()
    assert fwd(nbytes=need - 1) == EWORKSPACE and b"workspace" in err()
    # the workspace is that of ONE video whatever Q is
    assert l.tspo_selector_forward_questions(ctypes.byref(w), p, p, None, 17, T, D, H, M, win, 0.025, p, None, p, need - 1, None,
                                             0) == EWORKSPACE

    def clip(Q=3, txt=p, feat=p, out=p, T_=T):
        return l.tspo_clip_scores_questions(txt, feat, Q, T_, D, M, out, None)
    assert clip(Q=0) == EINVAL and b"bad dims" in err()
    assert clip(T_=0) == EINVAL and b"bad dims" in err()
    for kw in (dict(txt=None), dict(feat=None), dict(out=None)):
        assert clip(**kw) == EINVAL and b"clip_scores_questions: null pointer" in err(), kw


def test_questions_unit_register_audit(tmp_path):
    """Every kernel of questions.hip: no scratch, no VGPR or SGPR spills (the metadata hipcc writes; compiled like the selector
    audit of tests/test_abi.py).  Its kernels live outside selector.hip, whose symbol count that audit caps."""
    import subprocess
    from tspo_amd import build as b
    assert "questions.hip" in b.SOURCES
    asm = tmp_path / "questions.s"
    subprocess.check_call([b._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(b.CSRC, "questions.hip"), "-o", str(asm)])
    kernels = {}
    for md in re.findall(r"\n  - (\.agpr_count:.*?\.wavefront_size)", open(asm).read(), flags=re.S):
        kernels[re.search(r"\.name:\s+(\S+)", md).group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", md).group(1)) for k in
                                                               ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                                "sgpr_spill_count")}
    assert len(kernels) == 2 and any("score_questions_kernel" in n for n in kernels) \
        and any("clip_scores_questions_kernel" in n for n in kernels), sorted(kernels)
    for name, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)


# ------------------------------------------------------------------------------------------------------------ generate_video
class _StubModel:
    """What FrameIdGenerator needs of a TSPOModel, on the CPU: features are a function of the frames, a text feature of its
    question, the score of frame t for a question a fixed function of both; the questions form is the loop of the single form."""
    device, dtype = torch.device("cpu"), torch.float32
    encode_chunk_frames = None

    def __init__(self):
        self.encodes = self.single_encodes = 0

    @staticmethod
    def _text(problem):
        return torch.full((1, 4), float(sum(map(ord, problem)) % 97))

    def extract_feature(self, proc, video, problem, processor_type='llava'):
        self.single_encodes += 1
        image = video.float().reshape(len(video), -1)[:, :4].contiguous()
        text = self._text(problem)
        return image, text, (image @ text[0]) * 1e-3

    def extract_feature_questions(self, proc, video, problems, processor_type='llava'):
        self.encodes += 1
        image = video.float().reshape(len(video), -1)[:, :4].contiguous()
        texts = torch.stack([self._text(p) for p in problems])
        return image, texts, torch.stack([(image @ t[0]) * 1e-3 for t in texts])

    def temporal_sampling(self, image, text, clip, method, window_size, sample_num):
        assert window_size == 12
        score = torch.sin(clip * 50.0 + text.flatten()[0])
        return torch.sort(torch.topk(score, sample_num).indices).values, score

    def temporal_sampling_questions(self, image, texts, clips, method, window_size, sample_num):
        rows = [self.temporal_sampling(image, texts[q], clips[q], method, window_size, sample_num) for q in range(len(texts))]
        return torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows])


def _question(text):
    return f"<image>\nQuestion: {text}\nOptions:\nA. yes\nB. no"


def _generator(tmp_path, name, n_frames=40, sample_num=8):
    from tspo_amd import io as tio
    calls = []
    frames = torch.arange(n_frames * 6, dtype=torch.float32).reshape(n_frames, 2, 3) % 23
    sampled = torch.arange(0, 30 * n_frames, 30)

    def load_video(path, max_frames_num, fps, force_sample):
        calls.append(path)
        return frames, None, None, sampled
    model = _StubModel()
    gen = tio.FrameIdGenerator(model, None, str(tmp_path / name), sample_num=sample_num, load_video=load_video)
    return gen, model, calls, sampled


ITEMS = [(11, _question("what happens first?")), (12, _question("who enters the room?")), (13, _question("is it raining?"))]


def test_generate_video_decodes_and_encodes_once(tmp_path):
    from tspo_amd import io as tio
    gen, model, calls, _ = _generator(tmp_path, "a")
    out = gen.generate_video("v.mp4", ITEMS, "MLVU")
    assert list(out) == [11, 12, 13] and calls == ["v.mp4"] and model.encodes == 1 and model.single_encodes == 0
    assert (gen.cache_misses, gen.cache_hits, gen.videos_encoded) == (3, 0, 1)
    for index, _ in ITEMS:
        stat = torch.load(tio.feature_cache_path(str(tmp_path / "a"), "MLVU", index))
        assert sorted(stat) == ["clip_scores", "image", "sampled_idx", "text"]
        assert stat["image"].shape == (40, 4) and stat["text"].shape == (1, 4) and stat["clip_scores"].shape == (40,)
        assert len(out[index]) == 8 and out[index] == sorted(out[index]) and all(isinstance(x, float) for x in out[index])
    assert out[11] != out[12], "each question gets its own selection"
    # the same ids, and the same cache files, as a generate_inner loop on another root
    ref, rmodel, rcalls, _ = _generator(tmp_path, "b")
    for index, q in ITEMS:
        assert ref.generate_inner([{"value": "v.mp4"}, {"value": q}], index=index, dataset="MLVU") == out[index]
        a, b = (torch.load(tio.feature_cache_path(str(tmp_path / r), "MLVU", index)) for r in "ab")
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert len(rcalls) == 3 and rmodel.single_encodes == 3 and ref.videos_encoded == 3
    # a later generate_inner on the first root hits the files generate_video wrote
    for index, q in ITEMS:
        assert gen.generate_inner([{"value": "v.mp4"}, {"value": q}], index=index, dataset="MLVU") == out[index]
    assert gen.cache_hits == 3 and calls == ["v.mp4"]


def test_generate_video_mixed_and_fully_cached_groups(tmp_path):
    gen, model, calls, _ = _generator(tmp_path, "m")
    first = gen.generate_inner([{"value": "v.mp4"}, {"value": ITEMS[1][1]}], index=12, dataset="VideoMME")
    assert calls == ["v.mp4"] and gen.cache_misses == 1
    out = gen.generate_video("v.mp4", ITEMS, "VideoMME")
    assert out[12] == first and list(out) == [11, 12, 13]
    assert calls == ["v.mp4"] * 2 and model.encodes == 1, "one cached, two not: one more decode, one encode"
    assert (gen.cache_misses, gen.cache_hits, gen.videos_encoded) == (3, 1, 2)
    again = gen.generate_video("v.mp4", ITEMS, "VideoMME")
    assert again == out and calls == ["v.mp4"] * 2 and model.encodes == 1, "a fully cached group never opens the video"
    assert gen.cache_hits == 4
    gen.load_video = None
    assert gen.generate_video("v.mp4", ITEMS, "VideoMME") == out      # ... and needs no load_video plug-in


def test_generate_video_short_video_returns_the_sampled_frames(tmp_path):
    gen, model, calls, sampled = _generator(tmp_path, "s", n_frames=8, sample_num=8)
    out = gen.generate_video("short.mp4", ITEMS, "LVBench")
    assert all(out[i] == sampled.float().tolist() for i, _ in ITEMS) and model.encodes == 1 and calls == ["short.mp4"]


def test_group_by_video_keeps_first_seen_order():
    from tspo_amd import io as tio
    msgs = [(5, [{"value": "b.mp4"}, {"value": "q5"}]), (1, [{"value": "a.mp4"}, {"value": "q1"}]),
            (7, [{"value": "b.mp4"}, {"value": "q7"}]), (2, [{"value": "a.mp4"}, {"value": "q2"}]),
            (9, [{"value": "c.mp4"}, {"value": "q9"}])]
    assert list(tio.group_by_video(msgs)) == [("b.mp4", [(5, "q5"), (7, "q7")]), ("a.mp4", [(1, "q1"), (2, "q2")]),
                                              ("c.mp4", [(9, "q9")])]
    assert list(tio.group_by_video([])) == []
