"""Indexed, normalising preprocessing (tspo_preprocess_select) and the frames-driven training step - the parts that need no
GPU: argument validation of the C entry, the register audit of preprocess.hip, the haystack index plans against the
frame-level builders, PreprocessSpec detection, the problem-text derivation and the exact-size tap tables against Pillow."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from oracle import tspo_oracle as O
from tspo_amd import haystack, preprocess as P, synth


def _select_args(**over):
    """A complete, valid argument list of tspo_preprocess_select over dummy host buffers (never dereferenced: every case below
    is rejected before the device is touched)."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(pool=p, layout=0, P=4, H=32, W=32, index=p, N=2, hcoef=p, hbound=p, out_w=16, hk=5, vcoef=p, vbound=p, out_h=16, vk=5,
             ylo=0, nrows=32, out=p, out_dtype=0, rescale=1 / 255, mean=(ctypes.c_double * 3)(0.5, 0.5, 0.5),
             std=(ctypes.c_double * 3)(0.5, 0.5, 0.5), flag=None, ws=p, ws_bytes=1 << 20, stream=None, mt=None, mb=None, mx=None,
             nkb=0, span=0)
    a.update(over)
    return list(a.values()), buf


def test_select_argument_validation_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from tspo_amd import _lib
    l = _lib.lib()
    assert hasattr(l, "tspo_preprocess_select") and "tspo_preprocess_select" in _lib.SIGNATURES

    def rc(**over):
        args, keep = _select_args(**over)
        return l.tspo_preprocess_select(*args), l.tspo_last_error()

    r, msg = rc(pool=None)
    assert r == -1 and b"null pointer" in msg
    r, msg = rc(N=0)
    assert r == -1 and b"bad dims" in msg
    r, msg = rc(out_dtype=7)
    assert r == -1 and b"unknown out_dtype" in msg
    r, msg = rc(std=(ctypes.c_double * 3)(0.5, 0.0, 0.5))
    assert r == -1 and b"std == 0" in msg
    r, msg = rc(index=None, N=3)                       # index == NULL means 0..P-1
    assert r == -1 and b"N must equal P" in msg
    r, msg = rc(ws_bytes=16)
    assert r == -2 and b"workspace" in msg
    r, msg = rc(ylo=8, nrows=32)
    assert r == -1 and b"row window" in msg
    # uint8 output ignores mean / std
    r, msg = rc(out_dtype=3, mean=None, std=None, ws_bytes=16)
    assert r == -2


def test_select_frames_has_no_cpu_fallback():
    from tspo_amd._lib import TspoHipError
    with pytest.raises(TspoHipError):
        P.select_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), P.PreprocessSpec.clip_default())
    with pytest.raises(TspoHipError):
        P.select_frames(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), None, P.PreprocessSpec(size=(384, 384)))


def test_preprocess_kernel_register_audit(tmp_path):
    """Every kernel of preprocess.hip - the indexed forms of the three horizontal passes and the four output types of the two
    vertical passes included - runs without scratch and without register spills (device-only -S compile)."""
    import subprocess
    from tspo_amd import build as b
    asm = tmp_path / "preprocess.s"
    subprocess.check_call([b._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                           os.path.join(b.CSRC, "preprocess.hip"), "-o", str(asm)])
    txt = open(asm).read()
    kernels = {}
    for md in re.findall(r"\n  - (\.agpr_count:.*?\.wavefront_size)", txt, flags=re.S):
        kernels[re.search(r"\.name:\s+(\S+)", md).group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", md).group(1)) for k in
                                                               ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                                "sgpr_spill_count")}
    count = lambda pat: sum(bool(re.search(pat, n)) for n in kernels)
    assert count(r"resample_h_mfma_kernel") == 16      # 2 layouts x 4 K-block counts x (plain, indexed)
    assert count(r"resample_h_lds_kernel") == 4 and count(r"resample_h_kernel") == 2
    assert count(r"resample_v4_kernel") == 4 and count(r"resample_v_kernel") == 4      # uint8, fp32, bf16, f16
    for name, v in kernels.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
    assert not re.search(r"^\s*scratch_", txt, flags=re.M)


@pytest.mark.parametrize("L", [128, 64, 50, 37], ids=lambda v: f"L{v}")        # 50 and 37: the "whole video" branch
@pytest.mark.parametrize("r", [1, 2, 3, 4, None], ids=lambda v: f"r{v}")       # None: drawn from random.Random like the reference
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_plan_equals_sample(L, r, kind):
    seed = 1000 + L + (r or 0)
    video = synth.uniform_u8((L, 6, 5, 3), seed)
    video = torch.from_numpy(video) if kind == "torch" else video
    glen = min(L, 50)
    wrong = haystack.synthetic_distractors(12, glen, video, seed=seed)
    ra, pa = np.random.RandomState(seed), random.Random(seed)
    frames, mask = haystack.build_specific_sample(video, wrong, repeat_times=r, rng=ra, py_random=pa)
    rb, pb = np.random.RandomState(seed), random.Random(seed)
    plan, pmask = haystack.build_specific_plan(L, 12, repeat_times=r, rng=rb, py_random=pb)
    pool = haystack.haystack_pool(video, wrong)
    assert plan.dtype == torch.int64 and pmask.dtype == torch.bool and plan.shape == pmask.shape == (len(frames),)
    assert len(pool) == L + 12 * glen and int(plan.min()) >= 0 and int(plan.max()) < len(pool)
    got = pool[plan] if kind == "torch" else pool[plan.numpy()]
    assert np.array_equal(np.asarray(got), np.asarray(frames))
    assert torch.equal(pmask, mask)
    assert torch.equal(pmask, plan < L)                                        # true-clip frames are exactly the video's
    sa, sb = ra.get_state(), rb.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert pa.getstate() == pb.getstate()


def test_plan_default_random_stream_matches_the_frame_builder():
    """Without explicit generators both draw from numpy's global legacy generator and the `random` module, like the reference."""
    video = synth.uniform_u8((90, 4, 4, 3), 5)
    wrong = haystack.synthetic_distractors(12, 50, video, seed=1)
    np.random.seed(77), random.seed(77)
    frames, mask = haystack.build_specific_sample(video, wrong)
    np.random.seed(77), random.seed(77)
    plan, pmask = haystack.build_specific_plan(90, 12)
    assert np.array_equal(haystack.haystack_pool(video, wrong)[plan.numpy()], frames) and torch.equal(mask, pmask)


class _SigLipShaped:
    """The attribute shape of the reference's SigLipImageProcessor (llava/model/multimodal_encoder/siglip_encoder.py:34-45)."""

    def __init__(self, resample=3, size=(384, 384), mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        self.image_mean, self.image_std, self.size, self.resample = mean, std, size, resample
        self.rescale_factor, self.crop_size = 1 / 255, {"height": 384, "width": 384}


def test_spec_from_image_processor():
    from transformers import CLIPImageProcessor
    S = P.PreprocessSpec
    clip = S.from_image_processor(CLIPImageProcessor())
    assert clip == S.clip_default() and clip.out_hw == (224, 224) and clip.shortest_edge == 224 and clip.size is None
    assert P.processor_is_default_clip(CLIPImageProcessor())
    sig = S.from_image_processor(_SigLipShaped(), out_dtype=torch.bfloat16)
    assert sig == S(size=(384, 384), mean=(0.5,) * 3, std=(0.5,) * 3, out_dtype=torch.bfloat16) and sig.crop is None
    assert sig.out_hw == (384, 384) and sig.rescale == 1 / 255
    big = S.from_image_processor(CLIPImageProcessor(size={"shortest_edge": 336}, crop_size={"height": 336, "width": 336}))
    assert big is not None and big.shortest_edge == 336 and big.out_hw == (336, 336) and big != S.clip_default()
    assert S.from_image_processor(CLIPImageProcessor(resample=2)) is None                     # bilinear
    assert S.from_image_processor(_SigLipShaped(resample=1)) is None                          # lanczos
    assert S.from_image_processor(CLIPImageProcessor(do_pad=True)) is None                    # padded
    assert S.from_image_processor(CLIPImageProcessor(crop_size={"height": 256, "width": 256})) is None   # crop > image: pads
    assert S.from_image_processor(CLIPImageProcessor(do_normalize=False)) is None
    assert S.from_image_processor(object()) is None and S.from_image_processor(None) is None  # unknown
    for extra in ("do_image_splitting", "image_grid_pinpoints", "do_flip_channel_order", "do_pad"):   # same shape, does more
        ip = _SigLipShaped()
        setattr(ip, extra, [[384, 768]] if extra == "image_grid_pinpoints" else True)
        assert S.from_image_processor(ip) is None, extra
        setattr(ip, extra, False)
        assert S.from_image_processor(ip) is not None, extra
    bad = _SigLipShaped()
    bad.image_mean = "0.5"                                                                    # malformed: None, not an exception
    assert S.from_image_processor(bad) is None

    class _QwenShaped:                                                                        # smart_resize: min / max pixels
        resample, image_mean, image_std, rescale_factor = 3, [0.5] * 3, [0.5] * 3, 1 / 255
        min_pixels, max_pixels, patch_size, size = 3136, 12845056, 14, {"shortest_edge": 3136, "longest_edge": 12845056}
    assert S.from_image_processor(_QwenShaped()) is None
    with pytest.raises(ValueError):
        S(shortest_edge=224, size=(384, 384))
    with pytest.raises(ValueError):
        S(size=(384, 384), out_dtype=torch.float64)


def test_problem_text_both_option_formats():
    from tspo_amd.train import problem_text
    s1 = 'Please provide your answer by stating the letter followed by the full option.'
    s2 = 'Please respond with only the letter of the correct answer.'
    q = "<image>\nWhat does the man pick up after the dog leaves?"
    assert problem_text(q + "\nA. a cup\nB. a ball\n" + s2) == "What does the man pick up after the dog leaves?"
    assert problem_text(q + "\n(A) a cup\n(B) a ball\n" + s1) == "What does the man pick up after the dog leaves?"
    assert problem_text(s1 + q.replace("<image>\n", "") + "\nA. x") == "What does the man pick up after the dog leaves?"
    # the "\nA" test comes first and looks at the raw question, as in the reference: "\nAfter..." splits there
    assert problem_text("<image>\nBefore.\nAfter that?\n(A) x") == "Before."
    with pytest.raises(ValueError):
        problem_text("<image>\nno options here")


def _apply_tables(img, hk, hb, vk, vb, ylo, nrows):
    """The integer arithmetic of the kernels in numpy: horizontal pass into a rounded uint8 intermediate, then vertical."""
    x = img.astype(np.int64)
    ow, oh = hk.shape[0], vk.shape[0]
    tmp = np.zeros((nrows, ow, 3), np.int64)
    for o in range(ow):
        acc = np.full((nrows, 3), 1 << 21, np.int64)
        for i in range(hb[o, 1]):
            acc += x[ylo:ylo + nrows, hb[o, 0] + i] * int(hk[o, i])
        tmp[:, o] = np.clip(acc >> 22, 0, 255)
    out = np.zeros((oh, ow, 3), np.int64)
    for o in range(oh):
        acc = np.full((ow, 3), 1 << 21, np.int64)
        for i in range(vb[o, 1]):
            acc += tmp[vb[o, 0] - ylo + i] * int(vk[o, i])
        out[o] = np.clip(acc >> 22, 0, 255)
    return out.astype(np.uint8)


@pytest.mark.parametrize("hw", [(720, 1280), (240, 320), (333, 517)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_exact_size_tables_match_pil(hw):
    """384 x 384 without crop (the SigLIP rule): down-scaling with different factors per axis, up-scaling and an odd size."""
    from PIL import Image
    H, W = hw
    img = synth.uniform_u8((1, H, W, 3), 300 + H)[0]
    spec = P.PreprocessSpec(size=(384, 384))
    hk, hb, vk, vb, ylo, nrows = P._spec_tables(H, W, spec.geometry)
    assert hk.shape[0] == 384 and vk.shape[0] == 384 and ylo == 0 and nrows == H       # no crop: every input row is needed
    ref = np.array(Image.fromarray(img).resize((384, 384), resample=Image.BICUBIC))
    np.testing.assert_array_equal(O.pil_bicubic_resize_u8(img, 384, 384), ref)          # the Pillow-pinned oracle path
    np.testing.assert_array_equal(_apply_tables(img, hk, hb, vk, vb, ylo, nrows), ref)
    # the LDS sizing assumptions of the kernels hold for these tables (the numbers come from the one host-side restatement of
    # preprocess.hip's formulas, preprocess.kernel_lds_sizing): PV_R = 4 consecutive output rows touch at most `vspan` rows, a
    # 32-column chunk at most `span_px` pixels, and the matrix pass fits its 64 KB of LDS
    mf = P.mfma_h_tables(hk, hb)
    assert mf is not None and 1 <= mf[3] <= 4
    vspan, span_px, mfma_lds = P.kernel_lds_sizing(hk.shape[1], vk.shape[1], mf[4])
    for y0 in range(0, 384, 4):
        assert vb[y0 + 3, 0] + vb[y0 + 3, 1] - vb[y0, 0] <= vspan
    for x0 in range(0, 384, 32):
        assert hb[x0 + 31, 0] + hb[x0 + 31, 1] - hb[x0, 0] <= span_px
    assert mfma_lds <= 64 * 1024


def test_clip_spec_tables_equal_the_existing_ones():
    for H, W in [(360, 640), (480, 360), (720, 1280), (224, 224)]:
        a, b = P._tables(H, W, 224), P._spec_tables(H, W, P.PreprocessSpec.clip_default().geometry)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def test_bench_train_frames_arguments_and_json_shape(capsys):
    """tools/bench_train_frames.py without a GPU: argument checks and the shape of its one JSON line (--dry-run)."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_train_frames", os.path.join(root, "tools", "bench_train_frames.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.main(["--dry-run"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["G"] == 8 and d["k"] == 16 and d["frame"] == [720, 1280] and d["pool_frames"] == 728 and d["rounds"] >= 3
    assert sorted(d["by_T"]) == ["512", "800"]
    for r in d["by_T"].values():
        assert sorted(r["ms"]) == sorted(["upload", "front_end", "encode", "policy_step", "selected_frames"])
        assert sorted(r["selected_frames_ms"]) == ["new_entry", "parent_composition", "reference_cpu"]
        assert "prompts_per_s" in r and "policy_share" in r
    for bad in (["--rounds", "2"], ["--T", "8"], ["--iters", "0"]):
        with pytest.raises(SystemExit):
            mod.parse(bad)
    assert mod.summarise([3.0, 1.0, 2.0]) == {"median": 2.0, "min": 1.0, "max": 3.0}


def test_frame_dataset_rejects_batches_of_more_than_one_prompt():
    from tspo_amd import train as tt
    ds = object.__new__(tt.FrameDataset)
    with pytest.raises(ValueError, match="one prompt per micro-batch"):
        next(ds.batches(0, 1, 2))
