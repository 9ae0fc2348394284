"""Host side of the chunked encode (no GPU): the chunk planner tspo_clip_chunk_plan, tspo_clip_will_fold against the closed form it
replaces, and the argument validation of tspo_clip_vit_forward_chunked.

What the planner promises (include/tspo_hip.h): sizes sum to n_frames; every size <= chunk_frames; count = ceil(n_frames /
chunk_frames); every size but the last is a multiple of 64 frames; when n_frames folds, every chunk folds; chunk_frames below
the fold threshold, chunk_frames < 1, n_frames < 1 and a cap that is too small are TSPO_EINVAL with a message.  For some pairs
NO list of sizes meets all of these at once - CLIP-L/14 (fold threshold 64): 65 frames in two chunks of at most 64, each of at
least 64; 50 000 frames in exactly 50 chunks of at most 1000 of which 49 are multiples of 64 (49 x 960 + 1000 < 50 000).  There
the planner answers TSPO_EINVAL "no plan"; the test decides which pairs those are by exhaustive search over the number of
64-frame blocks in the leading chunks (`_feasible`), independently of the planner's arithmetic, and every other pair must get a
plan that meets every clause."""
import ctypes as C

import pytest

from tspo_amd import _lib, ops, synth

L14 = synth.CLIP_L14
VITB16 = dict(hidden=768, layers=1, heads=12, mlp=3072, patch=16, image=224, proj=512)      # tests/test_gpu_encoder_stages.py
FRAMES = (1, 63, 64, 65, 127, 128, 129, 1024, 1025, 4097, 50_000)
CHUNKS = (64, 128, 256, 1000, 2048)


def _cfg(c):
    return ops._clip_cfg_struct(c)


def _folds_closed_form(c, n):
    """What ClipVitWeights.library_folds restated in Python before it called the library (csrc/gemm_bf16.hip gemm_bf16_is_big)."""
    M = n * ((c["image"] // c["patch"]) ** 2 + 1)

    def big(N, K):
        return M * N >= 256 ** 3 and K >= 128 and N <= 4096
    return c["layers"] > 0 and big(c["hidden"], c["hidden"]) and big(c["hidden"], c["mlp"])


def _fold_threshold(c):
    return next((n for n in range(1, 8192) if _folds_closed_form(c, n)), None)


def _feasible(n, chunk, f):
    """Is there ANY list of ceil(n / chunk) sizes with every size in [f, chunk], all but the last multiples of 64, summing to n?"""
    k = -(-n // chunk)
    if k == 1:
        return True
    lo, hi = -(-f // 64), chunk // 64                 # 64-frame blocks a leading chunk may hold
    if hi < lo:
        return False
    return any(f <= n - 64 * j <= chunk for j in range((k - 1) * lo, (k - 1) * hi + 1))


def _plan_rc(c, n, chunk, cap=None):
    cap = max(1, n) if cap is None else cap
    sizes = (C.c_int * max(1, cap))()
    rc = _lib.lib().tspo_clip_chunk_plan(C.byref(_cfg(c)), n, chunk, sizes, cap)
    return rc, list(sizes[:max(rc, 0)]), _lib.lib().tspo_last_error().decode()


@pytest.mark.parametrize("name,c", [("clip_l14", L14), ("clip_tiny", synth.CLIP_TINY)])
def test_planner_properties(name, c):
    thr = _fold_threshold(c)
    assert thr == (64 if name == "clip_l14" else None)          # CLIP_TINY never folds: the fold clause is vacuous for it
    planned = 0
    for n in FRAMES:
        for chunk in CHUNKS:
            f = thr if _folds_closed_form(c, n) else 1
            if not _feasible(n, chunk, f):
                rc, _, msg = _plan_rc(c, n, chunk)
                assert rc == -1 and "no plan" in msg and "multiple of 64" in msg, (n, chunk, rc, msg)
                with pytest.raises(ValueError, match="no plan"):
                    ops.clip_chunk_plan(c, n, chunk)
                continue
            plan = ops.clip_chunk_plan(c, n, chunk)
            planned += 1
            assert sum(plan) == n, (n, chunk, plan)
            assert all(1 <= s <= chunk for s in plan), (n, chunk, plan)
            assert len(plan) == -(-n // chunk), (n, chunk, plan)
            assert all(s % 64 == 0 for s in plan[:-1]), (n, chunk, plan)
            folds = _lib.lib().tspo_clip_will_fold(C.byref(_cfg(c)), n)
            assert folds == int(_folds_closed_form(c, n))
            if folds:
                assert all(_lib.lib().tspo_clip_will_fold(C.byref(_cfg(c)), s) == 1 for s in set(plan)), (n, chunk, plan)
                assert min(plan) >= 64
            assert ops.clip_chunk_plan(c, n, chunk) == plan                       # a pure function of its arguments
            assert _plan_rc(c, n, chunk, cap=len(plan))[1] == plan                # ... and of nothing else (cap only bounds)
    # a chunk_frames that is a multiple of 64 and at least twice the threshold always has a plan: 3 of the 5 chunk sizes, every T
    assert planned >= 3 * len(FRAMES)
    for n in FRAMES:
        for chunk in (128, 256, 2048):
            assert _feasible(n, chunk, thr or 1)
    if name == "clip_l14":                                                         # the plans the GPU tests rely on
        assert ops.clip_chunk_plan(c, 200, 128) == [128, 72] and ops.clip_chunk_plan(c, 256, 128) == [128, 128]
        assert ops.clip_chunk_plan(ops._clip_cfg_struct(c), 64, 64) == [64]


def test_planner_rejects_bad_arguments():
    for n, chunk, cap, word in ((0, 128, 8, "n_frames=0"), (-3, 128, 8, "n_frames=-3"), (100, 0, 8, "chunk_frames=0"),
                                (100, -1, 8, "chunk_frames=-1"), (1024, 128, 7, "do not fit"), (1024, 128, 0, "do not fit")):
        rc, _, msg = _plan_rc(L14, n, chunk, cap)
        assert rc == -1 and word in msg, (n, chunk, cap, msg)
    for n in (1, 63, 64, 1000):                          # below the fold threshold: refused whatever n_frames is
        rc, _, msg = _plan_rc(L14, n, 63)
        assert rc == -1 and "chunk_frames=63 is below the 64 frames" in msg, msg
    rc, sizes, msg = _plan_rc(synth.CLIP_TINY, 100, 40)      # a config that never folds has no threshold, but the 64-frame rule holds
    assert rc == -1 and "no plan" in msg                 # 3 chunks of at most 40: no leading chunk can hold 64 frames
    assert _plan_rc(synth.CLIP_TINY, 40, 40)[:2] == (1, [40])
    l = _lib.lib()
    sizes = (C.c_int * 4)()
    assert l.tspo_clip_chunk_plan(None, 100, 128, sizes, 4) == -1 and b"null config" in l.tspo_last_error()
    assert l.tspo_clip_chunk_plan(C.byref(_cfg(L14)), 100, 128, None, 4) == -1
    with pytest.raises(ValueError, match="below the 64 frames"):
        ops.clip_chunk_plan(L14, 1024, 32)


@pytest.mark.parametrize("c,n,folds", [(dict(L14, layers=1), 63, False), (dict(L14, layers=1), 64, True),
                                       (VITB16, 110, False), (VITB16, 111, True)], ids=["l14_63", "l14_64", "vitb16_110", "vitb16_111"])
def test_will_fold_is_the_closed_form_at_the_boundaries(c, n, folds):
    l = _lib.lib()
    assert _folds_closed_form(c, n) == folds
    assert l.tspo_clip_will_fold(C.byref(_cfg(c)), n) == int(folds)
    w = ops.ClipVitWeights(synth.clip_vision_state(**c), c, "cpu")      # packing touches no GPU; library_folds asks the library
    assert w.library_folds(n) is folds
    for m in (1, n - 1, n, n + 1, 5000):
        assert l.tspo_clip_will_fold(C.byref(_cfg(c)), m) == int(_folds_closed_form(c, m))
    assert l.tspo_clip_will_fold(C.byref(_cfg(dict(c, layers=0))), 5000) == 0
    assert l.tspo_clip_will_fold(None, 64) == -1 and l.tspo_clip_will_fold(C.byref(_cfg(c)), 0) == -1


def test_chunked_forward_validates_before_touching_the_device():
    l = _lib.lib()
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    layers = (_lib.ClipLayer * 24)()
    w = _lib.ClipWeights()
    w.cfg = _cfg(L14)
    for nm in ("patch_w", "pos_emb", "pre_g", "pre_b", "post_g", "post_b", "proj_w"):
        setattr(w, nm, p)
    w.layers = C.cast(layers, C.POINTER(_lib.ClipLayer))
    call = lambda w_, px, feat, ws, nbytes, n=200, chunk=128, dtype=_lib.TSPO_U8, flags=0: \
        l.tspo_clip_vit_forward_chunked(w_, px, dtype, n, chunk, feat, ws, nbytes, None, flags)
    for args in ((None, p, p, p), (C.byref(w), None, p, p), (C.byref(w), p, None, p), (C.byref(w), p, p, None)):
        assert call(*args, 1 << 40) == -1 and b"null pointer" in l.tspo_last_error()
    need = l.tspo_clip_workspace_bytes(C.byref(w.cfg), 128)
    assert call(C.byref(w), p, p, p, need - 1) == -2                               # TSPO_EWORKSPACE: sized by the largest chunk
    assert b"workspace" in l.tspo_last_error() and b"128 frames" in l.tspo_last_error()
    assert call(C.byref(w), p, p, p, 256) == -2
    for chunk, word in ((0, b"chunk_frames=0"), (-5, b"chunk_frames=-5"), (63, b"below the 64 frames")):
        assert call(C.byref(w), p, p, p, 1 << 40, chunk=chunk) == -1 and word in l.tspo_last_error(), l.tspo_last_error()
    assert call(C.byref(w), p, p, p, 1 << 40, n=65, chunk=64) == -1 and b"no plan" in l.tspo_last_error()
    assert call(C.byref(w), p, p, p, 1 << 40, n=0) == -1
    assert call(C.byref(w), p, p, p, 1 << 40, dtype=9) == -1 and b"pixel_dtype" in l.tspo_last_error()
    assert call(C.byref(w), p, p, p, 1 << 40, flags=8) == -1 and b"unknown flags" in l.tspo_last_error()


def test_workspace_of_a_50000_frame_video_in_chunks_is_below_one_4096_frame_encode():
    l = _lib.lib()
    cfg = _cfg(L14)
    plan = ops.clip_chunk_plan(L14, 50_000, 2048)
    assert len(plan) == 25 and max(plan) == 2048 and min(plan) >= 64
    chunked = l.tspo_clip_workspace_bytes(C.byref(cfg), max(plan))
    assert 0 < chunked < l.tspo_clip_workspace_bytes(C.byref(cfg), 4096) < l.tspo_clip_workspace_bytes(C.byref(cfg), 50_000)
