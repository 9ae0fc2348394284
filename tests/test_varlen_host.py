"""Videos of different lengths in one padded batch - what can be checked without a GPU: the five `_len` entries are declared,
bound and exported; the library and the wrappers reject a bad `min_length` / `lengths` before any device work; `train._pad_stack`
on CPU tensors; and every default is what it was (the feature is opt-in)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN_ENTRIES = ("tspo_selector_forward_len", "tspo_selector_backward_len", "tspo_policy_backward_len", "tspo_gumbel_topk_len",
               "tspo_grpo_pg_grad_len")


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from tspo_amd import _lib
    return _lib, _lib.lib()


def test_len_entries_in_header_binding_and_library():
    L, l = _lib()
    hdr = open(os.path.join(ROOT, "include", "tspo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in LEN_ENTRIES:
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S)
        assert m, f"{name} is not declared in tspo_hip.h"
        assert re.search(r"const int32_t\*\s*lengths,\s*int min_length\s*$", m.group(1).strip()), f"{name}: the last two parameters"
        assert name in L.SIGNATURES and hasattr(l, name)
        base = name[:-4] + "_ex" if name != "tspo_grpo_pg_grad_len" else "tspo_grpo_pg_grad"
        assert L.SIGNATURES[name][1] == L.SIGNATURES[base][1] + [ctypes.c_void_p, ctypes.c_int], f"{name} = {base} + (lengths, min_length)"
    assert l.tspo_version() == 4                        # discovered by symbol lookup, not by a version bump


def test_library_validates_min_length_before_any_device_work():
    """No GPU here: a call that touched the device would fail differently (or crash on the fake pointers)."""
    L, l = _lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    T, k = 16, 4
    gumbel = lambda kk, ml, lengths=p: l.tspo_gumbel_topk_len(p, None, 0, 0, 1, 2, T, kk, 1.0, p, None, None, None, None, 0, lengths, ml)
    for ml in (0, -3, T + 1):
        assert gumbel(k, ml) == -1 and b"min_length" in l.tspo_last_error(), ml
    assert gumbel(k, k - 1) == -1                       # k > min_length: fewer frames than a rollout selects
    assert b"out of range" in l.tspo_last_error() and b"min_length" in l.tspo_last_error()
    assert gumbel(T + 1, T, None) == -1 and b"out of range" in l.tspo_last_error()      # lengths == NULL: the rule of the _ex entry
    w, g = L.SelectorWeights(), L.SelectorGrads()
    for ml in (0, T + 1):
        assert l.tspo_grpo_pg_grad_len(p, p, p, 1, 2, T, k, 1e-4, 1.0, p, p, None, None, p, ml) == -1
        assert b"min_length" in l.tspo_last_error()
        assert l.tspo_selector_forward_len(ctypes.byref(w), p, p, None, 1, T, 64, 8, 1, 12, 0.025, p, None, p, 1 << 30, None, 0, p, ml) == -1
        assert b"min_length" in l.tspo_last_error()
        assert l.tspo_selector_backward_len(ctypes.byref(w), p, p, p, 1, T, 64, 8, 1, 12, 0.025, ctypes.byref(g), p, 1 << 30, None, 0,
                                            p, ml) == -1
        assert b"min_length" in l.tspo_last_error()
        assert l.tspo_policy_backward_len(ctypes.byref(w), p, p, p, p, p, 1, T, 64, 8, 1, 12, 0.025, 2, k, 1e-4, 1.0, ctypes.byref(g),
                                          p, None, p, 1 << 30, None, 0, None, None, p, ml) == -1
        assert b"min_length" in l.tspo_last_error()
    # lengths == NULL: min_length is not looked at, the call goes on to the checks of the _ex entry (null weight pointers here)
    assert l.tspo_selector_forward_len(ctypes.byref(w), p, p, None, 1, T, 64, 8, 1, 12, 0.025, p, None, p, 1 << 30, None, 0, None, 0) == -1
    assert b"null weight pointer" in l.tspo_last_error()


def test_wrappers_validate_lengths_on_the_host():
    from tspo_amd import _lib as L, ops
    arg = lambda *a, **k: ops._lengths_arg(*a, device="cpu", what="t", **k)
    assert arg(None, None, 2, 8) == (None, 0)
    ln, ml = arg([8, 3], None, 2, 8)
    assert ln.dtype == torch.int32 and ln.tolist() == [8, 3] and ml == 3
    assert arg((5, 7), 2, 2, 8)[1] == 2                 # a caller may vouch for less than the minimum
    assert arg(torch.tensor([4, 6]), None, 2, 8)[1] == 4   # a host tensor is a host sequence
    for bad, mlen in (([0, 3], None), ([9, 3], None), ([3], None), ([4, 6], 5), ([4, 6], 0)):
        with pytest.raises(ValueError):
            arg(bad, mlen, 2, 8)
    with pytest.raises(ValueError, match="min_length without lengths"):
        arg(None, 3, 2, 8)
    with pytest.raises(RuntimeError, match="out of range"):
        arg([8, 3], None, 2, 8, k=4)
    # the ops themselves still refuse CPU tensors first (no CPU path), with or without lengths
    with pytest.raises(L.TspoHipError):
        ops.gumbel_topk(torch.zeros(2, 8), 2, lengths=[8, 3])


def _batch(tt, T, item, D=4, typ="specific", M=1):
    g = torch.Generator().manual_seed(item)
    return tt.Batch(torch.randn(1, T, D, generator=g), torch.randn(1, M, D, generator=g), torch.randn(1, T, generator=g),
                    torch.ones(1, T, dtype=torch.bool), typ, [{"item": item}], frames=[(f"pool{item}", f"plan{item}")])


def test_pad_stack_on_cpu_tensors():
    from tspo_amd import train as tt
    window = [_batch(tt, T, i) for i, T in enumerate((5, 9, 3))]
    assert not tt._stackable(window) and tt._paddable(window)
    p = tt._pad_stack(window)
    assert p.feats.shape == (3, 9, 4) and p.clip.shape == (3, 9) and p.mask.shape == (3, 9) and p.txt.shape == (3, 1, 4)
    assert p.lengths == [5, 9, 3] and p.item_type == "specific"
    assert [m["item"] for m in p.meta] == [0, 1, 2] and p.frames == [("pool0", "plan0"), ("pool1", "plan1"), ("pool2", "plan2")]
    for b, (src, L) in enumerate(zip(window, p.lengths)):
        assert torch.equal(p.feats[b, :L], src.feats[0]) and torch.equal(p.clip[b, :L], src.clip[0]) and torch.equal(p.txt[b], src.txt[0])
        assert bool(p.mask[b, :L].all()) and not bool(p.mask[b, L:].any())
        assert not bool(p.feats[b, L:].any()) and not bool(p.clip[b, L:].any())       # zero padding
    # a padded batch pads again (a window of padded micro-batches) and keeps the true lengths
    q = tt._pad_stack([tt._pad_stack(window[:2]), tt._pad_stack([window[2], window[0]])])
    assert q.feats.shape == (4, 9, 4) and q.lengths == [5, 9, 3, 5] and [m["item"] for m in q.meta] == [0, 1, 2, 0]
    assert not bool(q.feats[2, 3:].any()) and torch.equal(q.feats[3, :5], window[0].feats[0])
    # batches without frames: frames stays None; what does not pad together is refused
    bare = [tt.Batch(b.feats, b.txt, b.clip, b.mask, b.item_type) for b in window]
    assert tt._pad_stack(bare).frames is None
    for other in (_batch(tt, 5, 7, typ="general"), _batch(tt, 5, 7, M=2), _batch(tt, 5, 7, D=8)):
        assert not tt._paddable([window[0], other])
        with pytest.raises(ValueError):
            tt._pad_stack([window[0], other])
    with pytest.raises(ValueError):
        tt.Batch(window[0].feats, window[0].txt, window[0].clip, window[0].mask, lengths=[6])      # longer than T


def test_defaults_are_unchanged(capsys):
    import inspect
    from tspo_amd import ops, train as tt
    from tspo_amd.pipeline import PolicyTrainer
    from tspo_amd.temporal_agent import MultiModal_Align
    assert tt.TrainConfig().pad_variable_length is False
    assert inspect.signature(tt.FrameDataset.__init__).parameters["pad_batches"].default is False
    b = _batch(tt, 5, 0)
    assert b.lengths is None and tt._stackable([b, _batch(tt, 5, 1)])
    for fn in (ops.selector_forward, ops.selector_backward, ops.policy_backward, ops.gumbel_topk, ops.grpo_pg_grad,
               PolicyTrainer.rollout, PolicyTrainer.step, MultiModal_Align.forward_batched):
        ps = inspect.signature(fn).parameters
        assert ps["lengths"].default is None and ps["min_length"].default is None, fn
    ds = object.__new__(tt.FrameDataset)                # (as tests/test_select_frames.py does)
    with pytest.raises(ValueError, match="one prompt per micro-batch"):
        next(ds.batches(0, 1, 2))
    with pytest.raises(SystemExit):                     # the flag exists on the command line
        tt.main(["--help"])
    assert "--pad-variable-length" in capsys.readouterr().out
