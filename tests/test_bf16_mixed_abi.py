"""TSPO_SEL_BF16_MIXED - the reference's bf16 training precision (bf16 GEMM operands, fp32 accumulation, forward AND backward) - on
the CPU: the option word and the capability query of the C ABI, the Python mapping, the host-side guards of PolicyTrainer, the CPU
emulation the GPU tests rely on (tests/_bf16_mixed.py) and the reference's own bf16-vs-fp32 noise fixture."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import _bf16_mixed as BM
from inputs import SELECTOR_CASES, TRAIN_FULL_CASES, selector_inputs
from oracle import tspo_oracle as O
from tspo_amd import _lib, ops, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defs():
    hdr = open(os.path.join(ROOT, "include", "tspo_hip.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(TSPO_[A-Z0-9_]+)\s+(\d+|0x[0-9a-fA-F]+)\s*$", hdr, flags=re.M)}


def test_header_defines_bf16_mixed_and_binding_agrees():
    d = _defs()
    assert d["TSPO_SEL_BF16_MIXED"] == ops.SEL_BF16_MIXED == 8
    assert len({ops.SEL_BF16X3, ops.SEL_ACCUMULATE, ops.SEL_BF16, ops.SEL_BF16_MIXED}) == 4
    assert "int tspo_selector_supported_flags(int entry);" in open(os.path.join(ROOT, "include", "tspo_hip.h")).read()
    assert "tspo_selector_supported_flags" in _lib.SIGNATURES


def test_supported_flags_query():
    """entry 0 = tspo_selector_forward_ex, 1 = tspo_selector_backward_ex, 2 = tspo_policy_backward(_ex); host only (this runs without a
    device)."""
    L = _lib.lib()
    d = _defs()
    bx3, acc, b16, mix = d["TSPO_SEL_BF16X3"], d["TSPO_SEL_ACCUMULATE"], d["TSPO_SEL_BF16"], d["TSPO_SEL_BF16_MIXED"]
    assert L.tspo_selector_supported_flags(0) == bx3 | b16 | mix == 13
    assert L.tspo_selector_supported_flags(1) == bx3 | acc | mix == 11
    assert L.tspo_selector_supported_flags(2) == bx3 | acc | mix == 11
    for bad in (-1, 3, 1 << 20):
        assert L.tspo_selector_supported_flags(bad) == -1
        assert b"entry" in L.tspo_last_error()


def test_sel_flags_bf16_mixed():
    assert ops._sel_flags("bf16_mixed") == ops.SEL_BF16_MIXED
    assert ops._sel_flags("bf16_mixed", forward=True) == ops.SEL_BF16_MIXED
    assert ops._sel_flags("bf16_mixed", accumulate=True) == ops.SEL_BF16_MIXED | ops.SEL_ACCUMULATE
    with pytest.raises(ValueError):
        ops._sel_flags("bf16")                      # still forward-only
    with pytest.raises(ValueError):
        ops._sel_flags("bf16", accumulate=True)
    with pytest.raises(ValueError):
        ops._sel_flags("bf16-mixed")


def test_flag_combinations_rejected_on_the_host():
    """bf16_mixed is exclusive with bf16x3 (backward) and with bf16 / bf16x3 (forward): TSPO_EINVAL with an 'exclusive' message
    before any launch.  Unknown bits are refused as before."""
    L = _lib.lib()
    w, g = _lib.SelectorWeights(), _lib.SelectorGrads()
    p = C.c_void_p(16)     # never dereferenced: flag validation comes first
    for fl in (8 | 1, 8 | 4, 8 | 4 | 1):
        rc = L.tspo_selector_forward_ex(C.byref(w), p, p, None, 1, 8, 64, 8, 1, 4, 0.025, p, None, p, 1 << 30, None, fl)
        assert rc == -1 and b"exclusive" in L.tspo_last_error(), (fl, L.tspo_last_error())
    rc = L.tspo_selector_backward_ex(C.byref(w), p, p, p, 1, 8, 64, 8, 1, 4, 0.025, C.byref(g), p, 1 << 30, None, 8 | 1)
    assert rc == -1 and b"exclusive" in L.tspo_last_error()
    rc = L.tspo_selector_backward_ex(C.byref(w), p, p, p, 1, 8, 64, 8, 1, 4, 0.025, C.byref(g), p, 1 << 30, None, 4)
    assert rc == -1 and b"unknown flags" in L.tspo_last_error()


def test_policy_trainer_records_and_guards_precision():
    from tspo_amd.pipeline import PolicyTrainer, RolloutContext
    D = 64
    flat = torch.zeros(ops.flat_offsets(D)["__total__"][0])
    tr = PolicyTrainer(flat, dim=D, heads=8, window_size=4, gemm_precision="bf16_mixed")
    assert tr.gemm_precision == "bf16_mixed"
    with pytest.raises(ValueError):
        PolicyTrainer(flat, dim=D, heads=8, window_size=4, gemm_precision="bf16")
    feats, txt = torch.zeros(1, 8, D), torch.zeros(1, 1, D)
    idx = torch.zeros(1, 2, 2, dtype=torch.int64)
    ctx = RolloutContext(torch.zeros(16, dtype=torch.uint8), (1, 8, D), 1, 0.025, tr._param_version, 0, tr, idx, 1,
                         precision="bf16_mixed")
    tr.gemm_precision = "fp32"     # changed between rollout() and backward()
    with pytest.raises(RuntimeError, match="gemm_precision"):
        tr.backward(ctx, feats, txt, torch.zeros(1, 8), idx, torch.zeros(1, 2))
    assert not ctx.consumed and tr._micro == 0
    assert RolloutContext(None, (1, 8, D), 1, 0.025, 0, 0, tr).precision == "fp32"


def test_multimodal_align_training_precision_attribute():
    import inspect
    from tspo_amd.temporal_agent import MultiModal_Align
    m = MultiModal_Align(dim=64, num_heads=8)
    assert m.training_gemm_precision == "fp32" and m.inference_gemm_precision == "fp32"
    assert "training_gemm_precision" not in inspect.signature(MultiModal_Align.__init__).parameters


def test_train_config_takes_bf16_mixed():
    from tspo_amd import train
    cfg = train.TrainConfig(gemm_precision="bf16_mixed")
    assert cfg.gemm_precision == "bf16_mixed"


@pytest.mark.parametrize("case", [c for c in SELECTOR_CASES if c[0] in ("s32", "s40m3")], ids=lambda c: c[0])
def test_emulation_without_rounding_is_the_oracle(case):
    """The explicit-GEMM emulation of tests/_bf16_mixed.py with the rounding switched OFF equals the oracle's autograd (dense window
    mask, oracle.selector_forward) to fp32 tolerance: the emulation's structure - which operand of which GEMM, the ReLU mask,
    the fp32 bias column sums, the banded attention - is the oracle's; the GPU tests then only switch the rounding on."""
    name, T, D, H, w, tau, M, ks = case
    img, txt, clip, state = selector_inputs(name, T, D, M)
    B = 2
    img2 = torch.stack([torch.from_numpy(img), torch.from_numpy(img[::-1].copy())])
    txt2 = torch.stack([torch.from_numpy(txt)] * B)
    clip2 = torch.stack([torch.from_numpy(clip)] * B)
    ds = torch.from_numpy(synth.normal((B, T), 777, 0.05))
    params = {n: torch.from_numpy(v) for n, v in state.items()}
    s_em, g_em = BM.forward_backward(params, img2, txt2, clip2, ds, H, w, tau, rounding=False)
    s_or, g_or = BM.oracle_autograd(params, img2, txt2, clip2, ds, H, w, tau)
    np.testing.assert_allclose(s_em.numpy(), s_or.numpy(), rtol=1e-5, atol=1e-4)
    qb = np.abs(g_or["temporal.Self_q.bias"].numpy()).max()
    for n in BM.TRAINED:
        ref = g_or[n].numpy()
        if n == "temporal.Self_k.bias":   # mathematically zero (softmax is shift-invariant per query): both sides hold rounding noise
            assert np.abs(g_em[n].numpy()).max() <= 1e-4 * qb and np.abs(ref).max() <= 1e-4 * qb
            continue
        tol = 5e-5 * max(np.abs(ref).max(), 1e-6)
        np.testing.assert_allclose(g_em[n].numpy(), ref, rtol=1e-4, atol=tol, err_msg=n)
    # with the rounding ON it is a different computation (the GPU tests need this to discriminate)
    _, g_r = BM.forward_backward(params, img2, txt2, clip2, ds, H, w, tau, rounding=True)
    assert BM.rel_fro(g_r["mlp.0.weight"].numpy(), g_or["mlp.0.weight"].numpy()) > 1e-4


def test_bf16_train_noise_fixture_complete():
    """tests/golden/bf16_train_noise.json (make_golden_bf16_train.py: the reference's module in bf16 vs fp32 with the indices of
    train_full.npz) holds both timed cases and every trained tensor."""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "bf16_train_noise.json")))
    for name, B, T, D, H, w, tau, k, G in TRAIN_FULL_CASES:
        c = fx["cases"][name]
        assert c["index_sets"] == B * G and 0 <= c["changed_index_sets"] <= B * G
        for key in ("rel_fro", "rel_max"):
            assert sorted(c[key]) == sorted(BM.TRAINED), (name, key)
            for pn, v in c[key].items():
                assert np.isfinite(v) and v > 0, (name, key, pn)
        # the reference's bf16 step is far from exact: the bound the GPU tests use is not vacuous
        assert 1e-3 < c["rel_fro"]["mlp.0.weight"] < 1.0
