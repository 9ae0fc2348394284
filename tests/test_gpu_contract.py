"""The boundary contract of include/tspo_hip.h, asserted: every entry point launches only on the stream it is given, never
synchronises, never allocates, keeps no state between calls and is re-entrant across host threads with a thread-local
tspo_last_error().  (tools/bench_graph.py times a captured step; these tests assert.)

One table of cases (tests/_contract.py) is driven three ways, and every result must be BIT-IDENTICAL to the same case run eagerly
on the default stream with the same inputs:
  Part A  on a non-blocking side stream, behind a delay, with every live buffer poisoned until the ordered copy-in: a launch that
          went to the null stream (idle, not ordered after the side stream) or a host-side wait runs on poison;
  Part B  captured into a graph on one stream and replayed three times on three sets of inputs: a launch to the legacy stream, a
          synchronisation or an allocation by the library is an error at capture time;
  Part C  from two host threads at once, each on its own stream with its own objects.
The eager twin itself is held against the op's independent reference at the tolerance of the op's existing test
(test_eager_twin_against_the_independent_reference; each borrowed tolerance is named where it is used in _contract.py).

Entry points of include/tspo_hip.h that launch work, their internally different paths, and the case that reaches each
(tspo_clip_vit_profile is excluded: documented as the one entry that waits):
  tspo_topk_sorted            LDS-resident keys                       topk_sorted-B3-T777-k33
                              global-key path (T > 16384)             topk_sorted-B2-T16385-k64
  tspo_binmax                 both row lengths                        binmax-B3-T777-k33, binmax-B2-T16385-k64
  tspo_gumbel_topk(_ex)       injected noise + probs                  gumbel_topk-injected-T777-k33
                              in-kernel Philox + noise_out            gumbel_topk-philox-T777-k33
                              long rows (global keys)                 gumbel_topk-long-T16385-k48
                              prompts_per_offset = 1                  gumbel_topk-prompts_per_offset1
  tspo_grpo_advantage / tspo_pg_grad_logits / tspo_grpo_pg_grad       grpo_advantage, pg_grad_logits, grpo_pg_grad (B3 G8 T700 k16)
  tspo_selector_forward(_ex)  fp32 / bf16x3 / bf16_mixed / bf16, with temporal_attn (its device-to-device copy)
  tspo_selector_backward(_ex) fp32 / bf16x3 / bf16_mixed              selector-T96-D128-<precision> (B2 M2),
                              small-M forms + merged D % 384 launches selector-T300-D768-<precision> (B1 M1), ...-bf16-fwd
                              TSPO_SEL_ACCUMULATE                     selector-T96-D128-fp32-accumulate
  tspo_policy_backward        ballot path (G k <= 256)                policy_backward-G8-k16
                              binary search                           policy_backward-G3-k100
  tspo_policy_backward_ex + tspo_adamw_clip_step_ex                   policy_backward-G8-k16-norm_partials-adamw_clip_step
  tspo_grad_norm_scale + tspo_adamw_step, tspo_adamw_clip_step        grad_norm_scale+adamw_step-n*, adamw_clip_step-n*  (n = 100003,
                                                                      and 1003: the ragged tail)
  tspo_clip_scores                                                    clip_scores
  tspo_clip_vit_forward(_ex)  small batch, no fold                    clip_vit_forward-n3
                              fold, persistent GEMM + remainder phase, then TSPO_CLIP_FOLD_CACHED   clip_vit_forward-n70-fold-twice
                              TSPO_CLIP_NO_LN_FOLD                    clip_vit_forward-n70-nofold
                              TSPO_CLIP_PRUNE_LAST (the 2-D copy of the class-token rows)   clip_vit_forward-n70-prune_last
  tspo_clip_vit_forward_chunked   192 frames in chunks of 128         clip_vit_forward-chunked-n192-c128
  tspo_preprocess_select (what preprocess_frames and select_frames call; tspo_preprocess_frames(_ex) are its index == NULL, uint8 form)
                              matrix pass / LDS pass                  preprocess_frames-240x320-matrix, ...-lds
                              byte-granular kernels (out_w % 4)       preprocess_frames-97x131-bytes
                              device index (repeats, descending), uint8 / f32 / bf16 / f16 epilogues   select_frames-<dtype>
                              oob_flag with one out-of-range index    select_frames-oob_flag
  tspo_gemm_bf16              kernels 1, 77, 83; with the in-place residual   gemm_bf16-k<1|77|83>[-residual-in-place]
Composed: FrameScorer.__call__ and PolicyTrainer.step captured whole (Part B); the fold cache across streams (Part A)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import _contract as K
from _contract import CASES, DEV
from tspo_amd import _lib, ops, preprocess as P
from tspo_amd.pipeline import FrameScorer, PolicyTrainer

pytestmark = pytest.mark.gpu
NAMES = list(CASES)
SEEDS = (1, 2, 3)


# What the delay in front of the work under test must outlast: the HOST-side time of the longest case to issue all its launches -
# two 1-layer encodes of 70 frames, some 60 launches through ctypes at ~10 us each, well under 2 ms once the kernels are loaded
# (every case is warmed up first).  Six chained 8192^3 fp32 matmuls are 6.6 TFLOP: >= 40 ms at the card's fp32 matrix peak
# (157 TFLOP/s), twenty times the launch time.  Until it ends nothing ordered on the side stream has run: the live buffers hold
# poison, and a kernel that was sent anywhere else runs on it.
_DELAY = {}


def _delay_buffers():
    """Set-up, outside every region under test: the operands, and the first use of the BLAS library."""
    if not _DELAY:
        _DELAY["a"] = torch.randn(8192, 8192, device=DEV) * 0.01
        _DELAY["b"], _DELAY["c"] = torch.empty_like(_DELAY["a"]), torch.empty_like(_DELAY["a"])
        torch.mm(_DELAY["a"][:256, :256], _DELAY["a"][:256, :256], out=_DELAY["b"][:256, :256].contiguous())
        torch.cuda.synchronize()
    return _DELAY["a"], _DELAY["b"], _DELAY["c"]


def _delay():
    a, b, c = _delay_buffers()
    for _ in range(3):
        torch.mm(a, a, out=b)
        torch.mm(a, b, out=c)


@pytest.mark.parametrize("name", NAMES)
def test_eager_twin_against_the_independent_reference(name):
    case = CASES[name]
    out = K.eager(case, 0, fresh=True)
    case.check(case.real(0), out)


# --------------------------------------------------------------------------------------------------------------------- Part A
@pytest.mark.parametrize("name", NAMES)
def test_side_stream_behind_a_delay_on_poisoned_buffers(name):
    case = CASES[name]
    want = K.eager(case, 0)
    inst = K.Inst(case)
    _delay_buffers()
    S = torch.cuda.Stream()                       # non-blocking: the null stream does not wait for it
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        # Warm-up on S with the SAME sequence of allocations as the run under test (the delay first: the BLAS library may take
        # a workspace for this stream) but on the inputs of ANOTHER seed: code objects get loaded, S's allocator pool is filled,
        # and whatever stays behind in memory that poison() cannot reach - a wrapper's internal workspace, such as the one
        # select_frames keeps between its two passes - is wrong for the inputs of the run under test.
        _delay()
        inst.load(K.POISON_SEED)
        out = inst.run()
        S.synchronize()
        for t in out.values():                    # the output blocks go back to S's pool holding poison; the run under test, which
            K.poison_tensor(t)                    # allocates the same sizes in the same order from that pool, gets them again
        del out, t
        inst.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        _delay()
        inst.load(0)                              # the real inputs arrive as part of the ordered work
        got = inst.run()
    S.synchronize()                               # nothing was launched on the default stream meanwhile
    K.assert_same(got, want, f"{name} on a side stream")


def test_fold_cache_across_streams():
    """ops._fold_key names the stream: an encode on another stream must fold again (the fold written on the first stream is not
    ordered before it), the next one on that stream is cached, and all of them give the same bits."""
    W = K.new_clip_weights(70)
    px = K.randu8((70, 3, 224, 224), K.gen_(41))
    S = torch.cuda.Stream()
    f0 = ops.clip_vit_forward(W, px).clone()
    assert W._fold_key is not None and W._fold_key[2] == torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        f1 = ops.clip_vit_forward(W, px).clone()
        assert W._fold_key[2] == S.cuda_stream, "after an encode on S the fold key must name S"
        f2 = ops.clip_vit_forward(W, px).clone()
    S.synchronize()
    f3 = ops.clip_vit_forward(W, px).clone()
    torch.cuda.synchronize()
    for i, f in enumerate((f1, f2, f3), 1):
        assert K.bits_equal(f, f0), f"encode {i} differs from the first one"


# --------------------------------------------------------------------------------------------------------------------- Part B
def _warm_up_on_side_stream(fn):
    """As tools/bench_graph.py does before it captures."""
    S = torch.cuda.Stream()
    S.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(S):
        fn()
    torch.cuda.current_stream().wait_stream(S)
    torch.cuda.synchronize()
    return S


@pytest.mark.parametrize("name", NAMES)
def test_graph_capture_and_three_replays(name):
    case = CASES[name]
    want = {s: K.eager(case, s) for s in SEEDS}
    inst = K.Inst(case)
    S = _warm_up_on_side_stream(inst.run)
    inst.load(0)
    inst.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):       # one stream, no fork / join inside
        out = inst.run()
    for s in SEEDS:
        inst.poison()                             # live inputs, in-place state, workspaces ...
        for t in out.values():                    # ... and the static outputs
            K.poison_tensor(t)
        inst.load(s)                              # this replay's inputs; in-place state back to its pre-call values
        graph.replay()
        torch.cuda.synchronize()
        K.assert_same(out, want[s], f"{name}, replay on the inputs of seed {s}")
    del graph


def _poison_all(ts):
    for t in ts:
        if t is not None:
            K.poison_tensor(t)


def test_graph_frame_scorer_call():
    """FrameScorer.__call__ (encode -> clip score -> selector -> top-k) as ONE graph: 1-layer CLIP-L/14, T = 70, k = 8, fp32 selector."""
    T, k, D = 70, 8, 768
    W = K.new_clip_weights(T)
    flat = K.randn((ops.flat_offsets(D)["__total__"][0],), K.gen_(50), 0.5 / np.sqrt(D))
    scorer = FrameScorer(W, flat, selector_precision="fp32")
    real = {s: (K.randu8((1, T, 3, 224, 224), K.gen_(60 + s)), K.randn((1, 1, D), K.gen_(70 + s))) for s in (0,) + SEEDS}
    px, txt = real[0][0].clone(), real[0][1].clone()
    names = ("idx", "scores", "feats")
    want = {}
    for s in SEEDS:
        px.copy_(real[s][0]); txt.copy_(real[s][1])
        want[s] = {n: v.clone() for n, v in zip(names, scorer(px, txt, k))}
    S = _warm_up_on_side_stream(lambda: scorer(px, txt, k))
    W.invalidate_fold_cache()                     # the captured call folds: the replays start from a poisoned workspace
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        out = dict(zip(names, scorer(px, txt, k)))
    for s in SEEDS:
        _poison_all([px, txt, W._ws, scorer._sel_ws] + list(out.values()))
        px.copy_(real[s][0]); txt.copy_(real[s][1])
        graph.replay()
        torch.cuda.synchronize()
        K.assert_same(out, want[s], f"FrameScorer replay, seed {s}")


@pytest.mark.parametrize("precision", ["fp32", "bf16_mixed"])
def test_graph_policy_trainer_step(precision):
    """PolicyTrainer.step as ONE graph.  The host scalars of a step are kernel ARGUMENTS and so are baked into the graph at capture:
    the Philox offset (`_rollouts`), the AdamW step number and the learning rate.  A replay therefore repeats the step with the
    capture-time scalars on whatever the static buffers hold; its eager twin is a SECOND trainer built from the same initial state
    whose `_rollouts` and `step_no` are put back to their capture-time values before each call."""
    B, T, D, G, k, tau = 2, 96, 128, 8, 16, 0.05
    g = K.gen_(80)
    tot = ops.flat_offsets(D)["__total__"][0]
    flat0, m0, v0 = K.randn((tot,), g, 0.5 / np.sqrt(D)), K.randn((tot,), g, 1e-3), K.rand((tot,), g) * 1e-6
    table = K.rand((T,), g)
    reward_fn = lambda idx: table[idx].mean(-1)             # a pure device function of idx: [B,G,k] -> [B,G]
    real = {s: (K.randn((B, T, D), K.gen_(90 + s)), K.randn((B, 1, D), K.gen_(100 + s)), K.randn((B, T), K.gen_(110 + s), 0.1))
            for s in (0,) + SEEDS}
    keys = ("scores", "idx", "loss", "advantages")

    def trainer():
        tr = PolicyTrainer(flat0.clone(), dim=D, heads=8, window_size=12, gemm_precision=precision)
        return tr

    def restore(tr):
        tr.flat.copy_(flat0); tr.m.copy_(m0); tr.v.copy_(v0); tr.grad.zero_()
        tr._rollouts, tr.step_no = 0, 0                      # the capture-time values

    twin, want = trainer(), {}
    for s in SEEDS:
        restore(twin)
        st = twin.step(*real[s], reward_fn, G, k, tau)
        want[s] = {n: st[n].clone() for n in keys}
        want[s].update(flat=twin.flat.clone(), m=twin.m.clone(), v=twin.v.clone())
    tr = trainer()
    img, txt, clip = (t.clone() for t in real[0])
    restore(tr)
    S = _warm_up_on_side_stream(lambda: tr.step(img, txt, clip, reward_fn, G, k, tau))
    restore(tr)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=S):
        st = tr.step(img, txt, clip, reward_fn, G, k, tau)
    out = {n: st[n] for n in keys}
    out.update(flat=tr.flat, m=tr.m, v=tr.v)
    for s in SEEDS:
        _poison_all([img, txt, clip, tr._norm_part, tr._norm_out] + tr._ws_pool + [st[n] for n in keys])
        for dst, src in zip((img, txt, clip), real[s]):
            dst.copy_(src)
        tr.flat.copy_(flat0); tr.m.copy_(m0); tr.v.copy_(v0); tr.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        K.assert_same(out, want[s], f"PolicyTrainer.step ({precision}) replay, seed {s}")


# --------------------------------------------------------------------------------------------------------------------- Part C
ROUNDS = 12
FAIL_AT = {2: "gumbel", 5: "window", 9: "gumbel", 10: "window"}


class _ThreadCtx:
    """Everything one thread owns: weights, scorer, trainer, workspaces and inputs, from its own seed."""

    def __init__(self, seed):
        g = K.gen_(200 + seed)
        self.seed = seed
        self.W = K.new_clip_weights(70)
        self.scorer = FrameScorer(self.W, K.randn((ops.flat_offsets(768)["__total__"][0],), g, 0.5 / np.sqrt(768)))
        self.px = [K.randu8((70, 3, 224, 224), g) for _ in range(2)]
        self.txt = K.randn((1, 1, 768), g)
        D = 128
        self.trainer = PolicyTrainer(K.randn((ops.flat_offsets(D)["__total__"][0],), g, 0.5 / np.sqrt(D)), dim=D, seed=seed)
        self.img, self.txt2, self.clip = K.randn((2, 96, D), g), K.randn((2, 1, D), g), K.randn((2, 96), g, 0.1)
        table = K.rand((96,), g)
        self.reward_fn = lambda idx: table[idx].mean(-1)
        # select_frames on a different geometry per thread (both tap tables are uploaded by the runs that go first, alone)
        if seed % 2:
            self.pool, self.spec = K.randu8((4, 97, 131, 3), g), P.PreprocessSpec(out_dtype=torch.float32, **K.SPEC_BYTES)
        else:
            self.pool, self.spec = K.randu8((4, 240, 320, 3), g), P.PreprocessSpec.clip_default(out_dtype=torch.bfloat16)
        self.index = torch.tensor([3, 3, 1, 0, 2], device=DEV)
        # for the calls that only exist in the threaded run
        self.sel_ws = ops.selector_workspace(2, 96, D, 8, 1, 12, DEV)
        self.small = torch.zeros(2 * 3 * 97, dtype=torch.int64, device=DEV)
        self.rew, self.adv, self.sc = K.rand((2, 8), g), torch.zeros(2, 8, device=DEV), torch.zeros(2, 96, device=DEV)
        torch.cuda.synchronize()


def _sequence(c, hook=None):
    res = []
    for r in range(ROUNDS):
        feats = c.scorer.encode(c.px[r % 2])
        scores, clip = c.scorer.score(feats[None], c.txt)
        ro = ops.gumbel_topk(scores, 8, 4, seed=c.seed, offset=r)
        st = c.trainer.step(c.img, c.txt2, c.clip, c.reward_fn, 8, 16, 0.05)      # selector forward, rollouts, policy_backward_ex,
        sel = P.select_frames(c.pool, c.index, c.spec)                             # adamw_clip_step_ex
        res.append({"feats": feats, "clip": clip, "scores": scores, "idx": ro["idx"], "logp": ro["logp"], "t.scores": st["scores"],
                    "t.idx": st["idx"], "t.loss": st["loss"], "t.adv": st["advantages"], "t.flat": c.trainer.flat.clone(),
                    "t.norm": st["grad_norm_scale"].clone(), "sel": sel})
        if hook is not None and r in FAIL_AT:
            hook(c, FAIL_AT[r])
    return res


def _failing_call(c, kind):
    """An argument-validation failure: TSPO_EINVAL before any device work."""
    lib, st = _lib.lib(), ops._stream()
    if kind == "gumbel":                                    # k > T
        rc = lib.tspo_gumbel_topk(ops._ptr(c.clip), None, 1, 0, 2, 3, 96, 97, 1.0, ops._ptr(c.small), None, None, None, st)
    else:                                                   # window 0
        w = ops._sel_structs(c.trainer.flat, 128, _lib.SelectorWeights)
        rc = lib.tspo_selector_forward_ex(C.byref(w), ops._ptr(c.img), ops._ptr(c.txt2), None, 2, 96, 128, 8, 1, 0, 0.05,
                                          ops._ptr(c.sc), None, ops._ptr(c.sel_ws), c.sel_ws.numel(), st, 0)
    assert rc == -1, f"{kind}: expected TSPO_EINVAL (-1), got {rc}"
    return lib.tspo_last_error()


def test_two_host_threads():
    alone = []
    for seed in (0, 1):                                     # the same sequences, alone, on the default stream
        alone.append([{k: v.clone() for k, v in d.items()} for d in _sequence(_ThreadCtx(seed))])
        torch.cuda.synchronize()
    ctxs = [_ThreadCtx(0), _ThreadCtx(1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2, timeout=60)
    got, errs, seen = [None, None], [None, None], []

    def hook_failing(c, kind):
        msg = _failing_call(c, kind)
        assert msg and (kind != "window" or b"window" in msg), msg
        barrier.wait()                                      # the other thread now makes a successful call and reads ITS last error
        barrier.wait()
        assert _lib.lib().tspo_last_error() == msg, "tspo_last_error() of the failing thread changed under it"
        seen.append(("mine", kind, msg))

    def hook_succeeding(c, kind):
        barrier.wait()
        rc = _lib.lib().tspo_grpo_advantage(ops._ptr(c.rew), 2, 8, 1e-4, ops._ptr(c.adv), ops._stream())
        assert rc == 0
        seen.append(("other", kind, _lib.lib().tspo_last_error()))
        barrier.wait()

    def body(i):
        try:
            with torch.cuda.stream(streams[i]):             # the current stream is thread-local: entered inside the thread
                out = _sequence(ctxs[i], (hook_failing, hook_succeeding)[i])
                got[i] = [{k: v.clone() for k, v in d.items()} for d in out]
            streams[i].synchronize()
        except BaseException as e:                          # noqa: BLE001 - re-raised in the test
            errs[i] = e
            barrier.abort()

    threads = [threading.Thread(target=body, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a thread is still running"
    for e in errs:
        if e is not None:
            raise e
    torch.cuda.synchronize()
    for i in range(2):
        for r in range(ROUNDS):
            K.assert_same(got[i][r], alone[i][r], f"thread {i + 1}, round {r}")
    mine = [m for who, _, m in seen if who == "mine"]
    other = [m for who, _, m in seen if who == "other"]
    assert len(mine) == len(FAIL_AT) and len(other) == len(FAIL_AT)
    for m in other:                                         # thread 2 never sees thread 1's text
        assert m not in mine and b"window" not in (m or b""), m
