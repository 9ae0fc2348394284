"""Host side of the on-device CLIP image preprocessing.

`pil_bicubic_tables` restates Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` (src/libImaging/Resample.c:
bicubic a = -0.5, support scaled by the down-scale factor, double arithmetic, 22-bit fixed point) and the size
rule of `CLIPImageProcessor` (shortest edge -> 224 with int() truncation of the long side, centre crop 224).
The resampling itself runs in HIP (`tspo_preprocess_frames`)."""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
USE_MATRIX_PASS = True      # horizontal pass on the matrix pipe (tspo_preprocess_frames_ex); False = scalar kernels (tests A/B both)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_tables(in_size: int, out_size: int, first: int = 0, count: int = None) -> Tuple[np.ndarray, np.ndarray]:
    """int32 taps [count, ksize] and bounds [count, 2] (first input index, tap count) for output positions
    first .. first+count-1 of an in_size -> out_size resample.  out_size == in_size -> identity taps (Pillow skips
    the pass)."""
    count = out_size - first if count is None else count
    if out_size == in_size:
        kk = np.full((count, 1), 1 << PRECISION_BITS, np.int32)
        bounds = np.stack([np.arange(first, first + count), np.ones(count, np.int64)], 1).astype(np.int32)
        return kk, bounds
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((count, ksize), np.int32)
    bounds = np.zeros((count, 2), np.int32)
    ss = 1.0 / filterscale
    for i in range(count):
        xx = first + i
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = (xmin, xmax)
    return kk, bounds


def clip_resize_geometry(H: int, W: int, size: int = 224):
    """CLIPImageProcessor: shortest edge -> size (long side int(size * long / short)), then centre crop size x size."""
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = size, int(size * long / short)
    new_w, new_h = (new_short, new_long) if W <= H else (new_long, new_short)
    top, left = (new_h - size) // 2, (new_w - size) // 2
    return new_h, new_w, top, left


@functools.lru_cache(maxsize=32)
def _tables(H: int, W: int, size: int):
    new_h, new_w, top, left = clip_resize_geometry(H, W, size)
    hk, hb = pil_bicubic_tables(W, new_w, left, size)
    vk, vb = pil_bicubic_tables(H, new_h, top, size)
    ylo = int(vb[:, 0].min())
    yhi = int((vb[:, 0] + vb[:, 1]).max())
    return hk, hb, vk, vb, ylo, yhi - ylo


def mfma_h_tables(hk: np.ndarray, hb: np.ndarray):
    """Tables of the matrix-pipe horizontal pass (tspo_preprocess_frames_ex) from the tap table of the crop window:
    -> (taps int8 [nblk, nkb, 3, 64, 16], bias int32 [ow], xs int32 [nblk], nkb, span) or None when the window is not a
    whole number of 16-column blocks.  Block b covers output columns 16b..16b+15 and input columns xs[b] .. xs[b]+64*nkb-1;
    every 22-bit tap k is split into signed byte digits k = d0 + 256 d1 + 65536 d2 (|k| < 2^23, so d2 fits a byte too);
    lane l = q*16 + x of a fragment holds the 16 bytes of output column x for input columns q*16..q*16+15 of the K block."""
    ow, ksize = hk.shape
    if ow % 16 or ksize < 2:
        return None
    nblk = ow // 16
    xs = hb[::16, 0].astype(np.int64)
    last = hb[15::16]
    spans = last[:, 0] + last[:, 1] - xs
    nkb = int((spans.max() + 63) // 64)
    if nkb < 1 or nkb > 4:
        return None
    taps = np.zeros((nblk, nkb * 64, 16), np.int64)           # [block][input column within block][output column within block]
    for x in range(ow):
        b, xi = divmod(x, 16)
        o = int(hb[x, 0] - xs[b])
        taps[b, o:o + int(hb[x, 1]), xi] = hk[x, :int(hb[x, 1])]
    d0 = ((taps + 128) % 256) - 128
    t1 = (taps - d0) // 256
    d1 = ((t1 + 128) % 256) - 128
    d2 = (t1 - d1) // 256
    assert np.abs(d2).max() <= 127 and np.array_equal(d0 + 256 * d1 + 65536 * d2, taps)
    dig = np.stack([d0, d1, d2], 0).astype(np.int8)            # [digit][block][k][x]
    # -> [block][K block][digit][q][x][16 consecutive k]
    dig = dig.reshape(3, nblk, nkb, 4, 16, 16)                  # [d][b][kb][q][j][x]
    frag = np.ascontiguousarray(dig.transpose(1, 2, 0, 3, 5, 4)).reshape(nblk, nkb, 3, 64, 16)
    bias = (128 * hk.astype(np.int64).sum(1) + (1 << 21)).astype(np.int64)
    assert bias.max() < 2 ** 31
    # widest span of a chunk of four consecutive blocks (what one workgroup stages), in pixels
    span = max(int(xs[min(c + 3, nblk - 1)] + nkb * 64 - xs[c]) for c in range(0, nblk, 4))
    return frag, bias.astype(np.int32), xs.astype(np.int32), nkb, span


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass(frozen=True)
class PreprocessSpec:
    """What an image processor does to a uint8 RGB frame, in the terms `tspo_preprocess_select` takes.  Resize rule: either
    `shortest_edge` (shortest edge -> that many pixels, long side int()-truncated, then a centre crop `crop` = (h, w): the
    CLIPImageProcessor rule) or `size` = exact (h, w) without crop (the reference's SigLipImageProcessor,
    llava/model/multimodal_encoder/siglip_encoder.py:34-61); PIL antialiased bicubic either way.  Float outputs are
    (u * rescale - mean[c]) / std[c]; `out_dtype` torch.uint8 stops at the Pillow-exact bytes u."""
    shortest_edge: Optional[int] = None
    crop: Optional[Tuple[int, int]] = None
    size: Optional[Tuple[int, int]] = None
    rescale: float = 1 / 255
    mean: Tuple[float, float, float] = CLIP_MEAN
    std: Tuple[float, float, float] = CLIP_STD
    out_dtype: torch.dtype = torch.float32

    def __post_init__(self):
        if (self.shortest_edge is None) == (self.size is None):
            raise ValueError("PreprocessSpec: give either shortest_edge (+ crop) or an exact size")
        if self.shortest_edge is not None and self.crop is None:
            object.__setattr__(self, "crop", (int(self.shortest_edge), int(self.shortest_edge)))
        if self.size is not None and self.crop is not None:
            raise ValueError("PreprocessSpec: an exact size takes no crop")
        if self.out_dtype not in _OUT_DTYPES:
            raise ValueError(f"PreprocessSpec: out_dtype must be one of {sorted(map(str, _OUT_DTYPES))}")
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("PreprocessSpec: mean and std have one entry per RGB channel")
        object.__setattr__(self, "mean", tuple(float(v) for v in self.mean))
        object.__setattr__(self, "std", tuple(float(v) for v in self.std))

    @property
    def geometry(self):
        """The part the tap tables depend on."""
        return (self.shortest_edge, self.crop, self.size)

    @property
    def out_hw(self) -> Tuple[int, int]:
        return tuple(self.size) if self.size is not None else tuple(self.crop)

    def with_dtype(self, out_dtype: torch.dtype) -> "PreprocessSpec":
        return PreprocessSpec(self.shortest_edge, self.crop, self.size, self.rescale, self.mean, self.std, out_dtype)

    @classmethod
    def clip_default(cls, size: int = 224, out_dtype: torch.dtype = torch.float32) -> "PreprocessSpec":
        """openai/clip-vit-large-patch14's processor: what `processor_is_default_clip` recognises."""
        return cls(shortest_edge=size, crop=(size, size), out_dtype=out_dtype)

    @classmethod
    def from_image_processor(cls, ip, out_dtype: torch.dtype = torch.float32) -> Optional["PreprocessSpec"]:
        """The spec of an HF CLIPImageProcessor-shaped object or of the reference's SigLipImageProcessor shape
        (`size=(384, 384)`, `resample` bicubic, `image_mean`, `image_std`, `rescale_factor`), or None for anything the
        kernel does not reproduce exactly (another resampling filter, padding, a disabled stage, Qwen's smart_resize, a
        size rule it does not know): the caller then keeps its own processor - no silent approximation.  Frames handed to
        `select_frames` are 3-channel uint8, so `do_convert_rgb` is a no-op on them."""
        g = lambda n, d=None: getattr(ip, n, d)
        if ip is None or not all(hasattr(ip, n) for n in ("resample", "size", "image_mean", "image_std", "rescale_factor")):
            return None
        # anything that makes the processor do MORE than resize -> (crop) -> rescale -> normalize on one RGB image
        for extra in _UNSUPPORTED_PROCESSOR_ATTRS:
            if g(extra) not in (None, False):
                return None
        try:
            resample = int(g("resample"))
        except (TypeError, ValueError):
            return None
        if resample != 3:                                                       # PIL.Image.BICUBIC
            return None
        for stage in ("do_resize", "do_rescale", "do_normalize"):              # absent (SigLIP shape): the stage always runs
            if g(stage, True) is not True:
                return None
        mean, std, rescale = g("image_mean"), g("image_std"), g("rescale_factor")
        if (not isinstance(mean, (list, tuple)) or not isinstance(std, (list, tuple)) or not isinstance(rescale, (int, float))
                or len(mean) != 3 or len(std) != 3 or any(float(v) == 0 for v in std)):
            return None
        common = dict(rescale=float(rescale), mean=tuple(float(v) for v in mean), std=tuple(float(v) for v in std),
                      out_dtype=out_dtype)
        size = g("size")
        if isinstance(size, (tuple, list)):                                    # SigLipImageProcessor: exact (h, w), never crops
            if len(size) != 2 or hasattr(ip, "do_center_crop"):
                return None
            return cls(size=(int(size[0]), int(size[1])), **common)
        try:
            size = {k: v for k, v in dict(size).items() if v is not None}
        except (TypeError, ValueError):
            return None
        if set(size) == {"shortest_edge"}:
            cs = {k: v for k, v in dict(g("crop_size") or {}).items() if v is not None}
            if g("do_center_crop") is not True or set(cs) != {"height", "width"}:
                return None
            se, ch, cw = int(size["shortest_edge"]), int(cs["height"]), int(cs["width"])
            if ch > se or cw > se:                                             # a crop larger than the image pads
                return None
            return cls(shortest_edge=se, crop=(ch, cw), **common)
        if set(size) == {"height", "width"} and not g("do_center_crop", False):
            return cls(size=(int(size["height"]), int(size["width"])), **common)
        return None


# attributes of HF-style processors that split, tile, pad, flip or re-grid the image: a processor that sets one of them does
# something `tspo_preprocess_select` does not, so no spec is returned for it
_UNSUPPORTED_PROCESSOR_ATTRS = ("do_pad", "min_pixels", "max_pixels", "patch_size", "merge_size", "temporal_patch_size",
                                "do_image_splitting", "image_grid_pinpoints", "do_flip_channel_order", "do_convert_grayscale",
                                "do_thumbnail", "do_align_long_axis", "do_crop_margin", "do_pan_and_scan", "crop_to_patches",
                                "max_image_size", "size_divisor")


def kernel_lds_sizing(hk: int, vk: int, mfma_span: int = 0):
    """The three LDS sizing numbers of preprocess.hip (preprocess_impl), restated on the host so that tests can hold real tap
    tables against them - KEEP IN STEP with the kernel file: (vspan: input rows that PV_R = 4 consecutive output rows may
    touch; span_px: input pixels a 32-column chunk of the LDS-staged horizontal pass may touch; mfma_lds_bytes: LDS of the
    matrix-pass workgroup for a chunk span of `mfma_span` pixels, which must be <= 64 KB for that pass to be taken)."""
    vspan = ((4 - 1) * (vk - 1) + 3) // 4 + vk + 2 if vk > 1 else 4
    span_px = (31 * (hk - 1) + 3) // 4 + hk + 2
    mp = ((mfma_span + 16 + 3) // 4) * 4
    if ((mp >> 2) & 1) == 0:
        mp += 4
    return vspan, span_px, 3 * 32 * mp


_OUT_DTYPES = {torch.uint8: 3, torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}       # -> TSPO_U8 / F32 / BF16 / F16


def spec_resize_geometry(H: int, W: int, spec: PreprocessSpec):
    """-> (new_h, new_w, top, left, out_h, out_w): resize to new_h x new_w, output window of out_h x out_w at (top, left)."""
    if spec.size is not None:
        return spec.size[0], spec.size[1], 0, 0, spec.size[0], spec.size[1]
    new_h, new_w, _, _ = clip_resize_geometry(H, W, spec.shortest_edge)
    oh, ow = spec.crop
    if oh > new_h or ow > new_w:
        raise ValueError(f"crop {spec.crop} larger than the resized image {new_h}x{new_w}: padding is not reproduced")
    return new_h, new_w, (new_h - oh) // 2, (new_w - ow) // 2, oh, ow


@functools.lru_cache(maxsize=32)
def _spec_tables(H: int, W: int, geometry):
    spec = PreprocessSpec(shortest_edge=geometry[0], crop=geometry[1], size=geometry[2])
    new_h, new_w, top, left, oh, ow = spec_resize_geometry(H, W, spec)
    hk, hb = pil_bicubic_tables(W, new_w, left, ow)
    vk, vb = pil_bicubic_tables(H, new_h, top, oh)
    ylo = int(vb[:, 0].min())
    yhi = int((vb[:, 0] + vb[:, 1]).max())
    return hk, hb, vk, vb, ylo, yhi - ylo


_dev_tables = {}          # (H, W, spec geometry, device) -> device tables


def _frame_layout(frames: torch.Tensor, what: str):
    if frames.dtype != torch.uint8 or frames.ndim != 4:
        raise TypeError(f"{what} expects a uint8 tensor [T,H,W,3] or [T,3,H,W]")
    layout = 0 if frames.shape[-1] == 3 else 1
    if layout == 1 and frames.shape[1] != 3:
        raise ValueError(f"cannot infer the channel axis of {tuple(frames.shape)}")
    H, W = (frames.shape[1], frames.shape[2]) if layout == 0 else (frames.shape[2], frames.shape[3])
    return layout, int(H), int(W)


def select_frames(pool: torch.Tensor, index: Optional[torch.Tensor], spec: PreprocessSpec,
                  oob_flag: Optional[torch.Tensor] = None, what: str = "select_frames") -> torch.Tensor:
    """Frames `index` of the uint8 pool [P,H,W,3] / [P,3,H,W] through the image processor `spec` describes, in one HIP call
    (`tspo_preprocess_select`): -> [*index.shape, 3, h, w] of spec.out_dtype.  `index`: int64 on the pool's device, any shape
    (e.g. the [B,G,k] of a rollout), repeats and any order allowed, read ON THE DEVICE - nothing is copied to the host and
    nothing synchronises; None = every frame in order.  A value outside [0, P) is clamped to the nearest frame; pass
    `oob_flag` (int32 [1] on the device, zeroed) to learn that it happened.  Replaces tspo_trainer.py:516,524."""
    from . import _lib, ops
    ops._need_gpu(pool)
    layout, H, W = _frame_layout(pool, what)
    fr = pool.contiguous()
    P_ = int(fr.shape[0])
    if index is None:
        lead, N, ix = (P_,), P_, None
    else:
        ops._need_gpu(index)
        if index.dtype != torch.int64 or index.device != fr.device:
            raise TypeError("select_frames: index must be an int64 tensor on the pool's device")
        lead, ix = tuple(index.shape), index.reshape(-1).contiguous()
        N = int(ix.numel())
    if P_ < 1 or N < 1:
        raise ValueError(f"select_frames: empty pool or index (P={P_}, N={N})")
    key = (H, W, spec.geometry, fr.device)
    if key not in _dev_tables:
        hk, hb, vk, vb, ylo, nrows = _spec_tables(H, W, spec.geometry)
        mf = mfma_h_tables(hk, hb)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(fr.device)
        _dev_tables[key] = tuple(dev(a) for a in (hk, hb, vk, vb)) + (ylo, nrows) + \
            ((dev(mf[0]), dev(mf[1]), dev(mf[2]), mf[3], mf[4]) if mf is not None else (None, None, None, 0, 0))
    hk, hb, vk, vb, ylo, nrows, mtaps, mbias, mxs, mnkb, mspan = _dev_tables[key]
    oh, ow = spec.out_hw
    out = torch.empty((N, 3, oh, ow), dtype=spec.out_dtype, device=fr.device)
    nws = _lib.lib().tspo_preprocess_workspace_bytes(N, nrows, ow)
    ws = torch.empty((nws,), dtype=torch.uint8, device=fr.device)
    if oob_flag is not None and (oob_flag.dtype != torch.int32 or oob_flag.device != fr.device or oob_flag.numel() < 1):
        raise TypeError("select_frames: oob_flag must be an int32 tensor on the pool's device")
    P = lambda t_: None if t_ is None else C.c_void_p(t_.data_ptr())
    mean3, std3 = (C.c_double * 3)(*spec.mean), (C.c_double * 3)(*spec.std)
    _lib.check(_lib.lib().tspo_preprocess_select(
        C.c_void_p(fr.data_ptr()), layout, P_, H, W, P(ix), N, C.c_void_p(hk.data_ptr()), C.c_void_p(hb.data_ptr()), ow, hk.shape[1],
        C.c_void_p(vk.data_ptr()), C.c_void_p(vb.data_ptr()), oh, vk.shape[1], ylo, nrows, C.c_void_p(out.data_ptr()),
        _OUT_DTYPES[spec.out_dtype], float(spec.rescale), mean3, std3, P(oob_flag), C.c_void_p(ws.data_ptr()), ws.numel(),
        torch.cuda.current_stream().cuda_stream, P(mtaps) if USE_MATRIX_PASS else None, P(mbias), P(mxs), int(mnkb), int(mspan)),
        "tspo_preprocess_select")
    return out.view(*lead, 3, oh, ow)


def preprocess_frames(frames: torch.Tensor, size: int = 224) -> torch.Tensor:
    """uint8 CUDA frames [T,H,W,3] or [T,3,H,W] -> uint8 [T,3,size,size] (resize + centre crop, Pillow-exact)."""
    return select_frames(frames, None, PreprocessSpec.clip_default(size, torch.uint8), what="preprocess_frames")


class _StreamedEncodeState:
    """What `encode_frames_streamed` keeps between calls on a ClipVitWeights: its ONE side stream, the two pinned staging
    buffers, the two device raw-chunk buffers and, per buffer pair, the event of the last copy out of the staging buffer and of
    the last kernel that read the raw buffer (pinning host memory costs more than the copy it serves, so it is done once)."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.staging = [None, None]
        self.raw = [None, None]
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]      # H2D copy out of staging[b] / into raw[b] has finished
        self.consumed = [torch.cuda.Event(), torch.cuda.Event()]    # the preprocessing that read raw[b] has finished

    def buffers(self, b: int, nbytes: int, device, current):
        if self.staging[b] is None or self.staging[b].numel() < nbytes:
            self.copied[b].synchronize()                            # nothing still reads the buffers that are let go
            self.consumed[b].synchronize()
            self.staging[b] = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
            self.raw[b] = torch.empty((nbytes,), dtype=torch.uint8, device=device)
            self.stream.wait_stream(current)                        # the allocator hands out memory in `current`'s order
        self.raw[b].record_stream(current)
        return self.staging[b], self.raw[b]


def encode_frames_streamed(clip_weights, frames, chunk_frames: int, spec: Optional[PreprocessSpec] = None,
                           out: Optional[torch.Tensor] = None, fold_layernorm: bool = True,
                           prune_last_layer: bool = False) -> torch.Tensor:
    """Raw uint8 video frames -> CLIP features f32 [T, proj] on the encoder's device, chunk by chunk of
    `ops.clip_chunk_plan(clip_weights, T, chunk_frames)`, for frames that live in HOST memory: numpy or a CPU tensor, [T,H,W,3]
    or [T,3,H,W], pageable or pinned.  Per chunk: host copy into one of two pinned staging buffers -> asynchronous copy to the
    device on one side stream (owned by `clip_weights`, created on first use) -> event -> on the caller's current stream
    `select_frames(chunk, None, spec)` and `tspo_clip_vit_forward_ex` into out[lo:hi].  The copy of chunk i+1 runs while chunk i
    computes; a staging / raw buffer is reused only after an event shows its consumer has finished.  Device memory: two raw
    chunks, one preprocessed chunk and the encoder workspace of the largest chunk - independent of T.  No threads are started.
    `spec`: the image processor (default: CLIP's, uint8 output - the encoder normalises in its patch gather); its output size
    must be the encoder's image size.  Frames that are already on the device skip the copies and take the same loop.
    NOT capturable in a graph: it copies on the host and waits on events from the host.  Bitwise equal to `select_frames` of
    the whole video followed by `ops.clip_vit_forward_chunked` with the same chunk_frames."""
    from . import ops
    cfg = clip_weights.cfg
    if spec is None:
        spec = PreprocessSpec.clip_default(cfg["image"], torch.uint8)
    if tuple(spec.out_hw) != (cfg["image"], cfg["image"]):
        raise ValueError(f"encode_frames_streamed: spec produces {spec.out_hw}, the encoder takes {cfg['image']}x{cfg['image']}")
    fr = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.asarray(frames))
    _frame_layout(fr, "encode_frames_streamed")
    T = int(fr.shape[0])
    dev = clip_weights.device
    plan = ops.clip_chunk_plan(clip_weights, T, chunk_frames)
    feat = out if out is not None else torch.empty((T, cfg["proj"]), dtype=torch.float32, device=dev)
    if tuple(feat.shape) != (T, cfg["proj"]) or feat.dtype != torch.float32 or not feat.is_contiguous() or not feat.is_cuda:
        raise ValueError(f"encode_frames_streamed: out must be a contiguous float32 [{T}, {cfg['proj']}] tensor on the GPU")
    clip_weights._workspace(max(plan))         # sized once for the largest chunk: the per-chunk encodes below share it (and its fold)

    def encode(raw_chunk, lo, hi, read_event=None):
        px = select_frames(raw_chunk, None, spec, what="encode_frames_streamed")
        if read_event is not None:
            read_event.record(torch.cuda.current_stream(dev))     # the raw chunk has no reader after this point
        ops.clip_vit_forward(clip_weights, px, out=feat[lo:hi], fold_layernorm=fold_layernorm, prune_last_layer=prune_last_layer)

    lo = 0
    if fr.is_cuda:
        for n in plan:
            encode(fr[lo:lo + n], lo, lo + n)
            lo += n
        return feat
    st = getattr(clip_weights, "_streamed", None)
    if st is None:
        st = clip_weights._streamed = _StreamedEncodeState(dev)
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        per_frame = int(fr[0].numel())
        for i, n in enumerate(plan):
            b = i & 1
            staging, raw = st.buffers(b, max(plan) * per_frame, dev, cur)
            st.copied[b].synchronize()                               # the copy of chunk i-2 out of this staging buffer is done
            host = staging[:n * per_frame].view(n, *fr.shape[1:])
            host.copy_(fr[lo:lo + n])
            chunk = raw[:n * per_frame].view(n, *fr.shape[1:])
            st.stream.wait_event(st.consumed[b])                     # chunk i-2 has been read out of this raw buffer
            with torch.cuda.stream(st.stream):
                chunk.copy_(host, non_blocking=True)
                st.copied[b].record(st.stream)
            cur.wait_event(st.copied[b])
            encode(chunk, lo, lo + n, st.consumed[b])                # launches only: the host goes on to stage chunk i+1
            lo += n
    return feat


def processor_is_default_clip(image_processor, size: int = 224) -> bool:
    """True when a (HF) CLIPImageProcessor is configured exactly like openai/clip-vit-large-patch14's, i.e. when the
    on-device path is equivalent to calling it."""
    g = lambda n, d=None: getattr(image_processor, n, d)
    sz, cs = g("size", {}), g("crop_size", {})
    mean, std = g("image_mean", []), g("image_std", [])
    try:
        return bool(g("do_resize") and g("do_center_crop") and g("do_rescale") and g("do_normalize")
                    and dict(sz).get("shortest_edge") == size and int(g("resample")) == 3
                    and dict(cs).get("height") == size and dict(cs).get("width") == size
                    and abs(g("rescale_factor") - 1 / 255) < 1e-12
                    and np.allclose(mean, [0.48145466, 0.4578275, 0.40821073]) and np.allclose(std, [0.26862954, 0.26130258, 0.27577711]))
    except Exception:
        return False
