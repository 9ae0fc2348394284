// CLIP ViT frame encoder for gfx950 (MI355X): bf16 MFMA GEMMs (fp32 accumulate)
// with LDS-staged, XOR-swizzled tiles fed by global_load_lds (LDS-DMA), a
// 257-token flash-style attention kernel that keeps the whole score row in
// registers, wave-per-row LayerNorm and a fused patch gather (+u8 normalise).
//
// Replaces transformers' CLIPVisionTransformer + visual_projection as called
// by the reference at model/temporal_agent.py:166, tspo_trainer.py:401.
#include "gemm_bf16.h"
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

namespace {

// ===========================================================================
// LayerNorm over the last dim (C <= 4096, C % 8 == 0): one wave per row, the
// row lives in registers (16-byte loads), two-pass mean / variance in fp32.
// in_stride / out_stride in elements (lets the post-LN read only CLS rows).
// ===========================================================================
// LN_MAXCH = ceil(C / 512) 16-byte chunks per lane: a template parameter so that C = 1024 needs 16 value registers
// (8 waves/SIMD resident = twice the bytes in flight of the generic C <= 4096 instance).
template <int LN_MAXCH>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* in, bf16_t* out,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        long rows, int C, long in_stride, long out_stride, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* x = in + row * in_stride;
  float v[LN_MAXCH][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int e = (c * 64 + lane) * 8;
    if (e < C) {
      const uint4 u = *reinterpret_cast<const uint4*>(x + e);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[c][2 * i] = bf16_to_f32((uint16_t)(w[i] & 0xffff));
        v[c][2 * i + 1] = bf16_to_f32((uint16_t)(w[i] >> 16));
        s += v[c][2 * i] + v[c][2 * i + 1];
      }
    }
  }
  const float mean = wave_sum(s) / (float)C;
  float qv = 0.f;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int e = (c * 64 + lane) * 8;
    if (e < C) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = v[c][i] - mean; qv += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(qv) / (float)C + eps);
  bf16_t* y = out + row * out_stride;
#pragma unroll
  for (int c = 0; c < LN_MAXCH; ++c) {
    const int e = (c * 64 + lane) * 8;
    if (e < C) {
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + e), g1 = *reinterpret_cast<const f32x4*>(gamma + e + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + e), b1 = *reinterpret_cast<const f32x4*>(beta + e + 4);
      float o[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i] = (v[c][i] - mean) * rstd * g0[i] + b0[i];
        o[4 + i] = (v[c][4 + i] - mean) * rstd * g1[i] + b1[i];
      }
      uint4 u;
      u.x = pack_bf16x2(o[0], o[1]); u.y = pack_bf16x2(o[2], o[3]);
      u.z = pack_bf16x2(o[4], o[5]); u.w = pack_bf16x2(o[6], o[7]);
      *reinterpret_cast<uint4*>(y + e) = u;
    }
  }
}

// ===========================================================================
// Patch gather (im2col for the stride-p conv) + CLS rows.
// patches[(n*P + py*gw + px)][k = c*p*p + ky*p + kx] = pixel[n][c][py*p+ky][px*p+kx]
// Kp = roundup(3*p*p, 64), padding zero.  TSPO_U8 input gets (x/255-mean)/std fused.
// ===========================================================================
template <typename TP>
__device__ __forceinline__ float load_pixel(const TP* p, size_t i, int c);
template <> __device__ __forceinline__ float load_pixel<float>(const float* p, size_t i, int) { return p[i]; }
template <> __device__ __forceinline__ float load_pixel<bf16_t>(const bf16_t* p, size_t i, int) { return bf16_to_f32(p[i]); }
template <> __device__ __forceinline__ float load_pixel<_Float16>(const _Float16* p, size_t i, int) { return (float)p[i]; }
template <> __device__ __forceinline__ float load_pixel<uint8_t>(const uint8_t* p, size_t i, int c) {
  const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
  const float sd = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
  return ((float)p[i] / 255.0f - mean) / sd;
}

// IMAGE / PATCH / KP > 0: compile-time geometry (CLIP-L/14: 224 / 14 / 640) - every index division below is by a runtime
// value otherwise, ~30 instructions each, five per element
template <typename TP, int IMAGE = 0, int PATCH = 0, int KP = 0>
__global__ __launch_bounds__(256) void patch_gather_kernel(const TP* __restrict__ px, bf16_t* __restrict__ out,
                                                           int n_frames, int image_rt, int patch_rt, int Kp_rt) {
  const int image = IMAGE ? IMAGE : image_rt, patch = PATCH ? PATCH : patch_rt, Kp = KP ? KP : Kp_rt;
  const int gw = image / patch, P = gw * gw, pp = patch * patch, Kreal = 3 * pp;
  const int oct = Kp / 8;
  const size_t total = (size_t)n_frames * P * oct;
  for (size_t id = (size_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (size_t)gridDim.x * 256) {
    const int o8 = (int)(id % oct);
    const size_t m = id / oct;
    const int pidx = (int)(m % P);
    const size_t n = m / P;
    const int py = pidx / gw, pxx = pidx - py * gw;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = o8 * 8 + i;
      if (k < Kreal) {
        const int c = k / pp, rem = k - c * pp;
        const int ky = rem / patch, kx = rem - ky * patch;
        const size_t src = ((n * 3 + c) * image + (size_t)(py * patch + ky)) * image + (pxx * patch + kx);
        v[i] = load_pixel<TP>(px, src, c);
      } else {
        v[i] = 0.f;
      }
    }
    uint4 u;
    u.x = pack_bf16x2(v[0], v[1]); u.y = pack_bf16x2(v[2], v[3]);
    u.z = pack_bf16x2(v[4], v[5]); u.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4*>(out + m * Kp + (size_t)o8 * 8) = u;
  }
}

// x[n*S + 0][:] = pos_emb[0][:]  (class_embedding already folded into row 0)
// CLIP-L/14 on uint8 frames (the production front end): one workgroup per (frame, row of 16 patches).  The 3 x 14 image rows that
// row of patches covers are 42 contiguous 224-byte runs - 588 16-byte loads, every byte of the frame read exactly once, coalesced -
// staged through LDS; every thread then assembles five 8-value pieces of the 16 patch rows (k = c 196 + ky 14 + kx, zero beyond 588)
// from LDS bytes through a 3 x 256 table of load_pixel<uint8_t> (the same arithmetic, evaluated once per byte value) and stores them as 16 bytes.  (Round 5: the generic kernel above reads its
// eight pixels with eight 1-byte global loads at a 14-byte patch pitch: 0.33 ms per 1024 frames = 1.5 TB/s of input + output.)
__global__ __launch_bounds__(256) void patch_gather_u8_l14_kernel(const uint8_t* __restrict__ px, bf16_t* __restrict__ out) {
  constexpr int IMG = 224, PATCH = 14, GW = 16, KP = 640, KREAL = 588, ROWB = 224;
  __shared__ __attribute__((aligned(16))) uint8_t img[3 * PATCH * ROWB];   // [c][ky][224]
  __shared__ float lut[3][256];   // load_pixel<uint8_t> of every byte value per channel (two IEEE divisions each: once per workgroup, not per pixel)
  const int py = blockIdx.x;
  const size_t n = blockIdx.y;
  const int tid = threadIdx.x;
  {
    const uint8_t b = (uint8_t)tid;
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][tid] = load_pixel<uint8_t>(&b, 0, c);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int id = tid + j * 256;   // 16-byte chunk: (c, ky, x16)
    if (id < 3 * PATCH * (ROWB / 16)) {
      const int c = id / (PATCH * (ROWB / 16)), rem = id - c * (PATCH * (ROWB / 16));
      const int ky = rem / (ROWB / 16), x16 = rem - ky * (ROWB / 16);
      const size_t src = ((n * 3 + c) * IMG + (size_t)(py * PATCH + ky)) * IMG + x16 * 16;
      *reinterpret_cast<uint4*>(img + id * 16) = *reinterpret_cast<const uint4*>(px + src);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int q = tid + j * 256;    // (patch, 8-value piece): 16 x 80
    const int pxx = q / (KP / 8), o8 = q - pxx * (KP / 8);
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = o8 * 8 + i;
      if (k < KREAL) {
        const int c = k / (PATCH * PATCH), rem = k - c * (PATCH * PATCH);
        const int ky = rem / PATCH, kx = rem - ky * PATCH;
        v[i] = lut[c][img[(c * PATCH + ky) * ROWB + pxx * PATCH + kx]];
      } else {
        v[i] = 0.f;
      }
    }
    uint4 u;
    u.x = pack_bf16x2(v[0], v[1]); u.y = pack_bf16x2(v[2], v[3]);
    u.z = pack_bf16x2(v[4], v[5]); u.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4*>(out + ((n * (GW * GW) + (size_t)(py * GW + pxx)) * KP + (size_t)o8 * 8)) = u;
  }
}

__global__ __launch_bounds__(256) void cls_rows_kernel(const float* __restrict__ pos, bf16_t* __restrict__ x, int n_frames,
                                                       int S, int C) {
  const size_t total = (size_t)n_frames * C;
  for (size_t id = (size_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (size_t)gridDim.x * 256) {
    const size_t n = id / C;
    const int c = (int)(id - n * C);
    x[n * S * C + c] = f32_to_bf16(pos[c]);
  }
}

// ===========================================================================
// Attention for one (frame, head): S <= 288 tokens, head_dim 64, non-causal.
// K rows in LDS (swizzled like the GEMM tiles), V row-major in [32 keys][16 d] sub-tiles that the
// hardware transpose read (ds_read_b64_tr_b16) turns into V^T fragments.  Each wave owns 16-query tiles:
//   S^T = K Q^T  (18 key tiles -> 72 fp32 regs hold the full score row)
//   softmax over keys in registers (lane-local + 2 xor-shuffles)
//   O^T = V^T P^T with P taken straight from the S^T accumulators (the key
//   permutation inside each 32-key chunk is shared by both MFMA operands).
// ===========================================================================
#define AT_KEYS 288
#define AT_V_BYTES (9 * 4 * 1024)  // V: 9 key chunks x 4 d-tiles of row-major [32 keys][16 d] sub-tiles (1 KB each)
#define AT_LDS_BYTES (AT_KEYS * 128 + AT_V_BYTES)
typedef __attribute__((ext_vector_type(4))) short s16x4;

// NQ query tiles (16 queries each, tiles qt and qt+qstride) against all keys of one (frame, head).
template <int NQ, int S_CT>
__device__ __forceinline__ void attn_tiles(const bf16_t* __restrict__ base, bf16_t* __restrict__ out, const char* Ks,
                                           const char* Vt, int S_rt, int C, size_t ld, size_t f, int h, float scale, int qt0,
                                           int qstride, int l15, int q4) {
  const int S = S_CT ? S_CT : S_rt;   // S_CT = 257 (ViT-L/14 @ 224): every tile-skip / mask decision folds at compile time
  // V^T fragments come from ds_read_b64_tr_b16: the 16 lanes of a row each point at 4 contiguous bf16 of a
  // row-major [4 keys][16 d] block (lane i -> key i>>2, d-chunk i&3) and receive COLUMN i of it, i.e. 4 keys of
  // their own d - so V stays row-major in LDS (16-byte staging writes, no scattered 2-byte transposition).
  int voff[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) voff[dt][hh] = dt * 1024 + (hh * 16 + q4 * 4 + (l15 >> 2)) * 32 + (l15 & 3) * 8;
  const int koff = l15 * 128;
  const int ksw = l15 & 7;
  int qrow[NQ];
  bool qvalid[NQ];
  bf16x8 qf[NQ][2];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int r = (qt0 + n * qstride) * 16 + l15;
    qvalid[n] = r < S;
    qrow[n] = qvalid[n] ? r : S - 1;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qf[n][kk] = *reinterpret_cast<const bf16x8*>(base + (size_t)qrow[n] * ld + kk * 32 + q4 * 8);
  }
  f32x4 sc[NQ][18];
  // K fragments are software-pipelined one key tile ahead (the MFMA of tile kt never waits on an LDS read issued
  // just before it; before this the loop paid the LDS latency 36 times per pass)
  const int nkt = (S + 15) >> 4;   // key tiles that hold at least one valid key (17 for S = 257)
  bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(Ks + koff + ((q4 ^ ksw) << 4));
  bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(Ks + koff + (((4 + q4) ^ ksw) << 4));
#pragma unroll
  for (int kt = 0; kt < 18; ++kt) {
#pragma unroll
    for (int n = 0; n < NQ; ++n) sc[n][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 nf0 = kf0, nf1 = kf1;
    if (kt + 1 < 18) {   // rows past S are zero-filled in LDS, so the read itself is always safe
      nf0 = *reinterpret_cast<const bf16x8*>(Ks + (kt + 1) * 2048 + koff + ((q4 ^ ksw) << 4));
      nf1 = *reinterpret_cast<const bf16x8*>(Ks + (kt + 1) * 2048 + koff + (((4 + q4) ^ ksw) << 4));
    }
    if (kt < nkt) {  // key tiles entirely past the sequence are never multiplied (uniform branch)
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        sc[n][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf[n][0], sc[n][kt], 0, 0, 0);
        sc[n][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf[n][1], sc[n][kt], 0, 0, 0);
      }
    }
    if ((kt + 1) * 16 > S) {  // only the tile(s) straddling / past S need the key mask
#pragma unroll
      for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[n][kt][r] = (kt * 16 + q4 * 4 + r) < S ? sc[n][kt][r] : -INFINITY;
    }
    kf0 = nf0;
    kf1 = nf1;
  }
  // softmax over keys: lane holds keys kt*16 + q4*4 + r for query l15
  const float c2 = scale * 1.4426950408889634f;  // exp(x*scale) = 2^(x*scale*log2 e): one v_fma + one v_exp per score
  float inv[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 18; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[n][kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * c2;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 18; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(sc[n][kt][r], c2, -mc));
        sc[n][kt][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    inv[n] = 1.f / sum;
  }
  f32x4 o[NQ][4];
#pragma unroll
  for (int n = 0; n < NQ; ++n)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[n][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  union VF { bf16x8 v; s16x4 h2[2]; };
  auto ldv = [&](int step) {   // step = c * 4 + dt
    VF f;
    const int c = step >> 2, dt = step & 3;
    f.h2[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(Vt + voff[dt][0] + c * 4096));
    f.h2[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(Vt + voff[dt][1] + c * 4096));
    return f;
  };
  constexpr bool VPF = true;   // (A/B: without the V prefetch the paired path measured 18.0 ms vs 15.6 ms per video)
  VF vcur = ldv(0);
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    union { bf16x8 v; uint32_t u[4]; } pf[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      pf[n].u[0] = pack_bf16x2(sc[n][2 * c][0], sc[n][2 * c][1]);
      pf[n].u[1] = pack_bf16x2(sc[n][2 * c][2], sc[n][2 * c][3]);
      pf[n].u[2] = pack_bf16x2(sc[n][2 * c + 1][0], sc[n][2 * c + 1][1]);
      pf[n].u[3] = pack_bf16x2(sc[n][2 * c + 1][2], sc[n][2 * c + 1][3]);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int step = c * 4 + dt;
      VF vnext = vcur;
      if (VPF && step + 1 < 36) vnext = ldv(step + 1);
      if (!VPF) vcur = ldv(step);
#pragma unroll
      for (int n = 0; n < NQ; ++n) o[n][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vcur.v, pf[n].v, o[n][dt], 0, 0, 0);
      vcur = vnext;
    }
  }
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    if (qvalid[n]) {
      bf16_t* orow = out + (f * S + qrow[n]) * (size_t)C + (size_t)h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        uint2 pk;
        pk.x = pack_bf16x2(o[n][dt][0] * inv[n], o[n][dt][1] * inv[n]);
        pk.y = pack_bf16x2(o[n][dt][2] * inv[n], o[n][dt][3] * inv[n]);
        *reinterpret_cast<uint2*>(orow + dt * 16 + q4 * 4) = pk;
      }
    }
  }
}


template <int S_CT>
__global__ __launch_bounds__(256, 2) void clip_attn_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int S_rt,
                                                        int C, float scale) {
  const int S = S_CT ? S_CT : S_rt;
  __shared__ __attribute__((aligned(16))) char lds[AT_LDS_BYTES];
  char* Ks = lds;
  char* Vt = lds + AT_KEYS * 128;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l15 = lane & 15, q4 = lane >> 4;
  const int h = blockIdx.x;
  const size_t f = blockIdx.y;
  const size_t ld = (size_t)3 * C;
  const bf16_t* base = qkv + f * S * ld + (size_t)h * 64;

  // ---- stage K (swizzled rows) and V (row-major sub-tiles) -------------------
  // All 18 16-byte loads of a thread are issued before the first LDS write (rows past S are clamped and zeroed
  // afterwards, so there is no branch around a load): the rolled, branchy version of this loop exposed one full
  // memory latency per iteration - 9 round trips per workgroup.
  {
    uint4 kv[9], vv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int id = tid + i * 256;
      const int row = id >> 3, c = id & 7;
      const int rc = row < S ? row : S - 1;
      kv[i] = *reinterpret_cast<const uint4*>(base + (size_t)rc * ld + C + c * 8);
      vv[i] = *reinterpret_cast<const uint4*>(base + (size_t)rc * ld + 2 * C + c * 8);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int id = tid + i * 256;
      const int row = id >> 3, c = id & 7;
      const uint4 z = {0u, 0u, 0u, 0u};
      const uint4 k4 = row < S ? kv[i] : z, v4 = row < S ? vv[i] : z;
      *reinterpret_cast<uint4*>(Ks + row * 128 + ((c ^ (row & 7)) << 4)) = k4;
      *reinterpret_cast<uint4*>(Vt + ((row >> 5) * 4 + (c >> 1)) * 1024 + (row & 31) * 32 + (c & 1) * 16) = v4;
    }
  }
  __syncthreads();

  const int nqt = (S + 15) >> 4;
  // wave w owns query tiles w, w+4, w+8, ...; they are processed two at a time so every K / Vt fragment read from
  // LDS feeds two MFMAs (LDS bytes per MFMA halve: at one tile per pass the kernel read 1 KB of LDS per MFMA and
  // was co-limited by LDS bandwidth).
  int qt = wid;
  while (qt < nqt) {
    asm volatile("" ::: "memory");  // keep the loop-invariant K / Vt fragment reads inside the loop (register budget)
    if (qt + 4 < nqt) {
      attn_tiles<2, S_CT>(base, out, Ks, Vt, S, C, ld, f, h, scale, qt, 4, l15, q4);
      qt += 8;
    } else {
      attn_tiles<1, S_CT>(base, out, Ks, Vt, S, C, ld, f, h, scale, qt, 4, l15, q4);
      qt += 4;
    }
  }
}

// ===========================================================================
// Attention for S = 257 (ViT-L/14 @ 224), head_dim 64: one workgroup per (frame, head), whole K / V of the head staged once
// in LDS as above, but every wave works on FOUR 16-query tiles at once (64 queries: wave w owns queries 64w .. 64w+63) and
// walks the keys in three blocks of 96 with an online softmax (running max / sum per query, O rescaled per block).
// Why: the two-tiles-at-a-time kernel keeps the whole 288-key score row in registers (144 VGPRs), so it cannot take more
// queries per pass, and it reads one K / V^T fragment from LDS per two MFMAs - with 8 waves per CU that is ~0.75 KB of
// LDS reads per MFMA, i.e. the LDS pipe (and its 4-way conflicts on the V staging writes) ran as hot as the matrix pipe
// could have (measured: MFMA busy 22 %, 20 % of LDS cycles conflicts, profiles/r1_e_attn_sq_counters.json).  Here a
// fragment read feeds FOUR MFMAs, the score registers of a block are 96, and every wave runs exactly one pass.
// Token 256 - the 257th query, alone in query tile 16 - would cost one wave a whole extra pass; instead waves 0..2 each
// take ONE key block for that tile (12 + 12 MFMAs) and leave (max, sum, O row) partials in LDS, merged by wave 0.
// V sub-tiles [32 keys][16 d] are spaced 1056 B apart (not 1024): the 16-byte staging writes of a row then land on 8
// distinct bank groups instead of 2.
// ===========================================================================
#define A4_VSUB 1056
#define A4_V_BYTES (36 * A4_VSUB)
#define A4_PART_OFF (AT_KEYS * 128 + A4_V_BYTES)          // partials of the token-256 row: [3][68] floats
#define A4_LDS_BYTES (A4_PART_OFF + 3 * 68 * 4)

// NQ query tiles starting at tile qt0 against key blocks [b0, b1) (96 keys each).  Returns running max (already times
// log2e * scale), running sum and the un-normalised O^T accumulators.
template <int NQ>
__device__ __forceinline__ void attn257_load_q(const bf16_t* __restrict__ base, size_t ld, int qt0, int l15, int q4,
                                               bf16x8 (&qf)[NQ][2]) {
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int r = (qt0 + n) * 16 + l15;
    const int rc = r < 257 ? r : 256;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qf[n][kk] = *reinterpret_cast<const bf16x8*>(base + (size_t)rc * ld + kk * 32 + q4 * 8);
  }
}

// Row maximum of 4 * NT raw MFMA results, two per instruction.  v_maximum3_f32 (IEEE-754-2019 maximum, gfx950) and not
// fmaxf: in IEEE mode hipcc canonicalises every fmaxf operand it cannot prove quiet - a v_max_f32 x, x, x in front of
// each MFMA result, a third of the softmax's vector instructions - and an inline-asm v_max3 is not an option either, the
// hazard recogniser does not protect MFMA results that are read from asm (measured: wrong results).
#define AT_MAX(a, b) __builtin_elementwise_maximum((a), (b))
template <int NT>
__device__ __forceinline__ float at_rowmax(const f32x4 (&sc)[NT]) {
  float mx = AT_MAX(AT_MAX(sc[0][0], sc[0][1]), sc[0][2]);
  float carry = sc[0][3];
#pragma unroll
  for (int j = 1; j < NT; ++j) {
    mx = AT_MAX(AT_MAX(mx, carry), sc[j][0]);
    mx = AT_MAX(AT_MAX(mx, sc[j][1]), sc[j][2]);
    carry = sc[j][3];
  }
  return AT_MAX(mx, carry);
}

// KT = key tiles per block (6 in the main passes, 2 for the 8-way split of the token-256 row).  VROW: V lies in LDS like K
// ([key][64 d] rows of 128 B, 16-byte chunks XOR-swizzled by key & 7 - what an 8-row LDS-DMA piece writes) instead of
// the [32 keys][16 d] sub-tiles; ds_read_b64_tr_b16 takes per-lane addresses, so only the address arithmetic differs.
template <int NQ, int KT = 6, bool VROW = false>
__device__ __forceinline__ void attn257_blocks(const bf16x8 (&qf)[NQ][2], const char* Ks, const char* Vt, float scale, int b0,
                                               int b1, int l15, int q4, float (&mrun)[NQ], float (&lrun)[NQ],
                                               f32x4 (&o)[NQ][4]) {
  constexpr int S = 257;
  int voff[4][2];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int kr = hh * 16 + q4 * 4 + (l15 >> 2);
      voff[dt][hh] = VROW ? kr * 128 + (((dt * 2 + ((l15 & 3) >> 1)) ^ (kr & 7)) << 4) + (l15 & 1) * 8
                          : dt * A4_VSUB + kr * 32 + (l15 & 3) * 8;
    }
  const int koff = l15 * 128, ksw = l15 & 7;
  const float c2 = scale * 1.4426950408889634f;
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    mrun[n] = -INFINITY;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[n][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  union VF { bf16x8 v; s16x4 h2[2]; };
  f32x4 lsum[NQ];   // running row sums: every row of this accumulator tile is the same sum (all-ones V^T rows)
#pragma unroll
  for (int n = 0; n < NQ; ++n) lsum[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  union { bf16x8 v; uint32_t u[4]; } ones;
  ones.u[0] = ones.u[1] = ones.u[2] = ones.u[3] = 0x3f803f80u;   // bf16 1.0 x 8
  for (int b = b0; b < b1; ++b) {
    // ---- S^T = K Q^T for the 6 key tiles of this block (tile 17 does not exist; tile 16 holds only key 256) ----
    f32x4 sc[NQ][KT];
    const char* kb = Ks + b * KT * 2048 + koff;
    bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(kb + ((q4 ^ ksw) << 4));
    bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(kb + (((4 + q4) ^ ksw) << 4));
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      bf16x8 nf0 = kf0, nf1 = kf1;
      if (j + 1 < KT) {   // (rows past S are zero-filled in LDS: always safe to read)
        nf0 = *reinterpret_cast<const bf16x8*>(kb + (j + 1) * 2048 + ((q4 ^ ksw) << 4));
        nf1 = *reinterpret_cast<const bf16x8*>(kb + (j + 1) * 2048 + (((4 + q4) ^ ksw) << 4));
      }
      const bool live = b * KT + j <= 16;   // wave-uniform
      // the two K-halves of a score tile are a dependent MFMA pair: issue the first halves of all NQ query tiles, then the
      // second halves, so that a dependent MFMA follows its producer NQ issue slots later, not back to back
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        sc[n][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live) sc[n][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, qf[n][0], sc[n][j], 0, 0, 0);
      }
#pragma unroll
      for (int n = 0; n < NQ; ++n)
        if (live) sc[n][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, qf[n][1], sc[n][j], 0, 0, 0);
      if (b * KT + j >= 16) {   // key tile 16: only key 256 (row 0 of the tile) exists; tile 17: nothing
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) sc[n][j][r] = ((b * KT + j) * 16 + q4 * 4 + r) < S ? sc[n][j][r] : -INFINITY;
      }
      kf0 = nf0;
      kf1 = nf1;
    }
    // ---- online softmax: lane holds keys (tile j, rows q4*4 + r) of query l15.  The row SUM is not accumulated here:
    //      it comes out of the P V product below as an extra all-ones row of V^T (one more MFMA per key chunk instead
    //      of 24 adds and two cross-lane reductions per query tile; the matrix pipe has the slack, the VALU does not) ----
    float alpha[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      float mx = at_rowmax<KT>(sc[n]);
      // max over the 4 lanes of a query (rows of 16 lanes): v_permlane16_swap / v_permlane32_swap, no LDS round trip
      {
        const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = AT_MAX(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
        const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = AT_MAX(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
      }
      const float mnew = AT_MAX(mrun[n], mx * c2);
      alpha[n] = __builtin_amdgcn_exp2f(mrun[n] - mnew);   // first block: exp2(-inf) = 0 (o and l are 0 anyway)
      mrun[n] = mnew;
      const f32x2 c2v = {c2, c2}, nm = {-mnew, -mnew};
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        const f32x2 lo = {sc[n][j][0], sc[n][j][1]}, hi = {sc[n][j][2], sc[n][j][3]};
        const f32x2 tl = lo * c2v + nm, th = hi * c2v + nm;   // v_pk_fma_f32
        const int tile = b * KT + j;   // wave-uniform
        if (tile >= 17) {          // no such keys: P = 0
          sc[n][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        } else if (tile == 16) {   // key 256 alone (row 0 of the tile; the masked lanes hold -inf -> 0)
          sc[n][j] = (f32x4){__builtin_amdgcn_exp2f(tl[0]), 0.f, 0.f, 0.f};
        } else {
          sc[n][j][0] = __builtin_amdgcn_exp2f(tl[0]); sc[n][j][1] = __builtin_amdgcn_exp2f(tl[1]);
          sc[n][j][2] = __builtin_amdgcn_exp2f(th[0]); sc[n][j][3] = __builtin_amdgcn_exp2f(th[1]);
        }
      }
      lsum[n] *= alpha[n];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[n][dt] *= alpha[n];
    }
    // ---- O^T += V^T P^T over the 3 key chunks (32 keys) of this block ----
    const char* vb = Vt + (VROW ? b * (KT / 2) * 4096 : b * (KT / 2) * 4 * A4_VSUB);
    auto ldv = [&](int step) {   // step = c * 4 + dt
      VF f;
      const int c = step >> 2, dt = step & 3;
      const int co = VROW ? c * 4096 : c * 4 * A4_VSUB;
      f.h2[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + voff[dt][0] + co));
      f.h2[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + voff[dt][1] + co));
      return f;
    };
    VF vcur = ldv(0);
#pragma unroll
    for (int c = 0; c < KT / 2; ++c) {
      union { bf16x8 v; uint32_t u[4]; } pf[NQ];
#pragma unroll
      for (int n = 0; n < NQ; ++n) {
        pf[n].u[0] = pack_bf16x2(sc[n][2 * c][0], sc[n][2 * c][1]);
        pf[n].u[1] = pack_bf16x2(sc[n][2 * c][2], sc[n][2 * c][3]);
        pf[n].u[2] = pack_bf16x2(sc[n][2 * c + 1][0], sc[n][2 * c + 1][1]);
        pf[n].u[3] = pack_bf16x2(sc[n][2 * c + 1][2], sc[n][2 * c + 1][3]);
        lsum[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones.v, pf[n].v, lsum[n], 0, 0, 0);   // row sums of the bf16 P
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int step = c * 4 + dt;
        VF vnext = vcur;
        if (step + 1 < KT * 2) vnext = ldv(step + 1);
#pragma unroll
        for (int n = 0; n < NQ; ++n) o[n][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vcur.v, pf[n].v, o[n][dt], 0, 0, 0);
        vcur = vnext;
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NQ; ++n) lrun[n] = lsum[n][0];
}


// hm: qkv is the head-major image the q/k/v GEMM wrote (GE_BIAS_LN_HM: [3 * heads][M][64]): the item's q, k and v rows are three
// contiguous 33 KB blocks (row pitch 64) instead of 128-byte pieces of 6 KB rows - same values, the staging loads of a workgroup
// become one linear stream (measured with the round-4 layout experiment: 11.9 -> 11.1 ms per forward).
__global__ __launch_bounds__(256, 2) void clip_attn257_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int C,
                                                              float scale, int hm) {
  constexpr int S = 257;
  __shared__ __attribute__((aligned(16))) char lds[A4_LDS_BYTES];
  char* Ks = lds;
  char* Vt = lds + AT_KEYS * 128;
  float* part = reinterpret_cast<float*>(lds + A4_PART_OFF);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l15 = lane & 15, q4 = lane >> 4;
  // (frame, head) of this workgroup: consecutive items go to the SAME XCD (blockIdx % 8 observed = XCD; speed only), so the
  // 16 heads of a frame - the 16 x 128-byte slices of each 6 KB token row of qkv - are read through one L2 at about the
  // same time instead of being scattered over all eight
  const int nwg = gridDim.x * gridDim.y, bid = blockIdx.y * gridDim.x + blockIdx.x;
  const int item = (nwg & 7) == 0 ? (bid & 7) * (nwg >> 3) + (bid >> 3) : bid;
  const int h = item % (int)gridDim.x;
  const size_t f = item / (int)gridDim.x;
  const size_t ld = hm ? 64 : (size_t)3 * C;
  const size_t hm_part = (size_t)gridDim.x * gridDim.y * S * 64;   // one of q | k | v in the head-major image: heads * M * 64
  const bf16_t* base = hm ? qkv + (((size_t)h * gridDim.y * S + f * S) << 6) : qkv + f * S * ld + (size_t)h * 64;   // q rows
  const bf16_t* kbase = base + (hm ? hm_part : (size_t)C);
  const bf16_t* vbase = base + (hm ? 2 * hm_part : (size_t)2 * C);
  bf16x8 qf4[4][2];
  {   // stage K (swizzled 128-byte rows) and V (row-major [32 keys][16 d] sub-tiles): all loads in flight, then the writes
    uint4 kv[9], vv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int id = tid + i * 256;
      const int row = id >> 3, c = id & 7;
      const int rc = row < S ? row : S - 1;
      kv[i] = *reinterpret_cast<const uint4*>(kbase + (size_t)rc * ld + c * 8);
      vv[i] = *reinterpret_cast<const uint4*>(vbase + (size_t)rc * ld + c * 8);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int id = tid + i * 256;
      const int row = id >> 3, c = id & 7;
      const uint4 z = {0u, 0u, 0u, 0u};
      const uint4 k4 = row < S ? kv[i] : z, v4 = row < S ? vv[i] : z;
      *reinterpret_cast<uint4*>(Ks + row * 128 + ((c ^ (row & 7)) << 4)) = k4;
      *reinterpret_cast<uint4*>(Vt + ((row >> 5) * 4 + (c >> 1)) * A4_VSUB + (row & 31) * 32 + (c & 1) * 16) = v4;
      if (i == 0) attn257_load_q<4>(base, ld, wid * 4, l15, q4, qf4);   // this wave's Q fragments, behind the staging loads
    }
  }
  __syncthreads();

  {   // this wave's 64 queries
    float m4[4], l4[4];
    f32x4 o4[4][4];
    attn257_blocks<4>(qf4, Ks, Vt, scale, 0, 3, l15, q4, m4, l4, o4);
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int qrow = (wid * 4 + n) * 16 + l15;
      const float inv = 1.f / l4[n];
      bf16_t* orow = out + (f * S + qrow) * (size_t)C + (size_t)h * 64;
      // 16-byte stores (round 4: 13.0 -> 12.0 ms per forward on the same box): v_permlane16_swap exchanges the odd 16-lane rows
      // of d-tile 2p with the even rows of d-tile 2p+1, after which lane row q4 holds 8 consecutive d of tile 2p + (q4 & 1) at
      // (q4 >> 1) * 8 - half as many store instructions (the store tail of the epilogue is issue-bound; same pairing as the GEMM's)
      uint2 pk[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        pk[dt].x = pack_bf16x2(o4[n][dt][0] * inv, o4[n][dt][1] * inv);
        pk[dt].y = pack_bf16x2(o4[n][dt][2] * inv, o4[n][dt][3] * inv);
      }
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const auto w0 = __builtin_amdgcn_permlane16_swap(pk[2 * pr].x, pk[2 * pr + 1].x, false, false);
        const auto w1 = __builtin_amdgcn_permlane16_swap(pk[2 * pr].y, pk[2 * pr + 1].y, false, false);
        uint4 st;
        st.x = w0[0]; st.y = w1[0]; st.z = w0[1]; st.w = w1[1];
        *reinterpret_cast<uint4*>(orow + (2 * pr + (q4 & 1)) * 16 + (q4 >> 1) * 8) = st;
      }
    }
  }
  // token 256 (query tile 16, row 0): waves 0..2 take one key block each
  if (wid < 3) {
    float m1[1], l1[1];
    f32x4 o1[1][4];
    bf16x8 qf1[1][2];
    attn257_load_q<1>(base, ld, 16, l15, q4, qf1);
    attn257_blocks<1>(qf1, Ks, Vt, scale, wid, wid + 1, l15, q4, m1, l1, o1);
    if (l15 == 0) {
      float* pw = part + wid * 68;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[dt * 16 + q4 * 4 + r] = o1[0][dt][r];
      if (q4 == 0) { pw[64] = m1[0]; pw[65] = l1[0]; }
    }
  }
  __syncthreads();
  if (tid < 64) {   // lane d merges the three partials of output column d
    const float ma = part[64], mb = part[68 + 64], mc = part[136 + 64];
    const float m = fmaxf(ma, fmaxf(mb, mc));
    const float wa = __builtin_amdgcn_exp2f(ma - m), wb = __builtin_amdgcn_exp2f(mb - m), wc = __builtin_amdgcn_exp2f(mc - m);
    const float l = part[65] * wa + part[68 + 65] * wb + part[136 + 65] * wc;
    const float ov = (part[tid] * wa + part[68 + tid] * wb + part[136 + tid] * wc) / l;
    const float on = __shfl_down(ov, 1, 64);
    if ((tid & 1) == 0)
      *reinterpret_cast<uint32_t*>(out + (f * S + 256) * (size_t)C + (size_t)h * 64 + tid) = pack_bf16x2(ov, on);
  }
}


// Round 5, measured and not kept: lazy rescaling (the running maximum set by the first key block and moved only when a later block
// maximum exceeds it by more than 2^8 - no alpha multiplies on o / lsum in the common case; that form also allocates without the
// one spilled VGPR of this one): 11.60 -> 11.34 ms per forward on the same box (profiles/r5_b_step_ab_attention_and_nt.txt),
// mathematically the same quotient - but a different rounding draw, and on the heavy-tailed end-to-end videos that draw is the
// unluckier one on two of three (largest score error 1.51 x the reference's own bf16 noise on the first video against 1.49 x
// with this form, asserted <= 1.5 x).  0.2 % of the step is not worth a parity margin.  (The one spill of this form is an LDS
// offset kept for the token-256 pass: one scratch store + load per item, outside the key-block loop; forcing its recomputation
// costs 12 spills instead.)
// Measured and gone from the tree (results: profiles/r2_d_attn_ablation.json, r2_e_attn_persistent_ab.json; code: git
// history up to 99eb127): a persistent 8-wave form with LDS-DMA double-buffered staging (15.0-15.9 ms per forward on every box
// against 12.6-14.0 for the kernel above: its two-tiles-per-wave math phase is slower), an 8-wave / 2-tile form at <= 128
// registers (17.3 ms), a two-pass softmax (30.9 ms), staging-only / math-only ablation builds; round 4: K and V staged by LDS-DMA
// into [288][128 B] swizzled rows (no staging registers, no ds_write): 15.1 ms against 12.0 on the same box - the row-major V image
// costs the P V phase more (ds_read_b64_tr_b16 bank conflicts the [32 keys][16 d] sub-tiles avoid) than the staging saves.

// ===========================================================================
struct ClipWs {
  bf16_t *x, *h, *qkv, *a, *u, *patches, *pooled;
  // LayerNorm-folded path: row statistics, their per-slice partials, and every layer's folded weights (layer l at l * size)
  float *stats, *spart, *cq, *dq, *c1, *d1;
  bf16_t *wqkv_f, *w1_f;
  size_t bytes;
};

ClipWs clip_carve(void* ws, const tspo_clip_config& c, int n) {
  tspo::Carver cv(ws);
  ClipWs w;
  const int gw = c.image / c.patch, P = gw * gw, S = P + 1;
  const size_t M = (size_t)n * S;
  const int Kp = (int)tspo::align_up((size_t)3 * c.patch * c.patch, 64);
  // the LayerNorm-folded weights of EVERY layer, at the front (offsets independent of the batch size): a caller whose weights do
  // not change between calls says so (TSPO_CLIP_FOLD_CACHED) and the 2 x layers fold launches are skipped (round 5)
  const size_t Lf = (size_t)(c.layers > 0 ? c.layers : 1);
  w.wqkv_f = cv.take<bf16_t>(Lf * 3 * c.hidden * c.hidden);
  w.w1_f = cv.take<bf16_t>(Lf * c.mlp * c.hidden);
  w.cq = cv.take<float>(Lf * 3 * c.hidden);
  w.dq = cv.take<float>(Lf * 3 * c.hidden);
  w.c1 = cv.take<float>(Lf * c.mlp);
  w.d1 = cv.take<float>(Lf * c.mlp);
  w.x = cv.take<bf16_t>(M * c.hidden);
  w.h = cv.take<bf16_t>(M * c.hidden);
  w.qkv = cv.take<bf16_t>(M * 3 * c.hidden);
  w.a = cv.take<bf16_t>(M * c.hidden);
  w.u = cv.take<bf16_t>(M * c.mlp);
  w.patches = cv.take<bf16_t>((size_t)n * P * Kp);
  w.pooled = cv.take<bf16_t>((size_t)n * c.hidden);
  w.stats = cv.take<float>(M * 2);
  w.spart = cv.take<float>(M * (size_t)(c.hidden / 64) * 2);
  w.bytes = cv.bytes();
  return w;
}

int clip_check_cfg(const tspo_clip_config& c) {
  TSPO_REQUIRE(c.hidden >= 64 && c.hidden % 64 == 0 && c.hidden <= 4096, "clip: hidden=%d must be a multiple of 64 <= 4096", c.hidden);
  TSPO_REQUIRE(c.heads >= 1 && c.hidden == c.heads * 64, "clip: head_dim must be 64 (hidden=%d heads=%d)", c.hidden, c.heads);
  TSPO_REQUIRE(c.mlp >= 64 && c.mlp % 64 == 0, "clip: mlp=%d must be a multiple of 64", c.mlp);
  TSPO_REQUIRE(c.proj >= 8 && c.proj % 8 == 0, "clip: proj=%d must be a multiple of 8", c.proj);
  TSPO_REQUIRE(c.patch >= 1 && c.image >= c.patch && c.image % c.patch == 0, "clip: image=%d patch=%d", c.image, c.patch);
  const int gw = c.image / c.patch;
  TSPO_REQUIRE(gw * gw + 1 <= AT_KEYS, "clip: %d tokens exceed the %d-token attention kernel", gw * gw + 1, AT_KEYS);
  TSPO_REQUIRE(c.layers >= 0, "clip: layers=%d", c.layers);
  return TSPO_OK;
}

// Optional per-kernel-class timing with HIP events on the launch stream (bench / profiling only).
enum { PK_GEMM = 0, PK_ATTN = 1, PK_LN = 2, PK_GATHER = 3, PK_NKIND = 4 };
struct Prof {
  hipStream_t st;
  hipEvent_t ev[512];
  int kind[512];
  int n = 0;
  bool on = false;
  void start(hipStream_t s) { st = s; on = true; n = 0; tick(-1); }
  void tick(int k) {
    if (!on || n >= 512) return;
    (void)hipEventCreate(&ev[n]);
    (void)hipEventRecord(ev[n], st);
    kind[n] = k;
    ++n;
  }
  void finish(float* ms /* PK_NKIND + 2 */) {
    for (int i = 0; i < PK_NKIND + 2; ++i) ms[i] = 0.f;
    if (!on || n == 0) return;
    (void)hipEventSynchronize(ev[n - 1]);
    int ngemm = 0;
    for (int i = 1; i < n; ++i) {
      float t = 0.f;
      (void)hipEventElapsedTime(&t, ev[i - 1], ev[i]);
      ms[kind[i]] += t;
      ms[PK_NKIND] += t;
      ngemm += kind[i] == PK_GEMM;
    }
    ms[PK_NKIND + 1] = (float)ngemm;
    for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
  }
};

// ---------------------------------------------------------------------------
// Attention of the class-token query only (opt-in pruning of the LAST block: its other 256 token rows have no consumer,
// get_image_features pools row 0).  One wave per (frame, head): scores of q_0 against all S keys (lane j owns keys
// j, j+64, ...), softmax across the wave, then lane d accumulates sum_j p_j V[j][d] with p broadcast through LDS.
__global__ __launch_bounds__(64) void clip_attn_cls_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int S,
                                                           int C, float scale, int hm) {
  __shared__ float pl[AT_KEYS];
  const int lane = threadIdx.x, h = blockIdx.x;
  const size_t f = blockIdx.y, ld = hm ? 64 : (size_t)3 * C;
  const size_t hm_part = (size_t)gridDim.x * gridDim.y * S * 64;   // (see clip_attn257_kernel)
  const bf16_t* base = hm ? qkv + (((size_t)h * gridDim.y * S + f * S) << 6) : qkv + f * S * ld + (size_t)h * 64;
  const bf16_t* kbase = base + (hm ? hm_part : (size_t)C);
  const bf16_t* vbase = base + (hm ? 2 * hm_part : (size_t)2 * C);
  float q[64];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint4 raw = *reinterpret_cast<const uint4*>(base + c * 8);   // row 0, q columns (wave-uniform address)
    const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      q[c * 8 + 2 * j] = __uint_as_float(u[j] << 16);
      q[c * 8 + 2 * j + 1] = __uint_as_float(u[j] & 0xffff0000u);
    }
  }
  float sc[(AT_KEYS + 63) / 64];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < (AT_KEYS + 63) / 64; ++i) {
    const int key = lane + 64 * i;
    float d = -INFINITY;
    if (key < S) {
      const bf16_t* kr = kbase + (size_t)key * ld;
      d = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const uint4 raw = *reinterpret_cast<const uint4*>(kr + c * 8);
        const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          d += q[c * 8 + 2 * j] * __uint_as_float(u[j] << 16) + q[c * 8 + 2 * j + 1] * __uint_as_float(u[j] & 0xffff0000u);
      }
      d *= scale;
    }
    sc[i] = d;
    mx = fmaxf(mx, d);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < (AT_KEYS + 63) / 64; ++i) {
    const int key = lane + 64 * i;
    const float p = key < S ? __expf(sc[i] - mx) : 0.f;
    sum += p;
    if (key < AT_KEYS) pl[key] = p;
  }
  sum = wave_sum(sum);
  __syncthreads();
  float o = 0.f;
  const bf16_t* vb = vbase + lane;
  for (int key = 0; key < S; ++key) o += pl[key] * bf16_to_f32(vb[(size_t)key * ld]);
  o /= sum;
  // bf16 store of this head's 64 outputs of frame f (compact [n_frames, C] layout)
  const uint32_t pk = pack_bf16x2(o, __shfl_down(o, 1, 64));
  if ((lane & 1) == 0) *reinterpret_cast<uint32_t*>(out + f * (size_t)C + (size_t)h * 64 + lane) = pk;
}

// ---------------------------------------------------------------------------
// LayerNorm folded into the GEMMs around it (large batches).  LN(x) W^T = rstd * (x W'^T - mu * c) + (b + W beta) with
// W' = gamma o W and c[n] = sum_k W'[n,k]: the consumer GEMM reads the raw residual stream and its epilogue applies the
// per-row (mu, rstd); those come from partial sums the producer GEMM's residual epilogue writes (GE_RESID_ST), so the
// 48 per-layer LayerNorm passes (read + write of the whole [M, hidden] stream each) disappear.
// Fold of one weight matrix; one wave per output row n.  W' is rounded to bf16 exactly once (RNE) and c is the sum of the
// ROUNDED values, i.e. of what the MFMA multiplies, so the mean subtraction cancels exactly.
__global__ __launch_bounds__(256) void ln_fold_kernel(const bf16_t* __restrict__ W, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      int N, int K, bf16_t* __restrict__ Wf, float* __restrict__ c,
                                                      float* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const bf16_t* wr = W + (size_t)n * K;
  bf16_t* fr = Wf + (size_t)n * K;
  float cs = 0.f, ds = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const uint4 raw = *reinterpret_cast<const uint4*>(wr + k);
    const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + k), g1 = *reinterpret_cast<const f32x4*>(gamma + k + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + k), b1 = *reinterpret_cast<const f32x4*>(beta + k + 4);
    const float gm[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
    const float bt[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float w0 = __uint_as_float(u[j] << 16), w1 = __uint_as_float(u[j] & 0xffff0000u);
      o[j] = pack_bf16x2(w0 * gm[2 * j], w1 * gm[2 * j + 1]);
      cs += __uint_as_float(o[j] << 16) + __uint_as_float(o[j] & 0xffff0000u);
      ds += w0 * bt[2 * j] + w1 * bt[2 * j + 1];
    }
    *reinterpret_cast<uint4*>(fr + k) = make_uint4(o[0], o[1], o[2], o[3]);
  }
  cs = wave_sum(cs);
  ds = wave_sum(ds);
  if (lane == 0) {
    c[n] = cs;
    d[n] = bias[n] + ds;
  }
}

// (rstd, -mean*rstd) of each row of x [rows, C] (two-pass, the row lives in registers); one wave per row.  Only for the
// pre-LayerNorm output that enters layer 0; later statistics come out of the GEMM epilogues.
__global__ __launch_bounds__(256) void row_stats_kernel(const bf16_t* __restrict__ x, long rows, int C, float eps,
                                                        float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16_t* xr = x + row * C;
  float s = 0.f;
  for (int k = lane * 8; k < C; k += 512) {
    const uint4 raw = *reinterpret_cast<const uint4*>(xr + k);
    const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) s += __uint_as_float(u[j] << 16) + __uint_as_float(u[j] & 0xffff0000u);
  }
  const float mu = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int k = lane * 8; k < C; k += 512) {
    const uint4 raw = *reinterpret_cast<const uint4*>(xr + k);
    const uint32_t u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = __uint_as_float(u[j] << 16) - mu, b = __uint_as_float(u[j] & 0xffff0000u) - mu;
      q += a * a + b * b;
    }
  }
  const float var = wave_sum(q) / (float)C;
  const float rstd = rsqrtf(var + eps);
  if (lane == 0) *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(rstd, -mu * rstd);
}

// (rstd, -mean*rstd) from the per-64-column slice statistics (mean, centred sum of squares M2) a GE_RESID_ST epilogue
// wrote.  Slices are merged pairwise with Chan's formula (n = na + nb, d = mb - ma, mean = ma + d*nb/n,
// M2 = M2a + M2b + d*d*na*nb/n) in a fixed xor tree over 16 lanes per row -> deterministic and as robust as two passes.
__global__ __launch_bounds__(256) void stats_finalize_kernel(const float* __restrict__ part, long rows, int np, int C,
                                                             float eps, float* __restrict__ stats) {
  const int sub = threadIdx.x & 15;
  const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = row < rows;
  const float2* pr = reinterpret_cast<const float2*>(part) + (live ? row : 0) * np;
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int i = sub; i < np; i += 16) {   // (coalesced 128-byte reads per row)
    const float2 v = pr[i];
    const float nn = n + 64.f, d = v.x - mean;
    mean += d * (64.f / nn);
    m2 += v.y + d * d * (n * 64.f / nn);
    n = nn;
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const float nb = __shfl_xor(n, o, 16), mb = __shfl_xor(mean, o, 16), qb = __shfl_xor(m2, o, 16);
    const float nn = n + nb;
    if (nn > 0.f) {
      // symmetric in (a, b): both partners compute the same merged triple
      const float d = mb - mean;
      const float wgt = nb / nn;
      const float merged_mean = (n * mean + nb * mb) / nn;
      m2 = m2 + qb + d * d * (n * wgt);
      mean = merged_mean;
      n = nn;
    }
  }
  if (live && sub == 0) {
    const float var = fmaxf(m2 / (float)C, 0.f);
    const float rstd = rsqrtf(var + eps);
    *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(rstd, -mean * rstd);
  }
}

// The same for exactly 16 slices (C = 1024, CLIP-L): every merge of the tree joins two groups of EQUAL size, for which
// Chan's formula needs no division (mean = (ma + mb)/2, M2 = M2a + M2b + d*d*n_a/2).  4 lanes per row, each with 4
// consecutive slices in two 16-byte loads (a row's 128 bytes stay coalesced), 2 cross-lane rounds instead of 4:
// 24 -> 9 us per call, 47 calls per forward.
__global__ __launch_bounds__(256) void stats_finalize16_kernel(const float* __restrict__ part, long rows, int C, float eps,
                                                               float* __restrict__ stats) {
  const int sub = threadIdx.x & 3;
  const long row = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const bool live = row < rows;
  const f32x4* pr = reinterpret_cast<const f32x4*>(part) + ((live ? row : 0) * 16 + sub * 4) / 2;   // 2 (mean, M2) pairs each
  const f32x4 u = pr[0], v = pr[1];
  auto merge = [](float ma, float qa, float mb, float qb, float na, float& m, float& q) {   // two groups of na values each
    const float d = mb - ma;
    m = 0.5f * (ma + mb);
    q = (qa + qb) + d * d * (0.5f * na);
  };
  float m01, q01, m23, q23, mean, m2;
  merge(u[0], u[1], u[2], u[3], 64.f, m01, q01);
  merge(v[0], v[1], v[2], v[3], 64.f, m23, q23);
  merge(m01, q01, m23, q23, 128.f, mean, m2);
  float na = 256.f;
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {   // (symmetric in its operands up to the sign of d: both partners get the same pair)
    const float mb = __shfl_xor(mean, o, 4), qb = __shfl_xor(m2, o, 4);
    const float d = mb - mean;
    mean = 0.5f * (mean + mb);
    m2 = (m2 + qb) + d * d * (0.5f * na);
    na *= 2.f;
  }
  if (live && sub == 0) {
    const float var = fmaxf(m2 / (float)C, 0.f);
    const float rstd = rsqrtf(var + eps);
    *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(rstd, -mean * rstd);
  }
}

void launch_stats_finalize(const float* spart, long M, int C, float eps, float* stats, hipStream_t st) {
  if (C == 1024)
    hipLaunchKernelGGL(stats_finalize16_kernel, dim3((unsigned)((M + 63) / 64)), dim3(256), 0, st, spart, M, C, eps, stats);
  else
    hipLaunchKernelGGL(stats_finalize_kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, st, spart, M, C / 64, C, eps, stats);
}

int run_ln(const bf16_t* in, bf16_t* out, const float* g, const float* b, long rows, int C, long is, long os, float eps,
           hipStream_t st) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (C <= 1024) hipLaunchKernelGGL(layernorm_kernel<2>, grid, dim3(256), 0, st, in, out, g, b, rows, C, is, os, eps);
  else if (C <= 2048) hipLaunchKernelGGL(layernorm_kernel<4>, grid, dim3(256), 0, st, in, out, g, b, rows, C, is, os, eps);
  else hipLaunchKernelGGL(layernorm_kernel<8>, grid, dim3(256), 0, st, in, out, g, b, rows, C, is, os, eps);
  return tspo::check_launch("layernorm");
}

}  // namespace

extern "C" size_t tspo_clip_workspace_bytes(const tspo_clip_config* cfg, int n_frames) {
  if (!cfg || n_frames < 1 || cfg->patch < 1 || cfg->image < cfg->patch) return 0;
  return clip_carve(nullptr, *cfg, n_frames).bytes;
}

// The fold decision of an encode of n frames: the LayerNorm-folded epilogues exist only in the persistent 256x256 kernel, so the
// layer's GEMM shapes must be "big" problems (gemm_bf16_is_big).  The ONE place it is written down: clip_forward_impl,
// tspo_clip_will_fold and the chunk planner all call this.
static bool clip_folds(const tspo_clip_config& c, long n_frames) {
  const int gw = c.image / c.patch;
  const long M = n_frames * ((long)gw * gw + 1);
  return c.layers > 0 && tspo::gemm_bf16_is_big(M, c.hidden, c.hidden) && tspo::gemm_bf16_is_big(M, c.hidden, c.mlp);
}

// Smallest batch that folds (clip_folds is monotone in n_frames), or 0 for a config that never folds.
static int clip_min_fold_frames(const tspo_clip_config& c) {
  const int gw = c.image / c.patch;
  long hi = ((1L << 31) - 1) / ((long)gw * gw + 1);   // the forward entries take M < 2^31 rows
  if (!clip_folds(c, hi)) return 0;
  long lo = 1;
  while (lo < hi) {
    const long mid = lo + (hi - lo) / 2;
    if (clip_folds(c, mid)) hi = mid; else lo = mid + 1;
  }
  return (int)lo;
}

extern "C" int tspo_clip_will_fold(const tspo_clip_config* cfg, int n_frames) {
  TSPO_REQUIRE(cfg, "clip_will_fold: null config");
  TSPO_REQUIRE(n_frames >= 1, "clip_will_fold: n_frames=%d", n_frames);
  TSPO_REQUIRE(cfg->patch >= 1 && cfg->image >= cfg->patch, "clip_will_fold: image=%d patch=%d", cfg->image, cfg->patch);
  return clip_folds(*cfg, n_frames) ? 1 : 0;
}

// The chunk plan (include/tspo_hip.h).  With b = 64 frames: count = ceil(n / chunk); the first count-1 chunks hold j blocks of b
// frames in all, each between ceil(f / b) and floor(chunk / b) blocks, and the last chunk holds n - j b frames in [f, chunk], where
// f = the smallest folding batch when n frames fold, else 1.  The largest such j is taken (full leading chunks, the smallest tail
// that still folds) and spread evenly.  Returns count and, when sizes != nullptr, writes them; *largest gets the largest chunk.
static int clip_plan(const tspo_clip_config& c, int n, int chunk, int* sizes, int cap, int* largest) {
  TSPO_REQUIRE(n >= 1, "clip_chunk_plan: n_frames=%d", n);
  TSPO_REQUIRE(chunk >= 1, "clip_chunk_plan: chunk_frames=%d", chunk);
  // (only the geometry the fold decision reads is needed here, as for tspo_clip_workspace_bytes; the forward checks the rest)
  TSPO_REQUIRE(c.patch >= 1 && c.image >= c.patch, "clip_chunk_plan: image=%d patch=%d", c.image, c.patch);
  const int gw = c.image / c.patch;
  TSPO_REQUIRE((long)n * ((long)gw * gw + 1) < (1L << 31), "clip_chunk_plan: n_frames=%d too large", n);
  const int fmin = clip_min_fold_frames(c);
  TSPO_REQUIRE(fmin == 0 || chunk >= fmin,
               "clip_chunk_plan: chunk_frames=%d is below the %d frames at which this encoder folds its LayerNorms - such chunks "
               "would take the slower small-batch path and compute other bits", chunk, fmin);
  const long b = 64;
  const long f = clip_folds(c, n) ? fmin : 1;
  const long count = ((long)n + chunk - 1) / chunk;
  TSPO_REQUIRE(sizes && cap >= count, "clip_chunk_plan: %ld chunks do not fit sizes[%d]", count, sizes ? cap : 0);
  if (count == 1) {
    sizes[0] = n;
    if (largest) *largest = n;
    return 1;
  }
  const long bmax = chunk / b, bmin = (f + b - 1) / b, lead = count - 1;
  long j = (n - f) / b;
  if (j > lead * bmax) j = lead * bmax;
  TSPO_REQUIRE(bmax >= bmin && j >= lead * bmin && n - j * b <= chunk,
               "clip_chunk_plan: no plan cuts %d frames into %ld chunks of at most %d frames with every chunk but the last a multiple "
               "of 64 frames and none under %ld frames - use a chunk_frames that is a multiple of 64 and at least %ld",
               n, count, chunk, f, 2 * bmin * b);
  const long base = j / lead, extra = j % lead;
  int mx = 0;
  for (long i = 0; i < count; ++i) {
    const int s = (int)(i < lead ? (base + (i < extra ? 1 : 0)) * b : n - j * b);
    sizes[i] = s;
    if (s > mx) mx = s;
  }
  if (largest) *largest = mx;
  return (int)count;
}

extern "C" int tspo_clip_chunk_plan(const tspo_clip_config* cfg, int n_frames, int chunk_frames, int* sizes, int cap) {
  TSPO_REQUIRE(cfg, "clip_chunk_plan: null config");
  return clip_plan(*cfg, n_frames, chunk_frames, sizes, cap, nullptr);
}

extern "C" int tspo_gemm_bf16(const void* A, const void* W, const float* bias, const void* residual, void* C,
                              int out_dtype, int M, int N, int K, int act, tspo_stream_t stream) {
  TSPO_REQUIRE(A && W && C, "gemm_bf16: null pointer");
  TSPO_REQUIRE(M >= 1 && N >= 8 && N % 8 == 0 && K >= 64 && K % 64 == 0, "gemm_bf16: bad dims M=%d N=%d K=%d", M, N, K);
  GemmArgs g{};
  g.A = (const bf16_t*)A; g.W = (const bf16_t*)W; g.bias = bias; g.R = (const bf16_t*)residual; g.C = C;
  g.M = M; g.N = N; g.K = K; g.P = 1;
  const int variant = act >> 8;
  act &= 0xff;
  int epi;
  if (out_dtype == TSPO_F32) {
    TSPO_REQUIRE(!bias && !residual && act == 0, "gemm_bf16: f32 output supports no epilogue");
    epi = GE_F32;
  } else {
    TSPO_REQUIRE(out_dtype == TSPO_BF16, "gemm_bf16: out_dtype must be TSPO_BF16 or TSPO_F32");
    TSPO_REQUIRE(bias, "gemm_bf16: bf16 output needs a bias vector");
    TSPO_REQUIRE(!(residual && act), "gemm_bf16: residual and activation are exclusive");
    epi = residual ? GE_RESID : (act == 1 ? GE_GELU : GE_BIAS);
  }
  g.variant = variant;
  return tspo::gemm_bf16(epi, g, (hipStream_t)stream);
}

static int clip_forward_impl(const tspo_clip_weights* w, const void* pixels, int pixel_dtype, int n_frames, float* feat,
                             void* workspace, size_t workspace_bytes, tspo_stream_t stream, int flags, Prof& prof) {
  TSPO_REQUIRE(w && pixels && feat && workspace, "clip_vit_forward: null pointer");
  TSPO_REQUIRE(n_frames >= 1, "clip_vit_forward: n_frames=%d", n_frames);
  const tspo_clip_config& c = w->cfg;
  if (int e = clip_check_cfg(c)) return e;
  TSPO_REQUIRE((flags & ~(TSPO_CLIP_NO_LN_FOLD | TSPO_CLIP_PRUNE_LAST | TSPO_CLIP_FOLD_CACHED)) == 0,
               "clip_vit_forward: unknown flags 0x%x", flags);
  const bool fold_cached = (flags & TSPO_CLIP_FOLD_CACHED) != 0;   // the caller vouches for the folded weights in this workspace
  const bool no_fold = (flags & TSPO_CLIP_NO_LN_FOLD) != 0;   // keep the stand-alone LayerNorm passes
  const bool prune = (flags & TSPO_CLIP_PRUNE_LAST) != 0;     // opt-in: last block evaluated for the class-token row only
  TSPO_REQUIRE(w->patch_w && w->pos_emb && w->pre_g && w->pre_b && w->post_g && w->post_b && w->proj_w &&
                   (c.layers == 0 || w->layers),
               "clip_vit_forward: null weight pointer");
  ClipWs b = clip_carve(workspace, c, n_frames);
  if (workspace_bytes < b.bytes)
    return tspo::set_err(TSPO_EWORKSPACE, "clip_vit_forward: workspace %zu < %zu", workspace_bytes, b.bytes);
  hipStream_t st = (hipStream_t)stream;
  const int gw = c.image / c.patch, P = gw * gw, S = P + 1, C = c.hidden;
  const int Kp = (int)tspo::align_up((size_t)3 * c.patch * c.patch, 64);
  const long M = (long)n_frames * S;
  TSPO_REQUIRE(M * (long)c.mlp < (1L << 40) && M < (1L << 31), "clip_vit_forward: n_frames too large");

  // 1. patch gather (+ normalise) and CLS rows
  {
    const size_t total = (size_t)n_frames * P * (Kp / 8);
    unsigned nb = (unsigned)((total + 255) / 256);
    if (nb > 65536u) nb = 65536u;
    switch (pixel_dtype) {
      case TSPO_F32: hipLaunchKernelGGL(patch_gather_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)pixels, b.patches, n_frames, c.image, c.patch, Kp); break;
      case TSPO_BF16: hipLaunchKernelGGL(patch_gather_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)pixels, b.patches, n_frames, c.image, c.patch, Kp); break;
      case TSPO_F16: hipLaunchKernelGGL(patch_gather_kernel<_Float16>, dim3(nb), dim3(256), 0, st, (const _Float16*)pixels, b.patches, n_frames, c.image, c.patch, Kp); break;
      case TSPO_U8:
        if (c.image == 224 && c.patch == 14 && Kp == 640 && ((uintptr_t)pixels & 15) == 0)
          hipLaunchKernelGGL(patch_gather_u8_l14_kernel, dim3(16, n_frames), dim3(256), 0, st, (const uint8_t*)pixels, b.patches);
        else if (c.image == 224 && c.patch == 14 && Kp == 640)
          hipLaunchKernelGGL((patch_gather_kernel<uint8_t, 224, 14, 640>), dim3(nb), dim3(256), 0, st, (const uint8_t*)pixels, b.patches, n_frames, c.image, c.patch, Kp);
        else
          hipLaunchKernelGGL(patch_gather_kernel<uint8_t>, dim3(nb), dim3(256), 0, st, (const uint8_t*)pixels, b.patches, n_frames, c.image, c.patch, Kp);
        break;
      default: return tspo::set_err(TSPO_EINVAL, "clip_vit_forward: bad pixel_dtype %d", pixel_dtype);
    }
    unsigned cb = (unsigned)(((size_t)n_frames * C + 255) / 256);
    if (cb > 4096u) cb = 4096u;
    hipLaunchKernelGGL(cls_rows_kernel, dim3(cb), dim3(256), 0, st, w->pos_emb, b.x, n_frames, S, C);
    prof.tick(PK_GATHER);
  }
  // 2. patch embedding GEMM (+ position embedding, rows remapped past each frame's CLS row)
  {
    GemmArgs g{};
    g.A = b.patches; g.W = (const bf16_t*)w->patch_w; g.C = b.x; g.pos = w->pos_emb;
    g.M = n_frames * P; g.N = C; g.K = Kp; g.P = P;
    if (int e = tspo::gemm_bf16(GE_PATCH, g, st)) return e;
    prof.tick(PK_GEMM);
  }
  // 3. pre-LN (in place)
  if (int e = run_ln(b.x, b.x, w->pre_g, w->pre_b, M, C, C, C, c.ln_eps, st)) return e;
  prof.tick(PK_LN);
  // 4. transformer blocks.  Large batches: LayerNorm folded into the GEMMs (see ln_fold_kernel); otherwise stand-alone passes.
  const bool fold = !no_fold && clip_folds(c, n_frames);
  if (fold) {
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, b.x, M, C, c.ln_eps, b.stats);
    if (int e = tspo::check_launch("row_stats")) return e;
    prof.tick(PK_LN);
  }
  bool pooled_done = false;
  // the folded q/k/v GEMM writes its output head-major for the 257-token attention kernel (GE_BIAS_LN_HM, gemm_bf16.h)
  const int hm = (fold && S == 257 && c.heads * 64 == C) ? 1 : 0;
  for (int l = 0; l < c.layers; ++l) {
    const tspo_clip_layer& L = w->layers[l];
    TSPO_REQUIRE(L.ln1_g && L.ln1_b && L.wqkv && L.bqkv && L.wo && L.bo && L.ln2_g && L.ln2_b && L.w1 && L.b1 && L.w2 && L.b2,
                 "clip_vit_forward: null pointer in layer %d", l);
    GemmArgs g{};
    // this layer's folded weights / column sums / folded biases
    bf16_t* wqkv_f = b.wqkv_f + (size_t)l * 3 * C * C;
    bf16_t* w1_f = b.w1_f + (size_t)l * c.mlp * C;
    float *cq = b.cq + (size_t)l * 3 * C, *dq = b.dq + (size_t)l * 3 * C, *c1 = b.c1 + (size_t)l * c.mlp, *d1 = b.d1 + (size_t)l * c.mlp;
    if (fold) {
      if (!fold_cached) {
        hipLaunchKernelGGL(ln_fold_kernel, dim3((3 * C + 3) / 4), dim3(256), 0, st, (const bf16_t*)L.wqkv, L.bqkv, L.ln1_g, L.ln1_b,
                           3 * C, C, wqkv_f, cq, dq);
        hipLaunchKernelGGL(ln_fold_kernel, dim3((c.mlp + 3) / 4), dim3(256), 0, st, (const bf16_t*)L.w1, L.b1, L.ln2_g, L.ln2_b,
                           c.mlp, C, w1_f, c1, d1);
        if (int e = tspo::check_launch("ln_fold")) return e;
        prof.tick(PK_LN);
      }
      g.A = b.x; g.W = wqkv_f; g.bias = dq; g.lnc = cq; g.rstats = b.stats; g.C = b.qkv;
      g.M = (int)M; g.N = 3 * C; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(hm ? GE_BIAS_LN_HM : GE_BIAS_LN, g, st)) return e;
    } else {
      if (int e = run_ln(b.x, b.h, L.ln1_g, L.ln1_b, M, C, C, C, c.ln_eps, st)) return e;
      prof.tick(PK_LN);
      g.A = b.h; g.W = (const bf16_t*)L.wqkv; g.bias = L.bqkv; g.C = b.qkv; g.M = (int)M; g.N = 3 * C; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_BIAS, g, st)) return e;
    }
    prof.tick(PK_GEMM);
    if (prune && l == c.layers - 1) {
      // Only row 0 of every frame leaves the encoder (post-LN + projection of the class token), so the rest of this
      // block runs on the compact [n_frames, C] class-token rows: attention of q_0, out-proj, LN2, MLP.
      bf16_t* xc = b.h + (size_t)n_frames * C;   // class-token residual rows (b.h is free here); LN2 output goes to b.h
      hipLaunchKernelGGL(clip_attn_cls_kernel, dim3(c.heads, n_frames), dim3(64), 0, st, b.qkv, b.a, S, C, 0.125f, hm);
      if (int e = tspo::check_launch("clip_attn_cls")) return e;
      prof.tick(PK_ATTN);
      hipError_t ce = hipMemcpy2DAsync(xc, (size_t)C * 2, b.x, (size_t)S * C * 2, (size_t)C * 2, n_frames,
                                       hipMemcpyDeviceToDevice, st);
      if (ce != hipSuccess) return tspo::set_err(TSPO_ELAUNCH, "clip_vit_forward: class-row gather: %s", hipGetErrorString(ce));
      g = GemmArgs{};
      g.A = b.a; g.W = (const bf16_t*)L.wo; g.bias = L.bo; g.R = xc; g.C = xc; g.M = n_frames; g.N = C; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_RESID, g, st)) return e;
      prof.tick(PK_GEMM);
      if (int e = run_ln(xc, b.h, L.ln2_g, L.ln2_b, n_frames, C, C, C, c.ln_eps, st)) return e;
      prof.tick(PK_LN);
      g = GemmArgs{};
      g.A = b.h; g.W = (const bf16_t*)L.w1; g.bias = L.b1; g.C = b.u; g.M = n_frames; g.N = c.mlp; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_GELU, g, st)) return e;
      prof.tick(PK_GEMM);
      g = GemmArgs{};
      g.A = b.u; g.W = (const bf16_t*)L.w2; g.bias = L.b2; g.R = xc; g.C = xc; g.M = n_frames; g.N = C; g.K = c.mlp; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_RESID, g, st)) return e;
      prof.tick(PK_GEMM);
      if (int e = run_ln(xc, b.pooled, w->post_g, w->post_b, n_frames, C, C, C, c.ln_eps, st)) return e;
      prof.tick(PK_LN);
      pooled_done = true;
      break;
    }
    if (S == 257) hipLaunchKernelGGL(clip_attn257_kernel, dim3(c.heads, n_frames), dim3(256), 0, st, b.qkv, b.a, C, 0.125f, hm);
    else hipLaunchKernelGGL(clip_attn_kernel<0>, dim3(c.heads, n_frames), dim3(256), 0, st, b.qkv, b.a, S, C, 0.125f);
    if (int e = tspo::check_launch("clip_attn")) return e;
    prof.tick(PK_ATTN);
    g = GemmArgs{};
    g.A = b.a; g.W = (const bf16_t*)L.wo; g.bias = L.bo; g.R = b.x; g.C = b.x; g.M = (int)M; g.N = C; g.K = C; g.P = 1;
    g.spart = b.spart;
    if (int e = tspo::gemm_bf16(fold ? GE_RESID_ST : GE_RESID, g, st)) return e;
    prof.tick(PK_GEMM);
    g = GemmArgs{};
    if (fold) {
      launch_stats_finalize(b.spart, M, C, c.ln_eps, b.stats, st);
      if (int e = tspo::check_launch("stats_finalize")) return e;
      prof.tick(PK_LN);
      g.A = b.x; g.W = w1_f; g.bias = d1; g.lnc = c1; g.rstats = b.stats; g.C = b.u;
      g.M = (int)M; g.N = c.mlp; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_GELU_LN, g, st)) return e;
    } else {
      if (int e = run_ln(b.x, b.h, L.ln2_g, L.ln2_b, M, C, C, C, c.ln_eps, st)) return e;
      prof.tick(PK_LN);
      g.A = b.h; g.W = (const bf16_t*)L.w1; g.bias = L.b1; g.C = b.u; g.M = (int)M; g.N = c.mlp; g.K = C; g.P = 1;
      if (int e = tspo::gemm_bf16(GE_GELU, g, st)) return e;
    }
    prof.tick(PK_GEMM);
    g = GemmArgs{};
    g.A = b.u; g.W = (const bf16_t*)L.w2; g.bias = L.b2; g.R = b.x; g.C = b.x; g.M = (int)M; g.N = C; g.K = c.mlp; g.P = 1;
    g.spart = b.spart;
    const bool next_needs_stats = fold && l + 1 < c.layers;   // the last block's output only feeds the CLS post-LN
    if (int e = tspo::gemm_bf16(next_needs_stats ? GE_RESID_ST : GE_RESID, g, st)) return e;
    prof.tick(PK_GEMM);
    if (next_needs_stats) {
      launch_stats_finalize(b.spart, M, C, c.ln_eps, b.stats, st);
      if (int e = tspo::check_launch("stats_finalize")) return e;
      prof.tick(PK_LN);
    }
  }
  // 5. CLS pool + post-LN + projection
  if (!pooled_done) {
    if (int e = run_ln(b.x, b.pooled, w->post_g, w->post_b, n_frames, C, (long)S * C, C, c.ln_eps, st)) return e;
    prof.tick(PK_LN);
  }
  {
    GemmArgs g{};
    g.A = b.pooled; g.W = (const bf16_t*)w->proj_w; g.C = feat; g.M = n_frames; g.N = c.proj; g.K = C; g.P = 1;
    if (int e = tspo::gemm_bf16(GE_F32, g, st)) return e;
    prof.tick(PK_GEMM);
  }
  return TSPO_OK;
}

extern "C" int tspo_clip_vit_forward_ex(const tspo_clip_weights* w, const void* pixels, int pixel_dtype, int n_frames,
                                        float* feat, void* workspace, size_t workspace_bytes, tspo_stream_t stream,
                                        int flags) {
  Prof prof;
  return clip_forward_impl(w, pixels, pixel_dtype, n_frames, feat, workspace, workspace_bytes, stream, flags, prof);
}

extern "C" int tspo_clip_vit_forward_chunked(const tspo_clip_weights* w, const void* pixels, int pixel_dtype, int n_frames,
                                             int chunk_frames, float* feat, void* workspace, size_t workspace_bytes,
                                             tspo_stream_t stream, int flags) {
  TSPO_REQUIRE(w && pixels && feat && workspace, "clip_vit_forward_chunked: null pointer");
  TSPO_REQUIRE((flags & ~(TSPO_CLIP_NO_LN_FOLD | TSPO_CLIP_PRUNE_LAST | TSPO_CLIP_FOLD_CACHED)) == 0,
               "clip_vit_forward_chunked: unknown flags 0x%x", flags);
  size_t px_bytes;
  switch (pixel_dtype) {
    case TSPO_F32: px_bytes = 4; break;
    case TSPO_BF16: case TSPO_F16: px_bytes = 2; break;
    case TSPO_U8: px_bytes = 1; break;
    default: return tspo::set_err(TSPO_EINVAL, "clip_vit_forward_chunked: bad pixel_dtype %d", pixel_dtype);
  }
  const tspo_clip_config& c = w->cfg;
  if (int e = clip_check_cfg(c)) return e;
  TSPO_REQUIRE(n_frames >= 1 && chunk_frames >= 1, "clip_vit_forward_chunked: n_frames=%d chunk_frames=%d", n_frames, chunk_frames);
  const long count = ((long)n_frames + chunk_frames - 1) / chunk_frames;
  std::vector<int> sizes((size_t)count);   // host memory
  int largest = 0;
  const int nc = clip_plan(c, n_frames, chunk_frames, sizes.data(), (int)count, &largest);
  if (nc < 0) return nc;
  const size_t need = clip_carve(nullptr, c, largest).bytes;
  if (workspace_bytes < need)
    return tspo::set_err(TSPO_EWORKSPACE, "clip_vit_forward_chunked: workspace %zu < %zu (chunks of up to %d frames)",
                         workspace_bytes, need, largest);
  px_bytes *= (size_t)3 * c.image * c.image;
  Prof prof;
  size_t lo = 0;
  for (int i = 0; i < nc; ++i) {
    // every chunk folds when the first does (the plan), and the folded weights sit at offsets that do not depend on the batch
    const int fl = flags | (i > 0 ? TSPO_CLIP_FOLD_CACHED : 0);
    if (int e = clip_forward_impl(w, (const char*)pixels + lo * px_bytes, pixel_dtype, sizes[i], feat + lo * c.proj, workspace,
                                  workspace_bytes, stream, fl, prof))
      return e;
    lo += (size_t)sizes[i];
  }
  return TSPO_OK;
}

extern "C" int tspo_clip_vit_forward(const tspo_clip_weights* w, const void* pixels, int pixel_dtype, int n_frames,
                                     float* feat, void* workspace, size_t workspace_bytes, tspo_stream_t stream) {
  return tspo_clip_vit_forward_ex(w, pixels, pixel_dtype, n_frames, feat, workspace, workspace_bytes, stream, 0);
}

extern "C" int tspo_clip_vit_profile(const tspo_clip_weights* w, const void* pixels, int pixel_dtype, int n_frames,
                                     float* feat, void* workspace, size_t workspace_bytes, tspo_stream_t stream,
                                     float* host_ms6, int flags) {
  TSPO_REQUIRE(host_ms6, "clip_vit_profile: null host_ms6");
  static thread_local Prof prof;  // 512 events: keep it off the stack
  prof.start((hipStream_t)stream);
  const int rc = clip_forward_impl(w, pixels, pixel_dtype, n_frames, feat, workspace, workspace_bytes, stream, flags, prof);
  prof.finish(host_ms6);
  prof.on = false;
  return rc;
}
