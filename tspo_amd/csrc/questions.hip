// One video, Q questions: the text-dependent tail of the scoring path for gfx950.
//
// The reference's index generation is driven once per QUESTION (mp_tools/vlmeval/vlm/gen_id_tspo.py:59-92, cache keyed by the
// question's index), the benchmarks ask several questions per video, and only the last step of MultiModal_Align.forward reads the
// text (model/temporal_agent.py:135-141; clip scores :167).  These two kernels are that step for Q texts against ONE set of frame
// rows: each frame row is read once and Q outputs leave, every one the bits the per-question kernels of selector.hip
// (score_fwd_kernel, clip_scores_kernel) produce for it.
//
// Bit identity.  hipcc contracts a*b + c into an fma where it likes, and in score_fwd_kernel it liked differently per quantity
// and per 64-float4 chunk of the row (read off its ISA; what the compiler made of dot4 / row_dots of score_rows.h there):
//   h.e   fma(e.y, h.y, e.x h.x) + fma(e.w, h.w, e.z h.z)                       every chunk
//   e.e   fma(e.x, e.x, e.y e.y) + fma(e.z, e.z, e.w e.w)                       every chunk
//   h.h   (h.x h.x + h.y h.y) + (h.z h.z + h.w h.w), separate roundings          chunks 0, 1, 3
//         fma(h.x, h.x, h.y h.y) + fma(h.z, h.z, h.w h.w)                       chunk 2
//   |h||e| + 1e-6   multiply, then add (not fused); clip_scores_kernel: every accumulation one fma.
// A loop of another shape would be contracted another way, so this unit turns contraction off and spells those forms out;
// the additions keep the order of the source (no reassociation without fast-math).  tests/test_gpu_questions.py compares the bits
// against the per-question entries at every row form; if a compiler changes what it makes of score_fwd_kernel, that test fails
// and the table above is what to re-read from `hipcc -S`.
#include "score_rows.h"

#pragma clang fp contract(off)

namespace {

constexpr int kQChunk = 16;   // questions per workgroup row: h2 / feat are re-read once per chunk of 16 questions, not once per question

__device__ __forceinline__ float he4(const f32x4 h, const f32x4 e) {
  return __builtin_fmaf(e[1], h[1], e[0] * h[0]) + __builtin_fmaf(e[3], h[3], e[2] * h[2]);
}
__device__ __forceinline__ float ee4(const f32x4 e) {
  return __builtin_fmaf(e[0], e[0], e[1] * e[1]) + __builtin_fmaf(e[2], e[2], e[3] * e[3]);
}
__device__ __forceinline__ float hh4(const f32x4 h, int chunk) {
  if (chunk == 2) return __builtin_fmaf(h[0], h[0], h[1] * h[1]) + __builtin_fmaf(h[2], h[2], h[3] * h[3]);
  return (h[0] * h[0] + h[1] * h[1]) + (h[2] * h[2] + h[3] * h[3]);
}

// this lane's float4 chunks c0 + 64 i (i < 4) of a row of nv float4; zeros past the end, as row_dots
__device__ __forceinline__ void load4(const f32x4* __restrict__ r, int c0, int nv, f32x4 (&v)[4]) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + 64 * i;
    v[i] = c < nv ? r[c] : z;
  }
}

// scores[q, t] = (mean_m h_t.e_qm / (|h_t||e_qm| + 1e-6) + clip[q, t]) / tau for the questions of chunk blockIdx.y.
// One wave per frame row t, four rows per workgroup.  The first 256 float4 of the row (all of it for D <= 1024) stay in 16
// registers per lane for every text row; |h| is formed once.  Longer rows re-read their tail per text row (L2).
__global__ __launch_bounds__(256) void score_questions_kernel(const float* __restrict__ h, const float* __restrict__ txt,
                                                              const float* __restrict__ clip, float* __restrict__ scores,
                                                              int Q, int T, int D, int M, float tau) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int q0 = blockIdx.y * kQChunk, q1 = min(Q, q0 + kQChunk);
  const f32x4* hr = reinterpret_cast<const f32x4*>(h + row * D);
  const int nv = D >> 2;   // D % 64 == 0
  f32x4 h0[4];
  load4(hr, lane, nv, h0);
  float hh = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) hh += hh4(h0[i], i);
  for (int c0 = lane + 256; c0 < nv; c0 += 256) {
    f32x4 hv[4];
    load4(hr, c0, nv, hv);
#pragma unroll
    for (int i = 0; i < 4; ++i) hh += hh4(hv[i], i);
  }
  const float hn = sqrtf(wave_sum(hh));
  // text rows r = q M + m of this chunk; the first 256 float4 of row r + 1 are requested before the reductions of row r
  const f32x4* tr = reinterpret_cast<const f32x4*>(txt);
  const long r_last = (long)q1 * M - 1;
  f32x4 en_[4];
  load4(tr + (size_t)q0 * M * nv, lane, nv, en_);
  for (int q = q0; q < q1; ++q) {
    float acc = 0.f;
    for (int m = 0; m < M; ++m) {
      const long r = (long)q * M + m;
      const f32x4* er = tr + (size_t)r * nv;
      f32x4 ev[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ev[i] = en_[i];
      load4(tr + (size_t)(r < r_last ? r + 1 : r_last) * nv, lane, nv, en_);
      float de = 0.f, ee = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        de += he4(h0[i], ev[i]);
        ee += ee4(ev[i]);
      }
      for (int c0 = lane + 256; c0 < nv; c0 += 256) {
        f32x4 hv[4];
        load4(hr, c0, nv, hv);
        load4(er, c0, nv, ev);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          de += he4(hv[i], ev[i]);
          ee += ee4(ev[i]);
        }
      }
      de = wave_sum(de);
      const float en = sqrtf(wave_sum(ee));
      acc += de / (hn * en + 1e-6f);
    }
    if (lane == 0) {
      const size_t o = (size_t)q * T + row;
      float s = acc / (float)M;
      s = s + (clip ? clip[o] : 0.f);
      scores[o] = s / tau;
    }
  }
}

// clip[q, t] = cos(txt[q, 0, :], feat[t, :]) like torch.nn.CosineSimilarity(dim=-1, eps=1e-8): clip_scores_kernel's summation
// (4-byte loads, d = lane; d += 64, one fma per accumulation), one pass over the frame row for the nq <= kQChunk questions of
// blockIdx.y, |f|^2 once per pass.  N accumulator pairs, branch-free: slots j >= nq recompute question nq - 1 and are dropped, so
// the N text loads of a step are in flight together.
template <int N>
__device__ __forceinline__ void clip_rows(const float* __restrict__ er, const float* __restrict__ fr, float* __restrict__ out,
                                          size_t qs, int nq, int T, int D, int lane) {
  float de[N], ee[N], ff = 0.f;
  const float* ej[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    de[j] = ee[j] = 0.f;
    ej[j] = er + (size_t)(j < nq ? j : nq - 1) * qs;
  }
  for (int d = lane; d < D; d += 64) {
    const float x = fr[d];
    float e[N];
#pragma unroll
    for (int j = 0; j < N; ++j) e[j] = ej[j][d];
    ff = __builtin_fmaf(x, x, ff);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      de[j] = __builtin_fmaf(e[j], x, de[j]);
      ee[j] = __builtin_fmaf(e[j], e[j], ee[j]);
    }
  }
  ff = wave_sum(ff);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float d_ = wave_sum(de[j]), e_ = wave_sum(ee[j]);
    if (lane == 0 && j < nq) out[(size_t)j * T] = d_ / sqrtf(fmaxf(e_ * ff, 1e-16f));
  }
}
__global__ __launch_bounds__(256) void clip_scores_questions_kernel(const float* __restrict__ txt, const float* __restrict__ f,
                                                                    float* __restrict__ out, int Q, int T, int D, int M) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const int q0 = blockIdx.y * kQChunk, nq = min(Q - q0, kQChunk);
  const float* fr = f + row * D;
  const float* er = txt + (size_t)q0 * M * D;
  float* o = out + (size_t)q0 * T + row;
  const size_t qs = (size_t)M * D;
  if (nq > 4)
    clip_rows<kQChunk>(er, fr, o, qs, nq, T, D, lane);
  else if (nq > 1)
    clip_rows<4>(er, fr, o, qs, nq, T, D, lane);
  else
    clip_rows<1>(er, fr, o, qs, nq, T, D, lane);
}

}  // namespace

void tspo::launch_score_questions(const float* h, const float* txt, const float* clip, float* scores, int Q, int T, int D, int M,
                                  float tau, hipStream_t st) {
  hipLaunchKernelGGL(score_questions_kernel, dim3((T + 3) / 4, (Q + kQChunk - 1) / kQChunk), dim3(256), 0, st, h, txt, clip, scores,
                     Q, T, D, M, tau);
}

extern "C" int tspo_clip_scores_questions(const float* txt, const float* feat, int Q, int T, int D, int M, float* clip,
                                          tspo_stream_t stream) {
  TSPO_REQUIRE(txt && feat && clip, "clip_scores_questions: null pointer");
  TSPO_REQUIRE(Q >= 1 && T >= 1 && D >= 1 && M >= 1, "clip_scores_questions: bad dims Q=%d T=%d D=%d M=%d", Q, T, D, M);
  TSPO_REQUIRE(Q <= 1000000, "clip_scores_questions: Q=%d too large (<= 1000000)", Q);
  hipLaunchKernelGGL(clip_scores_questions_kernel, dim3((T + 3) / 4, (Q + kQChunk - 1) / kQChunk), dim3(256), 0, (hipStream_t)stream,
                     txt, feat, clip, Q, T, D, M);
  return tspo::check_launch("clip_scores_questions");
}
