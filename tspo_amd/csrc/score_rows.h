// Per-(frame row, text row) device helpers of the scoring tail, shared by selector.hip (score_fwd_kernel, score_bwd_kernel) and
// questions.hip (one video, Q questions), and the host launchers questions.hip provides to selector.hip.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }
// this lane's share of h.h, h.e and e.e over a row of nv float4 (lane + 64 i): the loads of up to 4 chunks of BOTH rows are issued
// together, then the arithmetic (D <= 1024: one round trip per row)
__device__ __forceinline__ void row_dots(const f32x4* __restrict__ hr, const f32x4* __restrict__ er, int nv, int lane, bool want_hh,
                                         float& hh, float& de, float& ee) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = lane; c0 < nv; c0 += 256) {
    f32x4 hv[4], ev[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i;
      hv[i] = c < nv ? hr[c] : z;
      ev[i] = c < nv ? er[c] : z;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (want_hh) hh += dot4(hv[i], hv[i]);
      de += dot4(hv[i], ev[i]);
      ee += dot4(ev[i], ev[i]);
    }
  }
}

namespace tspo {
// The scoring tail of tspo_selector_forward_questions (questions.hip): scores[q, t] for q < Q from ONE read of h2[t, :].
// h [T, D], txt [Q, M, D], clip [Q, T] or nullptr, scores [Q, T].  Launch only; the caller checks the launch.
void launch_score_questions(const float* h, const float* txt, const float* clip, float* scores, int Q, int T, int D, int M, float tau,
                            hipStream_t st);
}  // namespace tspo
