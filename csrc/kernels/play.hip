// Move selection for play: one move per position, drawn on the device from policy_ensemble's
// legal-move distribution with a temperature and a nucleus (top-p) cut.
// deep_go_amd/play/select.py holds the definition in words and the float64 oracle
// select_moves / select_uniform.  The launcher is built into its own small extension, _dgplay
// (play_bindings.cpp), imported only when a selection is asked for.
//
// The draw of a position is a pure 32-bit integer hash of (seed, game, ply): no generator
// state, so it does not depend on which chunk or batch slot carries the position, and the host
// repeats it bit for bit.
//
// Plain C++ with wave shuffles and LDS: no atomics, every sum in a fixed order, so the results
// are bit-reproducible from run to run.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int ST = 384;        // threads per workgroup: thread p < 361 owns point p
constexpr int SW = ST / 64;    // waves per workgroup

// select_uniform of play/select.py: h of three mix32 rounds, u = (h >> 8) * 2^-24 (exact in
// fp32: a 24-bit integer times a power of two)
__host__ __device__ inline float hash_uniform(unsigned long long seed, int game, int ply) {
  const uint32_t a = mix32(((uint32_t)seed ^ 0x3c6ef372u) + (uint32_t)(seed >> 32));
  const uint32_t b = mix32(a + (uint32_t)game);
  const uint32_t h = mix32(b ^ (uint32_t)ply);
  return (float)(h >> 8) * 0x1p-24f;
}

// Workgroup-wide reductions in a fixed order (wave butterfly, then the waves in index order).
// Every thread of the workgroup must call them (they contain barriers).
DG_DEV float wg_sum(float v, float* s_tmp) {
  v = wave_sum(v);
  __syncthreads();   // the previous use of s_tmp is over
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < SW; ++w) t += s_tmp[w];
  return t;
}
DG_DEV int wg_sum_int(int v, int* s_tmp) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < SW; ++w) t += s_tmp[w];
  return t;
}
DG_DEV int wg_min_int(int v, int* s_tmp) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s_tmp[0];
#pragma unroll
  for (int w = 1; w < SW; ++w) t = min(t, s_tmp[w]);
  return t;
}
// the point of largest v, ties to the lower index (NPTS when no thread offers one: idx = NPTS)
DG_DEV int wg_argmax(float v, int idx, float* s_tmp, int* s_tmpi) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s_tmp[threadIdx.x >> 6] = v; s_tmpi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  float bv = s_tmp[0];
  int bi = s_tmpi[0];
#pragma unroll
  for (int w = 1; w < SW; ++w)
    if (s_tmp[w] > bv || (s_tmp[w] == bv && s_tmpi[w] < bi)) { bv = s_tmp[w]; bi = s_tmpi[w]; }
  return bi;
}

// One workgroup per position i; thread p < 361 owns point p (threads 361..383 hold a zero).
// All branches on row properties are uniform over the workgroup.  The steps are those of
// play/select.py, in its notation.
__global__ void __launch_bounds__(ST)
policy_select_kernel(const float* __restrict__ prob, const int* __restrict__ game,
                     const int* __restrict__ ply, unsigned long long seed, float T, float top_p,
                     int* __restrict__ move, float* __restrict__ p_move,
                     int* __restrict__ kept) {
  __shared__ float s_w[NPTS];      // w, then the kept weights (0 at points not kept)
  __shared__ float s_red[SW];
  __shared__ int s_redi[SW];
  __shared__ float s_wk;
  const int i = blockIdx.x;
  const int p = threadIdx.x;
  const bool own = p < NPTS;
  const float v = own ? prob[(size_t)i * NPTS + p] : 0.f;

  // a non-finite or negative entry; a row of zeros
  const int bad = wg_sum_int(!(v >= 0.f && v <= 3.402823466e38f), s_redi);
  const int npos = wg_sum_int(v > 0.f, s_redi);
  if (bad || npos == 0) {
    if (p == 0) {
      move[i] = -1;
      if (p_move) p_move[i] = 0.f;
      if (kept) kept[i] = bad ? -1 : 0;
    }
    return;
  }

  float w = v;
  if (T != 0.f && T != 1.f) w = v > 0.f ? expf(logf(v) / T) : 0.f;
  const float W = T == 0.f ? 0.f : wg_sum(w, s_red);
  if (W == 0.f) {   // T == 0, or every tempered weight underflowed: the largest prob
    const int best = wg_argmax(v > 0.f ? v : -1.f, v > 0.f ? p : NPTS, s_red, s_redi);
    if (p == 0) {
      move[i] = best;
      if (p_move) p_move[i] = 1.f;
      if (kept) kept[i] = 1;
    }
    return;
  }

  // above[p]: the weight ahead of p, summed in index order (every thread reads the same
  // s_w[q] at the same time: an LDS broadcast)
  if (own) s_w[p] = w;
  __syncthreads();
  float above = 0.f;
  if (own)
    for (int q = 0; q < NPTS; ++q) {
      const float wq = s_w[q];
      if (wq > w || (wq == w && q < p)) above += wq;
    }
  const bool keep = own && w > 0.f && above < top_p * W;
  const int nkept = wg_sum_int(keep, s_redi);   // (its barriers end the reads of s_w above)
  if (own) s_w[p] = keep ? w : 0.f;
  __syncthreads();

  // c[p]: the kept weight up to and including p, in index order; Wk = c[360]
  float c = 0.f;
  if (own)
    for (int q = 0; q <= p; ++q) c += s_w[q];
  if (p == NPTS - 1) s_wk = c;
  __syncthreads();
  const float Wk = s_wk;
  const float u = hash_uniform(seed, game[i], ply[i]);
  int pick = wg_min_int(keep && c > u * Wk ? p : NPTS, s_redi);
  if (pick == NPTS) pick = NPTS - 1 - wg_min_int(keep ? NPTS - 1 - p : NPTS, s_redi);
  if (p == pick) {
    move[i] = p;
    if (p_move) p_move[i] = w / Wk;
    if (kept) kept[i] = nkept;
  }
}

}  // namespace

extern "C" {

float dg_select_uniform(unsigned long long seed, int game, int ply) {
  return hash_uniform(seed, game, ply);
}

hipError_t dg_policy_select(const float* prob, const int* game, const int* ply, int n,
                            unsigned long long seed, float temperature, float top_p, int* move,
                            float* p_move, int* kept, hipStream_t stream) {
  if (n < 0 || !prob || !game || !ply || !move) return hipErrorInvalidValue;
  if (!(temperature >= 0.f && temperature <= 3.402823466e38f)) return hipErrorInvalidValue;
  if (!(top_p > 0.f && top_p <= 1.f)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(policy_select_kernel, dim3(n), dim3(ST), 0, stream, prob, game, ply, seed,
                     temperature, top_p, move, p_move, kept);
  return hipGetLastError();
}

}  // extern "C"
