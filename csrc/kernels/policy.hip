// Move prediction helpers around the forward pass: the eight board symmetries of a batch of
// stored positions (symmetry_planes) and the legality-masked, symmetry-averaged top-k policy
// from the head's log-probabilities (policy_ensemble).  deep_go_amd/data/symmetry.py holds the
// definition of the symmetries and the float64 oracle of policy_ensemble.
//
// The symmetries T_s, s in 0..7, of a point p = 19 x + y are sym_fwd / sym_inv of dg_common.h.
//
// Plain C++ with wave shuffles: no atomics, every reduction in a fixed order, so the results
// are bit-reproducible from run to run.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int PLANES = 9;      // stored uint8 planes per position (data/features.py)
constexpr int PT = 256;        // threads per workgroup of both kernels
constexpr int PW = PT / 64;    // waves per workgroup
constexpr int MAX_TOPK = 64;

// ------------------------------------------------------------------------------------
// Destination board j = i S + s of a packed batch <- source board i moved by T_s: the nine
// planes (dst[T_s(p)] = src[p]), the same player and rank, the label T_s(label) (or -1).
// One thread per (destination board, destination point): it reads from the inverse point, so
// a wave's stores are contiguous.  Boards j >= n S are not written.
__global__ void __launch_bounds__(PT)
symmetry_planes_kernel(const uint8_t* __restrict__ src_planes,
                       const uint8_t* __restrict__ src_player,
                       const uint8_t* __restrict__ src_rank, const int* __restrict__ src_labels,
                       int n, int S, uint8_t* __restrict__ planes, uint8_t* __restrict__ player,
                       uint8_t* __restrict__ rank, int* __restrict__ labels) {
  const int idx = blockIdx.x * PT + threadIdx.x;
  if (idx >= n * S * NPTS) return;
  const int j = idx / NPTS;
  const int p = idx - j * NPTS;
  const int i = j / S, s = j - i * S;
  const uint8_t* src = src_planes + (size_t)i * PLANES * NPTS + sym_inv(s, p);
  uint8_t* dst = planes + (size_t)j * PLANES * NPTS + p;
#pragma unroll
  for (int c = 0; c < PLANES; ++c) dst[c * NPTS] = src[c * NPTS];
  if (p == 0) {
    player[j] = src_player[i];
    rank[j] = src_rank[i];
    const int y = src_labels[i];
    labels[j] = (y >= 0 && y < NPTS) ? sym_fwd(s, y) : -1;
  }
}

// ------------------------------------------------------------------------------------
// Workgroup-wide sums in a fixed order (wave butterfly, then the waves in index order).
// s_tmp: PW slots.  Every thread of the workgroup must call them (they contain barriers).
DG_DEV float block_sum(float v, float* s_tmp) {
  v = wave_sum(v);
  __syncthreads();   // the previous use of s_tmp is over
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < PW; ++w) t += s_tmp[w];
  return t;
}

DG_DEV int block_sum_int(int v, int* s_tmp) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < PW; ++w) t += s_tmp[w];
  return t;
}

// One workgroup per position i:
//   q[p]    = (1/S) sum_{s = 0..S-1, in that order} expf(logp[i S + s][T_s(p)])
//   legal   = !mask || (stones[p] == 0 && extra_illegal[p] == 0)
//   prob[p] = q[p] / sum_{legal} q at legal points, 0 elsewhere (all 0 without a legal point)
//   topk    = the K legal points of largest prob, ties to the lower index (K rounds of
//             workgroup argmax); tail -1 / 0 when fewer than K points are legal
//   label_rank = #legal r ahead of the label y in that order; -1 without a legal label
__global__ void __launch_bounds__(PT)
policy_ensemble_kernel(const float* __restrict__ logp, const uint8_t* __restrict__ stones,
                       int stones_stride, const uint8_t* __restrict__ extra_illegal,
                       const int* __restrict__ labels, int S, int K, int mask,
                       float* __restrict__ prob, int* __restrict__ topk_idx,
                       float* __restrict__ topk_p, int* __restrict__ label_rank) {
  __shared__ float s_p[NPTS];         // q, then prob
  __shared__ uint8_t s_legal[NPTS];
  __shared__ uint8_t s_avail[NPTS];   // legal and not yet taken by a top-k round
  __shared__ float s_red[PW];
  __shared__ int s_redi[PW];
  const int i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_s = 1.f / (float)S;

  float part = 0.f;
  int nleg = 0;
  for (int p = tid; p < NPTS; p += PT) {
    float q = 0.f;
    for (int s = 0; s < S; ++s) q += expf(logp[((size_t)i * S + s) * NPTS + sym_fwd(s, p)]);
    q *= inv_s;
    bool legal = true;
    if (mask) {
      legal = stones[(size_t)i * stones_stride + p] == 0;
      if (extra_illegal && extra_illegal[(size_t)i * NPTS + p] != 0) legal = false;
    }
    s_p[p] = q;
    s_legal[p] = legal;
    s_avail[p] = legal;
    if (legal) { part += q; ++nleg; }
  }
  const float tot = block_sum(part, s_red);
  nleg = block_sum_int(nleg, s_redi);
  for (int p = tid; p < NPTS; p += PT) {
    const float v = (nleg > 0 && s_legal[p]) ? s_p[p] / tot : 0.f;
    s_p[p] = v;
    prob[(size_t)i * NPTS + p] = v;
  }
  __syncthreads();

  // ---- rank of the label ----
  {
    const int y = labels ? labels[i] : -1;
    const bool ok = y >= 0 && y < NPTS && s_legal[y];   // uniform over the workgroup
    int ahead = 0;
    if (ok) {
      const float py = s_p[y];
      for (int r = tid; r < NPTS; r += PT)
        if (s_legal[r] && (s_p[r] > py || (s_p[r] == py && r < y))) ++ahead;
    }
    ahead = block_sum_int(ahead, s_redi);
    if (tid == 0) label_rank[i] = ok ? ahead : -1;
  }

  // ---- top-k: K rounds of argmax over the points still available ----
  for (int k = 0; k < K; ++k) {
    float bv = -1.f;          // below every probability
    int bi = NPTS;            // no candidate
    for (int p = tid; p < NPTS; p += PT)
      if (s_avail[p] && s_p[p] > bv) { bv = s_p[p]; bi = p; }   // ascending p: ties keep the lower
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();          // the previous round's reads of s_red / s_redi are over
    if (lane == 0) { s_red[wave] = bv; s_redi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
      float v = s_red[0];
      int idx = s_redi[0];
#pragma unroll
      for (int w = 1; w < PW; ++w)
        if (s_red[w] > v || (s_red[w] == v && s_redi[w] < idx)) { v = s_red[w]; idx = s_redi[w]; }
      const bool found = idx < NPTS;
      topk_idx[(size_t)i * K + k] = found ? idx : -1;
      topk_p[(size_t)i * K + k] = found ? s_p[idx] : 0.f;
      if (found) s_avail[idx] = 0;
    }
    __syncthreads();          // the winner has left s_avail
  }
}

}  // namespace

extern "C" {

hipError_t dg_symmetry_planes(const uint8_t* src_planes, const uint8_t* src_player,
                              const uint8_t* src_rank, const int* src_labels, int n, int S,
                              uint8_t* planes, uint8_t* player, uint8_t* rank, int* labels,
                              int B, hipStream_t s) {
  if (n < 0 || (S != 1 && S != 8) || B < 0 || (long long)n * S > B) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!src_planes || !src_player || !src_rank || !src_labels || !planes || !player || !rank ||
      !labels)
    return hipErrorInvalidValue;
  const int total = n * S * NPTS;
  hipLaunchKernelGGL(symmetry_planes_kernel, dim3((total + PT - 1) / PT), dim3(PT), 0, s,
                     src_planes, src_player, src_rank, src_labels, n, S, planes, player, rank,
                     labels);
  return hipGetLastError();
}

hipError_t dg_policy_ensemble(const float* logp, const uint8_t* stones, int stones_stride,
                              const uint8_t* extra_illegal, const int* labels, int n, int S,
                              int K, int mask, float* prob, int* topk_idx, float* topk_p,
                              int* label_rank, hipStream_t s) {
  if (n < 0 || (S != 1 && S != 8) || K < 1 || K > MAX_TOPK || (mask != 0 && mask != 1))
    return hipErrorInvalidValue;
  if (mask && (!stones || stones_stride < NPTS)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!logp || !prob || !topk_idx || !topk_p || !label_rank) return hipErrorInvalidValue;
  hipLaunchKernelGGL(policy_ensemble_kernel, dim3(n), dim3(PT), 0, s, logp, stones,
                     stones_stride, extra_illegal, labels, S, K, mask, prob, topk_idx, topk_p,
                     label_rank);
  return hipGetLastError();
}

}  // extern "C"
