// Global-norm gradient clipping over the flat gradient (dg_grad_clip: module _dgclip,
// clip_bindings.cpp, loaded only for grad_clip > 0).  deep_go_amd/train/optim.py clip_grad_ is
// the definition; with c = max_norm, once per applied step
//
//   norm  = |gscale| * sqrt(sum_i g[i]^2)
//   r     = c / (norm + 1e-6)
//   scale = r < 1 ? r : 1
//   g[i]  = g[i] * scale          (the optimizer behind it still applies gscale)
//
// which is torch.nn.utils.clip_grad_norm_(params, c, norm_type=2) applied to g * gscale.  An
// overflowing sum of squares gives norm = inf and scale = 0, a NaN norm scale = 1.
//
// Two launches on the stream, no atomics, every sum in one fixed order, so the record and the
// scaled gradient are bit-reproducible:
//
//   gradnorm_partial  up to CLIP_PARTIALS workgroups, each one fp32 partial of the sum of
//                     squares to part[blockIdx.x]
//   clip_apply        every workgroup sums the partials in double in the same order, so all
//                     derive the same norm and scale bits; workgroup 0 writes the record; the
//                     gradient is scaled
//
// Stream order between the two makes the partials race-free: no thread reads what a thread of
// its own launch writes.  Both return behind a closed gate (gate 0: a skipped step) before any
// access, which leaves the gradient, the partials and the record untouched.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int MT = 256;             // threads per workgroup; one 4-vector per thread and pass
constexpr int CLIP_PARTIALS = 1024; // the first launch's grid cap = the partial buffer's size
// the second launch's grid cap.  Every workgroup repeats the sum of the partials before it
// scales its share, so fewer, longer workgroups pay for it less often: measured against
// momentum_kernel's cap of 8192 at the 12x256 size, caps of 4096 / 2048 / 1024 took the
// clipping pair from 17.1 us to 14.2 / 12.5 / 12.0 us and the pair that does not clip from
// 13.0 us to 10.3 / 8.3 / 7.3 us (12x128: 9.8 -> 9.9 / 9.3 / 8.2 us clipping); the bits are
// the same (profiles/clip.txt)
constexpr int MAX_BLOCKS = 1024;
constexpr int AHEAD = 4;            // passes whose loads are issued before their sums
static_assert(CLIP_PARTIALS == 4 * MT, "clip_apply: four partials per thread");

// The device record: the last applied step's norm and scale, and how many applied steps clipped.
struct ClipRecord {
  float norm, scale;
  long long clipped;
};
static_assert(sizeof(ClipRecord) == 16, "the record's layout is part of the interface");

// Workgroup blockIdx.x's share of sum g[i]^2.  Thread tid takes 4-vector c0 + tid of every pass
// c0 = (blockIdx.x + k gridDim.x) MT and adds its four squares to one fp32 chain, element by
// element, passes in increasing k (the loads of AHEAD passes are issued together; the order of
// the sums does not change).  Workgroup 0's threads 0..2 append one element of the n % 4 tail.
// Then a fixed tree: the xor butterfly of a wave (every lane ends with the same bits), and
// (w0 + w1) + (w2 + w3) over the four waves.
template <typename G>
__global__ void __launch_bounds__(MT)
gradnorm_partial(const G* __restrict__ g, size_t n, float* __restrict__ part,
                 const float* __restrict__ gate) {
  // gate 0 skips the step: return before any access
  if (gate && *gate == 0.f) return;
  __shared__ float s_w[MT / 64];
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  const size_t stride = (size_t)gridDim.x * MT;
  float s = 0.f;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += AHEAD * stride) {
    decltype(grad4_raw(g, 0)) raw[AHEAD];
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const size_t i = c0 + k * stride + tid;
      if (i < n4) raw[k] = grad4_raw(g, i);
    }
#pragma unroll
    for (int k = 0; k < AHEAD; ++k) {
      const size_t i = c0 + k * stride + tid;
      if (i < n4) {
        const f32x4 v = grad4_f32(raw[k]);
#pragma unroll
        for (int j = 0; j < 4; ++j) s += v[j] * v[j];
      }
    }
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    const float v = grad_at(g, i);
    s += v * v;
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) s_w[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// Every workgroup: S = the sum of the np <= CLIP_PARTIALS partials in double, thread t taking
// (p[4t] + p[4t+1]) + (p[4t+2] + p[4t+3]) (absent ones count 0), then the same tree as above;
// norm = float(|gscale| sqrt(S)), r = c / (norm + 1e-6) in double from that fp32 norm, scale =
// r < 1 ? float(r) : 1.  All workgroups read the same partials in the same order: the same
// bits everywhere.  out == nullptr (the fp32 gradient): g is scaled in place, and left alone
// when scale == 1.  out given (the bf16 wire): out[i] = scale * float(g[i]) always; the twin g
// is only read.
template <typename G>
__global__ void __launch_bounds__(MT)
clip_apply(G* __restrict__ g, float* __restrict__ out, size_t n, const float* __restrict__ part,
           int np, ClipRecord* __restrict__ rec, float max_norm, float gscale,
           const float* __restrict__ gate) {
  // gate 0 skips the step: return before any access
  if (gate && *gate == 0.f) return;
  __shared__ double s_w[MT / 64];
  const int tid = threadIdx.x;
  double q[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = 4 * tid + j < np ? (double)part[4 * tid + j] : 0.0;
  double S = wave_sum_f64((q[0] + q[1]) + (q[2] + q[3]));
  if ((tid & 63) == 0) s_w[tid >> 6] = S;
  __syncthreads();
  S = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  const float norm = (float)(fabs((double)gscale) * sqrt(S));
  const double r = (double)max_norm / ((double)norm + 1e-6);
  const float scale = r < 1.0 ? (float)r : 1.f;     // (a NaN norm: scale 1)
  if (blockIdx.x == 0 && tid == 0) {
    rec->norm = norm;
    rec->scale = scale;
    if (scale < 1.f) rec->clipped += 1;
  }
  constexpr bool inplace = sizeof(G) == 4;
  if (inplace && scale == 1.f) return;
  const size_t n4 = n / 4;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    if (i < n4) {
      const f32x4 v = grad4_f32(grad4_raw(g, i)) * scale;
      if constexpr (inplace) ((f32x4*)g)[i] = v;
      else ((f32x4*)out)[i] = v;
    }
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    const float v = grad_at(g, i) * scale;
    if constexpr (inplace) g[i] = v;
    else out[i] = v;
  }
}

// one pass per workgroup up to cap, at least one workgroup (the tail, the record)
unsigned grid_blocks(size_t n, int cap) {
  size_t blocks = (n / 4 + MT - 1) / MT;
  if (blocks > (size_t)cap) blocks = cap;
  return blocks < 1 ? 1u : (unsigned)blocks;
}

// exactly one of g (fp32, 16-byte aligned) and g16 (bf16, 8-byte aligned); part holds part_n
// >= CLIP_PARTIALS floats
bool norm_args_ok(const float* g, const void* g16, const float* part, int part_n) {
  if (!(g || g16) || (g && g16) || !part || part_n < CLIP_PARTIALS) return false;
  return !(((uintptr_t)g & 15) || ((uintptr_t)g16 & 7) || ((uintptr_t)part & 3));
}

unsigned launch_norm(const float* g, const void* g16, size_t n, float* part, const float* gate,
                     hipStream_t s) {
  const unsigned blocks = grid_blocks(n, CLIP_PARTIALS);
  if (g16)
    hipLaunchKernelGGL(gradnorm_partial<bf16_t>, dim3(blocks), dim3(MT), 0, s,
                       (const bf16_t*)g16, n, part, gate);
  else
    hipLaunchKernelGGL(gradnorm_partial<float>, dim3(blocks), dim3(MT), 0, s, g, n, part, gate);
  return blocks;
}

}  // namespace

extern "C" {

int dg_clip_partials() { return CLIP_PARTIALS; }

hipError_t dg_grad_norm(const float* g, const void* g16, size_t n, float* part, int part_n,
                        const float* gate, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!norm_args_ok(g, g16, part, part_n)) return hipErrorInvalidValue;
  launch_norm(g, g16, n, part, gate, s);
  return hipGetLastError();
}

hipError_t dg_grad_clip(float* g, const void* g16, float* out, size_t n, float* part,
                        int part_n, void* rec, float max_norm, float gscale, const float* gate,
                        hipStream_t s) {
  // (written so that a NaN is refused too)
  if (!(max_norm > 0.f) || !(max_norm <= 3.402823466e38f) ||
      !(__builtin_fabsf(gscale) <= 3.402823466e38f))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!norm_args_ok(g, g16, part, part_n) || !rec || ((uintptr_t)rec & 7)) return hipErrorInvalidValue;
  // the bf16 twin is widened into out, the fp32 gradient is scaled in place
  if (g16 ? (!out || ((uintptr_t)out & 15)) : out != nullptr) return hipErrorInvalidValue;
  const int np = (int)launch_norm(g, g16, n, part, gate, s);
  if (hipError_t e = hipGetLastError()) return e;
  const unsigned blocks = grid_blocks(n, MAX_BLOCKS);
  if (g16)
    hipLaunchKernelGGL(clip_apply<const bf16_t>, dim3(blocks), dim3(MT), 0, s,
                       (const bf16_t*)g16, out, n, part, np, (ClipRecord*)rec, max_norm, gscale,
                       gate);
  else
    hipLaunchKernelGGL(clip_apply<float>, dim3(blocks), dim3(MT), 0, s, g, (float*)nullptr, n,
                       part, np, (ClipRecord*)rec, max_norm, gscale, gate);
  return hipGetLastError();
}

}  // extern "C"
