// The optimizers with a launch of their own over the flat fp32 master vector: SGD with momentum,
// Nesterov and weight decay (dg_momentum: module _dgopt), AdamW (dg_adamw, further down: module
// _dgadam) and LAMB (dg_lamb, last: module _dglamb).  This file is compiled once and linked into
// all three; each module has its own <name>_bindings.cpp and is loaded only for its optimizer=
// setting.  deep_go_amd/train/optim.py Momentum is the definition; per element i
//
//   gi = g[i] * gscale
//   gw = gi + wd * p[i]          if i lies in a decay range (the conv weights), else gi
//   v[i] = mu * v[i] + gw
//   u  = gw + mu * v[i]          if nesterov, else v[i]          (v[i]: the new value)
//   p[i] -= lr * u
//
// which is torch.optim.SGD(momentum, dampening 0, nesterov, weight_decay) with the learning
// rate outside the velocity.  The LR decay and the operand refresh stay with weight_refresh.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int MAX_RANGES = 20;   // elementwise.hip MAX_GU: one range per layer
constexpr int RANGE_ALIGN = 64;  // models/gocnn.py ALIGN: every tensor's first element
constexpr int MT = 256;          // threads per workgroup; one 4-vector per thread and pass
// the grid's cap: one pass per workgroup up to 8.4 M elements (12x256 has 7.2 M).  Measured at
// 12x256 against rmsprop: caps of 2048 (two vectors per thread) / 4096 / 8192 gave +0.58 /
// +0.35 / -0.28 us (profiles/opt_momentum.txt)
constexpr int MAX_BLOCKS = 8192;

// The decay ranges [b, e), sorted and disjoint, b a multiple of RANGE_ALIGN, as 32-bit element
// indices: by value in the kernel arguments (scalar loads, no scratch copy).  Unused rows hold
// NO_RANGE twice: they end after every chunk and begin inside none.
constexpr unsigned NO_RANGE = 0xFFFFFFFFu;
struct DecayRanges {
  unsigned b[MAX_RANGES];
  unsigned e[MAX_RANGES];
};

// The gradient is read with grad4_raw / grad4_f32 (dg_common.h): the raw bits are loaded first
// and widened only where the update needs them, so the wait for the load comes after the mask is
// found.

// The decay mask of one workgroup pass: MT consecutive 4-vectors from 4-vector c0, thread tid's
// four elements -> `in` inside a decay range, 0 elsewhere.  The chunk's position is uniform,
// so this is scalar work: the ends e[] sit in scalar registers (compile-time positions), r = how
// many ranges end at or before the chunk is a sum of 20 compares with no load behind it, and
// only the ranges from r on that begin inside the chunk (almost always one) are compared per
// element, as 32-bit offsets from the chunk's first element.  A range's end is no multiple of 4
// in general, hence per element.
constexpr int CE = MT * 4;          // elements per workgroup and pass
DG_DEV f32x4 chunk_mask(const DecayRanges& R, size_t c0, int tid, float in) {
  // the chunk [e0, e1) in elements, saturated: every range lies below 2^32 - 1
  const size_t c4 = c0 * 4;
  const unsigned e0 = c4 < NO_RANGE ? (unsigned)c4 : NO_RANGE;
  const unsigned e1 = c4 + CE < NO_RANGE ? (unsigned)(c4 + CE) : NO_RANGE;
  int r = 0;
#pragma unroll
  for (int q = 0; q < MAX_RANGES; ++q) r += R.e[q] <= e0 ? 1 : 0;
  f32x4 w = {0.f, 0.f, 0.f, 0.f};
  for (int q = r; q < MAX_RANGES && R.b[q] < e1; ++q) {
    // [lo, hi): the range in elements from the chunk's first, clipped to the chunk
    const int lo = R.b[q] > e0 ? (int)(R.b[q] - e0) : 0;
    const int hi = R.e[q] < e1 ? (int)(R.e[q] - e0) : CE;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid * 4 + j >= lo && tid * 4 + j < hi) w[j] = in;
  }
  return w;
}

// the same for one element of the n % 4 tail
DG_DEV float tail_mask(const DecayRanges& R, size_t i, float in) {
  float w = 0.f;
  for (int q = 0; q < MAX_RANGES; ++q)
    if (i >= R.b[q] && i < R.e[q]) w = in;
  return w;
}

// one element (and, with T = f32x4, one 4-vector): w = wd inside a decay range, else 0
template <typename T>
DG_DEV void momentum_update(T& p, T& v, const T g, const T w, float l, float mu, float gscale,
                            bool nesterov) {
  const T gw = g * gscale + w * p;
  v = mu * v + gw;
  p -= l * (nesterov ? gw + mu * v : v);
}

// One pass of a workgroup covers MT consecutive 4-vectors (a wave's loads are contiguous).
// Its loads are issued first; while they are in flight the workgroup finds the chunk's decay
// mask (chunk_mask).
template <typename G>
__global__ void __launch_bounds__(MT)
momentum_kernel(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ v, size_t n,
                const double* __restrict__ lr, float mu, int nesterov, float wd,
                const DecayRanges R, float gscale, const float* __restrict__ gate) {
  // gate 0 skips the update (sgd_kernel): return before any access
  if (gate && *gate == 0.f) return;
  const float l = (float)(*lr);
  const bool nes = nesterov != 0;
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    const bool live = i < n4;
    f32x4 pv, vv;
    decltype(grad4_raw(g, 0)) gv;
    if (live) {
      pv = ((const f32x4*)p)[i];
      vv = ((const f32x4*)v)[i];
      gv = grad4_raw(g, i);
    }
    const f32x4 w = chunk_mask(R, c0, tid, wd);
    if (live) {
      momentum_update(pv, vv, grad4_f32(gv), w, l, mu, gscale, nes);
      ((f32x4*)v)[i] = vv;
      ((f32x4*)p)[i] = pv;
    }
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    const float w = tail_mask(R, i, wd);
    float pi = p[i], vi = v[i];
    momentum_update(pi, vi, grad_at(g, i), w, l, mu, gscale, nes);
    v[i] = vi;
    p[i] = pi;
  }
}

// ------------------------------------------------------------------------------------- AdamW
// Adam with decoupled weight decay (deep_go_amd/train/optim.py AdamW is the definition).  Only
// an APPLIED step counts: t is a device counter of the optimizer's own, which a skipped step
// (gate 0) leaves alone, unlike step_count.  Per applied step, once:
//
//   t += 1;  c1 = 1 / (1 - beta1^t);  c2 = 1 / sqrt(1 - beta2^t)      (double, stored as fp32)
//
// and per element i
//
//   gi = g[i] * gscale
//   m[i] = beta1 * m[i] + (1 - beta1) * gi
//   v[i] = beta2 * v[i] + (1 - beta2) * gi * gi
//   p[i] = p[i] * (1 - lr * wd)                       if i lies in a decay range
//   p[i] = p[i] - (lr * c1) * m[i] / (sqrt(v[i]) * c2 + eps)
//
// which is torch.optim.AdamW(lr, betas, eps, weight_decay, amsgrad=False) with the decay ranges
// as one parameter group and the rest as another.
//
// The count lives in a 16-byte device record.  No thread reads a count that a thread of the
// same launch writes: adamw_tick, one wave, advances t and writes c1, c2 behind an open gate
// (nothing behind a closed one); adamw_kernel, launched after it on the same stream, only reads
// c1 and c2.  Stream order makes that race-free whatever the grid's size, and both launches are
// captured together.
struct AdamRecord {
  long long t;
  float c1, c2;
};
static_assert(sizeof(AdamRecord) == 16, "the record's layout is part of the interface");

__global__ void __launch_bounds__(64)
adamw_tick(AdamRecord* __restrict__ rec, float beta1, float beta2,
           const float* __restrict__ gate) {
  if (threadIdx.x != 0 || (gate && *gate == 0.f)) return;
  const long long t = rec->t + 1;
  // pow in double: beta^t underflows to 0 at large t, and both corrections become exactly 1
  const double d1 = 1.0 - pow((double)beta1, (double)t);
  const double d2 = 1.0 - pow((double)beta2, (double)t);
  rec->t = t;
  rec->c1 = (float)(1.0 / d1);
  rec->c2 = (float)(1.0 / sqrt(d2));
}

// one element: lw = lr wd inside a decay range, else 0 (p * (1 - 0) is exact); lc = lr c1;
// o1 = 1 - beta1, o2 = 1 - beta2.  `/` and sqrtf are the correctly rounded forms under the
// build's flags (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 and its two fma
// corrections): clang's HIP default.  The kernel is bound by its 28 bytes per element.
DG_DEV void adamw_update(float& p, float& m, float& v, float g, float lw, float lc, float b1,
                         float o1, float b2, float o2, float c2, float eps, float gscale) {
  const float gi = g * gscale;
  m = b1 * m + o1 * gi;
  v = b2 * v + (o2 * gi) * gi;
  p = p * (1.f - lw) - (lc * m) / (sqrtf(v) * c2 + eps);
}

// momentum_kernel's shape with a second state vector
template <typename G>
__global__ void __launch_bounds__(MT)
adamw_kernel(float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m,
             float* __restrict__ v, size_t n, const double* __restrict__ lr,
             const AdamRecord* __restrict__ rec, float b1, float o1, float b2, float o2,
             float eps, float wd, const DecayRanges R, float gscale,
             const float* __restrict__ gate) {
  // gate 0 skips the update: return before any access
  if (gate && *gate == 0.f) return;
  const float l = (float)(*lr);
  const float lc = l * rec->c1, c2 = rec->c2;
  const float lw = l * wd;
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    const bool live = i < n4;
    f32x4 pv, mv, vv;
    decltype(grad4_raw(g, 0)) gv;
    if (live) {
      pv = ((const f32x4*)p)[i];
      mv = ((const f32x4*)m)[i];
      vv = ((const f32x4*)v)[i];
      gv = grad4_raw(g, i);
    }
    const f32x4 w = chunk_mask(R, c0, tid, lw);
    if (live) {
      const f32x4 gf = grad4_f32(gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        adamw_update(pj, mj, vj, gf[j], w[j], lc, b1, o1, b2, o2, c2, eps, gscale);
        pv[j] = pj, mv[j] = mj, vv[j] = vj;
      }
      ((f32x4*)m)[i] = mv;
      ((f32x4*)v)[i] = vv;
      ((f32x4*)p)[i] = pv;
    }
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_update(pi, mi, vi, grad_at(g, i), tail_mask(R, i, lw), lc, b1, o1, b2, o2, c2,
                 eps, gscale);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

// -------------------------------------------------------------------------------------- LAMB
// Adam's update rescaled per conv-weight tensor by a trust ratio (deep_go_amd/train/optim.py
// Lamb is the definition; module _dglamb, lamb_bindings.cpp, loaded only for optimizer=lamb).
// The ranges R_k of the table are the adapted tensors; everything else takes ratio 1 and no
// decay.  With the tick's t, c1, c2 as above, per applied step and element i
//
//   gi = g[i] * gscale
//   m[i] = beta1 * m[i] + (1 - beta1) * gi
//   v[i] = beta2 * v[i] + (1 - beta2) * gi * gi
//   u[i] = (c1 * m[i]) / (sqrt(v[i]) * c2 + eps)  [+ wd * p[i]  if i lies in a range]
//   per range k:  SP = sum p^2, SU = sum u^2 over R_k (each rounded to fp32), wn = sqrt(SP),
//                 un = sqrt(SU) (fp32), phi = fp32(double(wn) / double(un)) if both are finite
//                 and > 0, else 1
//   p[i] = p[i] - (lr * phi_k) * u[i]                (phi = 1 outside every range)
//
// Four launches on the stream, no atomics, every sum in one fixed order that does not depend on
// the grid:
//
//   adamw_tick    as for AdamW
//   lamb_moments  adamw_kernel's shape; writes m, v and u, and per CHUNK (the CE elements of one
//                 workgroup pass) and range meeting it one fp32 pair (sum p^2, sum u^2) over the
//                 chunk's elements inside that range: thread chains in element order, the
//                 wave's xor butterfly, (w0 + w1) + (w2 + w3) — gradnorm_partial's order
//                 (clip.hip).  The pair of chunk c's j-th range (j counts from the first range
//                 that has not ended before the chunk) sits at part[(c LAMB_SLOTS + j) 2]; the
//                 n % 4 tail, which lies in at most one range because ranges begin on multiples
//                 of RANGE_ALIGN, has the chunk after the last to itself
//   lamb_ratio    one workgroup per range: its pairs summed in double (thread t takes the
//                 range's chunks t, t + MT, ... in order, then the same trees, then the tail's
//                 pair), {wn, un, phi} to row k of the record table
//   lamb_apply    p -= (lr phi) u with the chunk's ratios found by the same scalar lookup
//
// Stream order separates them: no thread reads what a thread of its own launch writes.  Each
// returns behind a closed gate before any access.
constexpr int LAMB_SLOTS = 4;     // ranges that may meet one chunk (the launcher checks)
constexpr int LAMB_ROW = 3;       // floats per row of the record table: wn, un, phi

// how many ranges end at or before element e0: the first that can meet a chunk beginning there
DG_DEV int ranges_before(const DecayRanges& R, unsigned e0) {
  int r = 0;
#pragma unroll
  for (int q = 0; q < MAX_RANGES; ++q) r += R.e[q] <= e0 ? 1 : 0;
  return r;
}

// the chunk [e0, e1) of 4-vector c0 in elements, saturated as in chunk_mask
DG_DEV void chunk_bounds(size_t c0, unsigned& e0, unsigned& e1) {
  const size_t c4 = c0 * 4;
  e0 = c4 < NO_RANGE ? (unsigned)c4 : NO_RANGE;
  e1 = c4 + CE < NO_RANGE ? (unsigned)(c4 + CE) : NO_RANGE;
}

// range q clipped to the chunk, in elements from the chunk's first
DG_DEV void chunk_span(const DecayRanges& R, int q, unsigned e0, unsigned e1, int& lo, int& hi) {
  lo = R.b[q] > e0 ? (int)(R.b[q] - e0) : 0;
  hi = R.e[q] < e1 ? (int)(R.e[q] - e0) : CE;
}

// one element: m, v as adamw_update; -> u without the decay term
DG_DEV float lamb_update(float& m, float& v, float g, float c1, float b1, float o1, float b2,
                         float o2, float c2, float eps, float gscale) {
  const float gi = g * gscale;
  m = b1 * m + o1 * gi;
  v = b2 * v + (o2 * gi) * gi;
  return (c1 * m) / (sqrtf(v) * c2 + eps);
}

template <typename G>
__global__ void __launch_bounds__(MT)
lamb_moments(const float* __restrict__ p, const G* __restrict__ g, float* __restrict__ m,
             float* __restrict__ v, float* __restrict__ u, size_t n,
             const AdamRecord* __restrict__ rec, float b1, float o1, float b2, float o2,
             float eps, float wd, const DecayRanges R, float gscale, float* __restrict__ part,
             const float* __restrict__ gate) {
  // gate 0 skips the update: return before any access
  if (gate && *gate == 0.f) return;
  __shared__ float s_w[2][MT / 64];
  const float c1 = rec->c1, c2 = rec->c2;
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    const bool live = i < n4;
    f32x4 pv = {0.f, 0.f, 0.f, 0.f}, uv = {0.f, 0.f, 0.f, 0.f}, mv, vv;
    decltype(grad4_raw(g, 0)) gv;
    if (live) {
      pv = ((const f32x4*)p)[i];
      mv = ((const f32x4*)m)[i];
      vv = ((const f32x4*)v)[i];
      gv = grad4_raw(g, i);
    }
    const f32x4 w = chunk_mask(R, c0, tid, wd);
    if (live) {
      const f32x4 gf = grad4_f32(gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = mv[j], vj = vv[j];
        uv[j] = lamb_update(mj, vj, gf[j], c1, b1, o1, b2, o2, c2, eps, gscale) + w[j] * pv[j];
        mv[j] = mj, vv[j] = vj;
      }
      ((f32x4*)m)[i] = mv;
      ((f32x4*)v)[i] = vv;
      ((f32x4*)u)[i] = uv;
    }
    // the chunk's pairs: uniform over the workgroup (almost always one range, often none)
    unsigned e0, e1;
    chunk_bounds(c0, e0, e1);
    const size_t slot0 = c0 / MT * LAMB_SLOTS;
    int q = ranges_before(R, e0);
    for (int j = 0; j < LAMB_SLOTS && q < MAX_RANGES && R.b[q] < e1; ++j, ++q) {
      int lo, hi;
      chunk_span(R, q, e0, e1, lo, hi);
      float sp = 0.f, su = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (live && tid * 4 + k >= lo && tid * 4 + k < hi) {
          sp += pv[k] * pv[k];
          su += uv[k] * uv[k];
        }
      sp = wave_sum(sp);
      su = wave_sum(su);
      if ((tid & 63) == 0) s_w[0][tid >> 6] = sp, s_w[1][tid >> 6] = su;
      __syncthreads();
      if (tid == 0)
        ((float2*)part)[slot0 + j] = float2{(s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]),
                                            (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3])};
      __syncthreads();
    }
  }
  // the n % 4 tail: at most three elements, all on one lane, in order; their pair goes to the
  // chunk after the last
  if (blockIdx.x == 0 && tid == 0 && n4 * 4 < n) {
    float sp = 0.f, su = 0.f;
    bool any = false;
    for (size_t i = n4 * 4; i < n; ++i) {
      const float in = tail_mask(R, i, 1.f);
      const float pi = p[i];
      float mi = m[i], vi = v[i];
      const float ui =
          lamb_update(mi, vi, grad_at(g, i), c1, b1, o1, b2, o2, c2, eps, gscale) +
          (in * wd) * pi;
      m[i] = mi;
      v[i] = vi;
      u[i] = ui;
      if (in != 0.f) {
        any = true;
        sp += pi * pi;
        su += ui * ui;
      }
    }
    if (any) ((float2*)part)[(n4 + MT - 1) / MT * LAMB_SLOTS] = float2{sp, su};
  }
}

// workgroup k: range k's pairs -> {wn, un, phi}
__global__ void __launch_bounds__(MT)
lamb_ratio(const float* __restrict__ part, size_t n, const DecayRanges R,
           float* __restrict__ tab, const float* __restrict__ gate) {
  // gate 0 skips the update: return before any access
  if (gate && *gate == 0.f) return;
  __shared__ double s_w[2][MT / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const size_t n4 = n / 4;
  const size_t b = R.b[k], e = R.e[k];
  const size_t lim = e < n4 * 4 ? e : n4 * 4;     // (the tail's elements are not in a chunk)
  double sp = 0.0, su = 0.0;
  if (b < lim) {
    const size_t last = (lim - 1) / CE;
    for (size_t c = b / CE + tid; c <= last; c += MT) {
      // the range's slot in chunk c: the ranges in front of it that reach into the chunk
      int j = 0;
      for (int q = 0; q < k; ++q) j += R.e[q] > c * CE ? 1 : 0;
      const float2 pr = ((const float2*)part)[c * LAMB_SLOTS + j];
      sp += (double)pr.x;
      su += (double)pr.y;
    }
  }
  sp = wave_sum_f64(sp);
  su = wave_sum_f64(su);
  if ((tid & 63) == 0) s_w[0][tid >> 6] = sp, s_w[1][tid >> 6] = su;
  __syncthreads();
  if (tid != 0) return;
  sp = (s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]);
  su = (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]);
  if (e > n4 * 4) {
    const float2 pr = ((const float2*)part)[(n4 + MT - 1) / MT * LAMB_SLOTS];
    sp += (double)pr.x;
    su += (double)pr.y;
  }
  // the sums rounded to fp32 (above its range: inf), the roots rounded to fp32, the ratio from
  // those fp32 norms in double
  const float wn = (float)sqrt((double)(float)sp), un = (float)sqrt((double)(float)su);
  const bool ok = wn > 0.f && un > 0.f && wn <= 3.402823466e38f && un <= 3.402823466e38f;
  tab[k * LAMB_ROW + 0] = wn;
  tab[k * LAMB_ROW + 1] = un;
  tab[k * LAMB_ROW + 2] = ok ? (float)((double)wn / (double)un) : 1.f;
}

// the ratios of thread tid's four elements in the chunk of 4-vector c0: chunk_mask's lookup
// with a value per range, 1 outside every range
DG_DEV f32x4 chunk_ratio(const DecayRanges& R, size_t c0, int tid, const float* tab) {
  unsigned e0, e1;
  chunk_bounds(c0, e0, e1);
  f32x4 f = {1.f, 1.f, 1.f, 1.f};
  for (int q = ranges_before(R, e0); q < MAX_RANGES && R.b[q] < e1; ++q) {
    int lo, hi;
    chunk_span(R, q, e0, e1, lo, hi);
    const float phi = tab[q * LAMB_ROW + 2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid * 4 + j >= lo && tid * 4 + j < hi) f[j] = phi;
  }
  return f;
}

__global__ void __launch_bounds__(MT)
lamb_apply(float* __restrict__ p, const float* __restrict__ u, size_t n,
           const double* __restrict__ lr, const float* __restrict__ tab, const DecayRanges R,
           const float* __restrict__ gate) {
  // gate 0 skips the update: return before any access
  if (gate && *gate == 0.f) return;
  const float l = (float)(*lr);
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    const bool live = i < n4;
    f32x4 pv, uv;
    if (live) {
      pv = ((const f32x4*)p)[i];
      uv = ((const f32x4*)u)[i];
    }
    const f32x4 f = chunk_ratio(R, c0, tid, tab);
    if (live) ((f32x4*)p)[i] = pv - (l * f) * uv;
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    float phi = 1.f;
    for (int q = 0; q < MAX_RANGES; ++q)
      if (i >= R.b[q] && i < R.e[q]) phi = tab[q * LAMB_ROW + 2];
    p[i] = p[i] - (l * phi) * u[i];
  }
}

}  // namespace

// the host table {begin, end} x n_ranges -> R, or false: more than MAX_RANGES rows, a count
// without a table, rows unsorted / overlapping / empty, a begin off RANGE_ALIGN, an end past n
// or at 2^32 - 1 and above
static bool decay_ranges(const long long* ranges, int n_ranges, size_t n, DecayRanges& R) {
  if (n_ranges < 0 || n_ranges > MAX_RANGES || (n_ranges && !ranges)) return false;
  long long prev = 0;
  for (int q = 0; q < MAX_RANGES; ++q) {
    R.b[q] = R.e[q] = NO_RANGE;
    if (q >= n_ranges) continue;
    const long long b = ranges[2 * q], e = ranges[2 * q + 1];
    if (b < prev || b % RANGE_ALIGN != 0 || e <= b || (unsigned long long)e > n ||
        e >= (long long)NO_RANGE)
      return false;
    R.b[q] = (unsigned)b;
    R.e[q] = (unsigned)e;
    prev = e;
  }
  return true;
}

// one pass per workgroup up to MAX_BLOCKS, at least one workgroup (the tail)
static unsigned grid_blocks(size_t n) {
  size_t blocks = (n / 4 + MT - 1) / MT;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  return blocks < 1 ? 1u : (unsigned)blocks;
}

extern "C" {

hipError_t dg_momentum(float* p, const float* g, float* v, size_t n, const double* lr, float mu,
                       int nesterov, float wd, const long long* ranges, int n_ranges,
                       float gscale, const float* gate, const void* g16, hipStream_t s) {
  DecayRanges R;
  if (!decay_ranges(ranges, n_ranges, n, R)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!p || !v || !lr || !(g || g16)) return hipErrorInvalidValue;
  // the 16-byte (bf16: 8-byte) vector accesses
  if ((((uintptr_t)p | (uintptr_t)v | (uintptr_t)g) & 15) || ((uintptr_t)g16 & 7))
    return hipErrorInvalidValue;
  const unsigned blocks = grid_blocks(n);
  if (g16)
    hipLaunchKernelGGL(momentum_kernel<bf16_t>, dim3(blocks), dim3(MT), 0, s, p,
                       (const bf16_t*)g16, v, n, lr, mu, nesterov, wd, R, gscale, gate);
  else
    hipLaunchKernelGGL(momentum_kernel<float>, dim3(blocks), dim3(MT), 0, s, p, g, v,
                       n, lr, mu, nesterov, wd, R, gscale, gate);
  return hipGetLastError();
}

hipError_t dg_adamw_tick(void* rec, float beta1, float beta2, const float* gate,
                         hipStream_t s) {
  // (written so that a NaN is refused too)
  if (!rec || ((uintptr_t)rec & 7) || !(beta1 >= 0.f && beta1 < 1.f) ||
      !(beta2 >= 0.f && beta2 < 1.f))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(adamw_tick, dim3(1), dim3(64), 0, s, (AdamRecord*)rec, beta1, beta2, gate);
  return hipGetLastError();
}

hipError_t dg_adamw(float* p, const float* g, float* m, float* v, size_t n, const double* lr,
                    void* rec, float beta1, float beta2, float eps, float wd,
                    const long long* ranges, int n_ranges, float gscale, const float* gate,
                    const void* g16, hipStream_t s) {
  DecayRanges R;
  if (!decay_ranges(ranges, n_ranges, n, R)) return hipErrorInvalidValue;
  // (written so that a NaN is refused too)
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!p || !m || !v || !lr || !rec || !(g || g16)) return hipErrorInvalidValue;
  // the 16-byte (bf16: 8-byte) vector accesses; the record's int64
  if ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)g) & 15) ||
      ((uintptr_t)g16 & 7) || ((uintptr_t)rec & 7))
    return hipErrorInvalidValue;
  const AdamRecord* r = (const AdamRecord*)rec;
  if (hipError_t e = dg_adamw_tick(rec, beta1, beta2, gate, s)) return e;
  const unsigned blocks = grid_blocks(n);
  const float o1 = 1.f - beta1, o2 = 1.f - beta2;
  if (g16)
    hipLaunchKernelGGL(adamw_kernel<bf16_t>, dim3(blocks), dim3(MT), 0, s, p,
                       (const bf16_t*)g16, m, v, n, lr, r, beta1, o1, beta2, o2, eps, wd, R,
                       gscale, gate);
  else
    hipLaunchKernelGGL(adamw_kernel<float>, dim3(blocks), dim3(MT), 0, s, p, g, m, v, n, lr, r,
                       beta1, o1, beta2, o2, eps, wd, R, gscale, gate);
  return hipGetLastError();
}

// the floats of LAMB's partial buffer for n elements: LAMB_SLOTS pairs per chunk and the tail's
// chunk; -1: an invalid table, or one with more than LAMB_SLOTS ranges meeting one chunk
long long dg_lamb_partials(size_t n, const long long* ranges, int n_ranges) {
  DecayRanges R;
  if (!decay_ranges(ranges, n_ranges, n, R)) return -1;
  // a chunk that several ranges meet holds the begin of one of them
  for (int k = 0; k < n_ranges; ++k) {
    const unsigned long long c = R.b[k] / CE;
    int meet = 0;
    for (int q = 0; q < n_ranges; ++q)
      meet += (R.b[q] < (c + 1) * CE && R.e[q] > c * CE) ? 1 : 0;
    if (meet > LAMB_SLOTS) return -1;
  }
  const size_t chunks = (n / 4 + MT - 1) / MT;
  return (long long)((chunks + 1) * LAMB_SLOTS * 2);
}

hipError_t dg_lamb(float* p, const float* g, float* m, float* v, float* u, size_t n,
                   const double* lr, void* rec, float* part, long long part_n, float* tab,
                   float beta1, float beta2, float eps, float wd, const long long* ranges,
                   int n_ranges, float gscale, const float* gate, const void* g16,
                   hipStream_t s) {
  DecayRanges R;
  if (!decay_ranges(ranges, n_ranges, n, R)) return hipErrorInvalidValue;
  const long long need = dg_lamb_partials(n, ranges, n_ranges);
  // (written so that a NaN is refused too)
  if (need < 0 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) ||
      !(eps > 0.f))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!p || !m || !v || !u || !lr || !rec || !part || !tab || !(g || g16))
    return hipErrorInvalidValue;
  // the 16-byte (bf16: 8-byte) vector accesses; the record's int64; the partials' pairs
  if ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)u | (uintptr_t)g) & 15) ||
      ((uintptr_t)g16 & 7) || ((uintptr_t)rec & 7) || ((uintptr_t)part & 7) ||
      ((uintptr_t)tab & 3) || part_n < need)
    return hipErrorInvalidValue;
  const AdamRecord* r = (const AdamRecord*)rec;
  if (hipError_t e = dg_adamw_tick(rec, beta1, beta2, gate, s)) return e;
  const unsigned blocks = grid_blocks(n);
  const float o1 = 1.f - beta1, o2 = 1.f - beta2;
  if (g16)
    hipLaunchKernelGGL(lamb_moments<bf16_t>, dim3(blocks), dim3(MT), 0, s, p,
                       (const bf16_t*)g16, m, v, u, n, r, beta1, o1, beta2, o2, eps, wd, R,
                       gscale, part, gate);
  else
    hipLaunchKernelGGL(lamb_moments<float>, dim3(blocks), dim3(MT), 0, s, p, g, m, v, u, n, r,
                       beta1, o1, beta2, o2, eps, wd, R, gscale, part, gate);
  if (hipError_t e = hipGetLastError()) return e;
  if (n_ranges > 0) {
    hipLaunchKernelGGL(lamb_ratio, dim3(n_ranges), dim3(MT), 0, s, part, n, R, tab, gate);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(lamb_apply, dim3(blocks), dim3(MT), 0, s, p, u, n, lr, tab, R, gate);
  return hipGetLastError();
}

}  // extern "C"
