// An exponential moving average of the flat parameter vector (dg_ema: module _dgema,
// ema_bindings.cpp, loaded only for ema_decay > 0).  deep_go_amd/train/optim.py WeightEMA is the
// definition.  Only an APPLIED step counts: t is a device counter of the average's own, which a
// skipped step (gate 0) leaves alone, unlike step_count.  Per applied step, once:
//
//   t   = t + 1
//   d   = min(decay, (1 + t) / (10 + t))        (double; the ramp is the usual warm-up)
//   omd = float(1.0 - d)
//
// and per element i, with p as the optimizer left it:
//
//   e[i] = fmaf(omd, p[i] - e[i], e[i])          (fp32: one rounded subtraction, one fma)
//
// The lerp form makes e == p a fixed point and keeps the result between e and p.  fmaf is
// written out, so that nothing is left to the compiler's contraction setting.
//
// The count lives in a 16-byte device record.  No thread reads what a thread of its own launch
// writes: ema_tick, one wave, advances t and writes omd behind an open gate (nothing behind a
// closed one); ema_kernel, launched after it on the same stream, only reads omd.  Stream order
// makes that race-free whatever the grid's size, and both launches are captured together.  No
// atomics, allocations or host syncs.
#include "dg_api.h"
#include "dg_common.h"

using namespace dg;

namespace {

constexpr int MT = 256;           // threads per workgroup; one 4-vector per thread and pass
// the grid's cap: optim.hip momentum_kernel's, one pass per workgroup up to 8.4 M elements
// (12x256 has 7.2 M).  Lower caps were tried as for clip.hip (tools/kbench_ema.py caps builds
// this file with -DDG_EMA_MAX_BLOCKS=...): profiles/ema.txt
#ifndef DG_EMA_MAX_BLOCKS
#define DG_EMA_MAX_BLOCKS 8192
#endif
constexpr int MAX_BLOCKS = DG_EMA_MAX_BLOCKS;

struct EmaRecord {
  long long t;
  float omd, pad;
};
static_assert(sizeof(EmaRecord) == 16, "the record's layout is part of the interface");

__global__ void __launch_bounds__(64)
ema_tick(EmaRecord* __restrict__ rec, double decay, const float* __restrict__ gate) {
  if (threadIdx.x != 0 || (gate && *gate == 0.f)) return;
  const long long t = rec->t + 1;
  const double td = (double)t;
  const double ramp = (1.0 + td) / (10.0 + td);
  const double d = decay < ramp ? decay : ramp;
  rec->t = t;
  rec->omd = (float)(1.0 - d);
}

// momentum_kernel's shape: one pass of a workgroup covers MT consecutive 4-vectors (a wave's
// loads are contiguous); p is only read
__global__ void __launch_bounds__(MT)
ema_kernel(const float* __restrict__ p, float* __restrict__ e, size_t n,
           const EmaRecord* __restrict__ rec, const float* __restrict__ gate) {
  // gate 0 skips the step: return before any access
  if (gate && *gate == 0.f) return;
  const float omd = rec->omd;
  const size_t n4 = n / 4;
  const int tid = threadIdx.x;
  for (size_t c0 = blockIdx.x * (size_t)MT; c0 < n4; c0 += (size_t)gridDim.x * MT) {
    const size_t i = c0 + tid;
    if (i < n4) {
      const f32x4 pv = ((const f32x4*)p)[i];
      f32x4 ev = ((const f32x4*)e)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) ev[j] = fmaf(omd, pv[j] - ev[j], ev[j]);
      ((f32x4*)e)[i] = ev;
    }
  }
  // the n % 4 tail: at most three elements, one lane each
  const size_t i = n4 * 4 + tid;
  if (blockIdx.x == 0 && i < n) {
    const float ei = e[i];
    e[i] = fmaf(omd, p[i] - ei, ei);
  }
}

// one pass per workgroup up to MAX_BLOCKS, at least one workgroup (the tail)
unsigned grid_blocks(size_t n) {
  size_t blocks = (n / 4 + MT - 1) / MT;
  if (blocks > MAX_BLOCKS) blocks = MAX_BLOCKS;
  return blocks < 1 ? 1u : (unsigned)blocks;
}

// (written so that a NaN is refused too)
bool tick_args_ok(const void* rec, double decay) {
  return rec && !((uintptr_t)rec & 7) && decay >= 0.0 && decay < 1.0;
}

}  // namespace

extern "C" {

hipError_t dg_ema_tick(void* rec, double decay, const float* gate, hipStream_t s) {
  if (!tick_args_ok(rec, decay)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ema_tick, dim3(1), dim3(64), 0, s, (EmaRecord*)rec, decay, gate);
  return hipGetLastError();
}

hipError_t dg_ema(const float* p, float* e, size_t n, void* rec, double decay, const float* gate,
                  hipStream_t s) {
  // every refusal comes before any GPU work (written so that a NaN is refused too)
  if (!(decay >= 0.0 && decay < 1.0)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  // the 16-byte vector accesses, the record's int64
  if (!p || !e || !tick_args_ok(rec, decay) || (((uintptr_t)p | (uintptr_t)e) & 15))
    return hipErrorInvalidValue;
  if (hipError_t err = dg_ema_tick(rec, decay, gate, s)) return err;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_blocks(n)), dim3(MT), 0, s, p, e, n,
                     (const EmaRecord*)rec, gate);
  return hipGetLastError();
}

}  // extern "C"
